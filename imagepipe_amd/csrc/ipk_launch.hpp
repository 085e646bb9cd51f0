// ipk_launch.hpp -- host-callable launchers of the gfx950 kernels (defined in ipk_kernels.hip).
// Plain C++ declarations so the C-ABI layer (ipk_api.cpp) never sees device code.
#pragma once
#include <hip/hip_runtime_api.h>
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include "ipk_host.hpp"

namespace ipk {

typedef Spline SplineHost;

// the per-stream task-queue heads of the row-walking kernels: one device block per library context, allocated on the device that is current when
// create_task_queues() is called (ipk_ctx_create) and released by destroy_task_queues() (ipk_ctx_destroy); null = every launch runs its static schedule
struct TaskQueues;
TaskQueues *create_task_queues();
void destroy_task_queues(TaskQueues *q);

template <typename T>
void launch_gofloat_cfa(const T *src, size_t owidth, size_t x, size_t y, size_t w, size_t h, float black0, float white0,
                        float *dst, hipStream_t s);
template <typename T>
void launch_gofloat_mono(const T *src, size_t owidth, size_t x, size_t y, size_t w, size_t h, float black0, float white0,
                         float *dst4, hipStream_t s);
template <typename T>
void launch_gofloat_rgb(const T *src, size_t owidth, size_t x, size_t y, size_t w, size_t h, const float *black4, const float *white4,
                        float *dst4, hipStream_t s);
void launch_gofloat_other_u8(const uint8_t *src, size_t owidth, size_t x, size_t y, size_t w, size_t h,
                             const void *gamma_reverse_pairs, float *dst4, hipStream_t s);
void launch_gofloat_other_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t w, size_t h, float *dst4, hipStream_t s);

void launch_demosaic_full(const float *src, size_t width, size_t img_height, size_t src_row0, size_t out_row0, size_t out_rows,
                          const uint32_t *lookups_dev, float *dst4, hipStream_t s);

// returns 0, or -4 when the launch could not be enqueued (hipGetLastError after the launch)
int launch_demosaic_bayer(const float *src, size_t width, size_t img_height, size_t src_row0, size_t out_row0, size_t out_rows,
                          int xoff, int yoff, const float *gen_cells, int gen_pw, int gen_ph, float *dst4, int num_cus, TaskQueues *queues, hipStream_t s);
void selftest_task_queue(bool enabled);   // test hook: false = every following launch runs the queue-less static schedule
// Launch log (test hook, host side only): which kernels of this library were launched while the log was enabled.  One entry per distinct kernel
// and tag, in the format
//     <mangled kernel symbol>            or            <mangled kernel symbol>[key=value,key=value...]
// The symbol is the code object's (hipKernelNameRefByPtr, resolved when the log is READ, never at launch).  The bracketed tag is attached by
// launchers whose kernel also branches on a value the host knows: k_gamma [vec4=,wrap=], k_output8 / k_output16 [vec4=] (16-byte groups or sample by
// sample; wrap: the grid cap holds), k_gofloat_cfa_v4 [rowwrap=] (more rows than grid rows), the ipk_raw_scaled_demosaic kernels
// [norm_fast=,norm_light=,fast_x=,fast_y=,xcd=] (xcd: 0 plain grid, 1 XCD row grouping, 2 grouping with leftover rows; their window launches,
// ipk_raw_scaled_demosaic_window, append win=1: [norm_fast=,...,xcd=,win=1]; the monochrome / three-sample launches of k_raw_scaled_demosaic by
// ipk_plain_scale_down append plain=1 / plain=3 behind that; its batch launches -- ipk_raw_scaled_demosaic_batch / ipk_plain_scale_down_batch -- append
// batch=1 behind all of it: [...,xcd=0,batch=1] / [...,xcd=0,plain=1,batch=1]; the frame-table launches -- ipk_scaled_demosaic_batch_each -- append frames=1
// behind batch=1 and print the four digits in front as 0: [norm_fast=0,...,xcd=0,batch=1,frames=1], the sized ones -- ipk_scaled_demosaic_batch_sized --
// sized=1 behind that), k_raster_scale_down [win=1] on window launches only (whole frames: no tag),
// k_pointwise_chain<false> / k_pointwise_chain_small / k_raster_chain / k_fused_resample [fast_ok=] (0: every pixel takes the literal form); the gather
// launches of k_pointwise_chain<false> / k_pointwise_chain_small / k_raster_chain<Rgbe32, 1 | 2> (a GatherSource: ipk_pipeline_run_cached_region) append
// gather=1: [fast_ok=,gather=1] -- flat launches never carry the key; the frame-table launches of k_pointwise_chain_small / k_raster_chain<Rgbe32, 1 | 2>
// (launch_chain_batch: ipk_pointwise_chain_out_batch) carry [fast_ok=,batch=1], fast_ok the AND over the launch's frames, and [fast_ok=,batch=1,orient=1]
// when at least one frame's record gathers (ipk_pointwise_chain_out_batch_oriented), sized=1 behind either when the records bring their own pixel counts
// (ipk_pointwise_chain_out_batch_sized);
// k_raster_chain's launches by ipk_plain_to_srgb append rect=1 in rectangle mode (a rectangle narrower than the source's pitch) and levels=1 / levels=2
// in the three-sample / monochrome raw sample modes, in that order: [fast_ok=,rect=1], [fast_ok=,levels=2], [fast_ok=,rect=1,levels=1] -- launches
// that use neither mode (ipk_raster_to_srgb, ipk_pointwise_chain_out, a full-width raster rectangle) carry [fast_ok=] and nothing else;
// k_fused_resample's axis-aligned mode (ipk_raw_to_srgb_scaled) [fast_ok=,axis=1]; k_fused_resample's window launches (launch_fused_resample with a
// ResampleWindow: ipk_raw_to_srgb_resampled_window / _scaled_window, regions under IPK_FUSED_WINDOW_REGIONS) append win=1: [fast_ok=,win=1] /
// [fast_ok=,axis=1,win=1] -- whole-frame launches never carry the key; its window launches over a cached 4-channel buffer (src_rgbe:
// ipk_pipeline_run_cached_region under IPK_FUSED_CACHED_RESAMPLE, both passes' second under IPK_FUSED_SCALED_ROTATECROP) append rgbe=1 behind that:
// [fast_ok=,win=1,rgbe=1]; its RGBE output mode (ipk_raw_demosaic_scaled / _window) [fast_ok=,axis=1,rgbe_out=1] / [fast_ok=,axis=1,rgbe_out=1,win=1]; the generic-CFA runtime-flag variants of k_fused_bayer /
// k_fused_bayer_window [four=1] on the launches of a filter with a fourth colour only (FusedLaunch::four) -- three-colour launches carry no tag.
void launch_log_enable(bool on);                 // clears the log, then switches it on or off
size_t launch_log_read(char *buf, size_t cap);   // entries sorted, newline-separated, NUL-terminated (truncated to cap); returns the bytes a full read needs

template <typename T>
void launch_transform_buffer(const T *src, size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                             int64_t blx, int64_t bly, size_t nwidth, size_t nheight, size_t components,
                             const uint8_t *cfa48_dev, T *dst, hipStream_t s);

// A rectangle of a launch's nwidth x nheight result (launch_raster_scale_down, launch_raw_scaled_demosaic, launch_fused_resample): non-empty and inside it
struct ResampleWindow { size_t row0, col0, rows, cols; };
// run_other + scale_down_opbuf in one pass over an RGB8 / RGB16 raster (gofloat.rs:171-201 + scaling.rs:147-160)
// win (optional, here and in launch_raw_scaled_demosaic): only that rectangle of the result is computed and dst4 holds rows * cols packed pixels; the
// grid is sized from the window, the kernel chosen as for the whole frame, and every pixel's bits are those of the whole-frame launch (the kernels
// work from absolute rows and columns).  Null: the whole frame, whose log entries are unchanged
void launch_raster_scale_down(const void *src, int src_is_u16, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                              size_t nwidth, size_t nheight, const void *gamma_reverse_pairs, float *dst4, hipStream_t s, const ResampleWindow *win = nullptr);
// plain (optional): the source is no mosaic but a monochrome (layout 1) or three-sample (layout 3) raw -- OpGoFloat::run_raw's 4-channel buffer through
// scale_down_opbuf, E = +0.0 -- with the level pairs of its channels (layout 1 reads pair 0 alone).  Such launches always take the general kernel
// k_raw_scaled_demosaic<T>, whatever the skips and dst4's alignment, read no filter (cfa48_dev may be null; black0 / white0, norm_fast and the pattern
// size are ignored), and append plain=1 / plain=3 to the tag: [norm_fast=0,...,xcd=0,plain=1] / [...,xcd=0,win=1,plain=3]
struct PlainLevels { int layout; float black[3], white[3]; };
struct ScaledDemosaicLaunch {
  const void *src; bool src_is_u16;
  size_t owidth, x, y, width, height;
  float black0, white0;
  int norm_fast, has_fourth_colour;
  size_t nwidth, nheight;
  const uint8_t *cfa48_dev; int pattern_width, pattern_height;
  float *dst4;
  size_t band_src_row0, band_out_row0, band_out_rows;      // band_out_rows == 0: the whole frame
  const ResampleWindow *win;                               // not together with a band
  const PlainLevels *plain;
  const void *const *batch_srcs; size_t batch_n;           // batch mode, below (src is not read)
};
void launch_raw_scaled_demosaic(const ScaledDemosaicLaunch &l, hipStream_t s);
// Which kernel a whole-frame, band or window launch of launch_raw_scaled_demosaic takes: true = the general kernel k_raw_scaled_demosaic<T> (a skip above
// 7 or below 1, a frame under 8 samples wide, a destination off a 16-byte boundary, every plain layout), false = a window-8 kernel.  The launcher's own
// test, with its f32 skips
inline bool raw_scaled_demosaic_general(size_t width, size_t height, size_t nwidth, size_t nheight, bool dst_aligned16, bool plain) {
  const float skip_x = ((float)((int64_t)width - 1) - 0.0f) / ((float)(nwidth - 1));
  const float skip_y = ((float)((int64_t)height - 1) - 0.0f) / ((float)(nheight - 1));
  return !(!plain && skip_x >= 1.0f && skip_x <= 7.0f && skip_y >= 1.0f && skip_y <= 7.0f && width >= 8 && dst_aligned16);
}
// Batch mode (batch_n > 0; whole frames only, and only where raw_scaled_demosaic_general holds -- nothing is launched otherwise): batch_srcs[0 .. batch_n)
// are the frames of one shape (a host array, read before the call returns: the pointers travel by value in the kernel's arguments), dst4 holds batch_n
// packed nwidth x nheight results one after another, slice i bit-identical to the single-frame launch of batch_srcs[i].  One launch per 64 frames,
// blockIdx.z the frame; the launches append batch=1 to the tag: [norm_fast=,...,xcd=0,batch=1] / [...,xcd=0,plain=1,batch=1]
// Frame-table mode (launch_raw_scaled_demosaic_each): n <= kScaledEachMax whole frames of one source type, layout (0 mosaic, 1 monochrome, 3 three-sample) and
// result size, frame i with the source, pitch, sensor window, levels (layout 0 and 1 read pair 0 alone) and -- layout 0 -- 48 x 48 device filter table of
// frames[i] (a host array, read before the call returns).  Every frame must select the general kernel for a 16-byte aligned destination
// (raw_scaled_demosaic_general; dst4 itself needs element alignment only).  The launcher writes one record per frame into table_dev --
// scaled_each_table_bytes(n) bytes of device memory the caller keeps alive until the launch has run (the context's scratch pool) -- with a stream-ordered
// copy in front of the ONE launch; blockIdx.z is the frame over the batch launch's grid, a block reads its frame's record where the other modes read the
// kernel's arguments and is otherwise the single launch of that frame: slice i of dst4 is bit-identical to it.  The tag appends frames=1 behind batch=1
// and prints the four digits in front, which describe no single frame, as 0: [norm_fast=0,norm_light=0,fast_x=0,fast_y=0,xcd=0,batch=1,frames=1] /
// [...,xcd=0,plain=1,batch=1,frames=1].  -1 (nothing enqueued) outside these bounds, -4 when the copy or the launch could not be enqueued
struct ScaledFrameLaunch { const void *src; size_t owidth, x, y, width, height; float black[3], white[3]; const uint8_t *cfa48_dev; };
constexpr size_t kScaledEachMax = 64;
size_t scaled_each_table_bytes(size_t n);
// sizes (optional, 2n entries: nwidth_i, nheight_i): the sized launch -- frame i has its own result size (nwidth and nheight are not read), its slice of
// nwidth_i * nheight_i * 4 floats begins where the earlier slices of the launch end (16-byte aligned whenever dst4 is), and every frame must select the
// general kernel for its own size.  The grid is laid over the widest and the tallest result; a block beyond its frame's columns leaves behind the filter
// barrier, one beyond its rows finds its loop empty.  Slice i is bit-identical to the single launch of frame i at its size.  The tag appends sized=1
// behind frames=1.  Null: the launch above
int launch_raw_scaled_demosaic_each(const ScaledFrameLaunch *frames, size_t n, bool src_is_u16, int layout, size_t nwidth, size_t nheight, float *dst4, void *table_dev,
                                    hipStream_t s, const size_t *sizes = nullptr);

void launch_tolab(const float *src4, size_t npix, const float *mul4, const float *cm12, const void *lab_pairs, float *dst3,
                  int num_cus, hipStream_t s);
void launch_basecurve(const float *src3, size_t npix, const SplineHost &sp, float *dst3, int num_cus, hipStream_t s);
void launch_fromlab(const float *src3, size_t npix, const float *m9, float *dst3, int num_cus, hipStream_t s);
void launch_gamma(const float *src, size_t n, const void *gam_pairs, float *dst, int num_cus, hipStream_t s);
template <typename T>   // float (OpBuffer) or uint8_t / uint16_t (the quantised image: same permutation, fewer bytes)
void launch_rotate(const T *src3, size_t owidth, size_t oheight, int64_t base_offset_px, int64_t x_step_px, int64_t y_step_px,
                   T *dst3, hipStream_t s);
void launch_output8(const float *src, size_t n, uint8_t *dst, int num_cus, hipStream_t s);
void launch_output16(const float *src, size_t n, uint16_t *dst, int num_cus, hipStream_t s);
// DynamicImage::to_rgb16 / to_rgb8 channel conversion of the raster fast path (image 0.24: c*257, (c+128)/257)
void launch_chan_8_to_16(const uint8_t *src, size_t n, uint16_t *dst, int num_cus, hipStream_t s);
void launch_chan_16_to_8(const uint16_t *src, size_t n, uint8_t *dst, int num_cus, hipStream_t s);

struct FusedLaunch {
  const void *src; void *dst;
  bool src_is_u16, src_aligned4;
  size_t width, height, owidth;
  size_t row_off, out_r0, out_r1;
  float black0, white0;
  int exact_norm;                // 1: gofloat's division must be a true division (see validate_cdiv)
  int fast_ok;                   // 1: matrix / multipliers / curve are finite and ordinary (fast point-wise form allowed)
  int xoff, yoff;
  const float *mul4, *cm12, *rgbm9;
  int has_curve, linear;
  const SplineHost *spline;
  int out_type;                  // 0 f32, 1 u8, 2 u16
  const void *lab_table, *gam_table;   // plain 8193-float tables (XYZ_LAB_TRANSFORM, SRGB gamma)
  const void *lab_pairs, *gam_pairs;   // the same two as 8192 x {v[i], v[i+1] - v[i]} (built at ipk_init): the LDS image of the pair form, copied without registers
  const void *gam_q8;                  // 8192 x {k, threshold}: OpGamma + output8bit as one step lookup (launch_build_q8), the 8-bit variants' LDS image
  int px_guard;                  // 0: u16 source whose levels and parameters the host found ordinary (kernel variant without per-pixel input guards)
  const float *gen_cells; int gen_pw, gen_ph, gen_check;   // generic-CFA mode (device cell records) or null: RGGB phase (xoff, yoff)
  int four = 0;                  // launch_fused_bayer only: 1 = the filter behind gen_cells has a fourth colour (RGBE ...): literal demosaic with a fourth bin and the
                                 // literal point-wise form for every pixel; whole frames, bands, batches (a launch per frame) and regions, ori == 0 (else -2)
  int num_cus;
  int schedule;                  // ipk_schedule (launch_fused_bayer, single frames on the static schedule only)
  TaskQueues *queues;            // the launching context's task queues (launch_fused_bayer only; may be null)
  int ori;                       // 0, or the ipk_orientation (Rotate90 / Rotate270) in whose rotated space the launch works: src is the permuted mosaic
  int roles[4];                  // ori != 0: demosaic role of the rotated-space pixel with parities (row & 1, col & 1), index 2 * row parity + col parity
  // launch_fused_bayer only: batch_n > 0 = that many frames of this shape and these parameters (host arrays of device pointers, src already
  // offset like `src`); one persistent launch per 64 frames where a batch variant of the kernel exists, one launch per frame otherwise
  int batch_n; const void *const *batch_src; void *const *batch_dst;
  // launch_fused_bayer only: win_c1 > 0 = a region launch (ipk_pipeline_run_region): the output columns [win_c0, win_c1) of the rows [out_r0, out_r1),
  // packed win_c1 - win_c0 pixels per row into dst.  Columns, like rows, are the cropped frame's: CFA phase and cells are not shifted
  size_t win_c0 = 0, win_c1 = 0;
};
// returns 0, -2 when f.ori != 0 and the parameters have no rotated-space variant or f.four is set without cells / with an orientation (nothing is launched), -4 when a launch could not be enqueued
int launch_fused_bayer(const FusedLaunch &f, hipStream_t s);
// gofloat + demosaic::full + transform_buffer(plan) + tolab..gamma (+ quantisation) as one launch (k_fused_resample): f.src = the cropped frame's first
// sample (pitch f.owidth), f.width x f.height the cropped frame, f.dst = nwidth * nheight * 3 samples of f.out_type; `lookups` = the device image of
// Cfa::demosaic_lookups of a three-colour filter.  Of f, the geometry, the levels, exact_norm and what launch_pointwise_chain reads are used.
// returns 0, or -4 when the launch could not be enqueued
// plan.axis (scaledown_plan): the kernel's axis-aligned stage 3, for scale_down_opbuf's transform
// win (optional): only the rows [row0, row0 + rows) and columns [col0, col0 + cols) of the nwidth x nheight result are computed, and f.dst holds exactly
// rows * cols * 3 packed samples (tiles are laid over the window from its origin; every pixel's bits are those of the whole-frame launch); it must be
// non-empty and lie inside the result.  Null: the whole frame, whose log entries are unchanged; a window launch adds the key win=1
// src_rgbe (f32 instantiations, general plans, window launches only: -1 otherwise, nothing launched): f.src is the demosaiced frame itself -- the dense
// 4-channel f32 buffer in front of OpRotateCrop, f.width x f.height pixels, f.owidth pixels per row, E = +0.0 in every pixel -- so the kernel loads each
// tile's box straight from it and skips its gofloat and demosaic stages; levels and lookups_dev are not read.  The launch adds the key rgbe=1
// rgbe_out (f.out_type 0 and plan.axis only, not with src_rgbe: -1 otherwise, nothing launched): the RGBE output mode -- f.dst holds the nwidth x nheight
// (or the window's) result of gofloat + demosaic::full + scale_down_opbuf as packed 4-channel f32 pixels, E = +0.0, what ipk_demosaic_run writes for such a
// frame; the point-wise parameters and tables of f are not read.  Whole frames and windows; the launch adds the key rgbe_out=1 behind axis=1
int launch_fused_resample(const FusedLaunch &f, const ResamplePlan &plan, size_t nwidth, size_t nheight, const uint32_t *lookups_dev, hipStream_t s,
                          const ResampleWindow *win = nullptr, int src_rgbe = 0, int rgbe_out = 0);
// rotate_buffer's permutation on a 1-channel image through an arbitrary source pitch / window (steps in source elements): |x_step| == 1 (flips, 180
// degrees) or |y_step| == 1 (the transposing orientations, oheight <= kRotate1MaxTransposedRows)
constexpr size_t kRotate1MaxTransposedRows = 65535u * 64u;
template <typename T>
void launch_rotate1(const T *src, size_t owidth, size_t oheight, int64_t base_offset, int64_t x_step, int64_t y_step, T *dst, hipStream_t s);
// Gather mode of the launches over a 4-channel f32 buffer (launch_pointwise_chain, launch_chain_quantised): the launch covers the npix = width * height
// packed pixels of a rectangle, and its pixel (col, row) is the 16-byte pixel base + col * x_step + row * y_step of f.src (steps in pixels, signed): a
// rectangle of a pitched buffer (x_step 1, y_step pitch), flipped (x_step -1 and / or y_step -pitch) or transposed (x_step +-pitch, y_step +-1) --
// rotate_buffer's walk as launch_rotate takes it, restricted to the rectangle, so OpTransform needs no pass of its own.  The caller keeps every such
// index inside the buffer; the kernels read each pixel's own 16 bytes and nothing else.  Null: the flat launch, whose log entries are unchanged.
// -1 (nothing launched) for width == 0, width >= 2^32 or npix no multiple of width
struct GatherSource { int64_t base, x_step, y_step; size_t width; };
// OpToLab..OpGamma in one pass over a 4-channel f32 buffer (src/dst, mul4, cm12, rgbm9, curve, linear, tables, fast_ok are read)
int launch_pointwise_chain(const FusedLaunch &f, size_t npix, hipStream_t s, const GatherSource *gather = nullptr);
int launch_tolab_fast(const FusedLaunch &f, size_t npix, hipStream_t s);   // OpToLab alone on the chain's fast form
// OpToLab..OpGamma + output8bit / output16bit in one pass over a 4-channel f32 buffer (f.out_type 1 / 2, f.gam_q8 set; npix >= 256): -1 otherwise
int launch_chain_quantised(const FusedLaunch &f, size_t npix, hipStream_t s, const GatherSource *gather = nullptr);
// The frame-table mode of the same launches (k_pointwise_chain_small for out_type 0 whatever the frame size, k_raster_chain<Rgbe32, 1 | 2> for 1 / 2):
// n <= kChainBatchMax buffers of npix pixels each, frame i with the src, dst, multipliers, matrix, curve, has_curve and fast_ok of frames[i] (a host array,
// read before the call returns; linear, rgbm9 and the tables must be the same in all of them).  The launcher writes one argument record per frame into
// table_dev -- chain_batch_table_bytes(n) bytes of device memory the caller keeps alive until the launch has run (the context's scratch pool) -- with a
// stream-ordered copy in front of the launch; the grid's y plane is the frame and chain_batch_blocks(...) blocks walk each frame, which reads its record
// instead of the kernel's arguments and is otherwise the single launch of that frame: bit-identical, the tail handling on the frame's own npix.  The log
// tags such launches [fast_ok=,batch=1]: fast_ok=1 when every frame's record allows the fast form, 0 when at least one frame takes the literal form
// throughout.  out_type 1 / 2 need npix >= 256.  -1 (nothing enqueued) outside these bounds, -4 when the copy or the launch could not be enqueued
// gathers (optional, n entries): frame i with gathers[i].width != 0 runs in gather mode on its own record -- its npix pixels are a gathers[i].width-wide
// rectangle read through gathers[i]'s base and steps (an orientation folded into the loads: npix % width == 0, else -1) -- and a launch with at least one
// such frame is tagged [fast_ok=,batch=1,orient=1].  Null, or every width 0: the launch and the tag above
constexpr size_t kChainBatchMax = 64;
size_t chain_batch_table_bytes(size_t n);
// blocks per frame: what a single launch of the frame gets (sixteen wave-chunks of 128 / 256 pixels per block), capped so that the launch's n planes
// together come to about one block per CU
inline unsigned chain_batch_blocks(size_t npix, int out_type, size_t n, unsigned cus) {
  const size_t chunks = out_type == 0 ? (npix + 127) / 128 : (npix + 255) / 256;
  return (unsigned)std::max<size_t>(1, std::min<size_t>((chunks + 15) / 16, (cus + n - 1) / n));
}
// npixs (optional, n entries): the sized launch -- frame i has npixs[i] pixels of its own (each within the bounds above: out_type 1 / 2 need 256), its record
// says so, and a block takes the count from its record where it otherwise takes the launch's: chunk count, clamped tail, last chunk and gather mode's last
// row are the frame's, bit-identical to a launch of that frame alone.  The grid's x is sized by the largest frame (npix is not read); blocks beyond a small
// frame's chunks find no work.  The tag appends sized=1: [fast_ok=,batch=1,sized=1] / [fast_ok=,batch=1,orient=1,sized=1].  Null: the launch above
int launch_chain_batch(const FusedLaunch *frames, size_t n, size_t npix, int out_type, void *table_dev, hipStream_t s, const GatherSource *gathers = nullptr,
                       const size_t *npixs = nullptr);
// run_other + OpToLab..OpGamma + quantisation in one pass over an RGB8 / RGB16 raster (npix >= 256; f.out_type selects the output)
// plain (optional; ipk_plain_to_srgb): the launch covers a width-pixel-wide rectangle of npix pixels whose first sample is f.src, inside an image whose rows
// are owidth pixels apart, and f.dst holds its npix * 3 packed samples.  levels: 0 the raster's samples; 1 a three-sample u16 raw, each channel
// min((s - black[c]) / (white[c] - black[c]), 1); 2 a monochrome u16 raw, ONE sample per pixel (owidth and width still count pixels) on black[0] /
// white[0], the pixel (v, v, v, +0.0).  width == owidth is the flat walk from f.src.  Both are runtime modes of the same six kernels; f32 raws have no
// instantiation to ride on and stay on the staged kernels.  -1 (nothing launched) for levels on a u8 source, npix no multiple of width, width > owidth
struct PlainSource { int levels; size_t owidth, width; float black[3], white[3]; };
int launch_raster_chain(const FusedLaunch &f, size_t npix, int src_is_u16, const void *gamma_reverse_pairs, hipStream_t s, const PlainSource *plain = nullptr);

// exhaustive on-device checks of the arithmetic shortcuts (see ipk_kernels.hip "Self-test kernels")
int launch_selftest_cdiv(float c, int variant, unsigned lo_bits, unsigned hi_bits, int include_special, void *out_dev, hipStream_t s);
void launch_copy_probe(const void *src, void *dst, size_t bytes, int num_cus, hipStream_t s);
void launch_mix_probe(const void *src, void *dst, size_t src_bytes, hipStream_t s);
void launch_clock_probe(void *out2_dev, unsigned long long spin_ticks, hipStream_t s);   // out2 = {shader-clock cycles, 100 MHz reference ticks} over the spin   // 1 : 3 read : write, dst holds 3 * src_bytes
int launch_selftest_spline3(const SplineHost &h, void *out_dev, hipStream_t s);
int launch_selftest_fract(void *out_dev, hipStream_t s);
int launch_selftest_clamp(void *out_dev, hipStream_t s);
int launch_selftest_quant8(void *out_dev, int variant, hipStream_t s);
int launch_selftest_quant16(void *out_dev, hipStream_t s);
void launch_build_q8(const void *gam_pairs, void *q8_out, hipStream_t s);        // q8_out: 8192 x 8 bytes of device memory
int launch_selftest_q8(const void *gam_pairs, const void *q8, void *out_dev, hipStream_t s);
// variants 0-2: the cube roots; 3-5: one Lab slot as pointwise4_fast evaluates it (3, 4) / the literal lab_lookup (5), on lab_pairs (the XYZ -> Lab pair table)
int launch_selftest_cbrt(const float *in, float *out, size_t n, int variant, const void *lab_pairs, hipStream_t s);

}  // namespace ipk
