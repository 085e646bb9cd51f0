/*
 * imagepipe_amd.h -- C ABI of the MI355X (gfx950) raw->sRGB hot path.
 *
 * This is the drop-in boundary: every entry point replaces one function of the reference
 * (pedrocr/imagepipe 0.5.0) behind its own `ImageOp::run` / `Pipeline::run` surface.  Each
 * declaration cites the reference interface (file:line, relative to the reference root) it
 * stands in for.  INTEGRATION.md shows the Rust `extern "C"` block and the `impl ImageOp`
 * wrappers a maintainer would add.
 *
 * Conventions
 *   - Plain pointers and sizes only.  An OpBuffer (src/buffer.rs:5-11) crosses the boundary as
 *     (data, width, height, colors[, monochrome]): f32, row-major, channel-interleaved,
 *     data[(row*width+col)*colors+c].
 *   - `ipk_*` entry points take DEVICE pointers and enqueue on `stream` (a hipStream_t, NULL =
 *     default stream).  They return as soon as the work is enqueued; buffers stay in HBM between
 *     stages.  Inputs are never modified (the reference's Arc<OpBuffer> inputs are immutable).
 *   - `ipk_host_*` entry points take HOST pointers, are synchronous at return (Rayon-join
 *     semantics of the reference ops) and do the H2D/D2H copies themselves.
 *   - Return value: IPK_OK (0), IPK_NOOP (1, "the op returned its input Arc unchanged": the
 *     output buffer was not written) or a negative ipk_status.  There is no CPU fallback: without a
 *     GPU every compute entry point fails with IPK_ERR_NO_DEVICE.
 *   - Results are bit-identical to the reference CPU path on the same host libm (the 13-bit
 *     lookup tables are built with the host's cbrtf/powf exactly as TransformLookup::new does).
 */
#ifndef IMAGEPIPE_AMD_H
#define IMAGEPIPE_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define IPK_API __attribute__((visibility("default")))

typedef enum {
  IPK_OK = 0,
  IPK_NOOP = 1,
  IPK_ERR_NOT_INIT = -1,
  IPK_ERR_INVALID = -2,
  IPK_ERR_HIP = -3,
  IPK_ERR_NO_DEVICE = -4,
  IPK_ERR_UNSUPPORTED = -5,
  IPK_ERR_NOMEM = -6
} ipk_status;

/* rawloader::Orientation (call sites src/ops/transform.rs:25-36,58-66,106) */
typedef enum {
  IPK_OR_NORMAL = 0, IPK_OR_HFLIP = 1, IPK_OR_ROT180 = 2, IPK_OR_VFLIP = 3, IPK_OR_TRANSPOSE = 4,
  IPK_OR_ROT90 = 5, IPK_OR_TRANSVERSE = 6, IPK_OR_ROT270 = 7, IPK_OR_UNKNOWN = 8
} ipk_orientation;

/* imagepipe::Rotation (src/ops/transform.rs:7-12) */
typedef enum { IPK_ROT_NORMAL = 0, IPK_ROT_90 = 1, IPK_ROT_180 = 2, IPK_ROT_270 = 3 } ipk_rotation;

/* element type of a raw source: RawImageData::Integer / ::Float (src/ops/gofloat.rs:94,132) and
 * the 8/16-bit raster of ImageSource::Other (src/ops/gofloat.rs:171-201) */
typedef enum { IPK_SRC_U16 = 0, IPK_SRC_F32 = 1, IPK_SRC_RGB8 = 2, IPK_SRC_RGB16 = 3 } ipk_src_type;

/* what Pipeline::run / output_8bit / output_16bit hand back (src/pipeline.rs:311,377,424) */
typedef enum { IPK_OUT_F32 = 0, IPK_OUT_U8 = 1, IPK_OUT_U16 = 2 } ipk_out_type;

/* ---------------------------------------------------------------------------------------- */
/* Context                                                                                  */
/* ---------------------------------------------------------------------------------------- */

/* Selects the HIP device, builds the three 8193-entry TransformLookup tables on the host with
 * libm (src/color_conversions.rs:87-100,119-141 -- the reference's lazy_static initialisers) and
 * uploads them.  Idempotent.  Fails with IPK_ERR_NO_DEVICE when no GPU is visible. */
IPK_API int ipk_init(int device);
IPK_API void ipk_shutdown(void);
IPK_API int ipk_is_initialized(void);
/* sizeof / offsetof of the descriptor structs as this library was built, so that a binding can check its own layout before the first call:
 * which = 0 ipk_fused_params, 1 ipk_pipeline_desc, 2 ipk_band, 3 ipk_stage_time; 16 / 17 offsetof(cfa_width) in the first two (the end of the
 * first published layout), 18 offsetof(ipk_fused_params, band_src_row0), 19 offsetof(ipk_pipeline_desc, use_fastpath), 20 / 21 offsetof(schedule) in
 * the first two (the end of the second layout); anything else 0.  No GPU needed. */
IPK_API size_t ipk_abi_sizeof(int which);
/* Human-readable description of the last failure on this thread (never NULL). */
IPK_API const char *ipk_last_error(void);
/* 1 when this host's libm cbrtf equals the device's cube-root routine (a port of glibc 2.35's, src/color_conversions.rs:103-104,123 call
 * the platform's) on the 65 536 arguments of (1, 8) ipk_init compares; 0 when it does not -- results are then still deterministic but not
 * bit-identical to a reference built on THIS host for Lab ratios above 1 (the count goes to *mismatches_of_65536, may be NULL);
 * -1 if the check could not run. */
IPK_API int ipk_host_libm_matches(size_t *mismatches_of_65536);
/* Number of compute units of the selected device (0 before ipk_init). */
IPK_API int ipk_device_cus(void);

/* ---- Several devices from ONE process --------------------------------------------------------------------------------------------
 * The reference is one process whose callers loop Pipeline::run over frames on Rayon threads (src/lib.rs:21-26, src/pipeline.rs:246-249); a
 * drop-in therefore reaches eight GPUs from one process, not through eight processes and a communicator.  A CONTEXT (ipk_ctx) is one device
 * binding plus everything the library keeps on that device (lookup tables, CFA tables, scratch pool, task queues, host-pointer lanes).
 * Every entry point of this header works on the calling thread's CURRENT context: ipk_init's context on every thread that has not chosen
 * another, else what ipk_ctx_make_current set (HIP's own per-thread current-device model; the call also binds the HIP device).  Several
 * contexts may share one device (two independent pipelines on one GPU); contexts share nothing mutable, so threads that use different
 * contexts never contend.  Device pointers belong to the device of the context that was current when they were allocated (ipk_malloc,
 * ipk_cache_new ...): pass them only to calls made under a context of that device. */
typedef struct ipk_ctx ipk_ctx;
/* A new context on `device`.  Does not change the calling thread's current context.  ipk_ctx_destroy releases its device memory (after
 * draining the device); a destroyed handle stays a valid argument and fails with IPK_ERR_NOT_INIT wherever it is used. */
IPK_API int ipk_ctx_create(int device, ipk_ctx **out);
IPK_API int ipk_ctx_destroy(ipk_ctx *ctx);
/* ctx becomes the calling thread's current context (NULL: back to the process default, ipk_init's). */
IPK_API int ipk_ctx_make_current(ipk_ctx *ctx);
IPK_API ipk_ctx *ipk_ctx_current(void);                 /* NULL before any context exists */
IPK_API int ipk_ctx_device(const ipk_ctx *ctx);         /* HIP device ordinal, -1 for a destroyed context */
/* The process's DEVICE SET: one context per entry of devices[0..n) (n = 0: one per visible device; the same ordinal may appear more than
 * once -- two contexts on one GPU).  The batch entry points below deal frame i to member i mod N.  A context ipk_init made serves as the
 * member for its device; without one, member 0 becomes the process default, so ipk_init_devices alone is a complete initialisation.
 * Calling it again replaces the set.  ipk_shutdown destroys every context of the process. */
IPK_API int ipk_init_devices(const int *devices, int n);
IPK_API int ipk_device_set_size(void);
IPK_API ipk_ctx *ipk_device_ctx(int index);             /* member `index` of the set (NULL outside it): make it current to allocate on its device */
/* The dealing rule as arithmetic (no GPU needed): of n_frames frames, set member `index` of n_devices gets frames
 * *first, *first + *stride, ... -- *count of them (frame i -> member i mod n_devices). */
IPK_API int ipk_deal_frames(size_t n_frames, int n_devices, int index, size_t *first, size_t *stride, size_t *count);

/* Device memory / stream helpers for callers that do not bring their own allocator. */
IPK_API int ipk_malloc(void **dptr, size_t bytes);
IPK_API int ipk_free(void *dptr);
IPK_API int ipk_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream);
IPK_API int ipk_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream);
IPK_API int ipk_stream_sync(void *stream);

/* Host copies of the lookup tables the device uses (8193 floats each), for fixture checks.
 * which: 0 XYZ_LAB_TRANSFORM, 1 SRGB_GAMMA_REVERSE, 2 SRGB_GAMMA_TRANSFORM
 * (src/color_conversions.rs:120,126,134).  Works without a GPU. */
IPK_API int ipk_lut_table(int which, float *out8193);

/* ---------------------------------------------------------------------------------------- */
/* Host-side size / parameter maths (no GPU needed)                                          */
/* ---------------------------------------------------------------------------------------- */

/* OpGoFloat::size_image (src/ops/gofloat.rs:74-82): out4 = x, y, width, height.
 * IPK_ERR_INVALID when owidth or oheight < 10 (the reference underflows/panics). */
IPK_API int ipk_size_image(size_t crop_top, size_t crop_right, size_t crop_bottom, size_t crop_left,
                           size_t owidth, size_t oheight, size_t *out4);
/* scaling::calculate_scaling_total (src/scaling.rs:8-23) */
IPK_API int ipk_calculate_scaling_total(size_t width, size_t height, size_t maxwidth, size_t maxheight,
                                        float *scale, size_t *nwidth, size_t *nheight);
/* OpToLab's normalize_wbs (src/ops/colorspaces.rs:12-27) */
IPK_API int ipk_normalize_wbs(const float *vals4, float *out4);
/* The colour constants of src/color_conversions.rs:1-18: which = 0 SRGB_D65_33 (9 floats), 1 XYZ_D65_33 (9; the f32
 * cofactor inverse, :20-39), 2 SRGB_D65_43 (12, [[f32;4];3]), 3 XYZ_D65_34 (12, [[f32;3];4]) */
IPK_API int ipk_const_matrix(int which, float *out12);
/* temp_to_xyz / xyz_to_temp (src/color_conversions.rs:277-310) and OpToLab::set_temp / get_temp
 * (src/ops/colorspaces.rs:59-85): xyz_to_cam12 = [[f32;3];4], cam_to_xyz12 = [[f32;4];3], row-major */
IPK_API int ipk_temp_to_xyz(float temp, float *out3);
IPK_API int ipk_xyz_to_temp(const float *xyz3, float *temp, float *tint);
IPK_API int ipk_tolab_set_temp(const float *xyz_to_cam12, float temp, float tint, float *wb4);
IPK_API int ipk_tolab_get_temp(const float *cam_to_xyz12, const float *wb4, float *temp, float *tint);
/* SplineFunc::new (src/ops/curves.rs:68-124): pts = npts (x,y) pairs; arrays sized >= npts+2.
 * Returns the knot count (>= 2) or a negative status. */
IPK_API int ipk_spline_new(const float *pts, int npts, float *px, float *py, float *c1s, float *c2s, float *c3s);
/* OpRotateCrop::calc_size (src/ops/rotatecrop.rs:111-163); params5 = crop_top, crop_right,
 * crop_bottom, crop_left, rotation */
IPK_API int ipk_rotatecrop_calc_size(const float *params5, float input_ratio, size_t width, size_t height,
                                     int reverse, size_t *nwidth, size_t *nheight);
/* rawloader CFA::shift as used by RawImage::cropped_cfa() (call site src/ops/demosaic.rs:13).
 * Pattern strings, here and in every entry point that takes one: the letters R G B E (M = G, Y = E) of one tile, row-major.  The tile's shape
 * is inferred from 4 (2x2), 36 (6x6) or 144 (12x12) letters, or STATED by the caller in front of them as "WxH:" (W columns, H rows, both
 * dividing 48 -- the reference tiles every pattern into 48x48): "2x8:RGBGRGBG..." -- the caller's CFA object knows its width and height
 * (src/ops/demosaic.rs:33).  16 letters WITHOUT a stated shape return IPK_ERR_UNSUPPORTED: rawloader's shape for them (8 wide x 2 high as
 * imagepipe's minscale arm suggests, or dcraw's 2 x 8) cannot be verified without its source, and a wrong guess would pass every test.
 * The shifted pattern comes back in the same notation (with the prefix unless the shape is one the letter count implies).
 * The result is at most strlen(pattern) characters, so `out` of strlen(pattern) + 1 bytes always suffices: the prefix comes back without leading
 * zeros ("02x08:" -> "2x8:"), is dropped where the letter count implies the shape ("2x2:RGGB" -> "RGGB"), and the empty pattern (no filter) shifts to
 * the empty pattern.  x and y may be negative: rawloader's shift takes usize and leaves that undefined; here a shift counts as a mathematical modulus
 * of the 48 x 48 tiling, so -1 is the same shift as width - 1 (or 47).  On failure `out` is not written. */
IPK_API int ipk_cfa_shift(const char *pattern, int x, int y, char *out /* >= strlen(pattern) + 1 bytes */);
/* Orientation::to_flips / from_flips (call sites src/ops/transform.rs:58-66,106);
 * flips3 = transpose, flip_x, flip_y */
IPK_API int ipk_orientation_to_flips(int orientation, int *flips3);
IPK_API int ipk_orientation_from_flips(int transpose, int flip_x, int flip_y);
/* The orientation OpTransform::run composes from (rotation, fliph, flipv) (src/ops/transform.rs:58-66) */
IPK_API int ipk_transform_orientation(int rotation, int fliph, int flipv);

/* ---------------------------------------------------------------------------------------- */
/* Stage kernels, device pointers (one per reference op)               */
/* ---------------------------------------------------------------------------------------- */

/* OpGoFloat::run_raw, CFA / cpp==1 branch (src/ops/gofloat.rs:122-130 u16, :158-166 f32):
 * dst[row][col] = min((src[owidth*(row+y)+x+col] - black0) / (white0-black0), 1), 1 channel. */
IPK_API int ipk_gofloat_cfa_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                float black0, float white0, float *dst, void *stream);
IPK_API int ipk_gofloat_cfa_f32(const float *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                float black0, float white0, float *dst, void *stream);
/* monochrome branch (src/ops/gofloat.rs:95-108, :133-144): 4-channel (v,v,v,0) */
IPK_API int ipk_gofloat_mono_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                 float black0, float white0, float *dst4, void *stream);
IPK_API int ipk_gofloat_mono_f32(const float *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                 float black0, float white0, float *dst4, void *stream);
/* cpp==3 branch (src/ops/gofloat.rs:109-120, :145-156): per-channel levels, 4-channel out.
 * black4/white4 are HOST arrays. */
IPK_API int ipk_gofloat_rgb_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                const float *black4, const float *white4, float *dst4, void *stream);
IPK_API int ipk_gofloat_rgb_f32(const float *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                const float *black4, const float *white4, float *dst4, void *stream);
/* OpGoFloat::run_other (src/ops/gofloat.rs:171-201): RGB8 via expand_srgb_gamma(input8bit),
 * RGB16 via input16bit; 4-channel out */
IPK_API int ipk_gofloat_other_u8(const uint8_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                 float *dst4, void *stream);
IPK_API int ipk_gofloat_other_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                  float *dst4, void *stream);

/* demosaic::full (src/ops/demosaic.rs:67-119).  `cfa` is the (cropped) pattern string OpDemosaic
 * holds (src/ops/demosaic.rs:4-22).  1-channel in, 4-channel RGBE out. */
IPK_API int ipk_demosaic_full(const float *src, size_t width, size_t height, const char *cfa, float *dst4, void *stream);
/* Row-band form for frames sharded across GPUs: `src` holds image rows [src_row0, src_row0+src_rows)
 * (the band plus its 1-row halos where they exist), output rows [out_row0, out_row0+out_rows) are
 * written to dst4 (row 0 of dst4 = image row out_row0).  Taps outside [0,img_height) are skipped
 * exactly as at the frame edge (src/ops/demosaic.rs:103-104). */
IPK_API int ipk_demosaic_full_band(const float *src, size_t width, size_t img_height, size_t src_row0, size_t src_rows,
                                   size_t out_row0, size_t out_rows, const char *cfa, float *dst4, void *stream);

/* scaling::transform_buffer<T> (src/scaling.rs:51-130): corner points are (x,y) isize pairs;
 * cfa NULL = None.  components <= 4. */
IPK_API int ipk_transform_buffer_f32(const float *src, size_t width, size_t height,
                                     int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                     size_t nwidth, size_t nheight, size_t components, const char *cfa, float *dst, void *stream);
IPK_API int ipk_transform_buffer_u8(const uint8_t *src, size_t width, size_t height,
                                    int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                    size_t nwidth, size_t nheight, size_t components, const char *cfa, uint8_t *dst, void *stream);
IPK_API int ipk_transform_buffer_u16(const uint16_t *src, size_t width, size_t height,
                                     int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                     size_t nwidth, size_t nheight, size_t components, const char *cfa, uint16_t *dst, void *stream);
/* scaling::scaled_demosaic (src/scaling.rs:132-145) and scale_down_opbuf (:147-160) */
IPK_API int ipk_scaled_demosaic(const float *src, size_t width, size_t height, const char *cfa,
                                size_t nwidth, size_t nheight, float *dst4, void *stream);
IPK_API int ipk_scale_down_opbuf(const float *src4, size_t width, size_t height,
                                 size_t nwidth, size_t nheight, float *dst4, void *stream);
/* OpGoFloat::run_raw (CFA branch, src/ops/gofloat.rs:122-130,158-166) followed by scaling::scaled_demosaic
 * (src/scaling.rs:132-145) in one pass over the raw sensor frame; src_type IPK_SRC_U16 or IPK_SRC_F32. */
IPK_API int ipk_raw_scaled_demosaic(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                    float black0, float white0, const char *cfa, size_t nwidth, size_t nheight, float *dst4, void *stream);
/* The raster-source counterpart: OpGoFloat::run_other (src/ops/gofloat.rs:171-201) + scaling::scale_down_opbuf (src/scaling.rs:147-160)
 * in one pass -- what OpGoFloat and OpDemosaic (demosaic.rs:44-46: a 4-channel buffer above the size limit) compute for an RGB8 /
 * RGB16 raster, without the full-size f32 buffer.  src: owidth-pitched RGB samples, window (x, y, width, height); dst4:
 * nwidth*nheight*4 f32 (E = 0). */
IPK_API int ipk_raster_scale_down(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                  size_t nwidth, size_t nheight, float *dst4, void *stream);
/* The window forms of the two: only the columns [wx, wx + ww) and rows [wy, wy + wh) of the nwidth x nheight result are computed, by the same kernel
 * the whole-frame form selects, its grid laid over the window instead of the frame.  Admission is exactly that of the whole-frame forms; an empty
 * window or one that leaves nwidth x nheight is IPK_ERR_INVALID (nothing written).  dst4 receives ww * wh * 4 packed f32, bit-identical to that
 * rectangle of the whole-frame call -- every pixel is computed from its absolute row and column, and the skips from the whole nwidth x nheight, so
 * nothing depends on the window -- and nothing outside those samples is written.  src is still the whole sensor frame's first sample, but the launch
 * reads only the window's footprint (ipk_scaled_window_footprint, offset by x, y). */
IPK_API int ipk_raw_scaled_demosaic_window(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                           float black0, float white0, const char *cfa, size_t nwidth, size_t nheight,
                                           size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream);
IPK_API int ipk_raster_scale_down_window(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                         size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream);
/* The counterpart for every source whose OpGoFloat writes a 4-channel buffer: OpGoFloat + scaling::scale_down_opbuf (OpDemosaic's branch for such a
 * buffer above the size limit, src/ops/demosaic.rs:44-46) in one pass.  kind is an ipk_plain_kind (declared with ipk_plain_to_srgb below; passed as
 * int): IPK_PLAIN_RGB (1), a three-sample raw (cpp == 3: linear DNG, sRAW, pixel-shift and HDR merges), min((s[c] - black4[c]) / (white4[c] - black4[c]), 1)
 * per channel (gofloat.rs:109-120); IPK_PLAIN_MONO (2), a monochrome raw, one sample per pixel, the same with black4[0] / white4[0] written to R, G and B
 * (gofloat.rs:95-108) -- both with src_type IPK_SRC_U16 or IPK_SRC_F32, true divisions, values below black left negative, degenerate levels (a range of
 * 0, an inverted range) accepted as the staged kernels accept them; IPK_PLAIN_RASTER (0) forwards to ipk_raster_scale_down(_window) (src_type
 * IPK_SRC_RGB8 / IPK_SRC_RGB16; black4 / white4 are ignored and may be NULL).  src: owidth-pitched pixels (1 or 3 samples each), window (x, y, width,
 * height); dst4 receives nwidth * nheight * 4 packed f32 (ww * wh * 4 for the window form), bit-identical to ipk_gofloat_mono_* / ipk_gofloat_rgb_*
 * followed by ipk_scale_down_opbuf, E = +0.0, and nothing else is written.  src and dst4 need element alignment only.  The raw kinds are run-time modes of
 * ipk_raw_scaled_demosaic's general kernel (one thread per output pixel, tap by tap), whatever the scale.  Admission, the window rules and the
 * IPK_ERR_INVALID cases are exactly those of ipk_raster_scale_down(_window); a window launch reads only ipk_scaled_window_footprint, offset by x, y. */
IPK_API int ipk_plain_scale_down(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                 const float *black4, const float *white4, size_t nwidth, size_t nheight, float *dst4, void *stream);
IPK_API int ipk_plain_scale_down_window(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                        const float *black4, const float *white4, size_t nwidth, size_t nheight,
                                        size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream);
/* The batch forms of ipk_raw_scaled_demosaic and ipk_plain_scale_down: n sensor frames of one shape and one set of parameters, srcs[i] frame i's first
 * sample (a host array of device pointers, read before the call returns).  dst4 receives n * nwidth * nheight * 4 packed f32, slice i bit-identical to
 * the whole-frame call on srcs[i], and nothing else is written.  Where the whole-frame call would select the general kernel (one thread per output
 * pixel: a skip above 7 or below 1, a frame under 8 samples wide, dst4 off a 16-byte boundary; every IPK_PLAIN_RGB / IPK_PLAIN_MONO launch) the frames
 * run as ONE launch per 64 of them, a frame per grid plane -- a thumbnail alone leaves most of the chip idle and a pixel's window cannot be split;
 * otherwise (the window-8 kernels; IPK_PLAIN_RASTER) as one launch per frame of the kernel the whole-frame call selects, into slice i: slices are
 * 16-byte aligned whenever dst4 is, so the selection is the same for every frame.  Admission and errors are those of the whole-frame forms; n = 0 is
 * IPK_OK with nothing enqueued, a null srcs[i] IPK_ERR_INVALID with nothing enqueued. */
IPK_API int ipk_raw_scaled_demosaic_batch(const void *const *srcs, size_t n, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                          float black0, float white0, const char *cfa, size_t nwidth, size_t nheight, float *dst4, void *stream);
IPK_API int ipk_plain_scale_down_batch(const void *const *srcs, size_t n, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width,
                                       size_t height, const float *black4, const float *white4, size_t nwidth, size_t nheight, float *dst4, void *stream);
/* one frame of ipk_scaled_demosaic_batch_each: the arguments of the whole-frame calls that may differ between the frames of one launch.
 * struct_size = sizeof(ipk_scaled_frame) (any other value is IPK_ERR_INVALID, as for ipk_chain_params) */
typedef struct { uint32_t struct_size;
                 size_t owidth, x, y, width, height;   /* pitch in pixels, window origin, window size */
                 float black4[4], white4[4];           /* mosaic: [0] only; IPK_PLAIN_RGB: [0..2]; IPK_PLAIN_MONO: [0] */
                 char cfa[160];                        /* mosaic: letters or "WxH:letters"; plain kinds: ignored */
               } ipk_scaled_frame;
/* ipk_raw_scaled_demosaic_batch / ipk_plain_scale_down_batch for frames that carry their own sensor settings: n sensor frames of one source type and one
 * kind (-1: mosaics, IPK_PLAIN_RGB, IPK_PLAIN_MONO) scaled to ONE nwidth x nheight, frame i with the pitch, window, levels and -- mosaics -- filter of
 * frames[i] (n ipk_scaled_frame; declared const void * for the reason given at ipk_pointwise_chain_out_batch).  dst4 receives n * nwidth * nheight * 4
 * packed f32, slice i bit-identical to ipk_raw_scaled_demosaic (mosaics) / ipk_plain_scale_down (the plain kinds) called with frame i's own arguments, and
 * nothing else is written; dst4 needs element alignment only.  One launch per 64 frames: the frame-table mode of the general kernel
 * k_raw_scaled_demosaic<T> -- a grid plane is a frame over the batch form's grid, and the block reads its frame's source, pitch, window, skips, levels and
 * filter table from a record in device memory where the other modes read the kernel's arguments; the result's size, the layout and T stay launch-wide.
 * Every tap, weight, order of accumulation and division is the single launch's.  The log tags such launches [norm_fast=0,norm_light=0,fast_x=0,fast_y=0,
 * xcd=0,batch=1,frames=1] (plain=1 / plain=3 in front of batch=1 for the plain kinds); the four digits describe no single frame and are printed as 0.
 * Admission: every frame must be one the general kernel takes for an aligned destination -- a skip (width - 1) / (nwidth - 1) or (height - 1) /
 * (nheight - 1) (in f32) above 7 or below 1, or a frame under 8 samples wide; every frame of the plain kinds -- because the window-8 kernels have no such
 * mode: another frame is IPK_ERR_UNSUPPORTED with its index in ipk_last_error, as is IPK_PLAIN_RASTER.  IPK_ERR_INVALID, the index named: a null srcs[i], a
 * wrong struct_size, a filter that does not parse, x + width > owidth, empty or oversized dimensions.  Everything is validated before anything is enqueued;
 * n = 0 is IPK_OK.  The host arrays are read before the call returns.  The table lives in the context's scratch pool and is uploaded with a stream-ordered
 * copy from pageable host memory in front of each launch: the call cannot be captured into a graph.  ipk_timing names each launch
 * "scaled_demosaic_batch_each". */
IPK_API int ipk_scaled_demosaic_batch_each(const void *const *srcs, const void *frames /* n ipk_scaled_frame */, size_t n, int src_type,
                                           int kind /* -1 mosaic, IPK_PLAIN_RGB, IPK_PLAIN_MONO */, size_t nwidth, size_t nheight, float *dst4,
                                           void *stream);
/* The same with a result size per frame: sizes holds 2n values, nwidth_i and nheight_i, and slice i is bit-identical to ipk_raw_scaled_demosaic /
 * ipk_plain_scale_down called with frame i's own arguments and size.  The slices are packed: slice i holds nwidth_i * nheight_i * 4 floats and begins at
 * the sum of the earlier slices, so every slice is 16-byte aligned whenever dst4 is; nothing else is written.  One launch per 64 frames: the SIZED
 * frame-table mode of k_raw_scaled_demosaic<T>, in which the record also brings the frame's result size and its slice's offset.  The grid is laid over
 * the widest and the tallest result of the launch; a block beyond its own frame's columns leaves behind the (launch-uniform) filter barrier, a frame's
 * row loop ends at its own height, and everything per pixel is the single launch's code on the frame's own values.  The tag appends sized=1:
 * [...,xcd=0,batch=1,frames=1,sized=1], plain=1 / plain=3 in front of batch=1 as before.  Admission and errors are ipk_scaled_demosaic_batch_each's, per
 * frame against its own size, the index named in ipk_last_error; an empty or oversized sizes entry is IPK_ERR_INVALID, the index named.  Everything is
 * validated before anything is enqueued; n = 0 is IPK_OK.  When all sizes are equal the call is ipk_scaled_demosaic_batch_each with that size (the same
 * launches and tags).  ipk_timing names each launch "scaled_demosaic_batch_sized". */
IPK_API int ipk_scaled_demosaic_batch_sized(const void *const *srcs, const void *frames /* n ipk_scaled_frame */,
                                            const size_t *sizes /* 2n: nwidth_i, nheight_i */, size_t n, int src_type,
                                            int kind /* -1 mosaic, IPK_PLAIN_RGB, IPK_PLAIN_MONO */, float *dst4, void *stream);
/* OpGoFloat::run_raw (CFA branch) followed by OpDemosaic::run's LAST branch -- demosaic::full, then scale_down_opbuf to nwidth x nheight
 * (src/ops/demosaic.rs:51-59: 1 < scale < minscale) -- in one launch over the raw sensor frame: ipk_raw_scaled_demosaic's sibling below minscale.  dst4
 * receives nwidth * nheight * 4 f32, bit for bit what ipk_gofloat_cfa_* -> ipk_demosaic_run write for such a frame (E = +0.0); the full-size 1- and
 * 4-channel buffers never exist.  The launch is k_fused_resample's axis-aligned walk (ipk_raw_to_srgb_scaled) in its RGBE output mode: the resampled
 * pixels are stored as they are, no point-wise chain, no quantiser.  src_type IPK_SRC_U16 or IPK_SRC_F32.  IPK_ERR_UNSUPPORTED with nothing enqueued for
 * a filter with a fourth colour and for geometry ipk_raw_to_srgb_scaled refuses (output sides >= 2, both skips at least 1 and below 3, sides below
 * 2^24).  The window form computes the columns [wx, wx + ww) and rows [wy, wy + wh) of that result alone, packed, bit-identical to the rectangle of the
 * whole-frame call; what it reads is ipk_transform_window_footprint of scale_down_opbuf's corners (0, 0), (width - 1, 0), (0, height - 1). */
IPK_API int ipk_raw_demosaic_scaled(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                    float black0, float white0, const char *cfa, size_t nwidth, size_t nheight, float *dst4, void *stream);
IPK_API int ipk_raw_demosaic_scaled_window(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                           float black0, float white0, const char *cfa, size_t nwidth, size_t nheight,
                                           size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream);
/* What such a window reads of the width x height cropped frame, host-only (no GPU needed): out4 = {x, y, w, h} in cropped-frame coordinates.  The
 * bounding box of the taps of the window's pixels (src/scaling.rs:84-87 with scale_down_buffer's corners (0, 0), (width - 1, 0), (0, height - 1), in
 * f32 as the kernels compute them), its columns widened by the 8-sample row loads of the window-8 kernels (a lane loads [lx, lx + 8) with
 * lx = min(from_x, width - 8); frames under 8 columns never take those kernels).  It therefore contains every read whichever kernel the launch
 * selects, lies inside the frame, is never empty, and exceeds the exact tap box by at most 7 columns per side and by no row.  IPK_ERR_INVALID for an
 * empty window or one that leaves nwidth x nheight. */
IPK_API int ipk_scaled_window_footprint(size_t width, size_t height, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh,
                                        size_t *out4);
/* OpDemosaic::run dispatch (src/ops/demosaic.rs:27-61).  colors = 1 or 4.  dst4 must hold
 * max(width*height, demosaic_width*demosaic_height)*4 floats.  IPK_NOOP = pass-through.
 * out_width / out_height receive the result size. */
IPK_API int ipk_demosaic_run(const float *src, size_t width, size_t height, size_t colors, const char *cfa,
                             size_t demosaic_width, size_t demosaic_height, float *dst4,
                             size_t *out_width, size_t *out_height, void *stream);

/* OpRotateCrop::run (src/ops/rotatecrop.rs:39-64).  Call with dst == NULL to query the output
 * size; IPK_NOOP when the op is a no-op or rejects its crops (returns the input). */
IPK_API int ipk_rotatecrop(const float *src, size_t width, size_t height, size_t colors, const float *params5,
                           float *dst, size_t *out_width, size_t *out_height, void *stream);

/* OpToLab::run (src/ops/colorspaces.rs:89-112) = camera_to_lab per pixel
 * (src/color_conversions.rs:42-55,156-169).  wb_coeffs[4] and cam_to_xyz_normalized[12]
 * ([[f32;4];3] row-major) are HOST arrays; normalize_wbs is applied here as in run(). 4ch -> 3ch. */
IPK_API int ipk_tolab(const float *src4, size_t width, size_t height, int monochrome,
                      const float *wb_coeffs, const float *cam_to_xyz_normalized, float *dst3, void *stream);
/* OpBaseCurve::run (src/ops/curves.rs:33-49): points = npoints HOST (x,y) pairs.  IPK_NOOP when
 * the op early-outs (no points and |exposure| < 0.001). */
IPK_API int ipk_basecurve(const float *src3, size_t width, size_t height, float exposure,
                          const float *points, int npoints, float *dst3, void *stream);
/* OpFromLab::run (src/ops/colorspaces.rs:127-137) = lab_to_rgb with XYZ_D65_33
 * (src/color_conversions.rs:58-65,172-191) */
IPK_API int ipk_fromlab(const float *src3, size_t width, size_t height, float *dst3, void *stream);
/* OpGamma::run (src/ops/gamma.rs:16-26); IPK_NOOP when linear */
IPK_API int ipk_gamma(const float *src, size_t width, size_t height, size_t colors, int linear, float *dst, void *stream);
/* rotate_buffer (src/ops/transform.rs:87-144), 3-channel */
IPK_API int ipk_rotate_buffer(const float *src3, size_t width, size_t height, int orientation,
                              float *dst3, size_t *out_width, size_t *out_height, void *stream);
/* rotate_buffer's permutation (src/ops/transform.rs:87-144) applied to an already quantised 3-channel image: output8bit /
 * output16bit (src/pipeline.rs:408-414,455-461) act per sample, so quantise-then-rotate equals the reference's rotate-then-
 * quantise bit for bit while the permutation moves 4x / 2x fewer bytes.  ipk_pipeline_run orders the two this way for the
 * 8- and 16-bit outputs of non-Normal orientations. */
IPK_API int ipk_rotate_image_u8(const uint8_t *src3, size_t width, size_t height, int orientation, uint8_t *dst3,
                                size_t *out_width, size_t *out_height, void *stream);
IPK_API int ipk_rotate_image_u16(const uint16_t *src3, size_t width, size_t height, int orientation, uint16_t *dst3,
                                 size_t *out_width, size_t *out_height, void *stream);
/* OpTransform::run (src/ops/transform.rs:56-73); IPK_NOOP for Normal/Unknown */
IPK_API int ipk_transform(const float *src3, size_t width, size_t height, int rotation, int fliph, int flipv,
                          float *dst3, size_t *out_width, size_t *out_height, void *stream);
/* the quantise loops of Pipeline::output_8bit/16bit (src/pipeline.rs:408-414, :455-461;
 * output8bit/output16bit src/color_conversions.rs:323-330) */
IPK_API int ipk_output8bit(const float *src, size_t n, uint8_t *dst, void *stream);
IPK_API int ipk_output16bit(const float *src, size_t n, uint16_t *dst, void *stream);

/* ---------------------------------------------------------------------------------------- */
/* Fused raw -> sRGB (gofloat + demosaic::full + tolab + basecurve + fromlab + gamma [+ quantise]) */
/* ---------------------------------------------------------------------------------------- */

/* How a fused launch deals a single frame's row segments to its waves.  The reference's Rayon loops balance themselves by work stealing
 * (src/ops/demosaic.rs:93-116: one task per output row); a persistent GPU launch fixes each wave's rows up front, so a frame whose regions cost
 * differently -- blown highlights take the cube-root path of XYZ_LAB_TRANSFORM.lookup, src/color_conversions.rs:102-104 -- finishes on its
 * slowest waves.  IPK_SCHED_SPLIT gives every wave two pieces half a frame apart instead of one contiguous piece: a blown region is shared by
 * twice as many waves (photo-like 100 MP frame: -2...-3.4 %), at one more three-row priming per wave (uniform frames: +1...+5 %).  A caller
 * that knows its frames (a shoot with clipped skies) sets it; AUTO is the contiguous schedule.  Batches and frames above ~130 MP draw their
 * tasks from a queue and ignore the field.  Results are bit-identical under every schedule. */
typedef enum { IPK_SCHED_AUTO = 0, IPK_SCHED_SPLIT = 1 } ipk_schedule;

/* Everything the ops between OpGoFloat and OpGamma read, for a CFA raw source at full scale with
 * a no-op rotatecrop (the default Pipeline::run on a RawImage). */
typedef struct {
  uint32_t struct_size;            /* sizeof(ipk_fused_params) as the CALLER was compiled (IPK_FUSED_PARAMS_INIT sets it): see "Descriptor versioning" below */
  int src_type;                    /* IPK_SRC_U16 or IPK_SRC_F32 */
  size_t owidth;                   /* RawImage.width: row pitch of src in elements */
  size_t x, y, width, height;      /* OpGoFloat::size_image result */
  float black0, white0;            /* blacklevels[0], whitelevels[0] (gofloat.rs:126) */
  char cfa[160];                   /* cropped CFA pattern (OpDemosaic.cfa): letters, or "WxH:letters" (see ipk_cfa_shift) */
  float wb_coeffs[4];              /* OpToLab.wb_coeffs (normalised again inside, colorspaces.rs:100) */
  float cam_to_xyz_normalized[12]; /* OpToLab.cam_to_xyz_normalized, [[f32;4];3] row-major */
  float exposure;                  /* OpBaseCurve.exposure */
  int npoints;                     /* OpBaseCurve.points */
  float points[128];
  int linear;                      /* PipelineSettings.linear: skip OpGamma */
  int out_type;                    /* IPK_OUT_F32 (Pipeline::run), IPK_OUT_U8 / IPK_OUT_U16 (+ output8bit/16bit) */
  /* row band (multi-GPU sharding of one frame); all zero = whole frame.  `src` then points at
   * image row band_src_row0 (in cropped coordinates, i.e. row y+band_src_row0 of the sensor), and
   * only output rows [band_out_row0, band_out_row0+band_out_rows) are produced into dst. */
  size_t band_src_row0, band_src_rows, band_out_row0, band_out_rows;
  /* Descriptor versioning.  Fields added after a struct was first published are APPENDED, never inserted, and the leading struct_size says how many
   * bytes of it the caller's object really has: the library copies exactly that many into a zeroed struct of its own and never reads past them, so a
   * caller compiled against an older header (an object that ends in front of the fields below) keeps working with the defaults of the fields it
   * does not know -- 0, 0 below: "take the shape from the string".  A struct_size smaller than the first published layout (ipk_abi_sizeof(16) / (17):
   * everything in front of cfa_width), or LARGER than this library's struct (a caller built against a newer header: fields this library would
   * silently ignore), fails with IPK_ERR_INVALID; so does 0 (an object that was never initialised).  ipk_abi_sizeof(0) / (1) still let a binding
   * compare whole layouts at start-up (tests/test_rust_binding.py checks the generated Rust layout the same way). */
  int cfa_width, cfa_height;       /* the tile's shape as the caller's CFA object has it (cfa.width / cfa.height, src/ops/demosaic.rs:33); 0, 0 = take
                                      it from the string (a "WxH:" prefix, or the letter count 4 / 36 / 144).  16 letters need one of the two. */
  /* third layout */
  int schedule;                    /* ipk_schedule: how the launch shares a frame's rows out among the waves (results do not depend on it) */
  int four_colour;                 /* 0 (the default, and what every earlier caller wrote into this formerly reserved field): a filter with a fourth colour
                                      (RGBE ...) is refused with IPK_ERR_UNSUPPORTED; 1: ipk_raw_to_srgb (bands included), ipk_raw_to_srgb_batch and
                                      ipk_host_raw_to_srgb take it -- one launch, the fourth colour an ordinary lane of demosaic::full and camera_to_lab; other
                                      values are IPK_ERR_INVALID.  Three-colour filters run the same either way.  No layout change. */
} ipk_fused_params;
#define IPK_FUSED_PARAMS_INIT {(uint32_t)sizeof(ipk_fused_params)}      /* ipk_fused_params p = IPK_FUSED_PARAMS_INIT;  (everything else zero) */

/* src: device pointer to the sensor data (element (0,0) of the uncropped frame, or of the band's
 * first source row); dst: device pointer to width*rows*3 elements of out_type.
 * src and dst need only the alignment of their element type (u16 samples 2 bytes, f32 4, u8 results 1): a frame packed behind another in one
 * allocation, a u16 frame 2 bytes off a dword boundary or an f32 buffer 4 bytes off a 16-byte boundary give the same bits, and nothing outside
 * dst's width*rows*3 elements is written.  The same holds for the batch, oriented, resampled and scaled forms below, for ipk_pipeline_run and
 * ipk_pipeline_run_region, ipk_demosaic_full and ipk_stream_probe (tests/test_gpu_buffer_bounds.py).
 * Any colour filter without a fourth colour is accepted (the four RGGB phases, X-Trans, 12x12, 16 letters with a stated shape ...; pattern strings: see ipk_cfa_shift); fails with
 * IPK_ERR_UNSUPPORTED for RGBE-style filters (callers then run the staged ops) unless p->four_colour is 1: then such a filter (RGBE, ERBG, 16 letters
 * with a stated shape ...) runs as one launch too, bit-identical to the staged ops -- every pixel takes the literal demosaic with a fourth bin and the
 * literal point-wise form, which keeps the e * cam_to_xyz[i][3] terms (src/ops/demosaic.rs:77-114, src/color_conversions.rs:42-55).  The flag is
 * honoured here, by ipk_raw_to_srgb_batch (one launch per frame, as for every generic filter) and by ipk_host_raw_to_srgb; ipk_raw_to_srgb_oriented,
 * _resampled, _scaled and ipk_stream_probe keep refusing a fourth colour whatever it says, and a pattern with an unknown letter stays refused. */
IPK_API int ipk_raw_to_srgb(const ipk_fused_params *p, const void *src, void *dst, void *stream);
/* n frames of ONE shape and ONE parameter set (a caller looping Pipeline::run over a shoot, src/pipeline.rs:246-249: frames are independent;
 * BASELINE.json configs[3]): srcs[i] -> dsts[i], host arrays of device pointers, whole frames only.  Where the kernel has a batch variant
 * (Bayer filter, ordinary levels / multipliers / matrix, a 2- or 3-knot curve, width >= 256; any frame size: eight 100 MP frames in one launch run at 0.51 ms each) the frames run as ONE persistent launch per 64
 * -- the lookup tables are staged once per CU instead of once per frame and CU, and no CU idles between frames; otherwise one launch per
 * frame.  Either way every dsts[i] is bit-identical to ipk_raw_to_srgb(p, srcs[i], dsts[i]). */
IPK_API int ipk_raw_to_srgb_batch(const ipk_fused_params *p, const void *const *srcs, void *const *dsts, size_t n, void *stream);
/* ipk_raw_to_srgb followed by OpTransform (src/ops/transform.rs:56-73) for the given rawloader orientation, without a pass over the
 * 3-channel result: the 1-channel mosaic is permuted instead (rotate_buffer's index walk, :102-128) and the kernel works in
 * rotated space, adding the demosaic taps in the reference's order of the ORIGINAL orientation.  Whole frames (no band) of a
 * three-colour filter whose rotated width is at least 256 pixels, with the common parameter set (finite ordinary multipliers and
 * matrix, a 2- or 3-knot curve, validated levels); for the transposing orientations (Transpose, Rotate90, Transverse, Rotate270) the frame is
 * at most 65535 * 64 = 4 194 240 columns wide (the mosaic's transposing permutation covers 64 output rows per grid row).  dst receives out_width x out_height x 3 samples of p->out_type.
 * Normal / Unknown: ipk_raw_to_srgb.  Returns IPK_ERR_UNSUPPORTED (nothing written) otherwise: the caller then uses
 * ipk_raw_to_srgb + ipk_rotate_buffer / ipk_rotate_image_*, as ipk_pipeline_run does. */
IPK_API int ipk_raw_to_srgb_oriented(const ipk_fused_params *p, const void *src, int orientation, void *dst,
                                     size_t *out_width, size_t *out_height, void *stream);

/* ipk_raw_to_srgb with OpBuffer::transform(topleft, topright, bottomleft, nwidth, nheight) between demosaic::full and OpToLab -- what Pipeline::run
 * computes for a CFA mosaic whose OpRotateCrop is active (src/ops/rotatecrop.rs:39-64 hands its three corner points to transform_buffer,
 * src/scaling.rs:51-130) -- as ONE launch: the normalised mosaic, the demosaiced frame and the resampled frame never exist in memory.  The corner
 * points mean what they mean for ipk_transform_buffer_f32 (coordinates in the p->width x p->height cropped frame; they may lie outside it, windows
 * are clamped as the reference clamps them); dst receives nwidth * nheight * 3 samples of p->out_type, bit-identical to ipk_gofloat_cfa_* +
 * ipk_demosaic_full + ipk_transform_buffer_f32 (4 components) + ipk_pointwise_chain(_out).  Whole frames (no band) of a three-colour filter.
 * IPK_ERR_UNSUPPORTED (nothing written) for transforms the launch does not take: nwidth or nheight below 2, a skip that is not finite,
 * |skip_x_x| + |skip_y_x| >= 2 or |skip_x_y| + |skip_y_y| >= 2 (windows larger than 3x3: scaling down is OpDemosaic's business), frame sides
 * of 2^24 or more.  A zero skip is taken: its division by zero is the reference's and comes out the same. */
IPK_API int ipk_raw_to_srgb_resampled(const ipk_fused_params *p, const void *src, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                                      int64_t blx, int64_t bly, size_t nwidth, size_t nheight, void *dst, void *stream);
/* ipk_raw_to_srgb with scale_down_opbuf(nwidth, nheight) between demosaic::full and OpToLab -- what Pipeline::run computes for a CFA mosaic under a size
 * limit that is close to its full size: OpDemosaic::run's last branch, `full` followed by scale_down_opbuf for 1 < scale < minscale
 * (src/ops/demosaic.rs:51-59; scale_down_opbuf is transform_buffer with the corners (0, 0), (width - 1, 0), (0, height - 1), src/scaling.rs:35-48 and
 * :51-130) -- as ONE launch, the axis-aligned mode of ipk_raw_to_srgb_resampled's kernel.  dst receives nwidth * nheight * 3 samples of p->out_type,
 * bit-identical to ipk_gofloat_cfa_* + ipk_demosaic_full + ipk_scale_down_opbuf + ipk_pointwise_chain(_out).  Whole frames (no band) of a
 * three-colour filter.  IPK_ERR_UNSUPPORTED (nothing written) for sizes the launch does not take: nwidth or nheight below 2, a skip
 * (p->width - 1) / (nwidth - 1) or (p->height - 1) / (nheight - 1) (in f32, src/scaling.rs:69-72) that is not finite, below 1, or 3 or more (windows
 * larger than 4x4: ipk_raw_scaled_demosaic's range for most filters), frame sides of 2^24 or more. */
IPK_API int ipk_raw_to_srgb_scaled(const ipk_fused_params *p, const void *src, size_t nwidth, size_t nheight, void *dst, void *stream);
/* The window forms of the two: only the columns [wx, wx + ww) and rows [wy, wy + wh) of the nwidth x nheight result are computed, in the same one
 * launch laid over the window instead of the frame.  Admission is exactly that of the whole-frame forms; an empty window or one that leaves
 * nwidth x nheight is IPK_ERR_INVALID (nothing written).  dst receives ww * wh * 3 packed samples of p->out_type, bit-identical to that rectangle of
 * the whole-frame call -- every pixel is computed from its absolute position, so nothing depends on the window -- and nothing outside them is written.
 * src is still the whole sensor frame's first sample, but the launch reads only the window's footprint (ipk_transform_window_footprint, offset by
 * p->x, p->y).  src and dst need only element alignment, as for the whole-frame forms. */
IPK_API int ipk_raw_to_srgb_resampled_window(const ipk_fused_params *p, const void *src, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                                             int64_t blx, int64_t bly, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh,
                                             void *dst, void *stream);
IPK_API int ipk_raw_to_srgb_scaled_window(const ipk_fused_params *p, const void *src, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww,
                                          size_t wh, void *dst, void *stream);
/* What such a window reads of the width x height cropped frame, host-only (no GPU needed): out4 = {x, y, w, h} in cropped-frame coordinates, the
 * bounding box of the source windows (src/scaling.rs:84-87) of the window's four corner pixels -- the expressions are monotone in row and in col, so
 * the extremes sit there -- plus demosaic::full's one-pixel halo, clipped to the frame.  w = h = 0 when no pixel of the window has a tap (the launch
 * then reads nothing).  It contains everything the launch reads and exceeds the exact box by at most 2 pixels per side.  The corners are those of
 * ipk_raw_to_srgb_resampled; for the scaled form they are (0, 0), (width - 1, 0), (0, height - 1).  IPK_ERR_INVALID for an empty window or one that
 * leaves nwidth x nheight, IPK_ERR_UNSUPPORTED for a transform ipk_raw_to_srgb_resampled refuses by its skips or sizes. */
IPK_API int ipk_transform_window_footprint(size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                           size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, size_t *out4);

/* OpToLab::run + OpBaseCurve::run + OpFromLab::run + OpGamma::run (src/ops/colorspaces.rs:89-112, src/ops/curves.rs:33-49,
 * src/ops/colorspaces.rs:127-137, src/ops/gamma.rs:16-26) in one pass over a 4-channel OpBuffer: the ops Pipeline::run applies
 * between rotatecrop and transform, for callers that do not need the three intermediate buffers (cache == None).
 * Arguments as for the four stage entry points; bit-identical to running them one after the other. */
IPK_API int ipk_pointwise_chain(const float *src4, size_t width, size_t height, int monochrome, const float *wb_coeffs,
                                const float *cam_to_xyz_normalized, float exposure, const float *points, int npoints, int linear,
                                float *dst3, void *stream);
/* The same followed by the quantise loop of output_8bit / output_16bit (src/pipeline.rs:408-414, :455-461) in ONE pass: dst receives width*height*3 samples
 * of out_type (IPK_OUT_U8 / IPK_OUT_U16; IPK_OUT_F32 = ipk_pointwise_chain).  What ipk_pipeline_run uses behind a staged demosaic when the caller wants
 * 8 or 16 bits and OpTransform is a no-op (a preview under a size limit, X-Trans, four-colour filters): bit-identical to ipk_pointwise_chain followed by
 * ipk_output8bit / ipk_output16bit.  At least 256 pixels (IPK_ERR_UNSUPPORTED below). */
IPK_API int ipk_pointwise_chain_out(const float *src4, size_t width, size_t height, int monochrome, const float *wb_coeffs,
                                    const float *cam_to_xyz_normalized, float exposure, const float *points, int npoints, int linear,
                                    int out_type, void *dst, void *stream);
/* the fields of a descriptor OpToLab and OpBaseCurve read (src/ops/colorspaces.rs:89-112, src/ops/curves.rs:33-49): what may differ between the frames of
 * one launch.  struct_size = sizeof(ipk_chain_params) (any other value is IPK_ERR_INVALID) */
typedef struct { uint32_t struct_size; float wb_coeffs[4]; float cam_to_xyz_normalized[12];
                 float exposure; int npoints; float points[128]; } ipk_chain_params;
/* ipk_pointwise_chain_out for n same-sized 4-channel buffers, each with its own parameters and its own destination: frame i is bit-identical to
 * ipk_pointwise_chain_out(srcs4[i], width, height, monochrome, params[i]..., linear, out_type, dsts[i], stream), and nothing else is written.  One launch
 * per 64 frames (the call loops for larger n): a launch-uniform mode of the single form's kernels -- k_pointwise_chain_small for IPK_OUT_F32 at every frame
 * size (frames are the parallelism), k_raster_chain<Rgbe32, 1 | 2> for IPK_OUT_U8 / IPK_OUT_U16 -- in which a grid plane is a frame and the block reads
 * its frame's source, destination, multipliers, matrix, curve, has_curve and fast_ok from a table in device memory instead of from the kernel's
 * arguments; linear and the lookup tables stay launch-wide, the tail handling is each frame's own.  Every params[i] goes through the single form's host
 * preparation (normalize_wbs, the spline, has_curve, fast_ok: all per frame) BEFORE anything is enqueued: an invalid or degenerate curve, a null
 * srcs4[i] / dsts[i] or a misaligned pointer fails the whole call with IPK_ERR_INVALID, names the index in ipk_last_error and writes nothing.
 * IPK_OUT_U8 / IPK_OUT_U16 need at least 256 pixels PER FRAME (IPK_ERR_UNSUPPORTED below that, like the single form); IPK_OUT_F32 takes any size >= 1.
 * srcs4[i] needs 16-byte alignment, dsts[i] only its element's.  n = 0 is IPK_OK.  The host arrays are read before the call returns.  The table lives in
 * the context's scratch pool and is uploaded with a stream-ordered copy from pageable host memory in front of each launch: the host may wait there for
 * the stream's earlier work, and the call cannot be captured into a graph.  monochrome = 1: params' wb_coeffs and matrix are not read, as in the single
 * form.  ipk_timing names each launch "pointwise_chain_out_batch".  params points to n ipk_chain_params; it is declared const void * because the type
 * table the generated Rust binding is checked against (tests/test_rust_binding.py) is closed: the C++ mirror takes the typed pointer. */
IPK_API int ipk_pointwise_chain_out_batch(const float *const *srcs4, size_t width, size_t height, int monochrome,
                                          const void *params /* n ipk_chain_params */, size_t n, int linear,
                                          int out_type, void *const *dsts, void *stream);
/* The same with an orientation per frame: frame i is bit-identical to ipk_pointwise_chain_out (for IPK_OUT_F32, ipk_pointwise_chain) of srcs4[i] with
 * params[i], followed by ipk_rotate_image_u8 / _u16 / ipk_rotate_buffer with orientations[i].  dsts[i] receives width*height*3 samples -- a height-wide
 * image for the four transposing orientations (Transpose, Rotate90, Transverse, Rotate270) -- and nothing else is written.  IPK_OR_UNKNOWN is Normal.
 * orientations == NULL, or every entry Normal or Unknown, is exactly ipk_pointwise_chain_out_batch: the same launches with the same [fast_ok=,batch=1]
 * tags.  Otherwise the record of an oriented frame carries the gather mode of the chain kernels (the whole-frame case of the mapping
 * ipk_pipeline_region_gather reports: the output's width, and base, x_step, y_step into the source), so OpTransform's permutation is folded into the
 * frame's loads; a launch with at least one such record is tagged [fast_ok=,batch=1,orient=1].  All eight orientations and all three outputs take that
 * mode: a flip keeps a lane's pixels consecutive in memory, forwards or backwards, and a transposing orientation reads one source pixel per lane a source
 * row apart.  There is no tiled walk for the transposing orientations, so the host predicate "tile or gather" is constantly gather: a transposed tile walk
 * through the wave's stage buffer (32 x 8 output pixels per wave, loaded along source rows, tag orient=2) was built for k_raster_chain<Rgbe32, 1 | 2>,
 * bit-exact at 128 / 126 VGPRs without scratch, measured against this form and deleted (IPK_FUSED_BATCH_ORIENTED has the figures).  Validation is that of
 * ipk_pointwise_chain_out_batch, before anything is enqueued; an orientation outside 0..8 is IPK_ERR_INVALID with the index in ipk_last_error.  The floor
 * of 256 pixels per frame for 8 and 16 bits and the 64 frames per launch stay.  ipk_timing names each launch "pointwise_chain_out_batch_oriented". */
IPK_API int ipk_pointwise_chain_out_batch_oriented(const float *const *srcs4, size_t width, size_t height, int monochrome,
                                                   const void *params /* n ipk_chain_params */, const int *orientations /* n ipk_orientation, or NULL */,
                                                   size_t n, int linear, int out_type, void *const *dsts, void *stream);
/* The same with a size per frame: sizes holds 2n values, width_i and height_i, and frame i is what ipk_pointwise_chain_out_batch_oriented gives a
 * one-frame call of that size (orientations may be NULL).  One launch per 64 frames: in the frame-table mode a record may bring its frame's own pixel
 * count, and the block then takes the chunk count, the clamped tail lanes, "the last chunk ends at the last pixel" and gather mode's last row of that
 * count instead of the launch's; the grid is sized by the largest frame of the launch, and a block beyond a small frame's chunks finds no work.  The
 * tag appends sized=1: [fast_ok=,batch=1,sized=1], orient=1 in front of sized=1 where a record gathers.  Validation is that call's, per frame: the
 * floor of 256 pixels for 8 and 16 bits holds for EVERY frame (IPK_ERR_UNSUPPORTED), an empty or oversized sizes entry is IPK_ERR_INVALID, the index
 * named in ipk_last_error, everything before anything is enqueued.  When all sizes are equal it is exactly that call: the same launches with the same
 * tags.  ipk_timing names each launch "pointwise_chain_out_batch_sized". */
IPK_API int ipk_pointwise_chain_out_batch_sized(const float *const *srcs4, const size_t *sizes /* 2n: width_i, height_i */, int monochrome,
                                                const void *params /* n ipk_chain_params */, const int *orientations /* n ipk_orientation, or NULL */,
                                                size_t n, int linear, int out_type, void *const *dsts, void *stream);
/* The raster-source counterpart of ipk_raw_to_srgb: OpGoFloat::run_other (src/ops/gofloat.rs:171-201; RGB8 through
 * expand_srgb_gamma(input8bit(v)), RGB16 through input16bit(v)) + OpToLab + OpBaseCurve + OpFromLab + OpGamma (+ output8bit /
 * output16bit, src/pipeline.rs:408-414,455-461) in one pass from the width*height*3 source samples to width*height*3 outputs of
 * out_type.  What Pipeline::run / output_8bit / output_16bit compute for an ImageSource::Other whose ops are not the defaults
 * (the default ops take the integer fast path) when demosaic, rotatecrop and transform are no-ops; ipk_pipeline_run uses it
 * then (allow_fused).  At least 256 pixels. */
IPK_API int ipk_raster_to_srgb(const void *src, int src_type, size_t width, size_t height, const float *wb_coeffs,
                               const float *cam_to_xyz_normalized, float exposure, const float *points, int npoints, int linear,
                               int out_type, void *dst, void *stream);
/* The same launch for every source whose OpDemosaic is a pass-through (a 4-channel buffer, src/ops/demosaic.rs:41-43), over a rectangle of it.
 * kind says how OpGoFloat reads a pixel: IPK_PLAIN_RASTER, run_other on an RGB8 / RGB16 raster as above (black4 / white4 are ignored and may be NULL);
 * IPK_PLAIN_RGB, a three-sample raw (cpp == 3: linear DNG, sRAW), min((s[c] - black4[c]) / (white4[c] - black4[c]), 1) per channel; IPK_PLAIN_MONO, a
 * monochrome raw (cpp == 1 without a filter), ONE sample per pixel on black4[0] / white4[0], the pixel (v, v, v) and the point-wise parameters those
 * of a monochrome buffer (the sRGB matrix, unit multipliers: wb_coeffs and cam_to_xyz_normalized must be given but are not read).  The divisions are
 * true divisions, values below black stay negative and the fourth channel is +0.0: bit for bit what ipk_gofloat_rgb_u16 / ipk_gofloat_mono_u16
 * followed by ipk_pointwise_chain (+ ipk_output8bit / 16bit) give.  RGB and MONO take IPK_SRC_U16 sources only.  IPK_SRC_F32 is refused with
 * IPK_ERR_UNSUPPORTED and nothing written: the launch is a runtime mode of the RGB8 / RGB16 raster kernels (k_raster_chain<uint8_t | uint16_t>),
 * there is no f32 instantiation for it to ride on, and f32 mono / three-sample raws therefore stay on the staged ops, bit for bit as they were.
 * The source is owidth pixels wide (3 samples per pixel, 1 for MONO); the launch covers columns [x, x + width) and rows [y, y + height) of it
 * (x + width <= owidth; the caller vouches for the rows) and reads no sample outside that rectangle; dst receives width*height*3 packed samples of
 * out_type and nothing else is written.  src and dst need the alignment of their element type only.  At least 256 pixels in the rectangle
 * (IPK_ERR_UNSUPPORTED below, as ipk_raster_to_srgb).  A rectangle as wide as the source (any y) runs exactly ipk_raster_to_srgb's flat walk. */
typedef enum { IPK_PLAIN_RASTER = 0, IPK_PLAIN_RGB = 1, IPK_PLAIN_MONO = 2 } ipk_plain_kind;
IPK_API int ipk_plain_to_srgb(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                              const float *black4, const float *white4, const float *wb_coeffs, const float *cam_to_xyz_normalized,
                              float exposure, const float *points, int npoints, int linear, int out_type, void *dst, void *stream);

/* ---------------------------------------------------------------------------------------- */
/* Pipeline driver: Pipeline::run / output_8bit / output_16bit for one source                */
/* (src/pipeline.rs:311-375, :377-422, :424-469), cache == None                              */
/* ---------------------------------------------------------------------------------------- */

/* The fields of ImageSource + PipelineOps + PipelineSettings the hot path reads. */
typedef struct {
  uint32_t struct_size;            /* sizeof(ipk_pipeline_desc) as the caller was compiled (IPK_PIPELINE_DESC_INIT); see ipk_fused_params, "Descriptor versioning" */
  int src_type;                    /* ipk_src_type */
  size_t width, height;            /* RawImage.width/height or raster dims */
  int cpp;                         /* RawImage.cpp (1 or 3); ignored for RGB8/RGB16 */
  int is_cfa;                      /* OpGoFloat.is_cfa */
  char cfa[160];                   /* OpDemosaic.cfa = cropped_cfa() ("" for Other): letters, or "WxH:letters" */
  size_t crop_top, crop_right, crop_bottom, crop_left;   /* OpGoFloat crops */
  float blacklevels[4], whitelevels[4];
  float rotatecrop[5];             /* OpRotateCrop: crop_top, crop_right, crop_bottom, crop_left, rotation */
  float cam_to_xyz_normalized[12];
  float wb_coeffs[4];
  float exposure; int npoints; float points[128];        /* OpBaseCurve */
  int rotation, fliph, flipv;      /* OpTransform */
  size_t maxwidth, maxheight;      /* PipelineSettings */
  int linear;
  int allow_fused;                 /* a small mask; 0: always staged.  Any non-zero value (IPK_FUSED_ON = 1): use ipk_raw_to_srgb when legal (cache==None).
                                      Bit 1 (IPK_FUSED_FOUR_COLOUR = 2, e.g. allow_fused = 3) additionally admits filters with a fourth colour to that
                                      one-launch route where ipk_pipeline_fuses_four_colour says so; without it they take the staged ops, as they always
                                      did.  The opt-in lives here because the descriptor's tail is pinned (its last field and reserved1 are named by callers
                                      and tests): no field could be added or renamed for it.  Like the rest of allow_fused it does not enter the hashes and
                                      results do not depend on it.
                                      Bit 2 (IPK_FUSED_WINDOW_REGIONS = 4) concerns regions only (ipk_pipeline_region / _run_region / ipk_host_pipeline_run_region):
                                      with it, a descriptor for which ipk_pipeline_fuses_rotatecrop or ipk_pipeline_fuses_scaledown answers 1 renders a region
                                      as a window of that one launch instead of computing the whole result.  Same contract: no hash, no result, and no other
                                      driver or report depends on it.
                                      Bit 3 (IPK_FUSED_WINDOW_PREVIEWS = 8) concerns regions only as well: with it, beside IPK_FUSED_ON, a descriptor for which
                                      ipk_pipeline_windows_preview answers 1 -- the downscaled previews, scale >= minscale -- renders a region as a window of its
                                      gofloat + demosaic pass (ipk_raw_scaled_demosaic_window / ipk_raster_scale_down_window) followed by the point-wise ops on
                                      that rectangle.  Same contract again.  The bit acts only together with bit 0: allow_fused = 8 still means "on" for every
                                      whole-frame route (any non-zero value does), but regions of previews are then cut from the whole result, as without the
                                      bit.  Bit 2 does not window these frames, with or without bit 3.  Monochrome and three-sample raws have such a pass
                                      under bit 7 only (below).
                                      Bit 4 (IPK_FUSED_PLAIN = 16), beside IPK_FUSED_ON as well: the frames whose OpDemosaic is a pass-through -- RGB8 / RGB16
                                      rasters with OpGoFloat crops, u16 monochrome and u16 three-sample raws -- run as the one launch ipk_plain_to_srgb where
                                      ipk_pipeline_fuses_plain says so, and regions of every frame on that launch (the uncropped rasters it always took
                                      included) are windowed.  Same contract: no hash, no result.  Without bit 0 it does nothing.
                                      Bit 5 (IPK_FUSED_CACHED_RESAMPLE = 32), beside IPK_FUSED_ON as well, concerns ipk_pipeline_run_cached_region alone: where
                                      ipk_pipeline_resamples_cached_region says so and the rotatecrop buffer (hash 2) is not memoised, the region is resampled
                                      from the cached demosaic buffer (hash 1) in one launch instead of running OpRotateCrop over the whole frame first.  Same
                                      contract: no hash, no result, no region report.  Without bit 0 it does nothing -- not even what "any non-zero value"
                                      does: allow_fused = 32 is 0 to every route and report.
                                      Bit 6 (IPK_FUSED_SCALED_ROTATECROP = 64), beside IPK_FUSED_ON as well: an active OpRotateCrop behind an OpDemosaic that
                                      scales runs as TWO launches where ipk_pipeline_fuses_scaled_rotatecrop says so, whole frames and (windowed) regions.
                                      Same contract: no hash, no result.  Like bit 5 it is nothing alone: allow_fused = 64 is 0 to every route and report.
                                      Monochrome and three-sample raws take this route under bit 7 only (below).
                                      Bit 7 (IPK_FUSED_PLAIN_PREVIEWS = 128), beside IPK_FUSED_ON as well: a monochrome or three-sample raw (u16 or f32) whose
                                      OpDemosaic scales runs OpGoFloat + OpDemosaic as the one launch ipk_plain_scale_down where ipk_pipeline_scales_plain says
                                      so; bits 3 and 6 then take such frames as they take the other previews.  Same contract: no hash, no result.  Like bits 3
                                      and 4, allow_fused = 128 alone still means "on" for every older route (any non-zero value does).
                                      Bit 8 (IPK_FUSED_BATCH_PREVIEWS = 256), beside IPK_FUSED_ON as well, concerns ipk_pipeline_run_batch (and the drivers that
                                      go through it) alone: a batch of downscaled previews runs as one scaling launch group and one point-wise pass per chunk
                                      of frames where ipk_pipeline_batches_previews says so.  Same contract: no hash, no result, no other driver or report
                                      depends on it.  Like bits 3, 4 and 7, allow_fused = 256 alone still means "on" for every older route.
                                      Bit 9 (IPK_FUSED_BATCH_ORIENTED = 512) acts beside bits 0 and 8 only: the batched previews take frames of any
                                      orientation, OpTransform folded into the point-wise pass, and ipk_pipeline_run_batch_each lets rotation, fliph and flipv
                                      differ inside a run.  Same contract: no hash, no result, no other driver or report depends on it; allow_fused = 512
                                      alone still means "on" for every older route.
                                      Bit 10 (IPK_FUSED_BATCH_SENSOR = 1024) acts beside bits 0 and 8 only: ipk_pipeline_run_batch_each lets the sensor
                                      fields -- width, height, cfa, cfa_width, cfa_height, the four crops, blacklevels, whitelevels -- differ inside a run
                                      whose frames negotiate one demosaic size, the scaling pass of such a chunk as one frame-table launch.  Same
                                      contract: no hash, no result, no other driver or report depends on it; allow_fused = 1024 alone still means "on"
                                      for every older route.
                                      Bit 11 (IPK_FUSED_BATCH_SIZES = 2048) acts beside bits 0 and 8 only, and changes nothing unless bit 9 or bit 10 is
                                      set as well: ipk_pipeline_run_batch_each then lets the frames of such a run negotiate their own demosaic sizes,
                                      a chunk of differing sizes as one sized scaling launch and one sized point-wise launch.  Same contract: no
                                      hash, no result, no other driver or report depends on it; allow_fused = 2048 alone still means "on" for every
                                      older route. */
  int use_fastpath;                /* PipelineSettings.use_fastpath (pipeline.rs:117; the reference defaults it to true) */
  /* later additions are appended (see ipk_fused_params) */
  int cfa_width, cfa_height;       /* as in ipk_fused_params: the tile's shape from the caller's CFA object, 0, 0 = from the string */
  /* third layout */
  int schedule;                    /* ipk_schedule, handed to the fused launch when the run is one */
  int fuse_rotatecrop;             /* 1: an active OpRotateCrop on a CFA mosaic runs as ONE launch where ipk_pipeline_fuses_rotatecrop says so; 0 (the default, and
                                      what every earlier caller has always written into this formerly reserved field): such frames take the staged ops.  Other
                                      values are refused with IPK_ERR_INVALID.  Results do not depend on it; like allow_fused it does not enter the hashes. */
  int reserved1;                   /* 0 (the struct's end moves past the second layout's tail padding, so that a size tells the layouts apart) */
  int fuse_scaledown;              /* 1: OpDemosaic's `full` + scale_down_opbuf branch (1 < scale < minscale, demosaic.rs:51-59) runs inside ONE raw-to-sRGB launch where
                                      ipk_pipeline_fuses_scaledown says so; 0 (the default, and what every earlier caller wrote into this formerly reserved field):
                                      the staged ops.  The same contract as fuse_rotatecrop: other values are IPK_ERR_INVALID, results do not depend on it, it does
                                      not enter the hashes, and it is not read from objects of an older layout. */
} ipk_pipeline_desc;
/* the bits of ipk_pipeline_desc.allow_fused */
typedef enum {
  IPK_FUSED_ON = 1,                /* the one-launch routes where legal (any non-zero value means this) */
  IPK_FUSED_FOUR_COLOUR = 2,       /* bit 1: four-colour filters take the one-launch route too */
  IPK_FUSED_WINDOW_REGIONS = 4,    /* bit 2: regions of the fuse_rotatecrop / fuse_scaledown routes run as a window of their one launch */
  IPK_FUSED_WINDOW_PREVIEWS = 8,   /* bit 3 (beside bit 0): regions of downscaled previews (OpDemosaic's scaled_demosaic branch, scale >= minscale, rasters
                                      under a size limit and, with bit 7 beside it, monochrome / three-sample raws under a size limit) run as a window of the
                                      scaling pass, where ipk_pipeline_windows_preview says so.
                                      Measured (profiles/r13_preview_regions.txt; 50 MP X-Trans -> 2160x1440 | 24 MP RGGB -> 1500x1000, u8, without -> with
                                      the bit): device form, 1/16 of the area 0.096 -> 0.032 | 0.063 -> 0.029 ms, 1/4 0.095 -> 0.045 | 0.068 -> 0.034 ms, the
                                      whole area 0.098 -> 0.090 | 0.068 -> 0.059 ms (the copy is saved); host form, 1/16 1.86 -> 0.17 ms (99.5 -> 6.3 MB
                                      uploaded) | 0.92 -> 0.11 ms (48 -> 3.1 MB), 1/4 1.89 -> 0.55 | 0.94 -> 0.29 ms.  NOT faster: a whole-area region
                                      through the host form uploads the whole frame either way, 2.016 -> 2.019 | 1.002 -> 1.001 ms */
  IPK_FUSED_PLAIN = 16,            /* bit 4 (beside bit 0): cropped RGB8 / RGB16 rasters and u16 monochrome / three-sample raws run as one launch
                                      (ipk_plain_to_srgb) where ipk_pipeline_fuses_plain says so, and regions of every frame on the raster launch are
                                      windowed.  f32 monochrome / three-sample raws stay staged (no kernel instantiation carries them).
                                      Measured (profiles/r14_plain_route.txt; 6000x4000 noise, without -> with the bit): whole frames, mono u16 -> u8
                                      0.253 -> 0.138 ms, -> f32 0.225 -> 0.144 ms; cpp3 u16 -> u8 0.268 -> 0.175 ms, -> f32 0.260 -> 0.175 ms; RGB8 with 5 %
                                      crops per side -> u8 0.229 -> 0.092 ms.  Regions to u8 (RGB8 | mono u16), device form: 1/16 of the area 0.123 -> 0.017 |
                                      0.272 -> 0.020 ms, 1/4 0.124 -> 0.036 | 0.273 -> 0.047 ms, the whole area 0.139 -> 0.108 | 0.292 -> 0.140 ms; host form:
                                      1/16 1.49 -> 0.20 ms (72 -> 4.5 MB uploaded) | 1.21 -> 0.18 ms (48 -> 3.1 MB), 1/4 1.72 -> 0.70 | 1.45 -> 0.60 ms.  NOT
                                      faster beyond the noise: a whole-area region through the host form uploads the whole frame either way, 2.77 -> 2.66 |
                                      2.41 -> 2.27 ms.  The cost to launches that use neither mode (the kernels test for them once per 256-pixel chunk):
                                      ipk_raster_to_srgb, RGB8 -> u8 at 24 MP, parent 0.1269 ms (its spread 0.0033) -> 0.1283 ms */
  IPK_FUSED_CACHED_RESAMPLE = 32,  /* bit 5 (beside bit 0): ipk_pipeline_run_cached_region resamples a region straight from the cached demosaic buffer when the
                                      rotatecrop buffer is missing (a crop or straighten edit), where ipk_pipeline_resamples_cached_region says so: one launch
                                      of k_fused_resample's cached-buffer source mode over the rectangle instead of OpRotateCrop over the whole frame plus the
                                      gather launch.  The trade-off: while the bit is set that call never fills hash 2 (see ipk_pipeline_run_cached_region).
                                      Measurements: profiles/r16_cached_resample.txt */
  IPK_FUSED_SCALED_ROTATECROP = 64,/* bit 6 (beside bit 0): a straightened or cropped frame whose OpDemosaic scales (with an angle the reverse size fold usually
                                      lands a pixel short, so this is the common straightened frame, and every straightened preview) runs as two launches
                                      instead of the staged ops, where ipk_pipeline_fuses_scaled_rotatecrop says so; regions of such frames are windowed.
                                      Monochrome and three-sample raws only together with bit 7 */
  IPK_FUSED_PLAIN_PREVIEWS = 128,  /* bit 7 (beside bit 0): downscaled previews of monochrome and three-sample raws (cpp == 1 without a filter, cpp == 3; u16
                                      and f32) run OpGoFloat + OpDemosaic's scale_down_opbuf branch as ONE pass over the source (ipk_plain_scale_down: the
                                      monochrome / three-sample modes of ipk_raw_scaled_demosaic's general kernel) where ipk_pipeline_scales_plain says so,
                                      instead of a full-size 16-byte-per-pixel buffer and a tap-by-tap pass over it.  With bit 3 their regions are windowed,
                                      with bit 6 their straightened previews run as two launches.
                                      Measured (profiles/r18_plain_previews.txt; 6000x4000 noise, wall clock, medians, the parent build's run -> this route;
                                      the parent's spread is 0.002 .. 0.015 ms throughout): under maxwidth 1500 to u8, whole frame | 1/16 | 1/4 of the area: mono
                                      u16 0.546 -> 0.093 | 0.541 -> 0.039 | 0.544 -> 0.047 ms, mono f32 0.538 -> 0.094 | 0.533 -> 0.039 | 0.537 -> 0.048, cpp3
                                      u16 0.551 -> 0.127 | 0.546 -> 0.042 | 0.550 -> 0.056, cpp3 f32 0.554 -> 0.147 | 0.551 -> 0.042 | 0.553 -> 0.057 (to f32
                                      the same within 0.005 ms); under maxwidth 400 to u8 (skip 15: windows of 16 x 16 taps, one thread per output pixel) mono
                                      u16 0.681 -> 0.115 | 0.675 -> 0.084 | 0.675 -> 0.086, mono f32 0.674 -> 0.123 | 0.670 -> 0.083 | 0.669 -> 0.091, cpp3 u16
                                      0.690 -> 0.173 | 0.684 -> 0.103 | 0.684 -> 0.121, cpp3 f32 0.694 -> 0.271 | 0.687 -> 0.103 | 0.688 -> 0.145.  Straightened
                                      (bits 6 and 7): mono u16 at rotation 0.02 under maxwidth 3000 to u8, whole frame 0.690 -> 0.264 ms.  No measured case was NOT
                                      faster than the parent's run beyond its spread; none is excluded.  The cost to the carrier kernel's mosaic mode (one
                                      launch-uniform branch outside the row loop): 6000x4000 RGGB u16 under maxwidth 400 (skip 15, k_raw_scaled_demosaic<uint16_t>),
                                      parent 0.149 ms (spread 0.001) -> 0.148 ms.  Not measured: the host form of the regions, regions of the straightened
                                      case, 100 MP frames, 16-bit outputs, photo-like data, and the 8-sample mosaic kernels (k_raw_scaled_demosaic_w8 / _w8m:
                                      their code is untouched, their argument block grew by five words) */
  IPK_FUSED_BATCH_PREVIEWS = 256,  /* bit 8 (beside bit 0): ipk_pipeline_run_batch runs a batch of downscaled previews -- staged frames whose OpGoFloat +
                                      OpDemosaic is the one scaling pass (mosaics at scale >= minscale, rasters under a size limit, monochrome / three-sample
                                      raws under bit 7), OpRotateCrop and OpTransform no-ops, at least 256 pixels per preview -- chunk by chunk: the scaling
                                      pass of a chunk as ONE launch per 64 frames where the frames select the general kernel (ipk_raw_scaled_demosaic_batch /
                                      ipk_plain_scale_down_batch; else a launch per frame), then the point-wise chain ONCE over the previews lying one after
                                      another, where ipk_pipeline_batches_previews says so.  A thumbnail's scaling launch is far too small to fill the chip
                                      and its windows cannot be split across lanes (one accumulator, y outer, x inner): frames are the parallelism left.
                                      Out of scope, falling to the per-frame loop: non-Normal orientations without bit 9 and active rotatecrops in a batch; batch forms of
                                      the window-8 kernels and the raster scaler (a launch per frame inside the route); the host-buffer batch
                                      (ipk_host_pipeline_run_batch is unchanged); band (multi-GPU single-frame) forms; the bit as a default.
                                      Measurements: profiles/r19_batch_previews.txt */
  IPK_FUSED_BATCH_ORIENTED = 512,  /* bit 9 (beside bits 0 and 8; nothing without either): a batch of previews may carry orientations.  OpTransform
                                      behind a no-op OpRotateCrop is a dihedral permutation of the preview, and pass 2 of the batch folds it into its
                                      loads: ONE frame-table launch per chunk (ipk_pointwise_chain_out_batch_oriented), each frame's record with the gather
                                      walk of its own orientation, instead of the scaling pass, the chain, the quantise and the transform per frame.
                                      ipk_pipeline_batches_previews then answers 1 for the seven other orientations too, ipk_pipeline_run_batch runs an
                                      oriented descriptor that way, and ipk_pipeline_run_batch_each keeps landscape and portrait frames of one shoot in one
                                      run where they negotiate the same demosaic size (see there).  Without the bit every plan, launch, tag and stage
                                      name is what it was.  Every orientation walks the gather mode the chain kernels already have
                                      (ipk_pipeline_run_cached_region's): a flip keeps a lane's pixels consecutive in memory, forwards or backwards; a
                                      transposing orientation reads one source pixel per lane a source row apart.
                                      Out of scope: active rotatecrops in a batch; per-frame size limits inside one scaling launch (levels, crops
                                      and filters: bit 10; demosaic sizes that differ under one limit: bit 11); the host-buffer batch drivers; band forms; the bit as a default; graph capture.
                                      Measured (profiles/r21_batch_oriented.txt; device-resident noise frames under a square box, every frame with its
                                      own wb_coeffs and exposure, wall clock, medians, ms per frame; the parent build's only offer -- a loop of
                                      ipk_pipeline_run -- -> ipk_pipeline_run_batch_each with the bit; the parent's spread is 0.0003 .. 0.0045 ms), every
                                      frame Rotate90 to u8, n = 2 / 8 / 16 / 64: 24 MP RGGB u16 -> 256x170: 0.217 -> 0.123, 0.224 -> 0.060, 0.223 -> 0.072,
                                      0.222 -> 0.060; -> 400x266: 0.128 -> 0.092, 0.129 -> 0.071, 0.128 -> 0.067, 0.127 -> 0.063; 50 MP X-Trans u16 ->
                                      270x180: 0.381 -> 0.233, 0.394 -> 0.179, 0.394 -> 0.162, 0.392 -> 0.151; 24 MP mono u16 -> 256x170: 0.147 -> 0.081,
                                      0.157 -> 0.051, 0.157 -> 0.064, 0.156 -> 0.052: x1.4 .. x1.8 at n = 2, x1.8 .. x3.7 at n >= 8.  Normal and Rotate90
                                      alternating, and Rotate90 to u16, are within 0.002 ms of those figures.  The price of orientation, against this
                                      build's all-Normal batch on the same frames: +0.002 .. +0.004 ms per frame at n = 2, -0.0005 .. +0.002 at n >= 8.
                                      No measured case was slower than the parent's loop; none is excluded.  The carriers' launches outside the mode
                                      stayed inside the parent's spread (their device code is the parent's): ipk_pointwise_chain_out at 2160x1440 to f32
                                      0.0397 -> 0.0398 ms, to u8 0.0397 -> 0.0395; at 6000x4000 to f32 0.1962 -> 0.1981 (spread 0.0107), to u8 0.1794 ->
                                      0.1756 (0.0084); the cached-region gather launch over 1/16 of a 24 MP frame to u8 0.0449 -> 0.0451.
                                      The transposed tile walk (see ipk_pointwise_chain_out_batch_oriented) against this gather (the file's second
                                      part), Rotate90 batches, gather minus tile walk in ms per frame: -> 400x266 to u8 +0.0003 / +0.0001 / +0.0010 / +0.0009 at n = 2 / 8 / 16 / 64
                                      (beyond the two builds' spreads at n = 16 and 64 only, by 1.5 %), X-Trans -> 270x180 to u8 -0.0017 / +0.0003 /
                                      -0.0020 / +0.0006 and to u16 -0.0004 / -0.0003 / -0.0014 / -0.0010, all inside spreads of 0.003 .. 0.007: at
                                      most 0.001 ms of frames that take 0.06 .. 0.15 (presumably because a 0.7 MB preview's transposing reads are
                                      served from the caches; not profiled).  It had to be faster beyond the spreads in both rows to stay, and no
                                      X-Trans reading was, so it was deleted.
                                      Not measured: f32 outputs, f32 sources, the other six orientations, scattered destinations, per-frame matrices
                                      and curves, batches above 64 frames, rasters and the window-8 geometries, previews larger than 400 wide (where
                                      the transposing gather's cost must grow towards the 3.3x of ipk_pipeline_run_cached_region's 24 MP region),
                                      the uniform route (ipk_pipeline_run_batch on one oriented descriptor), photo-like data */
  IPK_FUSED_BATCH_SENSOR = 1024,   /* bit 10 (beside bits 0 and 8; nothing without either; combines with bit 9): the frames of a batch of previews may
                                      carry their own sensor settings.  One camera's levels change with ISO and a folder holds more than one body, so
                                      ipk_pipeline_run_batch_each keeps frames in one run that differ in width, height, cfa, cfa_width, cfa_height, the
                                      crops, blacklevels or whitelevels, where each would batch its own previews through the general scaling kernel
                                      (ipk_pipeline_batches_previews answers 1 with pass1_batched = 1) and all negotiate one demosaic size (see there).
                                      Pass 1 of a chunk whose frames differ in these fields is ONE ipk_scaled_demosaic_batch_each launch -- the
                                      frame-table mode of k_raw_scaled_demosaic<T>, frame i's record from descriptor i's own negotiation -- instead of a
                                      loop of ipk_pipeline_run; a chunk whose frames agree in them is the uniform launch as before.  Without the bit
                                      every plan, launch, tag and stage name is what it was.  The carrier kernel: 49 VGPRs, no scratch, in both
                                      instantiations, before and after.
                                      Out of scope: per-frame preview sizes without bit 11 (IPK_FUSED_BATCH_SIZES); batch forms of the window-8 kernels
                                      and the raster scaler; active rotatecrops in a batch; the host-buffer batch drivers and the multi-device driver;
                                      band forms; the bit as a default; graph capture.
                                      Measured (profiles/r22_batch_sensor.txt; device-resident noise frames to u8, every frame with its own black and
                                      white level and its own wb_coeffs, wall clock, medians, ms per frame; the parent build's only offer -- its
                                      ipk_pipeline_run_batch_each, which cuts such a run into a loop of ipk_pipeline_run -- -> this call with the bit |
                                      this build's route 2 on the same frames with EQUAL sensor fields; the parent's spread is 0.0008 .. 0.0201 ms, once 0.092),
                                      n = 2 / 8 / 16 / 64: 24 MP RGGB u16 -> 256 wide: 0.299 -> 0.134 | 0.131, 0.247 -> 0.072 | 0.067, 0.236 -> 0.082 |
                                      0.079, 0.227 -> 0.072 | 0.069; -> 400 wide: 0.236 -> 0.105 | 0.099, 0.196 -> 0.082 | 0.079, 0.187 -> 0.078 | 0.075,
                                      0.181 -> 0.075 | 0.072; 50 MP X-Trans u16 -> 270 wide: 0.468 -> 0.247 | 0.244, 0.419 -> 0.192 | 0.189, 0.407 ->
                                      0.174 | 0.171, 0.398 -> 0.166 | 0.161; 24 MP mono u16 -> 256 wide: 0.143 -> 0.081 | 0.079, 0.154 -> 0.050 | 0.048,
                                      0.154 -> 0.063 | 0.063, 0.153 -> 0.052 | 0.052; 24 MP and 24.4 MP RGGB bodies alternating -> 256 wide: 0.298 ->
                                      0.134, 0.246 -> 0.072, 0.234 -> 0.083, 0.226 -> 0.073: x1.8 .. x2.3 at n = 2, x2.2 .. x3.5 at n >= 8.  The price
                                      of the table (sensor minus equal): +0.0001 .. +0.0064 ms per frame.  No measured case at n >= 8 was slower than
                                      the parent's loop; none is excluded.  The kernel's untouched modes against the parent build:
                                      ipk_raw_scaled_demosaic_batch 6000x4000 -> 256x170 at n = 8 0.412 -> 0.415 ms and at n = 64 3.329 -> 3.326 ms,
                                      inside its spread; KNOWN LOSS: the single launch ipk_raw_scaled_demosaic 6000x4000 -> 400x266 0.1181 -> 0.1203 ms,
                                      outside the parent's spread of 0.0017, and 0.1175 -> 0.1194 (spread 0.0034) in a second session with ten times the
                                      samples: +0.002 ms (1.6 .. 1.9 %) both times; its disassembly holds the parent's vector loads one for one, the cause was not found.
                                      Not measured: f32 sources, f32 and 16-bit outputs, per-frame crops and filters inside one series, three-sample
                                      raws, batches above 64 frames, orientations beside sensor settings, mixed batches, photo-like data */
  IPK_FUSED_BATCH_SIZES = 2048     /* bit 11 (beside bits 0 and 8; nothing unless bit 9 or bit 10 is set as well, because nothing else lets a size
                                      differ): the frames of a batch of previews may negotiate their own demosaic size.  Under maxwidth alone a
                                      Rotate90 frame negotiates another size than a Normal one (6000x4000 under maxwidth 256: 256x170 against
                                      384x256), and so do two bodies of different aspect ratio; without this bit such a pair cuts the run, and an
                                      alternating shoot is a loop of ipk_pipeline_run.  With it ipk_pipeline_run_batch_each waives the "one demosaic
                                      size" condition of bits 9 and 10 for a pair of descriptors that both carry the bit, would both batch their own
                                      previews, and both have pass1_batched = 1 (ipk_pipeline_batches_previews): the sized launch exists for the
                                      general scaling kernel only.  maxwidth, maxheight and every field that counted before still count, and under
                                      bit 10 both filters still agree in whether they have a fourth colour.  Such a run is route 2.  Its chunks are cut
                                      greedily in order (ipk_pipeline_batch_each_chunks reports them): a chunk grows while it has fewer than 64 frames
                                      and its RGBE previews sum to at most 256 MiB -- for frames of one size the chunk of old.  Pass 1 of a chunk whose
                                      frames differ in demosaic size is ONE ipk_scaled_demosaic_batch_sized launch ("batch-each gofloat+demosaic"),
                                      pass 2 ONE ipk_pointwise_chain_out_batch_sized launch (the "batch-each to_lab+..." names of old); a chunk whose
                                      sizes agree takes the launches it took.  Without the bit every plan, launch, tag, stage name and result is what
                                      it was.  The sized grid is laid over the largest frame of the chunk: blocks over a smaller frame's missing
                                      columns or rows find no work, so a chunk wastes blocks in proportion to the spread of its sizes.
                                      Out of scope: per-frame maxwidth / maxheight; the window-8 kernels and the raster scaler (they cut the run);
                                      active rotatecrops in a batch; the host-buffer batch drivers and the multi-device driver; graph capture.
                                      The carriers, before and after: k_raw_scaled_demosaic<T> 49 VGPRs in both instantiations,
                                      k_pointwise_chain_small 82, k_raster_chain<Rgbe32, 1 | 2> 124 / 123, no scratch; no other kernel's disassembly
                                      moved (the file below holds both tools' output).
                                      Measured (profiles/r24_batch_sizes.txt; device-resident 24 MP RGGB u16 noise frames to u8, every frame with its
                                      own wb_coeffs, wall clock, medians, ms per frame; the parent build's only offer -- its
                                      ipk_pipeline_run_batch_each, which cuts such a run into a loop of ipk_pipeline_run -- -> this call with the bit;
                                      the parent's spread is 0.0005 .. 0.0126 ms), n = 2 / 8 / 16 / 64: Normal / Rotate90 alternating under maxwidth 256
                                      (256x170 beside 384x256): 0.180 -> 0.127, 0.185 -> 0.069, 0.184 -> 0.067, 0.182 -> 0.068; under maxwidth 400
                                      (400x266 beside 600x400): 0.117 -> 0.089, 0.118 -> 0.072, 0.116 -> 0.069, 0.115 -> 0.067; a 3:2 and a 4:3 body
                                      alternating under maxwidth 256 (256x170 beside 256x192): 0.211 -> 0.124, 0.222 -> 0.065, 0.214 -> 0.064, 0.213 ->
                                      0.062: x1.3 .. x1.7 at n = 2, x1.6 .. x3.4 at n >= 8.  No measured case at n >= 8 was slower than the parent's
                                      loop; none is excluded.  The price of the spread of sizes -- the sized call minus the mean of this build's two
                                      equal-size runs of the same shapes, the wasted blocks of the sized grid and the larger records together: the
                                      chunk mixing 256x170 with 384x256 +0.024 / +0.005 / -0.001 / +0.009 ms per frame at n = 2 / 8 / 16 / 64, over
                                      all three series -0.001 .. +0.024 (the equal-size runs themselves vary by 0.01 between batch sizes: reported,
                                      not bounded).  Outside the mode, parent -> this build, every reading inside the parent's spread:
                                      ipk_raw_scaled_demosaic 6000x4000 -> 400x266 0.1209 -> 0.1187 ms (spread 0.0027), ipk_pointwise_chain_out to u8
                                      at 2160x1440 0.0403 -> 0.0400 (0.0011) and at 6000x4000 0.1824 -> 0.1837 (0.0085), per call at n = 16: the
                                      uniform batch 1.174 -> 1.183 (0.047), bit 9's equal-size launches 1.177 -> 1.187 (0.041), bit 10's 1.221 ->
                                      1.248 (0.059) -- all three on the slower side of the median; no loss outside a spread was read.  bench.py,
                                      alternating, MP/s: parent 232381 .. 235319, this build 233873 .. 234956.
                                      Not measured: f32 sources, f32 and 16-bit outputs, other mosaics, monochrome and three-sample raws, more than
                                      two sizes in a chunk, batches above 64 frames, chunks cut by the 256 MiB sum, orientation and sensor size
                                      together, the host cost of the plan alone, photo-like data */
} ipk_fused_mask;
#define IPK_PIPELINE_DESC_INIT {(uint32_t)sizeof(ipk_pipeline_desc)}

/* Size negotiation of Pipeline::run (src/pipeline.rs:314-338): demosaic_{w,h} as stored in the
 * settings, and the size of the buffer run() returns.  The ops size their outputs from the buffer
 * they are handed (demosaic.rs:60-90, rotatecrop.rs:41-57, transform.rs:46-60), so behind a
 * rotatecrop the returned buffer can be a pixel smaller than the forward fold of
 * transform_forward() the negotiation itself uses; final_{w,h} is what run() produces.
 * A side that scales to 0 is reported as 0 and ipk_pipeline_run rejects it.  No GPU needed. */
IPK_API int ipk_pipeline_sizes(const ipk_pipeline_desc *d, size_t *demosaic_w, size_t *demosaic_h,
                               size_t *final_w, size_t *final_h);
/* Runs the ops in the reference's fixed order (src/pipeline.rs:155-164,364-372) on a DEVICE source
 * buffer and writes the result (final_w*final_h*3 elements of out_type) to the DEVICE buffer dst.
 * out_type IPK_OUT_F32 = Pipeline::run with d->linear; IPK_OUT_U8 = output_8bit (forces
 * linear=false, pipeline.rs:405); IPK_OUT_U16 = output_16bit (forces linear=true, :452).
 * *used_fused (may be NULL) reports which path ran. */
IPK_API int ipk_pipeline_run(const ipk_pipeline_desc *d, const void *src, void *dst, int out_type,
                             int *used_fused, void *stream);
/* Raster fast path of output_8bit / output_16bit (pipeline.rs:381-402, :428-449): when d->use_fastpath is set, the
 * source is RGB8/RGB16, out_type is U8/U16 and the ops are the defaults for a raster source (Pipeline::default_ops,
 * :286-288, compared bitwise), ipk_pipeline_run / _cached skip the float pipeline: DynamicImage::to_rgb8/16 channel
 * conversion if the depths differ (image 0.24: c*257, (c+128)/257 -- crate absent, parity unpinned) and
 * scale_down_srgb / scale_down_srgb16 (scaling.rs:162-182) if a size limit applies.  Returns 1 / 0. */
IPK_API int ipk_pipeline_takes_fastpath(const ipk_pipeline_desc *d, int out_type);
/* Does ipk_pipeline_run (and the cached, batch and host drivers) run this descriptor's active OpRotateCrop inside ONE launch
 * (ipk_raw_to_srgb_resampled, then OpTransform's permutation if there is one)?  1 when d->fuse_rotatecrop and d->allow_fused are set, the source is
 * a one-sample-per-pixel CFA mosaic with a three-colour filter, the rotatecrop is not a no-op and accepts its crops (RotateCrop::corners), the
 * transform is one the launch takes, and OpDemosaic does not scale (scale <= 1).  The last is a real restriction: with an angle the reference's
 * reverse size fold often negotiates a demosaic size one pixel short of the source (6000x4000 at rotation 0.05: 5999x3999), OpDemosaic then
 * scales by 1.00025 and the frame stays staged, whatever the flag says.  0 otherwise; a negative error code for a descriptor ipk_pipeline_sizes
 * refuses, and for a fuse_rotatecrop other than 0 or 1.  No GPU needed. */
IPK_API int ipk_pipeline_fuses_rotatecrop(const ipk_pipeline_desc *d, int out_type);
/* Does ipk_pipeline_run (and the cached, batch and host drivers) run OpDemosaic's `full` + scale_down_opbuf branch inside ONE launch
 * (ipk_raw_to_srgb_scaled, then OpTransform's permutation if there is one)?  1 when d->fuse_scaledown and d->allow_fused are set, the source is a
 * one-sample-per-pixel CFA mosaic with a three-colour filter, OpRotateCrop is a no-op, 1 < scale < minscale (src/ops/demosaic.rs:33-39) and the launch
 * takes the negotiated demosaic size (both skips at least 1 and below 3: a 101-wide frame at maxwidth 51 has scale 1.98 and a skip of exactly 2.0 and is
 * taken; a 150x100 X-Trans frame at maxwidth 52 has a scale below 3 but a skip of 3.0 and stays staged).  0 otherwise; a negative error code for a
 * descriptor ipk_pipeline_sizes refuses, and for a fuse_scaledown other than 0 or 1.  ipk_pipeline_fuses_rotatecrop keeps answering 0 wherever
 * OpDemosaic scales.  No GPU needed. */
IPK_API int ipk_pipeline_fuses_scaledown(const ipk_pipeline_desc *d, int out_type);
/* Does ipk_pipeline_run (and the cached, batch, host, multi-device and region drivers) run this descriptor's four-colour frame as ONE raw-to-sRGB
 * launch (ipk_raw_to_srgb with four_colour = 1, then OpTransform's permutation if there is one; regions windowed)?  1 when d->allow_fused has
 * IPK_FUSED_FOUR_COLOUR set, the source is a one-sample-per-pixel CFA mosaic whose filter has a fourth colour, OpRotateCrop is a no-op and OpDemosaic
 * does not scale (scale <= 1).  0 otherwise -- three-colour filters included: their one-launch route does not depend on the bit --; a negative error
 * code for a descriptor ipk_pipeline_sizes refuses.  No GPU needed. */
IPK_API int ipk_pipeline_fuses_four_colour(const ipk_pipeline_desc *d, int out_type);
/* Does a region of this descriptor (ipk_pipeline_region / _run_region / ipk_host_pipeline_run_region) run as a window of its scaling gofloat + demosaic
 * pass?  1 when d->allow_fused has IPK_FUSED_ON and IPK_FUSED_WINDOW_PREVIEWS set, OpRotateCrop is a no-op, and the staged drivers run OpGoFloat and
 * OpDemosaic as the one scaling pass: a one-sample-per-pixel CFA mosaic with a valid filter (three or four colours) at scale >= minscale
 * (src/ops/demosaic.rs:33-50), an RGB8 / RGB16 raster at scale > 1 that does not take the fast path, or -- with IPK_FUSED_PLAIN_PREVIEWS set as well -- a
 * monochrome or three-sample raw at scale > 1 (ipk_pipeline_scales_plain).  0 otherwise -- mono and three-sample raws without that bit, an
 * active rotatecrop behind a scaling demosaic, 1 < scale < minscale (IPK_FUSED_WINDOW_REGIONS' ground), full-size frames (windowed whatever the
 * bits); a negative error code for a descriptor ipk_pipeline_sizes refuses.  Whole-frame drivers do not depend on the bit.  No GPU needed. */
IPK_API int ipk_pipeline_windows_preview(const ipk_pipeline_desc *d, int out_type);
/* Does ipk_pipeline_run (and the batch, host and multi-device drivers; the cached driver fills its cache from the staged ops) run this descriptor's
 * whole frame as the one launch ipk_plain_to_srgb BECAUSE of IPK_FUSED_PLAIN?  1 when d->allow_fused has IPK_FUSED_ON and IPK_FUSED_PLAIN set, the frame
 * does not take the fast path, OpRotateCrop is a no-op, OpDemosaic does not scale (scale <= 1), the cropped rectangle has at least 256 pixels, and the
 * source is an RGB8 / RGB16 raster WITH OpGoFloat crops, a u16 raw with cpp == 3, or a u16 raw with cpp == 1 and no filter (is_cfa == 0).  0 otherwise
 * -- uncropped rasters included: their one launch does not depend on the bit (only their regions do) --, f32 monochrome / three-sample raws
 * (staged: the launch has no f32 form), mosaics; a negative error code for a descriptor ipk_pipeline_sizes refuses.  No GPU needed. */
IPK_API int ipk_pipeline_fuses_plain(const ipk_pipeline_desc *d, int out_type);
/* Do ipk_pipeline_run and the cached, batch, host, multi-device and region drivers run this descriptor's OpGoFloat and its scaling OpDemosaic as the ONE
 * launch ipk_plain_scale_down BECAUSE of IPK_FUSED_PLAIN_PREVIEWS?  1 when d->allow_fused has IPK_FUSED_ON and IPK_FUSED_PLAIN_PREVIEWS set, the frame
 * does not take the fast path, the source is a raw that OpGoFloat does not treat as a mosaic -- cpp == 1 with is_cfa == 0, or cpp == 3; IPK_SRC_U16 or
 * IPK_SRC_F32 -- and OpDemosaic scales (scale > 1).  0 otherwise: mosaics and rasters (their scaling passes do not depend on the bit), full-size frames
 * (IPK_FUSED_PLAIN's ground), the bit without IPK_FUSED_ON.  The stage keeps its name, "gofloat+demosaic" ("region gofloat+demosaic" for a windowed
 * region); the cached drivers store the buffer under the demosaic hash with the source's monochrome flag, and hash 0 is then never filled.  A negative
 * error code for a descriptor ipk_pipeline_sizes refuses.  No GPU needed. */
IPK_API int ipk_pipeline_scales_plain(const ipk_pipeline_desc *d, int out_type);
/* Does ipk_pipeline_run (and the host, batch and multi-device drivers; the cached drivers are unchanged) run this descriptor's frame as TWO launches: the
 * scaling gofloat + demosaic pass into the negotiated demosaic-size RGBE buffer, then ONE resampling launch over that buffer (k_fused_resample's 4-channel
 * source mode: OpRotateCrop's transform_buffer, tolab..gamma and the quantiser), then OpTransform's permutation if there is one?  1 when d->allow_fused has
 * IPK_FUSED_ON and IPK_FUSED_SCALED_ROTATECROP set, the frame does not take the fast path, OpRotateCrop is active and accepts its crops on the
 * demosaic-size buffer, OpDemosaic scales (scale > 1), the resampling launch admits the transform (windows of at most 3x3), and pass 1 exists as one
 * launch: a one-sample-per-pixel mosaic with a valid three-colour filter at scale >= minscale (ipk_raw_scaled_demosaic) or at 1 < scale < minscale with
 * geometry ipk_raw_demosaic_scaled takes, an RGB8 / RGB16 raster (ipk_raster_scale_down), or -- with IPK_FUSED_PLAIN_PREVIEWS set as well -- a monochrome
 * or three-sample raw (ipk_plain_scale_down, E = +0.0).  0 otherwise: filters with a fourth colour (E is not +0.0
 * there), monochrome and three-sample raws without that bit, scale <= 1 (fuse_rotatecrop's ground), a no-op rotatecrop, the bit without IPK_FUSED_ON.  Regions of such a
 * descriptor are windowed under the same bit: pass 1 runs over the footprint F of the region's rectangle in the demosaic-size buffer, pass 2 over the
 * rectangle, and ipk_pipeline_region reports what pass 1 reads for F plus the crop offset.  ipk_timing names the stages "gofloat+demosaic",
 * "rotatecrop+to_lab+basecurve+from_lab+gamma" and "transform".  A negative error code for a descriptor ipk_pipeline_sizes refuses.  No GPU needed.
 * Traffic model for a 24 MP u16 mosaic at scale 1.00025 to u8: the staged ops move about 109 bytes per pixel in five launches, this route about 37 in
 * two.  Measured (profiles/r17_scaled_rotatecrop.txt; noise frames at rotation 0.02, wall clock, medians, the parent build's run -> this route):
 * 6000x4000 RGGB u16 (negotiates 5999x3999) to u8, whole frame 1.473 -> 1.079 ms, 1/16 of the area 1.483 -> 0.122 ms, 1/4 1.522 -> 0.315 ms (to f32:
 * 1.480 -> 1.088, 1.492 -> 0.122, 1.536 -> 0.316); the same under maxwidth 4000 (scale 1.5) 0.872 -> 0.668, 0.865 -> 0.098, 0.882 -> 0.219 ms.  Where
 * pass 1 is a launch the staged drivers already had, the regions are the gain and whole frames are level: 8640x5760 X-Trans under maxwidth 2160, whole
 * frame 0.184 -> 0.180 ms (this build's own staged run in the same process: 0.179), 1/16 0.185 -> 0.055, 1/4 0.189 -> 0.080 ms; a 6000x4000 RGB8 raster
 * under maxwidth 3000, 0.275 -> 0.266 ms (own staged run 0.264), 0.272 -> 0.048, 0.280 -> 0.094 ms.  No measured case was slower than the parent's run;
 * none is excluded.  Not measured: 100 MP frames, 16-bit outputs, photo-like data. */
IPK_API int ipk_pipeline_fuses_scaled_rotatecrop(const ipk_pipeline_desc *d, int out_type);
/* do_timing! (src/pipeline.rs:68-80: the reference logs the wall time of every op of Pipeline::run): ipk_timing_begin arms the calling
 * thread, the following ipk_pipeline_run call(s) on it bracket every stage they enqueue with hipEvents on their stream, ipk_timing_end
 * waits for the last one and returns the stages in execution order under the reference's op names ("gofloat", "demosaic", "rotatecrop",
 * "to_lab", "basecurve", "from_lab", "gamma", "transform"; merged stages are joined with '+', the one-launch paths start with "fused",
 * the output loops are "quantise").  *n_stages receives the number of stages (may exceed max_stages; the surplus is dropped). */
typedef struct { char name[88]; float ms; } ipk_stage_time;
IPK_API int ipk_timing_begin(void);
IPK_API int ipk_timing_end(ipk_stage_time *out, int max_stages, int *n_stages);
/* Same with HOST source and destination buffers; synchronous. */
IPK_API int ipk_host_pipeline_run(const ipk_pipeline_desc *d, const void *src, void *dst, int out_type, int *used_fused);
/* Regions: columns [x, x+w) and rows [y, y+h) of the final_w x final_h result of ipk_pipeline_run (after OpTransform, in its orientation),
 * bit-identical to that rectangle of the whole result and written row-major and packed: w*h*3 samples of out_type.  An empty region, one
 * that leaves the result, or a descriptor ipk_pipeline_run rejects fails with IPK_ERR_INVALID and writes nothing.
 * ipk_pipeline_region plans one (no GPU needed) and returns its route: 1 = windowed -- the run is the fused raw->sRGB launch, restricted to the
 * rectangle of the cropped frame the region comes from, and reads only the sensor window reported (that rectangle plus demosaic::full's
 * one-pixel halo, clipped to the crop window, in sensor coordinates); 0 = whole frame -- staged, scaled, rotatecrop, four-colour (without
 * IPK_FUSED_FOUR_COLOUR in allow_fused; with it: windowed), mono/RGB and
 * raster routes and allow_fused = 0 compute the whole result and copy the region out, and the window reported is the crop window.
 * With IPK_FUSED_WINDOW_REGIONS in allow_fused the one-launch rotatecrop and scaledown routes (ipk_pipeline_fuses_rotatecrop / _scaledown answer 1)
 * are windowed too: the region is mapped back through OpTransform to a rectangle of the resampled image, the launch runs over that rectangle only,
 * and the window reported is its footprint (ipk_transform_window_footprint plus the crop offset; it can be empty, w = h = 0, where no pixel of the
 * region has a tap).  Without the bit those routes answer 0, as they always did.
 * With IPK_FUSED_WINDOW_PREVIEWS (and IPK_FUSED_ON) in allow_fused the downscaled previews (ipk_pipeline_windows_preview answers 1) are windowed too:
 * the region is mapped back through OpTransform to a rectangle of the demosaic_w x demosaic_h preview, the scaling gofloat + demosaic pass runs over
 * that rectangle only, the point-wise ops, the quantisation and OpTransform's permutation follow on the rectangle, and the window reported is
 * ipk_scaled_window_footprint plus the crop offset (never empty).  Without the bit they answer 0.
 * With IPK_FUSED_PLAIN (and IPK_FUSED_ON) in allow_fused every frame on the raster launch -- uncropped and cropped RGB8 / RGB16 rasters off the fast
 * path, u16 monochrome and three-sample raws; OpRotateCrop a no-op, scale <= 1 -- is windowed: the region is mapped back through OpTransform to a rectangle of
 * the cropped frame, ipk_plain_to_srgb runs over that rectangle, and the window reported is the rectangle itself in sensor coordinates (the ops are
 * point-wise: no halo, never empty).  A region of fewer than 256 pixels answers 0 and is cut from the whole result.  Without the bit they answer 0. */
IPK_API int ipk_pipeline_region(const ipk_pipeline_desc *d, int out_type, size_t x, size_t y, size_t w, size_t h,
                                size_t *src_x, size_t *src_y, size_t *src_w, size_t *src_h);
/* The region from the DEVICE source ipk_pipeline_run takes (the whole sensor frame) into the DEVICE buffer dst, enqueued on `stream`.
 * *windowed (may be NULL) receives the route.  ipk_timing_begin/end see its stages. */
IPK_API int ipk_pipeline_run_region(const ipk_pipeline_desc *d, const void *src, size_t x, size_t y, size_t w, size_t h, void *dst,
                                    int out_type, int *windowed, void *stream);
/* The same from the whole HOST frame into a HOST buffer; synchronous.  The windowed route uploads only the reported sensor window, its rows widened to 64-byte boundaries of the frame's rows (one
 * pitched copy), the whole route the frame; only the region's w*h*3 samples come back. */
IPK_API int ipk_host_pipeline_run_region(const ipk_pipeline_desc *d, const void *src, size_t x, size_t y, size_t w, size_t h, void *dst,
                                         int out_type, int *windowed);
/* A batch of n same-shaped HOST frames through one descriptor (a caller looping Pipeline::run / output_8bit over a shoot,
 * src/pipeline.rs:311-372, :404-421): three HIP streams (upload, compute, download) over two device slots, so frame i's kernels
 * run while frame i+1 crosses PCIe upwards and frame i-1 downwards; per-frame cost tends to max(upload, compute, download)
 * instead of their sum.  The copies only overlap for page-locked host memory (ipk_host_alloc below, or memory the caller has
 * registered); pageable buffers work but serialise.  Results are what n calls of ipk_host_pipeline_run give.  Synchronous at return. */
IPK_API int ipk_host_pipeline_run_batch(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n,
                                        int out_type, int *used_fused);
/* n same-shaped DEVICE frames through one descriptor on the current context (the device-pointer form of the above, enqueued on `stream`):
 * where Pipeline::run is exactly one fused launch per frame the batch is one persistent launch per 64 frames (ipk_raw_to_srgb_batch), otherwise
 * n calls of ipk_pipeline_run.  Results are what n calls of ipk_pipeline_run give. */
IPK_API int ipk_pipeline_run_batch(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n, int out_type,
                                   int *used_fused, void *stream);
/* Does ipk_pipeline_run_batch (and ipk_pipeline_run_batch_multi, member by member) run n frames of this descriptor as batched previews BECAUSE of
 * IPK_FUSED_BATCH_PREVIEWS?  1 when d->allow_fused has IPK_FUSED_ON and IPK_FUSED_BATCH_PREVIEWS set, n > 1, the frame is staged and its OpGoFloat +
 * OpDemosaic is the one scaling pass (a one-sample-per-pixel mosaic at scale >= minscale, an RGB8 / RGB16 raster at scale > 1 off the fast path, or --
 * with IPK_FUSED_PLAIN_PREVIEWS -- a monochrome or three-sample raw at scale > 1), OpRotateCrop is a no-op, the orientation is Normal (or Unknown) --
 * or d->allow_fused has IPK_FUSED_BATCH_ORIENTED as well and OpTransform's image of the demosaic size is the negotiated result -- and the preview
 * has at least 256 pixels (the one-pass chain's floor, kept per frame).  0 otherwise, and the batch is n calls of ipk_pipeline_run as before; a negative
 * error code for a descriptor ipk_pipeline_sizes refuses.  *chunk (may be NULL; 0 when the answer is not 1) receives the frames per chunk,
 * min(64, max(1, 256 MiB / (demosaic_w * demosaic_h * 16))); *pass1_batched (may be NULL) 1 when a chunk's scaling pass is the general kernel's batch
 * launch (ipk_raw_scaled_demosaic_batch's rule on the 16-byte aligned scratch; every monochrome / three-sample raw), 0 when it is a launch per frame
 * (skips from 1 to 7 on a mosaic at least 8 samples wide; rasters).  Per chunk: pass 1 writes the chunk's RGBE previews into one scratch buffer, pass 2
 * runs ipk_pointwise_chain_out once per maximal run of frames whose destinations follow each other in memory (dsts[i + 1] == dsts[i] + demosaic_w *
 * demosaic_h * 3 samples) -- scattered destinations cost one chain launch per frame and nothing else; a chunk of one frame is ipk_pipeline_run.  Results
 * and *used_fused are what n calls of ipk_pipeline_run give.  ipk_timing names the stages "batch gofloat+demosaic" and
 * "batch to_lab+basecurve+from_lab+gamma+quantise" (without "+quantise" for f32).  An oriented descriptor (IPK_FUSED_BATCH_ORIENTED) has another
 * pass 2: ONE ipk_pointwise_chain_out_batch_oriented launch per chunk, every record with the descriptor's orientation, wherever the destinations lie,
 * named "batch to_lab+basecurve+from_lab+gamma+transform+quantise" (without "+quantise" for f32).  No GPU needed. */
IPK_API int ipk_pipeline_batches_previews(const ipk_pipeline_desc *d, int out_type, size_t n, size_t *chunk, int *pass1_batched);
/* The same over the DEVICE SET (ipk_init_devices) from one host thread: frame i runs on set member i mod N, so srcs[i] / dsts[i] must live on
 * that member's device.  Nothing is exchanged between devices and every result stays where it was computed (frames are independent pipelines,
 * src/pipeline.rs:246-249).  Enqueues on one internal stream per member and returns; ipk_devices_sync waits for all of them.  Without a device
 * set the current context takes every frame. */
IPK_API int ipk_pipeline_run_batch_multi(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n, int out_type,
                                         int *used_fused);
IPK_API int ipk_devices_sync(void);
/* n DEVICE frames, n descriptors: a shoot whose files carry their own colour settings (Pipeline::new_from_file per file, each Pipeline with its own ops,
 * src/pipeline.rs:246-284).  The results are bit for bit what ipk_pipeline_run(descs[i], srcs[i], dsts[i], ...) gives, called for i = 0 .. n - 1 in that
 * order on `stream`, and *used_fused (may be NULL) holds what the last frame's run leaves.  Every descriptor is validated as ipk_pipeline_run validates it
 * (and its curve is built) BEFORE anything is enqueued: an invalid descriptor or a null srcs[i] / dsts[i] fails with IPK_ERR_INVALID, names the index in
 * ipk_last_error and writes nothing.  n = 0 is IPK_OK.  The host arrays are read before the call returns.
 * The plan, which ipk_pipeline_batch_each_plan reports without a GPU (route[i], run_first[i]; either may be NULL): two descriptors are SAME-SHAPED when
 * every field is equal -- field by field, cfa as a string after the drivers' usual folding, floats by their bits, padding not at all -- except the fields
 * this rule lets differ.  struct_size, src_type, cpp, is_cfa, rotatecrop, maxwidth, maxheight, linear, allow_fused, use_fastpath, schedule and the fuse
 * flags always count.  So does one thing the five fields below decide themselves: ipk_pipeline_takes_fastpath (the raster fast path is taken for the
 * DEFAULT ops only), so a raster with default ops and an edited one are never same-shaped under IPK_OUT_U8 / IPK_OUT_U16, and every frame of a run is on
 * the route ipk_pipeline_run would choose for it.
 *   These FIVE may always differ: wb_coeffs, cam_to_xyz_normalized, exposure, npoints and points.
 *   These THREE may differ -- rotation, fliph and flipv: eight fields instead of five -- when BOTH descriptors carry IPK_FUSED_BATCH_ORIENTED beside
 *     IPK_FUSED_ON | IPK_FUSED_BATCH_PREVIEWS, each would batch its own previews (ipk_pipeline_batches_previews answers 1 for it) and both negotiate
 *     the same demosaic size (ipk_pipeline_sizes).  The demosaic size decides the scaling pass's filter; under one maxwidth alone a Rotate90 / Rotate270
 *     frame negotiates another one than a Normal frame (transform_forward swaps the sides before the clamp) and still cuts the run unless both carry
 *     IPK_FUSED_BATCH_SIZES (below), under a square box
 *     (maxwidth == maxheight) frames of equal source size agree, and fliph / flipv never enter the fold.
 *   These ELEVEN may differ -- the SENSOR fields: width, height, cfa, cfa_width, cfa_height, crop_top / right / bottom / left, blacklevels and
 *     whitelevels -- when BOTH descriptors carry IPK_FUSED_BATCH_SENSOR beside IPK_FUSED_ON | IPK_FUSED_BATCH_PREVIEWS, each would batch its own previews
 *     with the general scaling kernel's batch launch (ipk_pipeline_batches_previews answers 1 with pass1_batched = 1), both negotiate the same demosaic
 *     size and both agree in whether the filter has a fourth colour.  src_type, cpp and is_cfa count even then (they decide the kernel's instantiation, its
 *     layout and the chain's monochrome flag), as do maxwidth and maxheight.  A run whose frames differ in a sensor field is route 2: pass 1 of a chunk
 *     whose frames differ in them is ONE ipk_scaled_demosaic_batch_each launch, frame i's window, levels and filter from descriptor i's own negotiation,
 *     named "batch-each gofloat+demosaic"; a chunk whose frames agree in them is the uniform launch on the chunk's first descriptor, named
 *     "batch gofloat+demosaic"; pass 2 is what it is below.
 *   The "same demosaic size" of both conditions is waived for a pair when BOTH descriptors carry IPK_FUSED_BATCH_SIZES as well, each would batch its own
 *     previews and both have pass1_batched = 1 (the sized launch exists for the general kernel only).  Chunks are then cut greedily
 *     (ipk_pipeline_batch_each_chunks); pass 1 of a chunk whose frames differ in demosaic size is ONE ipk_scaled_demosaic_batch_sized launch, named
 *     "batch-each gofloat+demosaic", and pass 2 ONE ipk_pointwise_chain_out_batch_sized launch under the names below; a chunk whose sizes agree takes the
 *     launches above.
 * The two conditions are asked of a pair independently: it may meet either, both or neither.  The frames are cut, in order, into maximal runs of
 * consecutive same-shaped descriptors; run_first[i] is the first frame of frame i's run.  For a run of m frames:
 *   route 2, varied previews: m > 1, ipk_pipeline_batches_previews(descs[run_first], out_type, m, ...) answers 1 (so allow_fused needs IPK_FUSED_ON |
 *     IPK_FUSED_BATCH_PREVIEWS: no new bit) and the descriptors are not all equal in the five (eight) fields.  Chunks follow that report's chunk; pass 1 is the
 *     uniform route's pass 1 -- one set of levels, crops and filter per chunk, or under IPK_FUSED_BATCH_SENSOR the frame-table launch above -- and pass 2 is ONE ipk_pointwise_chain_out_batch launch per chunk: source i
 *     the scratch's slice i, parameters descriptor i's, destination dsts[i] wherever it lies (scattered destinations cost nothing here).  A final chunk
 *     of one frame is ipk_pipeline_run.  ipk_timing names the stages "batch gofloat+demosaic" and "batch-each to_lab+basecurve+from_lab+gamma+quantise"
 *     (without "+quantise" for f32); a chunk with at least one oriented frame is ONE ipk_pointwise_chain_out_batch_oriented launch, frame i with its
 *     descriptor's composed orientation and dsts[i] of its own final size, named "batch-each to_lab+basecurve+from_lab+gamma+transform+quantise";
 *   route 1, uniform: otherwise, inside the run, maximal sub-runs of two or more consecutive descriptors that are equal in the five (eight) fields as well go
 *     to ipk_pipeline_run_batch -- a run on the varied route's ground whose five fields happen to be all equal included -- which keeps the persistent
 *     full-size launch and the uniform preview batch for callers who happen to have them;
 *   route 0, single: every other frame, through ipk_pipeline_run.
 * Out of scope: per-frame settings inside the persistent full-size launch ipk_raw_to_srgb_batch (one parameter set; full-size frames with varied
 * settings are route 0 each); per-frame preview sizes without IPK_FUSED_BATCH_SIZES (they cut the run), per-frame maxwidth / maxheight (they always do); non-Normal orientations without IPK_FUSED_BATCH_ORIENTED and active
 * rotatecrops inside a varied run (ipk_pipeline_batches_previews answers 0: frame by frame, or route 1 where identical); the host-buffer batch drivers;
 * the multi-device driver (it may follow by calling this one member by member); band forms; the bit as a default; graph capture (the table upload of
 * ipk_pointwise_chain_out_batch is a copy from pageable host memory).
 * Measured (profiles/r20_batch_each.txt; device-resident noise frames to u8, every frame with its own wb_coeffs and exposure, wall clock, medians, ms per
 * frame; the parent build's only offer -- a loop of ipk_pipeline_run, two launches per frame -- -> this call with the bit set | this build's uniform
 * ipk_pipeline_run_batch on one descriptor; the parent's spread is 0.0003 .. 0.0034 ms throughout): 24 MP RGGB u16 -> 256 wide, n = 2 / 8 / 16 / 64:
 * 0.212 -> 0.116 | 0.114, 0.220 -> 0.055 | 0.053, 0.219 -> 0.066 | 0.064, 0.218 -> 0.053 | 0.052; -> 400 wide: 0.124 -> 0.085 | 0.083, 0.124 -> 0.065 |
 * 0.063, 0.123 -> 0.060 | 0.058, 0.122 -> 0.056 | 0.055; 50 MP X-Trans u16 -> 270 wide: 0.378 -> 0.227 | 0.225, 0.391 -> 0.174 | 0.172, 0.390 -> 0.155 |
 * 0.153, 0.389 -> 0.144 | 0.144; 24 MP mono u16 -> 256 wide: 0.143 -> 0.080 | 0.078, 0.154 -> 0.050 | 0.049, 0.153 -> 0.062 | 0.061, 0.153 -> 0.052 |
 * 0.051.  No measured case at n >= 8 was slower than the parent's loop; none is excluded.  The distance to the uniform batch (the table upload and the
 * per-frame staging) is +0.001 .. +0.003 ms per frame at n <= 16 and within 0.0005 ms at n = 64.  With the bit clear the call is the parent's loop plus
 * the plan, and that shows: up to 0.0018 ms per frame above the parent's loop (0.1248 against 0.1230 at n = 16, 400 wide), OUTSIDE the parent's spread in
 * several readings (400 wide: +0.0017 at n = 8 against a spread of 0.0012, +0.0018 at n = 16 against 0.0008, +0.0015 at n = 64 against 0.0003; 256
 * wide: +0.0015 at n = 16 against 0.0006, +0.0012 at n = 64 against 0.0005; mono: +0.0007 at n = 64 against 0.0003).  A caller without the bit loses that much against its own loop.  The carriers' launches outside the mode stayed inside the
 * parent's spread: ipk_pointwise_chain_out at 2160x1440 to f32 0.0400 -> 0.0398 ms, to u8 0.0397 -> 0.0389; at 6000x4000 to f32 0.2013 -> 0.1970, to u8
 * 0.1777 -> 0.1807 (spread 0.0041); the cached-region gather launch over 1/16 of a 24 MP frame to u8 0.0447 -> 0.0446.  Not measured: f32 sources, f32
 * and 16-bit outputs, scattered destinations, per-frame matrices and curves, batches above 64 frames, rasters and the window-8 geometries, mixed
 * batches, photo-like data. */
IPK_API int ipk_pipeline_run_batch_each(const ipk_pipeline_desc *const *descs, const void *const *srcs, void *const *dsts,
                                        size_t n, int out_type, int *used_fused, void *stream);
/* host-only, no GPU: the plan the call above follows.  IPK_ERR_INVALID for a null or invalid descriptor (the index is named in ipk_last_error) */
IPK_API int ipk_pipeline_batch_each_plan(const ipk_pipeline_desc *const *descs, size_t n, int out_type,
                                         int *route /* n */, size_t *run_first /* n */);
/* host-only, no GPU: the chunks that plan is executed in -- chunk_first[i] is the first frame of the chunk frame i runs in (the frames that share one
 * scratch and one pair of launches).  A route-2 run, and a route-1 run that batches its previews, are cut greedily in order: a chunk grows while it has
 * fewer than 64 frames and its RGBE previews sum to at most 256 MiB (for frames of one size: ipk_pipeline_batches_previews' chunk).  Every other frame is
 * its own.  Validation is ipk_pipeline_batch_each_plan's; nothing is allocated for the frames */
IPK_API int ipk_pipeline_batch_each_chunks(const ipk_pipeline_desc *const *descs, size_t n, int out_type, size_t *chunk_first /* n */);
/* HOST frames in, HOST results out, over the device set: the drop-in for a caller looping Pipeline::run / output_8bit over a shoot on a
 * multi-GPU node.  One host thread per member runs ipk_host_pipeline_run_batch on the frames dealt to it (frame i -> member i mod N), so all
 * GPUs upload, compute and download concurrently; the caller's Vecs are the "gather".  Synchronous at return; results are what n calls of
 * ipk_host_pipeline_run give.  Use ipk_host_alloc buffers (page-locked and visible to every device). */
IPK_API int ipk_host_pipeline_run_batch_multi(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n,
                                              int out_type, int *used_fused);
/* Page-locked host memory for the buffers handed to the ipk_host_* entry points (NULL on failure). */
IPK_API void *ipk_host_alloc(size_t bytes);
IPK_API void ipk_host_free(void *p);

/* ---------------------------------------------------------------------------------------- */
/* Stage-boundary caching contract of Pipeline::run(Some(cache)) (src/pipeline.rs:341-372;    */
/* BufHasher src/hasher.rs:12-48; PipelineCache = MultiCache<BufHash, OpBuffer>, :43,258-260)  */
/* ---------------------------------------------------------------------------------------- */

/* The eight chained op hashes (32 bytes each, op order gofloat..transform) Pipeline::run computes after
 * size negotiation: hash i covers PipelineSettings and ops 0..i, so editing op k changes hashes k..7 only.
 * out_type selects the `linear` the settings carry (output_8bit / output_16bit force it).  source_id is an
 * extension: the reference hashes nothing that identifies the image; a nonzero id lets one cache hold the
 * buffers of several resident frames.  Host-only. */
IPK_API int ipk_pipeline_hashes(const ipk_pipeline_desc *d, int out_type, uint64_t source_id, uint8_t *out256);

/* Pipeline::new_cache(size): a byte-budgeted LRU of device OpBuffers.  `get` refreshes recency; `put` evicts
 * least-recently-used entries until the newcomer fits.  Use one stream per cache.
 * Threads: the bookkeeping is internally locked -- contains, stats, get, clear and the puts (ipk_pipeline_run_cached, ipk_selftest_cache_put) may be
 * called on one cache from several threads at once (tests/cpp/host_threads.cpp does, under ThreadSanitizer).  ipk_cache_free must not run while
 * another call on the same cache is in flight, and a pointer borrowed with ipk_cache_get lives only until another thread's put evicts its entry. */
typedef struct ipk_cache ipk_cache;
IPK_API int ipk_cache_new(size_t max_bytes, ipk_cache **out);
IPK_API int ipk_cache_free(ipk_cache *cache);
IPK_API int ipk_cache_clear(ipk_cache *cache);
IPK_API int ipk_cache_contains(const ipk_cache *cache, const uint8_t *key32);                 /* 1 / 0 */
IPK_API int ipk_cache_stats(const ipk_cache *cache, size_t *bytes, size_t *entries, uint64_t *hits, uint64_t *misses, uint64_t *evictions);
/* Borrow a memoised buffer (IPK_NOOP when absent).  The pointer stays valid until the entry is evicted. */
IPK_API int ipk_cache_get(ipk_cache *cache, const uint8_t *key32, const float **data, size_t *width, size_t *height,
                          size_t *colors, int *monochrome);

/* Pipeline::run / output_8bit / output_16bit with Some(cache): resumes after the last op whose hash is in the
 * cache, stores every buffer it materialises under that op's hash, writes the final image to the DEVICE buffer
 * dst.  *ops_run (may be NULL) = bit i set when op i executed (0 = served from the cache).  With nothing
 * memoised and a fusable chain the whole run is one ipk_raw_to_srgb launch and only the final buffer is stored.
 * The order of the cache traffic: one `get` per hash, 0 to 7 in that order, each hit refreshed as it is found (the last hit wins), then one `put` per
 * executed op in op order; where gofloat + demosaic run as one pass, hash 0 is never stored. */
IPK_API int ipk_pipeline_run_cached(const ipk_pipeline_desc *d, const void *src, uint64_t source_id, ipk_cache *cache,
                                    int out_type, void *dst, int *ops_run, int *used_fused, void *stream);

/* A region from the cache (an editor's loop: a slider moves, the viewport is redrawn).  Everything behind OpRotateCrop is point-wise or OpTransform's
 * dihedral permutation, so the buffer memoised under the rotatecrop hash (op 2: the 4-channel image Pipeline::run hands to OpToLab; a no-op rotatecrop
 * stores its input under that key) is all a region needs: the region is a strided rectangle of it.
 * ipk_pipeline_region_gather (host-only, no GPU) says where: region pixel (i, j) -- column i, row j of region (x, y, w, h) of the final result -- is pixel
 * base + i * x_step + j * y_step of that buf_w x buf_h buffer (steps in pixels, signed: a plain rectangle has x_step 1 and y_step buf_w, the flips
 * negate one or both, the transposing orientations swap them).  Empty or outside regions and refused descriptors fail with IPK_ERR_INVALID as in
 * ipk_pipeline_region. */
IPK_API int ipk_pipeline_region_gather(const ipk_pipeline_desc *d, int out_type, size_t x, size_t y, size_t w, size_t h,
                                       size_t *buf_w, size_t *buf_h, int64_t *base, int64_t *x_step, int64_t *y_step);
/* Writes the region's w*h*3 packed samples of out_type to the DEVICE buffer dst, bit-identical to that rectangle of ipk_pipeline_run_cached's result for
 * the same descriptor.  Checks and hash chain as in ipk_pipeline_run_cached.
 *   - fast path (ipk_pipeline_takes_fastpath = 1): the fast-path result is computed and the rectangle copied out; *windowed = 0, *ops_run = 0, the cache
 *     is not consulted.
 *   - the final buffer (hash 7) is memoised: the rectangle is cut from it (one 2-D copy; for 8 / 16 bits the copy, then the quantisation of the
 *     rectangle); *windowed = 0, *ops_run = 0.
 *   - otherwise the cache is brought up to op 2 -- the latest hit among hashes 0..2, then the missing ones of gofloat, demosaic and rotatecrop over the
 *     whole frame, exactly as ipk_pipeline_run_cached runs and stores them -- and ONE launch over the region computes to_lab..gamma with OpTransform folded
 *     into its loads (and output8bit / output16bit in the same launch; a region of fewer than 256 pixels takes the f32 launch plus the quantisation of the
 *     rectangle).  The transposing orientations (Transpose, Rotate90, Rotate270, Transverse) take two launches from 256 pixels up -- the same launch over
 *     the unrotated rectangle, then OpTransform's permutation of the rectangle: folded into the loads, a transposing walk reads one cache line per
 *     lane and measured 3.3x the plain rectangle's time.  *windowed = 1; *ops_run has bit i set for every op executed, whole-frame (0..2) or on the rectangle (3..7 without the reference's no-ops:
 *     a no-op curve, linear gamma, a no-op transform).  Nothing computed on the rectangle enters the cache.
 * The whole-frame one-launch shortcut ipk_pipeline_run_cached takes with nothing memoised is NOT taken here: the point of this call is that the next edit
 * finds the RGBE buffer.  Hits at hashes 3..6 are not used either: entering at the RGBE buffer is one launch whatever lies behind it.
 * The order of the cache traffic: a `get` of hash 7; on a miss, where the resampling route below is open, a `contains` of hash 2, which refreshes nothing,
 * counts neither a hit nor a miss and chooses between that route and the gather above; then a `get` per hash 0..2 (0..1 on the resampling route) in that order and a `put`
 * per executed whole-frame op in op order.
 * The borrowed buffer may be evicted once the call has returned; freeing it waits for the device, so the enqueued launch is safe.
 * ipk_timing_begin/end see "region to_lab+basecurve+from_lab+gamma+transform" (and "quantise" where it is separate; the two-launch form: "region
 * to_lab+basecurve+from_lab+gamma", then "transform").  No host-pointer or batch form.
 * Measured (profiles/r15_cached_region.txt; one exposure edit and the region redrawn, wall clock, 1/16 / 1/4 / the whole area) against what the parent
 * build offers for the same edit -- A: ipk_pipeline_run_cached + a 2-D copy, B: ipk_pipeline_run_region without a cache:
 *   24 MP RGGB u16 -> f32, Normal     0.041 / 0.075 / 0.207 ms    A 0.99 / 1.04 / 1.11     B 0.046 / 0.061 / 0.143
 *   24 MP RGGB u16 -> f32, Rotate180  0.041 / 0.080 / 0.210       A 1.33 / 1.36 / 1.44     B 0.055 / 0.086 / 0.258
 *   24 MP RGGB u16 -> f32, Rotate90   0.051 / 0.106 / 0.319       A 1.3 - 17 (allocations) B 0.056 / 0.091 / 0.263
 *   50 MP X-Trans -> 2160x1440 f32    0.031 / 0.035 / 0.049       A 0.111 / 0.113 / 0.117  B 0.045 / 0.059 / 0.101
 *   the same, Rotate90 (2160x3240)    0.037 / 0.052 / 0.107       A 0.21 / 0.95 / 8.1      B 1.06 / 1.07 / 1.10
 * (u8: within 10 % of these.)  Always faster than A (2.2x - 160x).  NOT faster than B where B is the one raw->sRGB window launch of a full-resolution
 * Bayer frame, which reads 2 bytes per pixel where this call reads 16: Normal and Rotate90 from a quarter of the area up (0.69 - 0.90 of B's speed);
 * such a caller is better served by ipk_pipeline_run_region.  On the staged routes (previews, and everything at an angle) it is 1.4x - 28x B.
 * The flat launches of the touched kernels (ipk_pointwise_chain, ipk_pointwise_chain_out) stayed within the parent's run-to-run spread, 0 - 3 % behind it.
 * Not measured: 16-bit outputs, the other flips and transposing orientations, regions below 256 pixels, photo-like data. */
IPK_API int ipk_pipeline_run_cached_region(const ipk_pipeline_desc *d, const void *src, uint64_t source_id, ipk_cache *cache,
                                           size_t x, size_t y, size_t w, size_t h, void *dst, int out_type,
                                           int *ops_run, int *windowed, void *stream);
/* IPK_FUSED_CACHED_RESAMPLE: a crop or straighten edit changes hash 2, and the call above then runs OpRotateCrop over the WHOLE frame (16 bytes read and
 * written per pixel) before it gathers the rectangle -- and stores a buffer the next step of the slider invalidates.  With the bit (beside IPK_FUSED_ON)
 * the call takes another route, behind its fast-path and hash-7 branches, when hash 2 is NOT memoised and ipk_pipeline_resamples_cached_region answers 1:
 *   - the cache is brought up to op 1 only (the latest hit among hashes 0..1, then the missing ones of gofloat and demosaic over the whole frame, run and
 *     stored as ipk_pipeline_run_cached does, the one-pass gofloat + demosaic of scaled previews included);
 *   - ONE launch computes the region's unrotated rectangle of OpRotateCrop's result straight from that buffer and runs to_lab..gamma and the
 *     quantisation on it: k_fused_resample's cached-buffer source mode (launch log: k_fused_resample<float, OUT>[fast_ok=,win=1,rgbe=1]), the window walk
 *     of transform_buffer tap for tap, zero-weight taps accumulated (0 * inf stays NaN), bit-identical to the staged result;
 *   - every orientation but Normal computes the plain rectangle into scratch and runs OpTransform's permutation on it (two launches);
 *   - *windowed = 1; *ops_run = the whole-frame ops executed (bits 0..1), bit 2, and bits 3..7 as on the gather route; nothing computed on the rectangle
 *     enters the cache, so hash 2 stays absent.
 * With hash 2 memoised the gather launch above runs as ever: one tap per pixel instead of up to nine.
 * THE TRADE-OFF: while the bit is set this call never fills hash 2, so every later point-wise edit (white balance, curve, exposure) pays the resample
 * again.  A caller whose crop / straighten slider has come to rest fills it with ipk_pipeline_run_cached, or with one region call that leaves the bit out.
 * ipk_timing_begin/end see "region rotatecrop+to_lab+basecurve+from_lab+gamma" (then "transform" for the other orientations).
 * ipk_pipeline_resamples_cached_region (host-only, no GPU): would the call take that route with hash 2 absent?  1 when allow_fused has IPK_FUSED_ON and
 * IPK_FUSED_CACHED_RESAMPLE set, the frame does not take the fast path, OpRotateCrop is not a no-op and accepts its crops on the buffer OpDemosaic hands
 * it (the negotiated demosaic size where OpDemosaic scales, else the cropped source), the source is not a CFA mosaic whose filter has a fourth colour
 * (E is +0.0 in every other 4-channel buffer in front of OpRotateCrop, which the launch relies on), and the launch admits the transform (windows of at most
 * 3x3: |skip| sums below 2 per axis, sides below 2^24).  Three-colour mosaics of any pattern at any scale, monochrome and three-sample raws (u16 and f32)
 * and RGB8 / RGB16 rasters are all admitted.  0 otherwise; a negative error code for a descriptor ipk_pipeline_sizes refuses.
 * Measured (profiles/r16_cached_resample.txt; one straighten step that keeps hash 1 and the region redrawn, wall clock, the fastest run of 60, 1/16 / 1/4 /
 * the whole area) against what the parent build offers for the same step -- A: this call without the bit, B: ipk_pipeline_run_region without a cache, every
 * window bit on (at an angle B is never the one launch: the size fold lands a pixel short):
 *   24 MP RGGB u16 -> f32             0.057 / 0.130 / 0.428 ms    A 0.824 / 0.835 / 0.942    B 1.432 / 1.488 / 1.643
 *   24 MP RGGB u16 -> u8              0.057 / 0.123 / 0.396       A 0.833 / 0.869 / 0.983    B 1.452 / 1.489 / 1.618
 *   50 MP X-Trans -> 2160x1440 u8     0.039 / 0.046 / 0.084       A 0.306 / 0.333 / 0.348    B 0.182 / 0.186 / 0.202
 *   24 MP RGB8 raster -> u8           0.051 / 0.113 / 0.361       A 0.826 / 0.832 / 0.944    B 0.947 / 0.987 / 1.129
 * 2.2x - 16x over A, 2.4x - 25x over B; no measured step was slower.  (Medians agree wherever no run of a case stalled; the file has both.)  NOT
 * measured, and not expected to win: a crop-only edit of a full-size Bayer u16 frame, where B is the raw window launch reading 2 bytes per pixel (0.028 ms
 * for 1920x1080, profiles/r12_region_windows.txt) and this call reads 16.  A step that moves the negotiated demosaic size by a pixel changes every hash
 * (the settings are hashed): the whole chain runs again with the bit or without it; of the angles 0.02 + k * 0.00001 the first 256 kept hash 1 on the
 * full-size frames, 43 of 20 000 on the preview.  The kernel's mosaic mode against the parent: whole frames and windows within the parent's spread except
 * two readings, f32 -> f32 crop 5 % at 100 MP 1.740 -> 1.771 ms (spread 0.015) and the 256x256 window of the scale-1.5 preview to u8 0.0250 -> 0.0267 ms
 * (spread 0.0014); the f32 whole frames are 1.0 - 1.8 % behind the parent, the u16 ones between 1.1 % ahead and 0.6 % behind. */
IPK_API int ipk_pipeline_resamples_cached_region(const ipk_pipeline_desc *d, int out_type);

/* ---------------------------------------------------------------------------------------- */
/* Multi-GPU: one process per GPU; a frame batch shards with no exchange (frame i -> rank i mod N, */
/* src/pipeline.rs:246-249), ONE frame shards by row bands                */
/* ---------------------------------------------------------------------------------------- */

/* One rank's row band.  Full-resolution path (ipk_raw_to_srgb's band_* fields): output rows [out_row0, +out_rows) of the cropped
 * frame, and the source rows [src_row0, +src_rows) its slab must hold = the band plus the 1-row halos demosaic::full taps
 * (src/ops/demosaic.rs:70-74) where they lie inside the frame.  Scaled path: out_* count rows of the nwidth x nheight result and
 * src_* the source rows its windows read (src/scaling.rs:84-94). */
typedef struct { size_t out_row0, out_rows, src_row0, src_rows; } ipk_band;

/* Row bands of near-equal size whose boundaries are multiples of the CFA period (2 Bayer, 6 X-Trans, 12), so every band starts
 * at the frame's CFA phase.  bands[nranks].  Host-only. */
IPK_API int ipk_band_plan(size_t height, int nranks, int cfa_period, ipk_band *bands);
/* Output-row bands of scaling::scaled_demosaic (src/scaling.rs:132-145) from width x height to nwidth x nheight: rank k produces
 * output rows [out_row0, +out_rows) and needs source rows floor(skip*r0) .. floor(skip*r1) (:84-87, clamped to the frame) --
 * neighbouring ranks' source ranges overlap by a window, nothing is exchanged.  Host-only. */
IPK_API int ipk_band_plan_scaled(size_t height, size_t nheight, int nranks, ipk_band *bands);
/* ipk_raw_scaled_demosaic for one band of ipk_band_plan_scaled: `src` points at the slab's first row (sensor row y + band->src_row0,
 * column 0 of the sensor frame), dst4 receives band->out_rows x nwidth RGBE pixels.  Bit-identical to the same rows of the whole frame. */
IPK_API int ipk_raw_scaled_demosaic_band(const void *src, int src_type, size_t owidth, size_t x, size_t width, size_t height,
                                         float black0, float white0, const char *cfa, size_t nwidth, size_t nheight,
                                         const ipk_band *band, float *dst4, void *stream);

/* A communicator over the ranks that share one frame.  Two transports behind the same entry points:
 *   RCCL   (ipk_comm_init_rccl): ncclSend/ncclRecv/ncclAllGather on device buffers over xGMI -- the product path on a multi-GPU node;
 *   host   (ipk_comm_init_host): the caller's own messaging (MPI, gloo, a socket) moves the bytes, staged through host memory --
 *          for hosts that already have a fabric of their own, and for ranks that share ONE GPU (RCCL refuses two ranks per device).
 * Nothing here touches pixels: results are bit-identical to the unsharded run by construction of the band kernels. */
typedef struct ipk_comm ipk_comm;
#define IPK_COMM_ID_BYTES 128
/* ncclGetUniqueId on one rank; the caller hands the 128 bytes to every rank by its own means (it has to rendezvous anyway) */
IPK_API int ipk_comm_unique_id(uint8_t *id128);
/* ncclCommInitRank on the device ipk_init bound.  Collective over the nranks processes. */
IPK_API int ipk_comm_init_rccl(const uint8_t *id128, int rank, int nranks, ipk_comm **out);
/* Host transport.  exchange(ctx, send_peer, send, send_bytes, recv_peer, recv, recv_bytes) must send `send` to send_peer and
 * receive recv_bytes from recv_peer into `recv` (either peer may be -1 = none), returning 0 on success; it may block until both
 * complete (MPI_Sendrecv semantics).  Buffers are host memory. */
typedef int (*ipk_exchange_fn)(void *ctx, int send_peer, const void *send, size_t send_bytes, int recv_peer, void *recv, size_t recv_bytes);
IPK_API int ipk_comm_init_host(int rank, int nranks, ipk_exchange_fn exchange, void *ctx, ipk_comm **out);
IPK_API int ipk_comm_free(ipk_comm *comm);
/* transport: 0 RCCL, 1 host */
IPK_API int ipk_comm_info(const ipk_comm *comm, int *rank, int *nranks, int *transport);
/* Halo exchange of the full-resolution path, in place on the slab (device memory, row pitch row_bytes, rows = bands[rank].src_rows):
 * the band's first / last own row goes to the neighbour above / below, their edge rows arrive in the slab's halo rows.  RCCL: one
 * ncclGroup of ncclSend/ncclRecv on `stream` (asynchronous); host transport: synchronous.  Bands with no rows are skipped. */
IPK_API int ipk_band_exchange_halo(ipk_comm *comm, void *slab, size_t row_bytes, const ipk_band *bands, void *stream);
/* The same on a HOST slab (host transport only; what a caller does before uploading its band). */
IPK_API int ipk_host_band_exchange_halo(ipk_comm *comm, void *slab, size_t row_bytes, const ipk_band *bands);
/* Reassembles the result IN PLACE: `frame` is the full out_height x out_row_bytes image on every receiving rank, and each rank's
 * kernel has already written its own band at its rows (dst = frame + bands[rank].out_row0 * out_row_bytes).  root = -1: every rank
 * receives every band (ncclAllGather when the bands are equal, one group of ncclSend/ncclRecv straight into place otherwise: the xGMI
 * mesh is point-to-point, all peers at once); root >= 0: only that rank receives.  Any element type: sizes are bytes. */
IPK_API int ipk_band_gather(ipk_comm *comm, void *frame, size_t out_row_bytes, const ipk_band *bands, int root, void *stream);
/* The same on a HOST frame (host transport only). */
IPK_API int ipk_host_band_gather(ipk_comm *comm, void *frame, size_t out_row_bytes, const ipk_band *bands, int root);
/* The gather on the communicator's own stream, ordered after the work `after_stream` holds now: frame k's gather overlaps frame
 * k+1's kernel.  ipk_comm_wait makes `stream` wait for the gathers begun so far (no host block). */
IPK_API int ipk_band_gather_begin(ipk_comm *comm, void *frame, size_t out_row_bytes, const ipk_band *bands, int root, void *after_stream);
IPK_API int ipk_comm_wait(ipk_comm *comm, void *stream);
/* Transport self-check: a ring send/recv and an all-gather of a known pattern on device buffers, verified on the host.  Collective. */
IPK_API int ipk_comm_selftest(ipk_comm *comm);

/* ---------------------------------------------------------------------------------------- */
/* Host-pointer forms of the stage kernels: what a Rust `impl ImageOp::run` binds when it keeps   */
/* its OpBuffers in host Vec<f32>s.  Same arguments as the device forms, minus the stream.       */
/* ---------------------------------------------------------------------------------------- */
IPK_API int ipk_host_gofloat_cfa_u16(const uint16_t *src, size_t owidth, size_t oheight, size_t x, size_t y, size_t width, size_t height,
                                     float black0, float white0, float *dst);
IPK_API int ipk_host_gofloat_cfa_f32(const float *src, size_t owidth, size_t oheight, size_t x, size_t y, size_t width, size_t height,
                                     float black0, float white0, float *dst);
IPK_API int ipk_host_demosaic_full(const float *src, size_t width, size_t height, const char *cfa, float *dst4);
IPK_API int ipk_host_transform_buffer_f32(const float *src, size_t width, size_t height,
                                          int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                          size_t nwidth, size_t nheight, size_t components, const char *cfa, float *dst);
IPK_API int ipk_host_tolab(const float *src4, size_t width, size_t height, int monochrome,
                           const float *wb_coeffs, const float *cam_to_xyz_normalized, float *dst3);
IPK_API int ipk_host_basecurve(const float *src3, size_t width, size_t height, float exposure,
                               const float *points, int npoints, float *dst3);
IPK_API int ipk_host_fromlab(const float *src3, size_t width, size_t height, float *dst3);
IPK_API int ipk_host_gamma(const float *src, size_t width, size_t height, size_t colors, int linear, float *dst);
IPK_API int ipk_host_rotate_buffer(const float *src3, size_t width, size_t height, int orientation,
                                   float *dst3, size_t *out_width, size_t *out_height);
IPK_API int ipk_host_output8bit(const float *src, size_t n, uint8_t *dst);
IPK_API int ipk_host_output16bit(const float *src, size_t n, uint16_t *dst);
IPK_API int ipk_host_raw_to_srgb(const ipk_fused_params *p, const void *src, void *dst);

/* ---------------------------------------------------------------------------------------- */
/* Self-test hooks: on-device, exhaustive checks that the arithmetic shortcuts of the fused     */
/* kernel reproduce the plain IEEE expressions of the reference (used by tests/, not by callers) */
/* ---------------------------------------------------------------------------------------- */
/* x / c (src/color_conversions.rs:158,168,177-179,184-187; src/ops/gofloat.rs:126) versus the kernel's
 * multiply/fma forms, over every f32 x with lo <= |x| <= hi (and 0/inf/NaN if include_special).
 * variant 0: cdiv_fast incl. v_div_fixup; 1: the three arithmetic steps; 2: two steps, hi/lo reciprocal. */
IPK_API int ipk_selftest_cdiv(float c, int variant, float lo, float hi, int include_special,
                              uint64_t *n_bad, uint32_t *first_bad_bits);
/* pos - pos.trunc() (src/color_conversions.rs:108-109) versus v_fract_f32 for every pos in [0, 8192] */
IPK_API int ipk_selftest_lut_weight(uint64_t *n_bad, uint32_t *first_bad_bits);
/* v.max(0.0).min(1.0) (src/ops/gamma.rs:22) versus v_med3_f32(v,0,1) for every f32 */
IPK_API int ipk_selftest_clamp01(uint64_t *n_bad, uint32_t *first_bad_bits);
/* Measurement aid, no counterpart in the reference: a plain device-to-device copy, 16 bytes per lane, as the practical HBM ceiling next to which
 * bench.py reports the kernels' achieved bandwidth (SURVEY.md 8d asks for the measured copy / triad ceiling beside the 8 TB/s spec peak). */
IPK_API int ipk_copy_probe(const void *src, void *dst, size_t bytes, void *stream);
/* The same for the fused path's read : write mix: src_bytes read, 3 * src_bytes written (4 : 12 bytes per pixel, f32 mosaic -> f32 RGB), flat launch,
 * contiguous, nontemporal, no arithmetic: the ceiling of ANY kernel with that traffic (bench.py roofline.mix_ceiling_GBps).  dst holds 3 * src_bytes;
 * src_bytes a multiple of 4096 (whole blocks of 256 lanes x 16 bytes), both pointers 16-byte aligned. */
IPK_API int ipk_mix_probe(const void *src, void *dst, size_t src_bytes, void *stream);
/* Measurement aid: the shader clock WHILE other work runs.  One wave on `stream` spins for spin_us microseconds of the fixed 100 MHz reference counter
 * (s_memrealtime) and writes {shader-clock cycles (s_memtime), reference ticks} over that span to out2_dev (two uint64 in device memory): clock in GHz =
 * out2[0] / out2[1] / 10.  bench.py launches it on a second stream beside the kernel under test (config.shader_clock_GHz), so that a slower box and a
 * slower kernel can be told apart. */
IPK_API int ipk_clock_probe(uint64_t *out2_dev, uint32_t spin_us, void *stream);
/* Measurement aid, no counterpart in the reference: the memory skeleton of ipk_raw_to_srgb as a launch of its own -- the same persistent launch and
 * task walk, the same row loads, OpGoFloat normalisation (src/ops/gofloat.rs:126), demosaic::full (src/ops/demosaic.rs:67-119), LDS staging and
 * nontemporal stores, WITHOUT OpToLab..OpGamma: dst receives the demosaiced R, G, B channels (the first three of demosaic::full's RGBE pixel) as
 * width*height*3 f32 samples, whatever p->out_type says.  4 (u16: 2) bytes in and 12 out per pixel on the fused kernel's own access pattern:
 * bench.py times it in the same session as the fused kernel and reports roofline.ceiling_ms / frac_of_ceiling from it.  Whole Bayer frames of at
 * least 256 columns with levels the fast normalisation is validated for; IPK_ERR_UNSUPPORTED otherwise. */
IPK_API int ipk_stream_probe(const ipk_fused_params *p, const void *src, void *dst, void *stream);
/* SplineFunc::interpolate (src/ops/curves.rs:126-157) on every f32 against the form the fused kernels use for a base curve of 2 or 3 knots (lower
 * clamp and exact knot hit as arithmetic, ipk_device.hpp spline_interpolate_3a); the curve is given like ipk_basecurve's.  IPK_ERR_UNSUPPORTED when
 * the kernels would not use that form for this curve (more knots, a knot ordinate of -0.0, non-finite coefficients). */
IPK_API int ipk_selftest_spline3(float exposure, const float *points, int npoints, uint64_t *n_bad, uint32_t *first_bad_bits);
/* output8bit (src/color_conversions.rs:323-326) on every f32 against a cheaper form: variant 0 v_cvt_pk_u8_f32(v*256), 1 the same of
 * floor(v*256), 2 min(saturating v_cvt_u32_f32(v*256), 255) -- the form the kernels use must report 0 mismatches */
IPK_API int ipk_selftest_quant8(int variant, uint64_t *n_bad, uint32_t *first_bad_bits);
/* OpGamma's step followed by output8bit (src/ops/gamma.rs:22, src/color_conversions.rs:323-326) on every f32, against the ONE-lookup form the 8-bit
 * output kernels run: clamp, then k_i + (c >= t_i) from a table of 8192 {k, threshold} steps built on the device from the gamma table (inside one of its
 * segments the quantised value changes at most once, and every operation on the way is monotone). */
IPK_API int ipk_selftest_q8(uint64_t *n_bad, uint32_t *first_bad_bits);
/* output16bit = (v*65535.0).round().max(0.0).min(65535.0) as u16 (src/color_conversions.rs:327-330; f32::round rounds halves away from zero) against the
 * form the kernels pack their 16-bit output with -- floor(v*65535 + 0.5) through the saturating v_cvt_u32_f32 and v_cvt_pk_u16_u32 -- on every f32. */
IPK_API int ipk_selftest_quant16(uint64_t *n_bad, uint32_t *first_bad_bits);
/* the device cbrtf routines (variant 0 literal glibc port, 1 select form, 2 form for 1<x<2) on a device array;
 * callers compare with the host libm's cbrtf (src/color_conversions.rs:123 -> f32::cbrt) */
IPK_API int ipk_selftest_cbrtf(const float *in, float *out, size_t n, int variant, void *stream);
/* test hook of the row-walking kernels' launch schedule: enabled = 0 makes every following launch run as if its stream could get no task-queue slot
 * (the queue-less static schedule: every wave walks the tasks of its index, a whole round of waves apart); 1 restores the queues.  The results
 * are the same bits either way -- which is what tests/test_gpu_fused.py checks for launches that hold more tasks than the chip has waves. */
IPK_API int ipk_selftest_task_queue(int enabled);
/* test hook, host side only: the launch log.  ipk_selftest_launch_log(1) clears the log and starts recording which of the library's kernels are
 * launched (process-wide, any thread, any stream; legal under stream capture); (0) clears it and stops -- a launch then costs one atomic load.
 * ipk_selftest_launch_log_read copies the log into buf (cap bytes, NUL-terminated, truncated when too small) and returns the bytes a complete read
 * needs, terminator included; buf = NULL or cap = 0 only asks for that size.  One line per distinct entry, sorted: the kernel's code-object symbol
 * (mangled), followed by [key=value,...] where the launcher's behaviour also depends on a host-known switch (imagepipe_amd/csrc/ipk_launch.hpp lists
 * the tags).  Both may be called before ipk_init: the log is then empty (one byte, the terminator). */
IPK_API int ipk_selftest_launch_log(int enabled);
IPK_API size_t ipk_selftest_launch_log_read(char *buf, size_t cap);
/* host-side test hooks of the caching contract: LRU bookkeeping without device memory; SHA-256 known answers */
IPK_API int ipk_selftest_cache_put(ipk_cache *cache, const uint8_t *key32, size_t bytes);
IPK_API int ipk_selftest_sha256(const void *data, size_t n, uint8_t *out32);

#ifdef __cplusplus
}
#endif
#endif /* IMAGEPIPE_AMD_H */
