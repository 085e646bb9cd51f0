// ipk_api.cpp -- the C ABI (include/imagepipe_amd.h): context, host-side parameter preparation,
// the Pipeline::run driver and the host-pointer wrappers.  No device code here; kernels are
// reached through ipk_launch.hpp.  There is deliberately no CPU implementation of any pixel
// loop in this file: without a GPU every compute entry point fails with IPK_ERR_NO_DEVICE.
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstddef>
#include <cstring>
#include <atomic>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <thread>
#include <vector>

#include "../../include/imagepipe_amd.h"
#include "ipk_hash.hpp"
#include "ipk_host.hpp"
#include "ipk_internal.hpp"
#include "ipk_launch.hpp"

namespace {

thread_local char g_err[512] = "";
int fail(int code, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}
#define HIPCHK(expr)                                                                               \
  do { hipError_t e_ = (expr);                                                                     \
       if (e_ != hipSuccess) return fail(IPK_ERR_HIP, "%s failed: %s", #expr, hipGetErrorString(e_)); } while (0)

struct DevCfa { uint32_t *lookups = nullptr; uint8_t *cfa48 = nullptr; float *gen_cells = nullptr; int gen_pw = 0, gen_ph = 0; };   // gen_cells: the row-walking kernel's cell records (Cfa::gen_cells; a filter with a fourth colour has them too)

}  // namespace

namespace {
// The streams, events and device slots of the host-pointer pipeline driver.  One set per context, grown on demand and kept
// between calls (a fresh hipMalloc of two input and two output slots costs more than moving a frame), released with the context.
struct HostLanes {
  static constexpr int kSlots = 2;
  std::mutex mu;                                  // one host-pointer pipeline call at a time per context
  hipStream_t up = nullptr, run = nullptr, down = nullptr;
  hipEvent_t up_done[kSlots] = {}, run_done[kSlots] = {}, down_done[kSlots] = {};
  void *in[kSlots] = {}, *out[kSlots] = {};
  size_t in_cap = 0, out_cap = 0;
  bool made = false;
  int ensure(size_t in_bytes, size_t out_bytes);
  void release();
};
}  // namespace

// One library context: a device binding plus everything the entry points keep on that device -- the lookup tables, the CFA table cache, the
// stream-ordered scratch pool, the task-queue heads of the row-walking kernels, the host-pointer driver's lanes.  A process may hold several
// (one per GPU for a batch dealt frame i -> device i mod N from ONE process -- the reference is one process, src/lib.rs:21-26 -- or several on one
// GPU); every entry point works on the calling thread's CURRENT context (ipk_ctx_make_current), which defaults to the one ipk_init made.
// Contexts are never deallocated before process exit (ipk_ctx_destroy releases the device resources and marks the object dead), so a stale
// handle on another thread fails with IPK_ERR_NOT_INIT instead of touching freed memory.
struct ipk_ctx {
  bool ready = false;
  int libm_matches = -1; size_t libm_mismatches = 0;      // init-time comparison of the host's cbrtf with the device routine
  int device = -1;
  int num_cus = 0;
  void *lut_pairs[3] = {nullptr, nullptr, nullptr};      // device, 8192 x {v, dv}
  void *lut_plain[3] = {nullptr, nullptr, nullptr};      // device, 8193 floats
  void *lut_q8 = nullptr;                                // device, 8192 x {k, threshold}: OpGamma + output8bit as one step lookup
  std::map<std::string, DevCfa> cfa_cache;
  std::map<std::string, float *> rot_cells;              // generic-CFA cell records laid out for a rotated space (pattern, orientation, frame phase)
  // stream-ordered scratch pool for the staged pipeline's intermediate OpBuffers
  // last: the stream its most recent user enqueued on; clean: the device has been drained since the block came back
  struct Block { void *p; size_t bytes; bool busy; hipStream_t last; bool clean; };
  std::vector<Block> pool;
  std::mutex mu;
  ipk::TaskQueues *queues = nullptr;
  HostLanes lanes;
  hipStream_t multi_stream = nullptr;                    // the stream ipk_pipeline_run_batch_multi enqueues on for this context
};

namespace {
typedef ipk_ctx Context;
// host-side state every context shares (immutable once built)
struct HostTables {
  std::mutex mu;
  std::vector<float> lut_host[3];
  float xyz_d65_33[9];
} g_host;
std::mutex g_reg_mu;                                      // registry, default context, device set
std::vector<std::unique_ptr<Context>> g_registry;         // every context ever created (dead ones stay: see ipk_ctx)
std::atomic<Context *> g_default{nullptr};                             // ipk_init's context: current on every thread that has not chosen another
std::vector<Context *> g_devset;                          // ipk_init_devices: one context per listed device
thread_local Context *t_current = nullptr;
Context g_none;                                           // ready == false: what cx() answers before any context exists
Context &cx() {
  Context *c = t_current ? t_current : g_default.load(std::memory_order_acquire);
  return c ? *c : g_none;
}

void build_host_luts() {
  std::lock_guard<std::mutex> lk(g_host.mu);
  if (!g_host.lut_host[0].empty()) return;
  for (int i = 0; i < 3; ++i) g_host.lut_host[i] = ipk::build_lut(static_cast<ipk::LutId>(i));
  const ipk::Mat33 inv = ipk::inverse(ipk::srgb_d65_33());
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) g_host.xyz_d65_33[r * 3 + c] = inv.m[r][c];
}

// HIP's current device is per host thread: a caller on another thread than the context's creator (a Rayon worker), or one that switched
// contexts, must land on the context's GPU.  hipGetDevice is a thread-local read; asking every time (instead of remembering what this
// library set last) stays correct when the host application calls hipSetDevice itself between two calls.
int bind_device(int device) {
  int now = -1;
  if (hipGetDevice(&now) != hipSuccess || now != device) HIPCHK(hipSetDevice(device));
  return IPK_OK;
}
int require_init() {
  Context &c = cx();
  if (!c.ready) return fail(IPK_ERR_NOT_INIT, "no live context on this thread: ipk_init() / ipk_ctx_create() has not succeeded (no MI355X/HIP device bound) or the current context was destroyed; there is no CPU fallback");
  return bind_device(c.device);
}
#define REQUIRE_INIT() do { int rc_ = require_init(); if (rc_) return rc_; } while (0)
}  // namespace
namespace ipk {
int internal_fail(int code, const char *fmt, ...) {
  va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap);
  return code;
}
int internal_require_init() { return require_init(); }
int internal_device() { return cx().device; }
}  // namespace ipk
namespace {

hipStream_t S(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

bool dims_ok(size_t w, size_t h) { return w >= 1 && h >= 1 && w < (1ull << 31) && h < (1ull << 31); }

// 16-letter patterns without a stated shape are refused, not guessed: rawloader's tile shape for them is unverified (ipk_host.hpp Cfa::parse)
int cfa_fail(const char *pat) {
  if (ipk::Cfa::unpinned_length(pat))
    return fail(IPK_ERR_UNSUPPORTED, "16-letter CFA pattern \"%s\": state the tile's shape (\"8x2:...\" / \"2x8:...\", or cfa_width / cfa_height); it is not guessed", pat);
  return fail(IPK_ERR_INVALID, "invalid CFA pattern \"%s\"", pat ? pat : "(null)");
}
// A descriptor's pattern in its CANONICAL spelling, with the shape its cfa_width / cfa_height fields state folded in (the fields are zeroed): plain
// letters when the tile's shape is the one the letter count implies (4 -> 2x2, 36 -> 6x6, 144 -> 12x12), "WxH:letters" otherwise.  A caller that
// fills the fields from its CFA object, one that writes a redundant "2x2:" prefix and one that passes the plain pattern therefore reach the same
// device tables and -- through hash_chain -- the same ipk_pipeline_hashes / cache keys, which stay the hash of the reference's plain pattern string
// (src/ops/demosaic.rs:13).  False: the fields contradict a prefix already in the string, or the result does not fit the buffer.
// Every descriptor that crosses the ABI is first TAKEN: struct_size bytes of the caller's object into a zeroed struct of this library's layout
// (include/imagepipe_amd.h, "Descriptor versioning"), so nothing is ever read past what the caller has, fields the caller's header did not know
// keep their zero defaults, and an object from a newer header is refused instead of half understood.  Then the CFA shape is folded (below).
#define IPK_FOLD_CFA(T, d) \
  T d##_folded; \
  if (d) { \
    { const int trc_ = take_desc((d), d##_folded); if (trc_) return trc_; } \
    if (!fold_cfa_shape(d##_folded)) \
      return (d##_folded.cfa_width == 0 && d##_folded.cfa_height == 0) ? fail(IPK_ERR_INVALID, "invalid CFA shape prefix (expected \"WxH:letters\" with W*H letters)") \
                                                                        : fail(IPK_ERR_INVALID, "cfa_width / cfa_height do not fit the pattern string"); \
    (d) = &d##_folded; \
  }
template <typename Desc>
static int take_desc(const Desc *in, Desc &out) {
  const size_t have = in->struct_size, oldest = offsetof(Desc, cfa_width);
  if (have == 0) return fail(IPK_ERR_INVALID, "descriptor.struct_size is 0: initialise the descriptor with IPK_*_INIT (struct_size = sizeof of the struct as the caller was compiled)");
  if (have < oldest) return fail(IPK_ERR_INVALID, "descriptor.struct_size %zu is smaller than the first published layout (%zu bytes)", have, oldest);
  if (have > sizeof(Desc)) return fail(IPK_ERR_INVALID, "descriptor.struct_size %zu is larger than this library's struct (%zu bytes): the caller was built against a newer header", have, sizeof(Desc));
  // Appended fields arrive in whole published layouts only: an object shorter than this library's struct is an object of the FIRST layout (its own
  // sizeof is `oldest` rounded up to the struct's alignment -- the bytes between are that compiler's tail padding, indeterminate, and must not land in
  // cfa_width), so exactly the fields of the newest whole layout the object covers are copied.  A later layout adds its boundary to this list.
  const size_t layouts[] = {oldest, offsetof(Desc, schedule), sizeof(Desc)};
  size_t take = oldest;
  for (size_t b : layouts) if (b <= have) take = b;
  std::memset(static_cast<void *>(&out), 0, sizeof(Desc));
  std::memcpy(static_cast<void *>(&out), in, take);
  out.struct_size = (uint32_t)sizeof(Desc);
  return IPK_OK;
}
template <typename Desc>
static bool fold_cfa_shape(Desc &d) {
  d.cfa[sizeof(d.cfa) - 1] = 0;
  if (d.cfa_width == 0 && d.cfa_height == 0 && !std::strchr(d.cfa, ':')) return true;      // plain letters, nothing stated: canonical already
  if ((d.cfa_width != 0 || d.cfa_height != 0) && (d.cfa_width < 1 || d.cfa_height < 1 || d.cfa_width > 48 || d.cfa_height > 48)) return false;
  int w = 0, h = 0; const char *letters = d.cfa;
  if (!ipk::Cfa::split_dims(d.cfa, w, h, letters)) return false;
  if (w != 0 && d.cfa_width != 0 && (w != d.cfa_width || h != d.cfa_height)) return false;
  if (w == 0) { w = d.cfa_width; h = d.cfa_height; }
  const size_t len = std::strlen(letters);
  const bool inferred = w == h && ((w == 2 && len == 4) || (w == 6 && len == 36) || (w == 12 && len == 144));
  char buf[sizeof(d.cfa) + 16];
  const int n = inferred ? std::snprintf(buf, sizeof(buf), "%s", letters) : std::snprintf(buf, sizeof(buf), "%dx%d:%s", w, h, letters);
  if (n < 0 || (size_t)n >= sizeof(d.cfa)) return false;
  std::memcpy(d.cfa, buf, (size_t)n + 1);
  d.cfa_width = 0; d.cfa_height = 0;
  return true;
}

// device-side tables for one CFA pattern string (uploaded once, cached)
int get_cfa(const char *pat, ipk::Cfa &cfa, DevCfa &dev) {
  if (!ipk::Cfa::parse(pat, cfa) || !cfa.valid()) return cfa_fail(pat);
  std::lock_guard<std::mutex> lk(cx().mu);
  auto it = cx().cfa_cache.find(pat);
  if (it != cx().cfa_cache.end()) { dev = it->second; return IPK_OK; }
  uint32_t lookups[48 * 48];
  cfa.demosaic_lookups(lookups);
  DevCfa d;
  HIPCHK(hipMalloc(reinterpret_cast<void **>(&d.lookups), sizeof(lookups)));
  HIPCHK(hipMalloc(reinterpret_cast<void **>(&d.cfa48), 48 * 48));
  HIPCHK(hipMemcpy(d.lookups, lookups, sizeof(lookups), hipMemcpyHostToDevice));
  HIPCHK(hipMemcpy(d.cfa48, &cfa.pattern[0][0], 48 * 48, hipMemcpyHostToDevice));
  std::vector<float> cells;
  if (cfa.gen_cells(cells)) {                                            // arithmetic form of demosaic::full for the row-walking kernel
    HIPCHK(hipMalloc(reinterpret_cast<void **>(&d.gen_cells), cells.size() * sizeof(float)));
    HIPCHK(hipMemcpy(d.gen_cells, cells.data(), cells.size() * sizeof(float), hipMemcpyHostToDevice));
    d.gen_pw = cfa.width; d.gen_ph = cfa.height;
  }
  cx().cfa_cache[pat] = d;
  dev = d;
  return IPK_OK;
}

// scratch pool: buffers are handed out and returned in stream order -- a block goes back as soon as its last user is enqueued, and
// the next user on the SAME stream runs after it.  Nothing is enqueued for the hand-over (round 2 recorded an event per returned
// block; each such marker cost the queue ~5 us of idle time between two runs -- a tenth of a 2160x1440 preview).  A stream never
// takes a block another stream used last: it gets a new one, so after a few runs every stream of a multi-stream caller owns the blocks it
// cycles through.  Only when memory runs out is the device drained, after which every idle block may go anywhere.  No stream handle is
// ever touched except the caller's current one (a previous one may have been destroyed).
// hipStreamPerThread is ONE handle that names a different stream in every host thread: the pool's "same stream" test keys it by the calling
// thread (as the task queues do), so two threads on their per-thread streams never hand each other a block without an ordering between them.
// (A handle value that HIP reuses for a new stream after hipStreamDestroy while the old stream's work is still in flight cannot be told apart:
// callers synchronise a stream before destroying it -- INTEGRATION.md.)
static hipStream_t pool_key(hipStream_t s) {
  static thread_local char per_thread_key;
  return s == hipStreamPerThread ? reinterpret_cast<hipStream_t>(&per_thread_key) : s;
}
static int pool_pick(size_t bytes, hipStream_t stream) {
  int best = -1;
  for (size_t i = 0; i < cx().pool.size(); ++i) {
    const auto &b = cx().pool[i];
    if (!b.busy && b.bytes >= bytes && (b.clean || b.last == stream) && (best < 0 || b.bytes < cx().pool[best].bytes)) best = (int)i;
  }
  return best;
}
int pool_get(size_t bytes, void **out, hipStream_t stream) {
  stream = pool_key(stream);
  std::lock_guard<std::mutex> lk(cx().mu);
  int best = pool_pick(bytes, stream);
  if (best < 0) {
    bool foreign_fits = false;
    for (const auto &b : cx().pool) foreign_fits = foreign_fits || (!b.busy && b.bytes >= bytes);
    // nothing fits on any stream: the idle blocks are all too small for this frame size, so they go before a larger one is allocated
    // (a long-running process that moves between frame sizes keeps only what its current size needs; hipFree waits for their users)
    if (!foreign_fits)
      for (size_t i = cx().pool.size(); i-- > 0;)
        if (!cx().pool[i].busy) { (void)hipFree(cx().pool[i].p); cx().pool.erase(cx().pool.begin() + (long)i); }
    void *p = nullptr;
    if (hipMalloc(&p, bytes ? bytes : 1) == hipSuccess) {
      cx().pool.push_back({p, bytes, true, stream, false});
      *out = p;
      return IPK_OK;
    }
    (void)hipGetLastError();
    // out of memory: drain the device -- every idle block is then free of users -- and look again, dropping what is too small
    if (hipDeviceSynchronize() != hipSuccess) return fail(IPK_ERR_HIP, "hipDeviceSynchronize failed");
    for (auto &b : cx().pool) if (!b.busy) b.clean = true;
    best = pool_pick(bytes, stream);
    if (best < 0) {
      for (size_t i = cx().pool.size(); i-- > 0;)
        if (!cx().pool[i].busy) { (void)hipFree(cx().pool[i].p); cx().pool.erase(cx().pool.begin() + (long)i); }
      if (hipMalloc(&p, bytes ? bytes : 1) != hipSuccess) return fail(IPK_ERR_NOMEM, "hipMalloc(%zu) failed", bytes);
      cx().pool.push_back({p, bytes, true, stream, false});
      *out = p;
      return IPK_OK;
    }
  }
  auto &b = cx().pool[best];
  b.busy = true; b.last = stream; b.clean = false; *out = b.p;
  return IPK_OK;
}
void pool_put(void *p, hipStream_t stream) {
  if (!p) return;
  stream = pool_key(stream);
  std::lock_guard<std::mutex> lk(cx().mu);
  for (auto &b : cx().pool) if (b.p == p) { b.last = stream; b.busy = false; return; }
}
struct Scratch {                       // RAII: returns its buffers to the pool
  hipStream_t stream;
  std::vector<void *> bufs;
  explicit Scratch(hipStream_t s) : stream(s) {}
  ~Scratch() { for (void *p : bufs) pool_put(p, stream); }
  int get(size_t bytes, void **out) { int rc = pool_get(bytes, out, stream); if (!rc) bufs.push_back(*out); return rc; }
  void release(void *p) { pool_put(p, stream); bufs.erase(std::remove(bufs.begin(), bufs.end(), p), bufs.end()); }
};


// Can OpGoFloat's `(v - black) / range` run as the 4-instruction cdiv_fast in the fused kernel?
// The kernel-side proof obligations (ipk_device.hpp): range positive and ordinary, the fast quotient equal to the
// true one on the dividends this source can produce, and (u16 sources, which the kernel does not guard) every
// nonzero dividend inside [2^-100, 2^100].  Anything else makes the kernel use true divisions.
// u16 sources: is every normalised sample min((v - black) / range, 1.0) "ordinary" (zero or inside [2^-20, 2^20], the
// device's gen_sample_bad)?  Then the kernels need no sample checks at all.
bool gen_levels_ok_u16(float black, float range) {
  static thread_local struct { uint32_t b, r; int ok; bool set; } memo = {0, 0, 0, false};
  uint32_t bb, rb; std::memcpy(&bb, &black, 4); std::memcpy(&rb, &range, 4);
  if (memo.set && memo.b == bb && memo.r == rb) return memo.ok != 0;
  bool ok = true;
  for (uint32_t v = 0; v < 65536 && ok; ++v) {
    const float q = std::fmin(((float)v - black) / range, 1.0f);
    const float a = std::fabs(q);
    ok = (q == 0.0f) || (a >= 0x1p-20f && a <= 0x1p20f);
  }
  memo = {bb, rb, ok ? 1 : 0, true};
  return ok;
}
bool validate_cdiv_for_range_uncached(float black, float range, bool src_is_u16);
bool validate_cdiv_for_range(float black, float range, bool src_is_u16) {
  // one-entry memo: a pipeline is launched many times with the same levels
  static thread_local struct { uint32_t b, r; int u16, ok; bool set; } memo = {0, 0, 0, 0, false};
  uint32_t bb, rb; std::memcpy(&bb, &black, 4); std::memcpy(&rb, &range, 4);
  if (memo.set && memo.b == bb && memo.r == rb && memo.u16 == (int)src_is_u16) return memo.ok != 0;
  const bool ok = validate_cdiv_for_range_uncached(black, range, src_is_u16);
  memo = {bb, rb, (int)src_is_u16, ok ? 1 : 0, true};
  return ok;
}
bool validate_cdiv_for_range_uncached(float black, float range, bool src_is_u16) {
  if (!(range >= 0x1p-60f && range <= 0x1p60f)) return false;             // also rejects NaN, <= 0
  const float rc = 1.0f / range;
  auto ok = [&](float d) {
    if (d == 0.0f || d != d || std::isinf(d)) return true;                // v_div_fixup_f32 supplies these
    const float ad = std::fabs(d);
    if (ad < 0x1p-100f || ad > 0x1p100f) return !src_is_u16;              // f32 kernels guard this zone themselves
    const float q0 = d * rc;
    const float r = std::fma(-q0, range, d);
    return std::fma(r, rc, q0) == d / range;
  };
  if (src_is_u16) {
    for (uint32_t v = 0; v < 65536; ++v) if (!ok((float)v - black)) return false;
    return true;
  }
  // f32 sources: any dividend can occur.  Every dividend mantissa against this divisor (a proof for the guarded exponent zone,
  // ipk_host.hpp), then a spread of exponents as a check of the scaling argument itself.
  if (!ipk::cdiv_mantissa_exhaustive_ok(range)) return false;
  uint64_t st = 0x9E3779B97F4A7C15ull;
  for (int i = 0; i < 4096; ++i) {
    st = st * 6364136223846793005ull + 1442695040888963407ull;
    uint32_t bits = (uint32_t)(st >> 32);
    bits = (bits & 0x807FFFFFu) | ((27u + (bits >> 23) % 200u) << 23);      // exponent in [2^-100, 2^100)
    float d; std::memcpy(&d, &bits, 4);
    if (!ok(d)) return false;
  }
  return true;
}

// One cached OpBuffer: device memory owned by the cache (and by whoever still holds the shared_ptr).
struct CBuf {
  void *p = nullptr; size_t w = 0, h = 0, colors = 0; int mono = 0;
  ~CBuf() { if (p) (void)hipFree(p); }
  size_t bytes() const { return w * h * colors * sizeof(float); }        // pipeline.rs:369
};
using CBufP = std::shared_ptr<CBuf>;
int cbuf_new(size_t w, size_t h, size_t colors, int mono, CBufP &out) {
  out = std::make_shared<CBuf>();
  out->w = w; out->h = h; out->colors = colors; out->mono = mono;
  if (hipMalloc(&out->p, std::max<size_t>(out->bytes(), 1)) != hipSuccess) { out->p = nullptr; return fail(IPK_ERR_NOMEM, "hipMalloc(%zu) failed", out->bytes()); }
  return IPK_OK;
}

}  // namespace

struct ipk_cache {
  ipk::LruByteCache<CBuf> lru;
  ipk_ctx *owner;                        // the context (device) whose memory the cached OpBuffers live in; null for a cache made before any context
  explicit ipk_cache(size_t bytes, ipk_ctx *o) : lru(bytes), owner(o) {}
};

namespace {
template <typename T>
int rotate_typed(const T *src3, size_t bwidth, size_t bheight, int orientation, T *dst3, size_t *out_width, size_t *out_height, void *stream) {
  REQUIRE_INIT();
  if (!src3 || !dst3 || !out_width || !out_height || !dims_ok(bwidth, bheight)) return fail(IPK_ERR_INVALID, "bad rotate arguments");
  bool transpose, flip_x, flip_y;
  ipk::orientation_to_flips(orientation, transpose, flip_x, flip_y);
  // transform.rs:102-128 in units of pixels
  int64_t width = (int64_t)bwidth, height = (int64_t)bheight;
  int64_t base = 0, x_step = 1, y_step = width;
  if (flip_x) { x_step = -x_step; base += width - 1; }
  if (flip_y) { y_step = -y_step; base += width * (height - 1); }
  if (transpose) { std::swap(width, height); std::swap(x_step, y_step); }
  *out_width = (size_t)width; *out_height = (size_t)height;
  ipk::launch_rotate<T>(src3, (size_t)width, (size_t)height, base, x_step, y_step, dst3, S(stream));
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
}  // namespace

extern "C" {

// ------------------------------------------------------------------------------------------
// context
// ------------------------------------------------------------------------------------------
// Everything a context keeps on its device.  `c` is not yet visible to any other thread; the caller has the device bound.
static int ctx_build(Context &c, int device) {
  hipDeviceProp_t prop;
  HIPCHK(hipGetDeviceProperties(&prop, device));
  c.device = device;
  c.num_cus = prop.multiProcessorCount;
  build_host_luts();
  for (int t = 0; t < 3; ++t) {
    // {table[i], table[i+1]-table[i]}: the subtraction of lookup() (color_conversions.rs:112) hoisted
    std::vector<float> pairs(2 * 8192);
    for (int i = 0; i < 8192; ++i) { pairs[2 * i] = g_host.lut_host[t][i]; pairs[2 * i + 1] = g_host.lut_host[t][i + 1] - g_host.lut_host[t][i]; }
    HIPCHK(hipMalloc(&c.lut_pairs[t], pairs.size() * sizeof(float)));
    HIPCHK(hipMemcpy(c.lut_pairs[t], pairs.data(), pairs.size() * sizeof(float), hipMemcpyHostToDevice));
    HIPCHK(hipMalloc(&c.lut_plain[t], ipk::kLutLen * sizeof(float)));
    HIPCHK(hipMemcpy(c.lut_plain[t], g_host.lut_host[t].data(), ipk::kLutLen * sizeof(float), hipMemcpyHostToDevice));
  }
  // OpGamma + output8bit as one step lookup (ipk_device.hpp Q8Entry): built on the device from THIS host's gamma table, and checked against the literal
  // composition on every f32 before the context goes live (a few milliseconds) -- the 8-bit kernels have no other form to fall back to, so a table that
  // failed the check (it cannot, by the slope argument; a broken powf could) stops ipk_init loudly instead of producing wrong bytes
  HIPCHK(hipMalloc(&c.lut_q8, 8192 * 8));
  ipk::launch_build_q8(c.lut_pairs[ipk::kLutGamma], c.lut_q8, nullptr);
  HIPCHK(hipGetLastError());
  {
    struct { unsigned long long bad; unsigned int first; unsigned int pad; } h = {0, 0xFFFFFFFFu, 0};
    void *dev = nullptr;
    HIPCHK(hipMalloc(&dev, sizeof(h)));
    HIPCHK(hipMemcpy(dev, &h, sizeof(h), hipMemcpyHostToDevice));
    ipk::launch_selftest_q8(c.lut_pairs[ipk::kLutGamma], c.lut_q8, dev, nullptr);
    const hipError_t e = hipMemcpy(&h, dev, sizeof(h), hipMemcpyDeviceToHost);
    (void)hipFree(dev);
    if (e != hipSuccess) return fail(IPK_ERR_HIP, "the 8-bit step table could not be verified: %s", hipGetErrorString(e));
    if (h.bad != 0) return fail(IPK_ERR_UNSUPPORTED, "the 8-bit step table disagrees with OpGamma + output8bit on %llu inputs (first 0x%08x): this host's gamma table is not monotone?", h.bad, h.first);
  }
  // the row-walking kernels' task-queue heads, one block for all streams of this context (nothing is allocated at launch time, so launches can be captured)
  c.queues = ipk::create_task_queues();
  if (!c.queues) return fail(IPK_ERR_HIP, "task queue allocation failed");
  // The device's cbrtf reproduces glibc 2.35's routine; the lookup tables above and a reference built on THIS host use this host's libm.
  // If the two disagree (another libc, a newer glibc with a correctly rounded cbrtf) results stay deterministic but are no longer
  // bit-identical to that reference for Lab ratios above 1: checked here on 65 536 arguments spread over (1, 8) and reported through
  // ipk_host_libm_matches() -- never silently.
  {
    const size_t n = 65536;
    std::vector<float> in(n), out(n);
    for (size_t i = 0; i < n; ++i) { const uint32_t bits = 0x3F800001u + (uint32_t)((i * 0x017FFFFFull) / n); std::memcpy(&in[i], &bits, 4); }   // (1, 8)
    void *din = nullptr, *dout = nullptr;
    c.libm_matches = -1;
    if (hipMalloc(&din, n * 4) == hipSuccess && hipMalloc(&dout, n * 4) == hipSuccess &&
        hipMemcpy(din, in.data(), n * 4, hipMemcpyHostToDevice) == hipSuccess) {
      ipk::launch_selftest_cbrt(static_cast<const float *>(din), static_cast<float *>(dout), n, 1, nullptr, nullptr);
      if (hipMemcpy(out.data(), dout, n * 4, hipMemcpyDeviceToHost) == hipSuccess) {
        size_t bad = 0;
        for (size_t i = 0; i < n; ++i) { const float h = cbrtf(in[i]); bad += std::memcmp(&h, &out[i], 4) != 0; }
        c.libm_matches = bad == 0 ? 1 : 0;
        c.libm_mismatches = bad;
      }
    }
    if (din) (void)hipFree(din);
    if (dout) (void)hipFree(dout);
  }
  c.ready = true;
  return IPK_OK;
}
// releases what ctx_build and later calls put on the device; the object itself stays in the registry (dead)
static void ctx_release(Context &c) {
  if (c.device < 0) return;
  int prev = -1;
  (void)hipGetDevice(&prev);
  if (hipSetDevice(c.device) != hipSuccess) { (void)hipGetLastError(); return; }
  c.ready = false;
  // only this context's work has to be over: its lanes, its batch stream and whatever its callers enqueued (their streams are theirs to drain
  // before destroying a context -- the device-wide wait below is the backstop, as it was for ipk_shutdown)
  (void)hipDeviceSynchronize();
  for (int t = 0; t < 3; ++t) { if (c.lut_pairs[t]) (void)hipFree(c.lut_pairs[t]); c.lut_pairs[t] = nullptr; if (c.lut_plain[t]) (void)hipFree(c.lut_plain[t]); c.lut_plain[t] = nullptr; }
  if (c.lut_q8) { (void)hipFree(c.lut_q8); c.lut_q8 = nullptr; }
  {
    std::lock_guard<std::mutex> lk(c.mu);
    for (auto &kv : c.cfa_cache) { (void)hipFree(kv.second.lookups); (void)hipFree(kv.second.cfa48); if (kv.second.gen_cells) (void)hipFree(kv.second.gen_cells); }
    c.cfa_cache.clear();
    for (auto &kv : c.rot_cells) (void)hipFree(kv.second);
    c.rot_cells.clear();
    for (auto &b : c.pool) (void)hipFree(b.p);
    c.pool.clear();
  }
  { std::lock_guard<std::mutex> lk(c.lanes.mu); c.lanes.release(); }
  if (c.multi_stream) { (void)hipStreamDestroy(c.multi_stream); c.multi_stream = nullptr; }
  ipk::destroy_task_queues(c.queues); c.queues = nullptr;
  c.num_cus = 0;
  if (prev >= 0 && prev != c.device) (void)hipSetDevice(prev);
}
static int ctx_create_locked(int device, Context **out) {      // g_reg_mu held
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) { (void)hipGetLastError(); return fail(IPK_ERR_NO_DEVICE, "no HIP device visible"); }
  if (device < 0 || device >= n) return fail(IPK_ERR_INVALID, "device %d out of range (%d visible)", device, n);
  HIPCHK(hipSetDevice(device));
  std::unique_ptr<Context> c(new Context);
  const int rc = ctx_build(*c, device);
  if (rc) { ctx_release(*c); return rc; }
  *out = c.get();
  g_registry.push_back(std::move(c));
  return IPK_OK;
}
static bool ctx_known_locked(const Context *c) {
  for (const auto &p : g_registry) if (p.get() == c) return true;
  return false;
}

int ipk_init(int device) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  { Context *d0 = g_default.load(); if (d0 && d0->ready && d0->device == device) return IPK_OK; }
  Context *c = nullptr;
  const int rc = ctx_create_locked(device, &c);
  if (rc) return rc;
  // re-initialising on another device replaces the process default; the old default goes unless the device set still uses it
  Context *old = g_default.load();
  g_default = c;
  if (old && old->ready && std::find(g_devset.begin(), g_devset.end(), old) == g_devset.end()) { ctx_release(*old); (void)bind_device(device); }
  return IPK_OK;
}
int ipk_host_libm_matches(size_t *mismatches_of_65536) {
  if (!cx().ready) return fail(IPK_ERR_NOT_INIT, "ipk_init() has not succeeded");
  if (mismatches_of_65536) *mismatches_of_65536 = cx().libm_mismatches;
  return cx().libm_matches;
}

void ipk_shutdown(void) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  for (auto &c : g_registry) if (c->ready) ctx_release(*c);
  g_default = nullptr;
  g_devset.clear();
  t_current = nullptr;
}
int ipk_is_initialized(void) { return cx().ready ? 1 : 0; }

// ---- contexts (several devices from one process) ------------------------------------------------------------------------------
int ipk_ctx_create(int device, ipk_ctx **out) {
  if (!out) return fail(IPK_ERR_INVALID, "null output");
  *out = nullptr;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  int prev = -1; (void)hipGetDevice(&prev);
  const int rc = ctx_create_locked(device, out);
  // creating a context does not move the calling thread: its current context (and that context's device) stay what they were
  if (prev >= 0) (void)hipSetDevice(prev);
  (void)hipGetLastError();
  return rc;
}
int ipk_ctx_destroy(ipk_ctx *ctx) {
  if (!ctx) return IPK_OK;
  std::lock_guard<std::mutex> lk(g_reg_mu);
  if (!ctx_known_locked(ctx)) return fail(IPK_ERR_INVALID, "not a context of this library");
  if (ctx->ready) ctx_release(*ctx);
  if (g_default.load() == ctx) g_default = nullptr;
  g_devset.erase(std::remove(g_devset.begin(), g_devset.end(), ctx), g_devset.end());
  if (t_current == ctx) t_current = nullptr;
  return IPK_OK;
}
int ipk_ctx_make_current(ipk_ctx *ctx) {
  if (!ctx) { t_current = nullptr; return cx().ready ? bind_device(cx().device) : IPK_OK; }
  { std::lock_guard<std::mutex> lk(g_reg_mu);
    if (!ctx_known_locked(ctx)) return fail(IPK_ERR_INVALID, "not a context of this library");
    if (!ctx->ready) return fail(IPK_ERR_NOT_INIT, "the context has been destroyed"); }
  t_current = ctx;
  return bind_device(ctx->device);
}
ipk_ctx *ipk_ctx_current(void) { Context &c = cx(); return c.ready ? &c : nullptr; }
int ipk_ctx_device(const ipk_ctx *ctx) { return (ctx && ctx->ready) ? ctx->device : -1; }

int ipk_init_devices(const int *devices, int n) {
  int visible = 0;
  if (hipGetDeviceCount(&visible) != hipSuccess || visible <= 0) { (void)hipGetLastError(); return fail(IPK_ERR_NO_DEVICE, "no HIP device visible"); }
  if (n < 0 || n > 64 || (n > 0 && !devices)) return fail(IPK_ERR_INVALID, "bad device list");
  std::vector<int> want;
  if (n == 0) for (int i = 0; i < visible; ++i) want.push_back(i);       // every visible device
  else want.assign(devices, devices + n);
  for (int d : want) if (d < 0 || d >= visible) return fail(IPK_ERR_INVALID, "device %d out of range (%d visible)", d, visible);
  std::lock_guard<std::mutex> lk(g_reg_mu);
  int prev = -1; (void)hipGetDevice(&prev);
  // the previous set goes (its contexts are released unless one is the process default)
  Context *const dflt = g_default.load();
  for (Context *c : g_devset) if (c != dflt && c->ready) ctx_release(*c);
  g_devset.clear();
  int rc = IPK_OK;
  for (size_t i = 0; i < want.size() && rc == IPK_OK; ++i) {
    Context *c = nullptr;
    // the process default serves its own device's first entry: a caller of ipk_init(0) + ipk_init_devices({0..7}) has eight contexts, not nine
    if (dflt && dflt->ready && dflt->device == want[i] && std::find(g_devset.begin(), g_devset.end(), dflt) == g_devset.end()) c = dflt;
    else rc = ctx_create_locked(want[i], &c);
    if (rc == IPK_OK) g_devset.push_back(c);
  }
  if (rc != IPK_OK) {
    for (Context *c : g_devset) if (c != dflt && c->ready) ctx_release(*c);
    g_devset.clear();
  } else if (!dflt || !dflt->ready) {
    g_default = g_devset[0];                                             // ipk_init_devices alone is a complete initialisation
  }
  { Context *d1 = g_default.load();
    if (d1 && d1->ready && !t_current) (void)hipSetDevice(d1->device);
    else if (prev >= 0) (void)hipSetDevice(prev); }
  (void)hipGetLastError();
  return rc;
}
int ipk_device_set_size(void) { std::lock_guard<std::mutex> lk(g_reg_mu); return (int)g_devset.size(); }
ipk_ctx *ipk_device_ctx(int index) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  return (index >= 0 && (size_t)index < g_devset.size()) ? g_devset[(size_t)index] : nullptr;
}
// The dealing rule of the multi-device batch entry points, as arithmetic a caller (and the CPU tests) can ask for: frame i of n goes to set
// member i mod n_devices, so member `index` gets frames index, index + n_devices, ... -- *count of them.  Frames are independent pipelines
// (src/pipeline.rs:246-249): nothing else is shared out.
int ipk_deal_frames(size_t n_frames, int n_devices, int index, size_t *first, size_t *stride, size_t *count) {
  if (n_devices < 1 || index < 0 || index >= n_devices) return fail(IPK_ERR_INVALID, "bad device index %d of %d", index, n_devices);
  const size_t nd = (size_t)n_devices, ix = (size_t)index;
  if (first) *first = ix;
  if (stride) *stride = nd;
  if (count) *count = n_frames > ix ? (n_frames - ix - 1) / nd + 1 : 0;   // ceil((n_frames - ix) / nd) without the sum that wraps near 2^64
  return IPK_OK;
}

// the layout this library was built with, for bindings to check theirs against (no GPU needed)
size_t ipk_abi_sizeof(int which) {
  switch (which) {
    case 0: return sizeof(ipk_fused_params);
    case 1: return sizeof(ipk_pipeline_desc);
    case 2: return sizeof(ipk_band);
    case 3: return sizeof(ipk_stage_time);
    case 16: return offsetof(ipk_fused_params, cfa_width);
    case 17: return offsetof(ipk_pipeline_desc, cfa_width);
    case 18: return offsetof(ipk_fused_params, band_src_row0);
    case 19: return offsetof(ipk_pipeline_desc, use_fastpath);
    case 20: return offsetof(ipk_fused_params, schedule);
    case 21: return offsetof(ipk_pipeline_desc, schedule);
    default: return 0;
  }
}
const char *ipk_last_error(void) { return g_err; }
int ipk_device_cus(void) { return cx().num_cus; }

int ipk_malloc(void **dptr, size_t bytes) { REQUIRE_INIT(); HIPCHK(hipMalloc(dptr, bytes ? bytes : 1)); return IPK_OK; }
int ipk_free(void *dptr) { REQUIRE_INIT(); HIPCHK(hipFree(dptr)); return IPK_OK; }
int ipk_memcpy_h2d(void *dst, const void *src, size_t bytes, void *stream) {
  REQUIRE_INIT(); HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, S(stream))); return IPK_OK;
}
int ipk_memcpy_d2h(void *dst, const void *src, size_t bytes, void *stream) {
  REQUIRE_INIT(); HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, S(stream))); return IPK_OK;
}
int ipk_stream_sync(void *stream) { REQUIRE_INIT(); HIPCHK(hipStreamSynchronize(S(stream))); return IPK_OK; }

int ipk_lut_table(int which, float *out8193) {
  if (which < 0 || which > 2 || !out8193) return fail(IPK_ERR_INVALID, "bad table id");
  build_host_luts();
  std::memcpy(out8193, g_host.lut_host[which].data(), ipk::kLutLen * sizeof(float));
  return IPK_OK;
}

// ------------------------------------------------------------------------------------------
// host-side maths
// ------------------------------------------------------------------------------------------
int ipk_size_image(size_t crop_top, size_t crop_right, size_t crop_bottom, size_t crop_left,
                   size_t owidth, size_t oheight, size_t *out4) {
  ipk::Rect r;
  if (!ipk::size_image(crop_top, crop_right, crop_bottom, crop_left, owidth, oheight, r))
    return fail(IPK_ERR_INVALID, "image %zux%zu is smaller than 10x10", owidth, oheight);
  out4[0] = r.x; out4[1] = r.y; out4[2] = r.width; out4[3] = r.height;
  return IPK_OK;
}
int ipk_calculate_scaling_total(size_t width, size_t height, size_t maxwidth, size_t maxheight,
                                float *scale, size_t *nwidth, size_t *nheight) {
  const ipk::Scaling s = ipk::calculate_scaling_total(width, height, maxwidth, maxheight);
  *scale = s.scale; *nwidth = s.width; *nheight = s.height;
  return IPK_OK;
}
int ipk_normalize_wbs(const float *vals4, float *out4) { ipk::normalize_wbs(vals4, out4); return IPK_OK; }
int ipk_const_matrix(int which, float *out12) {
  if (!out12) return fail(IPK_ERR_INVALID, "ipk_const_matrix: null output");
  const ipk::Mat33 s = ipk::srgb_d65_33(), x = ipk::inverse(s);
  switch (which) {
    case 0: for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) out12[r * 3 + c] = s.m[r][c]; return IPK_OK;      // SRGB_D65_33
    case 1: for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) out12[r * 3 + c] = x.m[r][c]; return IPK_OK;      // XYZ_D65_33
    case 2: ipk::srgb_d65_43(out12); return IPK_OK;                                                                   // SRGB_D65_43
    case 3: for (int r = 0; r < 4; ++r) for (int c = 0; c < 3; ++c) out12[r * 3 + c] = r < 3 ? x.m[r][c] : 0.0f; return IPK_OK;   // XYZ_D65_34
  }
  return fail(IPK_ERR_INVALID, "ipk_const_matrix: which must be 0..3");
}
int ipk_temp_to_xyz(float temp, float *out3) { ipk::temp_to_xyz(temp, out3); return IPK_OK; }
int ipk_xyz_to_temp(const float *xyz3, float *temp, float *tint) { ipk::xyz_to_temp(xyz3, *temp, *tint); return IPK_OK; }
int ipk_tolab_set_temp(const float *xyz_to_cam12, float temp, float tint, float *wb4) { ipk::tolab_set_temp(xyz_to_cam12, temp, tint, wb4); return IPK_OK; }
int ipk_tolab_get_temp(const float *cam_to_xyz12, const float *wb4, float *temp, float *tint) { ipk::tolab_get_temp(cam_to_xyz12, wb4, *temp, *tint); return IPK_OK; }
int ipk_spline_new(const float *pts, int npts, float *px, float *py, float *c1s, float *c2s, float *c3s) {
  ipk::Spline s;
  if (!s.build(pts, npts)) return fail(IPK_ERR_INVALID, "invalid curve (%d points)", npts);
  std::memcpy(px, s.px, s.npoints * sizeof(float)); std::memcpy(py, s.py, s.npoints * sizeof(float));
  std::memcpy(c1s, s.c1, s.npoints * sizeof(float));
  std::memcpy(c2s, s.c2, s.nseg * sizeof(float)); std::memcpy(c3s, s.c3, s.nseg * sizeof(float));
  return s.npoints;
}
int ipk_rotatecrop_calc_size(const float *p, float input_ratio, size_t width, size_t height, int reverse,
                             size_t *nwidth, size_t *nheight) {
  ipk::RotateCrop rc;
  rc.crop_top = p[0]; rc.crop_right = p[1]; rc.crop_bottom = p[2]; rc.crop_left = p[3]; rc.rotation = p[4];
  rc.input_ratio = input_ratio;
  rc.calc_size(width, height, reverse != 0, *nwidth, *nheight);
  return IPK_OK;
}
int ipk_cfa_shift(const char *pattern, int x, int y, char *out) {
  ipk::Cfa c;
  if (!ipk::Cfa::parse(pattern, c)) return cfa_fail(pattern);
  const std::string s = c.shifted_name(x, y);
  std::memcpy(out, s.c_str(), s.size() + 1);
  return IPK_OK;
}
int ipk_orientation_to_flips(int orientation, int *f) {
  bool t, x, y; ipk::orientation_to_flips(orientation, t, x, y); f[0] = t; f[1] = x; f[2] = y; return IPK_OK;
}
int ipk_orientation_from_flips(int transpose, int flip_x, int flip_y) { return ipk::orientation_from_flips(transpose, flip_x, flip_y); }
int ipk_transform_orientation(int rotation, int fliph, int flipv) {
  if (rotation < 0 || rotation > 3) return fail(IPK_ERR_INVALID, "bad rotation");
  return ipk::transform_orientation(rotation, fliph != 0, flipv != 0);
}

// ------------------------------------------------------------------------------------------
// stage kernels (device pointers)
// ------------------------------------------------------------------------------------------
#define GOFLOAT_ARGS_OK() do { REQUIRE_INIT(); if (!src || !dst || !dims_ok(width, height) || !dims_ok(owidth, 1)) return fail(IPK_ERR_INVALID, "bad gofloat arguments"); } while (0)

int ipk_gofloat_cfa_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                        float black0, float white0, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_cfa<uint16_t>(src, owidth, x, y, width, height, black0, white0, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_cfa_f32(const float *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                        float black0, float white0, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_cfa<float>(src, owidth, x, y, width, height, black0, white0, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_mono_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                         float black0, float white0, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_mono<uint16_t>(src, owidth, x, y, width, height, black0, white0, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_mono_f32(const float *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                         float black0, float white0, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_mono<float>(src, owidth, x, y, width, height, black0, white0, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_rgb_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                        const float *black4, const float *white4, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_rgb<uint16_t>(src, owidth, x, y, width, height, black4, white4, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_rgb_f32(const float *src, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                        const float *black4, const float *white4, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_rgb<float>(src, owidth, x, y, width, height, black4, white4, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_other_u8(const uint8_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_other_u8(src, owidth, x, y, width, height, cx().lut_pairs[ipk::kLutGammaReverse], dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_gofloat_other_u16(const uint16_t *src, size_t owidth, size_t x, size_t y, size_t width, size_t height, float *dst, void *stream) {
  GOFLOAT_ARGS_OK(); ipk::launch_gofloat_other_u16(src, owidth, x, y, width, height, dst, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}

int ipk_demosaic_full_band(const float *src, size_t width, size_t img_height, size_t src_row0, size_t src_rows,
                           size_t out_row0, size_t out_rows, const char *cfa_pat, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst4 || !dims_ok(width, img_height) || out_rows == 0 || out_row0 + out_rows > img_height)
    return fail(IPK_ERR_INVALID, "bad demosaic arguments");
  // the band must carry every in-image tap row of its output rows
  const size_t need0 = out_row0 > 0 ? out_row0 - 1 : 0;
  const size_t need1 = std::min(img_height, out_row0 + out_rows + 1);
  if (src_row0 > need0 || src_row0 + src_rows < need1) return fail(IPK_ERR_INVALID, "band rows [%zu,%zu) do not cover taps [%zu,%zu)", src_row0, src_row0 + src_rows, need0, need1);
  ipk::Cfa cfa; DevCfa dev;
  int rc = get_cfa(cfa_pat, cfa, dev); if (rc) return rc;
  int xoff, yoff;
  int lrc = 0;
  if (cfa.bayer_phase(xoff, yoff))       // the four RGGB phases: row-walking kernel (coalesced loads, register window, staged stores)
    lrc = ipk::launch_demosaic_bayer(src, width, img_height, src_row0, out_row0, out_rows, xoff, yoff, nullptr, 0, 0, dst4, cx().num_cus, cx().queues, S(stream));
  else if (dev.gen_cells && cfa.three_colour())   // any other three-colour filter (X-Trans ...): same kernel, generic-CFA mode
    lrc = ipk::launch_demosaic_bayer(src, width, img_height, src_row0, out_row0, out_rows, 0, 0, dev.gen_cells, dev.gen_pw, dev.gen_ph, dst4, cx().num_cus, cx().queues, S(stream));
  else ipk::launch_demosaic_full(src, width, img_height, src_row0, out_row0, out_rows, dev.lookups, dst4, S(stream));
  if (lrc) return fail(IPK_ERR_HIP, "kernel launch failed (nothing was enqueued)");
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_demosaic_full(const float *src, size_t width, size_t height, const char *cfa, float *dst4, void *stream) {
  return ipk_demosaic_full_band(src, width, height, 0, height, 0, height, cfa, dst4, stream);
}

#define TRANSFORM_BODY(T)                                                                                    \
  REQUIRE_INIT();                                                                                            \
  if (!src || !dst || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || components < 1 || components > 4) \
    return fail(IPK_ERR_INVALID, "bad transform_buffer arguments");                                          \
  const uint8_t *cfa48 = nullptr;                                                                            \
  if (cfa_pat) { ipk::Cfa cfa; DevCfa dev; int rc = get_cfa(cfa_pat, cfa, dev); if (rc) return rc; cfa48 = dev.cfa48; } \
  ipk::launch_transform_buffer<T>(src, width, height, tlx, tly, trx, try_, blx, bly, nwidth, nheight, components, cfa48, dst, S(stream)); \
  HIPCHK(hipGetLastError());                                                                                 \
  return IPK_OK;

int ipk_transform_buffer_f32(const float *src, size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                             int64_t blx, int64_t bly, size_t nwidth, size_t nheight, size_t components, const char *cfa_pat,
                             float *dst, void *stream) { TRANSFORM_BODY(float) }
int ipk_transform_buffer_u8(const uint8_t *src, size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                            int64_t blx, int64_t bly, size_t nwidth, size_t nheight, size_t components, const char *cfa_pat,
                            uint8_t *dst, void *stream) { TRANSFORM_BODY(uint8_t) }
int ipk_transform_buffer_u16(const uint16_t *src, size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                             int64_t blx, int64_t bly, size_t nwidth, size_t nheight, size_t components, const char *cfa_pat,
                             uint16_t *dst, void *stream) { TRANSFORM_BODY(uint16_t) }

// scale_down_buffer's corners (src/scaling.rs:35-48)
int ipk_scaled_demosaic(const float *src, size_t width, size_t height, const char *cfa, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  if (!cfa) return fail(IPK_ERR_INVALID, "scaled_demosaic needs a CFA");
  return ipk_transform_buffer_f32(src, width, height, 0, 0, (int64_t)width - 1, 0, 0, (int64_t)height - 1, nwidth, nheight, 4, cfa, dst4, stream);
}
int ipk_scale_down_opbuf(const float *src4, size_t width, size_t height, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return ipk_transform_buffer_f32(src4, width, height, 0, 0, (int64_t)width - 1, 0, 0, (int64_t)height - 1, nwidth, nheight, 4, nullptr, dst4, stream);
}

// OpGoFloat (CFA branch) + scaled_demosaic in one pass over the raw frame (used by ipk_pipeline_run when OpDemosaic::run
// would take its scaled_demosaic branch: the 1-channel f32 intermediate never exists)
namespace {
// a window of an nwidth x nheight result: non-empty and inside it
bool window_ok(size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh) {
  return ww != 0 && wh != 0 && wx <= nwidth && ww <= nwidth - wx && wy <= nheight && wh <= nheight - wy;
}
// One launch of the scaling kernels (ipk_launch.hpp, ScaledDemosaicLaunch).  scaled_geometry states what every form shares -- the sensor window, the result's size,
// the destination -- and the caller adds its band, window or batch; launch_scaled adds what the source is: a mosaic (cfa_pat: its device tables, black[0] /
// white[0] as its levels and whether their division has the fast form) or, cfa_pat == null, a monochrome / three-sample raw of plain_kind with its level pairs
ipk::ScaledDemosaicLaunch scaled_geometry(const void *src, size_t owidth, size_t x, size_t y, size_t width, size_t height, size_t nwidth, size_t nheight, float *dst4) {
  ipk::ScaledDemosaicLaunch l{};
  l.src = src; l.owidth = owidth;
  l.x = x; l.y = y; l.width = width; l.height = height;
  l.nwidth = nwidth; l.nheight = nheight;
  l.dst4 = dst4;
  return l;
}
int launch_scaled(ipk::ScaledDemosaicLaunch l, int src_type, const char *cfa_pat, int plain_kind, const float *black, const float *white, void *stream) {
  ipk::PlainLevels pl;
  l.src_is_u16 = src_type == IPK_SRC_U16;
  if (cfa_pat) {
    ipk::Cfa cfa; DevCfa dev; int rc = get_cfa(cfa_pat, cfa, dev); if (rc) return rc;
    l.black0 = black[0]; l.white0 = white[0];
    l.norm_fast = validate_cdiv_for_range(l.black0, l.white0 - l.black0, l.src_is_u16) ? 1 : 0;
    l.has_fourth_colour = cfa.three_colour() ? 0 : 1;
    l.cfa48_dev = dev.cfa48; l.pattern_width = (int)cfa.width; l.pattern_height = (int)cfa.height;
  } else {
    pl.layout = plain_kind == IPK_PLAIN_MONO ? 1 : 3;
    for (int c = 0; c < 3; ++c) { pl.black[c] = black[c]; pl.white[c] = white[c]; }
    l.plain = &pl;
  }
  ipk::launch_raw_scaled_demosaic(l, S(stream));
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
// the whole-frame form (win == null) and the window form: one admission, one launcher
int raw_scaled_demosaic_impl(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, float black0, float white0,
                             const char *cfa_pat, size_t nwidth, size_t nheight, const ipk::ResampleWindow *win, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst4 || !cfa_pat || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32))
    return fail(IPK_ERR_INVALID, "bad raw_scaled_demosaic arguments");
  if (win && !window_ok(nwidth, nheight, win->col0, win->row0, win->cols, win->rows))
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", win->col0, win->row0, win->cols, win->rows, nwidth, nheight);
  ipk::ScaledDemosaicLaunch l = scaled_geometry(src, owidth, x, y, width, height, nwidth, nheight, dst4);
  l.win = win;
  return launch_scaled(l, src_type, cfa_pat, 0, &black0, &white0, stream);
}
int raster_scale_down_impl(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, size_t nwidth, size_t nheight,
                           const ipk::ResampleWindow *win, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst4 || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_RGB8 && src_type != IPK_SRC_RGB16))
    return fail(IPK_ERR_INVALID, "bad raster_scale_down arguments");
  if (x + width > owidth) return fail(IPK_ERR_INVALID, "raster_scale_down: window wider than the source pitch");
  if (win && !window_ok(nwidth, nheight, win->col0, win->row0, win->cols, win->rows))
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", win->col0, win->row0, win->cols, win->rows, nwidth, nheight);
  ipk::launch_raster_scale_down(src, src_type == IPK_SRC_RGB16, owidth, x, y, width, height, nwidth, nheight, cx().lut_pairs[ipk::kLutGammaReverse],
                                dst4, S(stream), win);
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
// gofloat_mono / gofloat_rgb + scale_down_opbuf in one pass: the monochrome and three-sample modes of k_raw_scaled_demosaic<T>.  IPK_PLAIN_RASTER forwards
// to the raster kernel; admission is raster_scale_down_impl's
int plain_scale_down_impl(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height, const float *black4,
                          const float *white4, size_t nwidth, size_t nheight, const ipk::ResampleWindow *win, float *dst4, void *stream) {
  if (kind == IPK_PLAIN_RASTER) return raster_scale_down_impl(src, src_type, owidth, x, y, width, height, nwidth, nheight, win, dst4, stream);
  REQUIRE_INIT();
  if (kind != IPK_PLAIN_RGB && kind != IPK_PLAIN_MONO) return fail(IPK_ERR_INVALID, "bad plain kind");
  if (!src || !dst4 || !black4 || !white4 || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32))
    return fail(IPK_ERR_INVALID, "bad plain_scale_down arguments");
  if (x + width > owidth) return fail(IPK_ERR_INVALID, "plain_scale_down: window wider than the source pitch");
  if (win && !window_ok(nwidth, nheight, win->col0, win->row0, win->cols, win->rows))
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", win->col0, win->row0, win->cols, win->rows, nwidth, nheight);
  ipk::ScaledDemosaicLaunch l = scaled_geometry(src, owidth, x, y, width, height, nwidth, nheight, dst4);
  l.win = win;
  return launch_scaled(l, src_type, nullptr, kind, black4, white4, stream);
}
}  // namespace
int ipk_plain_scale_down(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height, const float *black4,
                         const float *white4, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return plain_scale_down_impl(src, src_type, kind, owidth, x, y, width, height, black4, white4, nwidth, nheight, nullptr, dst4, stream);
}
int ipk_plain_scale_down_window(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height, const float *black4,
                                const float *white4, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream) {
  const ipk::ResampleWindow win = {wy, wx, wh, ww};
  return plain_scale_down_impl(src, src_type, kind, owidth, x, y, width, height, black4, white4, nwidth, nheight, &win, dst4, stream);
}
int ipk_raw_scaled_demosaic(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                            float black0, float white0, const char *cfa_pat, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return raw_scaled_demosaic_impl(src, src_type, owidth, x, y, width, height, black0, white0, cfa_pat, nwidth, nheight, nullptr, dst4, stream);
}
// n frames of one shape into n packed results: the general kernel's batch launch (one per 64 frames) where the whole-frame call would select that kernel,
// else the whole-frame call's own launch per frame, into slice i (a slice is nwidth * nheight * 16 bytes, so every slice is aligned as dst4 is and the
// selection is the same for all).  Nothing is enqueued unless every frame is admitted
namespace {
int raw_scaled_demosaic_batch_impl(const void *const *srcs, size_t n, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, float black0,
                                   float white0, const char *cfa_pat, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (n == 0) return IPK_OK;
  if (!srcs || !dst4 || !cfa_pat || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32))
    return fail(IPK_ERR_INVALID, "bad raw_scaled_demosaic_batch arguments");
  for (size_t i = 0; i < n; ++i) if (!srcs[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
  const size_t slice = nwidth * nheight * 4;
  if (!ipk::raw_scaled_demosaic_general(width, height, nwidth, nheight, (reinterpret_cast<uintptr_t>(dst4) & 15) == 0, false)) {
    for (size_t i = 0; i < n; ++i) {
      const int rc = raw_scaled_demosaic_impl(srcs[i], src_type, owidth, x, y, width, height, black0, white0, cfa_pat, nwidth, nheight, nullptr, dst4 + i * slice, stream);
      if (rc) return rc;
    }
    return IPK_OK;
  }
  ipk::ScaledDemosaicLaunch l = scaled_geometry(nullptr, owidth, x, y, width, height, nwidth, nheight, dst4);
  l.batch_srcs = srcs; l.batch_n = n;
  return launch_scaled(l, src_type, cfa_pat, 0, &black0, &white0, stream);
}
// the same for monochrome and three-sample raws, whose launches are always the general kernel's; IPK_PLAIN_RASTER forwards frame by frame
int plain_scale_down_batch_impl(const void *const *srcs, size_t n, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                const float *black4, const float *white4, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (n == 0) return IPK_OK;
  if (!srcs) return fail(IPK_ERR_INVALID, "bad plain_scale_down_batch arguments");
  for (size_t i = 0; i < n; ++i) if (!srcs[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
  const size_t slice = nwidth * nheight * 4;
  if (kind == IPK_PLAIN_RASTER) {
    for (size_t i = 0; i < n; ++i) {
      const int rc = raster_scale_down_impl(srcs[i], src_type, owidth, x, y, width, height, nwidth, nheight, nullptr, dst4 ? dst4 + i * slice : nullptr, stream);
      if (rc) return rc;
    }
    return IPK_OK;
  }
  if (kind != IPK_PLAIN_RGB && kind != IPK_PLAIN_MONO) return fail(IPK_ERR_INVALID, "bad plain kind");
  if (!dst4 || !black4 || !white4 || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32))
    return fail(IPK_ERR_INVALID, "bad plain_scale_down_batch arguments");
  if (x + width > owidth) return fail(IPK_ERR_INVALID, "plain_scale_down_batch: window wider than the source pitch");
  ipk::ScaledDemosaicLaunch l = scaled_geometry(nullptr, owidth, x, y, width, height, nwidth, nheight, dst4);
  l.batch_srcs = srcs; l.batch_n = n;
  return launch_scaled(l, src_type, nullptr, kind, black4, white4, stream);
}
}  // namespace
int ipk_raw_scaled_demosaic_batch(const void *const *srcs, size_t n, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                  float black0, float white0, const char *cfa_pat, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return raw_scaled_demosaic_batch_impl(srcs, n, src_type, owidth, x, y, width, height, black0, white0, cfa_pat, nwidth, nheight, dst4, stream);
}
int ipk_plain_scale_down_batch(const void *const *srcs, size_t n, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                               const float *black4, const float *white4, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return plain_scale_down_batch_impl(srcs, n, src_type, kind, owidth, x, y, width, height, black4, white4, nwidth, nheight, dst4, stream);
}
// the columns [wx, wx + ww) and rows [wy, wy + wh) of the same result: the same kernel, its grid laid over the window
int ipk_raw_scaled_demosaic_window(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, float black0, float white0,
                                   const char *cfa_pat, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream) {
  const ipk::ResampleWindow win = {wy, wx, wh, ww};
  return raw_scaled_demosaic_impl(src, src_type, owidth, x, y, width, height, black0, white0, cfa_pat, nwidth, nheight, &win, dst4, stream);
}
// one output-row band of the same (ipk_band_plan_scaled): multi-GPU sharding of a frame that OpDemosaic scales
int ipk_raw_scaled_demosaic_band(const void *src, int src_type, size_t owidth, size_t x, size_t width, size_t height, float black0, float white0,
                                 const char *cfa_pat, size_t nwidth, size_t nheight, const ipk_band *band, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst4 || !cfa_pat || !band || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32))
    return fail(IPK_ERR_INVALID, "bad raw_scaled_demosaic_band arguments");
  if (band->out_rows == 0) return IPK_OK;
  if (band->out_row0 + band->out_rows > nheight || band->src_row0 + band->src_rows > height) return fail(IPK_ERR_INVALID, "band outside the frame");
  if (nheight < 2) return fail(IPK_ERR_INVALID, "a banded scaled demosaic needs at least two output rows");
  {
    // the slab must hold every source row the band's windows read (scaling.rs:84-94; the same f32 expressions as ipk_band_plan_scaled): a slab
    // that does not -- a hand-built band, a plan made for another output height -- would make the kernel read outside it
    const float skip = ((float)((int64_t)height - 1) - 0.0f) / ((float)(nheight - 1));
    const size_t from = std::min(height - 1, ipk::f32_to_usize(std::floor(0.0f + skip * (float)band->out_row0)));
    const size_t to = std::min(height - 1, ipk::f32_to_usize(std::floor(0.0f + skip * (float)(band->out_row0 + band->out_rows))));
    if (band->src_row0 > from || band->src_row0 + band->src_rows <= to)
      return fail(IPK_ERR_INVALID, "band slab rows [%zu,%zu) do not cover the window rows [%zu,%zu]", band->src_row0, band->src_row0 + band->src_rows, from, to);
  }
  ipk::ScaledDemosaicLaunch l = scaled_geometry(src, owidth, x, 0, width, height, nwidth, nheight, dst4);
  l.band_src_row0 = band->src_row0; l.band_out_row0 = band->out_row0; l.band_out_rows = band->out_rows;
  return launch_scaled(l, src_type, cfa_pat, 0, &black0, &white0, stream);
}

// OpGoFloat::run_other + scale_down_opbuf in one pass over a raster (used by the pipeline drivers when OpDemosaic::run would take its
// scale_down_opbuf branch for a raster source: the full-size 4-channel f32 buffer never exists)
int ipk_raster_scale_down(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                          size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return raster_scale_down_impl(src, src_type, owidth, x, y, width, height, nwidth, nheight, nullptr, dst4, stream);
}
int ipk_raster_scale_down_window(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, size_t nwidth, size_t nheight,
                                 size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream) {
  const ipk::ResampleWindow win = {wy, wx, wh, ww};
  return raster_scale_down_impl(src, src_type, owidth, x, y, width, height, nwidth, nheight, &win, dst4, stream);
}
// What such a window launch reads of the width x height cropped frame (host only): ipk::scaled_window_footprint
int ipk_scaled_window_footprint(size_t width, size_t height, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, size_t *out4) {
  if (!out4) return fail(IPK_ERR_INVALID, "null output");
  if (!dims_ok(width, height) || !dims_ok(nwidth, nheight)) return fail(IPK_ERR_INVALID, "bad scaled_window_footprint sizes");
  if (!window_ok(nwidth, nheight, wx, wy, ww, wh))
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", wx, wy, ww, wh, nwidth, nheight);
  const ipk::ResampleFootprint f = ipk::scaled_window_footprint(width, height, nwidth, nheight, wy, wx, wh, ww);
  out4[0] = f.x; out4[1] = f.y; out4[2] = f.w; out4[3] = f.h;
  return IPK_OK;
}

// OpDemosaic::run's dispatch (demosaic.rs:41-59) on the input's shape and the negotiated size: the branch and the output's size, or an error.  No GPU
enum DemosaicBranch { kDemosaicNoop, kDemosaicScaleOpbuf, kDemosaicScaled, kDemosaicFullScaled, kDemosaicFull };
static int demosaic_plan(size_t width, size_t height, size_t colors, const char *cfa_pat, size_t demosaic_width, size_t demosaic_height,
                         size_t *out_width, size_t *out_height) {
  if (colors != 1 && colors != 4) return fail(IPK_ERR_INVALID, "demosaic expects 1 or 4 colours");
  const float scale = ipk::calculate_scaling_total(width, height, demosaic_width, demosaic_height).scale;
  ipk::Cfa cfa;
  if (!ipk::Cfa::parse(cfa_pat ? cfa_pat : "", cfa)) return cfa_fail(cfa_pat);
  const float minscale = ipk::demosaic_minscale(cfa.width);
  *out_width = demosaic_width; *out_height = demosaic_height;
  if (scale <= 1.0f && colors == 4) { *out_width = width; *out_height = height; return kDemosaicNoop; }   // demosaic.rs:41-43
  if (colors == 4) return kDemosaicScaleOpbuf;                                                             // :44-46
  if (scale >= minscale) return kDemosaicScaled;                                                           // :47-50
  if (scale > 1.0f) return kDemosaicFullScaled;                                                            // :54-56
  *out_width = width; *out_height = height;                                                                // :57-59
  return kDemosaicFull;
}
// the launches of a branch demosaic_plan chose (a negative `branch`, its error, is handed back)
static int demosaic_launch(int branch, const float *src, size_t width, size_t height, const char *cfa_pat, size_t demosaic_width, size_t demosaic_height,
                           float *dst4, void *stream) {
  switch (branch) {
    case kDemosaicNoop: return IPK_NOOP;
    case kDemosaicScaleOpbuf: return ipk_scale_down_opbuf(src, width, height, demosaic_width, demosaic_height, dst4, stream);
    case kDemosaicScaled: return ipk_scaled_demosaic(src, width, height, cfa_pat, demosaic_width, demosaic_height, dst4, stream);
    case kDemosaicFullScaled: {
      Scratch sc(S(stream)); void *full = nullptr;
      int rc = sc.get(width * height * 4 * sizeof(float), &full); if (rc) return rc;
      rc = ipk_demosaic_full(src, width, height, cfa_pat, static_cast<float *>(full), stream); if (rc) return rc;
      return ipk_scale_down_opbuf(static_cast<float *>(full), width, height, demosaic_width, demosaic_height, dst4, stream);
    }
    case kDemosaicFull: return ipk_demosaic_full(src, width, height, cfa_pat, dst4, stream);
  }
  return branch;
}
int ipk_demosaic_run(const float *src, size_t width, size_t height, size_t colors, const char *cfa_pat,
                     size_t demosaic_width, size_t demosaic_height, float *dst4, size_t *out_width, size_t *out_height, void *stream) {
  REQUIRE_INIT();
  const int branch = demosaic_plan(width, height, colors, cfa_pat, demosaic_width, demosaic_height, out_width, out_height);
  return demosaic_launch(branch, src, width, height, cfa_pat, demosaic_width, demosaic_height, dst4, stream);
}

int ipk_rotatecrop(const float *src, size_t width, size_t height, size_t colors, const float *p, float *dst,
                   size_t *out_width, size_t *out_height, void *stream) {
  ipk::RotateCrop rc;
  rc.crop_top = p[0]; rc.crop_right = p[1]; rc.crop_bottom = p[2]; rc.crop_left = p[3]; rc.rotation = p[4];
  int64_t pts[6]; size_t nw, nh;
  if (!rc.corners(width, height, pts, nw, nh)) { *out_width = width; *out_height = height; return IPK_NOOP; }
  *out_width = nw; *out_height = nh;
  if (!dst) return IPK_OK;
  return ipk_transform_buffer_f32(src, width, height, pts[0], pts[1], pts[2], pts[3], pts[4], pts[5], nw, nh, colors, nullptr, dst, stream);
}

int ipk_tolab(const float *src4, size_t width, size_t height, int monochrome, const float *wb_coeffs,
              const float *cam_to_xyz_normalized, float *dst3, void *stream) {
  REQUIRE_INIT();
  if (!src4 || !dst3 || !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad tolab arguments");
  float mul[4], cm[12];
  if (monochrome) { ipk::srgb_d65_43(cm); mul[0] = mul[1] = mul[2] = mul[3] = 1.0f; }                     // colorspaces.rs:90-101
  else { std::memcpy(cm, cam_to_xyz_normalized, sizeof(cm)); ipk::normalize_wbs(wb_coeffs, mul); }
  // the fused kernels' per-pixel form (proven multiply/fma divisions, literal redo behind a wave-uniform branch) when the parameters
  // are finite and ordinary; else the literal kernel.  Round 2: 0.67 -> see DESIGN.md section 5 (the staged path of caching callers)
  bool ok = true;
  for (int i = 0; i < 4; ++i) ok = ok && std::fabs(mul[i]) <= 0x1p20f;
  for (int i = 0; i < 12; ++i) ok = ok && std::fabs(cm[i]) <= 0x1p20f;
  if (ok && width * height >= 256) {
    ipk::FusedLaunch f;
    std::memset(&f, 0, sizeof(f));
    f.src = src4; f.dst = dst3; f.mul4 = mul; f.cm12 = cm; f.rgbm9 = g_host.xyz_d65_33; f.fast_ok = 1; f.has_curve = 0; f.linear = 1;
    f.lab_table = cx().lut_plain[ipk::kLutXyzLab]; f.gam_table = cx().lut_plain[ipk::kLutGamma]; f.lab_pairs = cx().lut_pairs[ipk::kLutXyzLab]; f.gam_pairs = cx().lut_pairs[ipk::kLutGamma]; f.num_cus = cx().num_cus;
    ipk::launch_tolab_fast(f, width * height, S(stream));
  } else {
    ipk::launch_tolab(src4, width * height, mul, cm, cx().lut_pairs[ipk::kLutXyzLab], dst3, cx().num_cus, S(stream));
  }
  HIPCHK(hipGetLastError());
  return IPK_OK;
}

static int build_curve(float exposure, const float *points, int npoints, ipk::Spline &sp) {
  if (npoints < 0 || npoints > 64) return fail(IPK_ERR_INVALID, "curve with %d points (max 64)", npoints);
  float fp[128];
  const float m = std::exp2(exposure);                                                                    // curves.rs:38-41
  for (int i = 0; i < npoints; ++i) { fp[2 * i] = points[2 * i]; fp[2 * i + 1] = points[2 * i + 1] * m; }
  if (!sp.build(fp, npoints)) return fail(IPK_ERR_INVALID, "degenerate curve");
  return IPK_OK;
}
static bool curve_is_noop(float exposure, int npoints) { return npoints == 0 && std::fabs(exposure) < 0.001f; }   // curves.rs:34-36

int ipk_basecurve(const float *src3, size_t width, size_t height, float exposure, const float *points, int npoints,
                  float *dst3, void *stream) {
  REQUIRE_INIT();
  if (curve_is_noop(exposure, npoints)) return IPK_NOOP;
  if (!src3 || !dst3 || !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad basecurve arguments");
  ipk::Spline sp; int rc = build_curve(exposure, points, npoints, sp); if (rc) return rc;
  ipk::launch_basecurve(src3, width * height, sp, dst3, cx().num_cus, S(stream));
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_fromlab(const float *src3, size_t width, size_t height, float *dst3, void *stream) {
  REQUIRE_INIT();
  if (!src3 || !dst3 || !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad fromlab arguments");
  ipk::launch_fromlab(src3, width * height, g_host.xyz_d65_33, dst3, cx().num_cus, S(stream));
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_gamma(const float *src, size_t width, size_t height, size_t colors, int linear, float *dst, void *stream) {
  REQUIRE_INIT();
  if (linear) return IPK_NOOP;                                                                             // gamma.rs:17-18
  if (!src || !dst || !dims_ok(width, height) || colors < 1) return fail(IPK_ERR_INVALID, "bad gamma arguments");
  ipk::launch_gamma(src, width * height * colors, cx().lut_pairs[ipk::kLutGamma], dst, cx().num_cus, S(stream));
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_rotate_buffer(const float *src3, size_t bwidth, size_t bheight, int orientation, float *dst3,
                      size_t *out_width, size_t *out_height, void *stream) {
  return rotate_typed<float>(src3, bwidth, bheight, orientation, dst3, out_width, out_height, stream);
}
int ipk_rotate_image_u8(const uint8_t *src3, size_t bwidth, size_t bheight, int orientation, uint8_t *dst3,
                        size_t *out_width, size_t *out_height, void *stream) {
  return rotate_typed<uint8_t>(src3, bwidth, bheight, orientation, dst3, out_width, out_height, stream);
}
int ipk_rotate_image_u16(const uint16_t *src3, size_t bwidth, size_t bheight, int orientation, uint16_t *dst3,
                         size_t *out_width, size_t *out_height, void *stream) {
  return rotate_typed<uint16_t>(src3, bwidth, bheight, orientation, dst3, out_width, out_height, stream);
}
int ipk_transform(const float *src3, size_t width, size_t height, int rotation, int fliph, int flipv, float *dst3,
                  size_t *out_width, size_t *out_height, void *stream) {
  if (rotation < 0 || rotation > 3) return fail(IPK_ERR_INVALID, "bad rotation");
  const int o = ipk::transform_orientation(rotation, fliph != 0, flipv != 0);
  if (o == IPK_OR_NORMAL || o == IPK_OR_UNKNOWN) { *out_width = width; *out_height = height; return IPK_NOOP; }   // transform.rs:68-69
  return ipk_rotate_buffer(src3, width, height, o, dst3, out_width, out_height, stream);
}
int ipk_output8bit(const float *src, size_t n, uint8_t *dst, void *stream) {
  REQUIRE_INIT(); if (!src || !dst) return fail(IPK_ERR_INVALID, "null buffer");
  ipk::launch_output8(src, n, dst, cx().num_cus, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}
int ipk_output16bit(const float *src, size_t n, uint16_t *dst, void *stream) {
  REQUIRE_INIT(); if (!src || !dst) return fail(IPK_ERR_INVALID, "null buffer");
  ipk::launch_output16(src, n, dst, cx().num_cus, S(stream)); HIPCHK(hipGetLastError()); return IPK_OK;
}

// ------------------------------------------------------------------------------------------
// fused raw -> sRGB
// ------------------------------------------------------------------------------------------
namespace {
// what tolab..gamma need besides the pixels: normalised multipliers, the matrix, the curve, the tables -- and whether all of it
// is ordinary enough for the fast point-wise form (pointwise4_fast; otherwise the kernels evaluate the literal form)
struct PointwisePrep {
  float mul[4], cm[12];
  ipk::Spline sp;
  ipk::FusedLaunch f;                    // zeroed here, so a caller may fill in its own fields before or after prepare()
  PointwisePrep() { std::memset(&f, 0, sizeof(f)); }
  int prepare(int monochrome, const float *wb_coeffs, const float *cam_to_xyz_normalized, float exposure, const float *points, int npoints, int linear) {
    if (npoints < 0 || npoints > 64 || (npoints > 0 && !points)) return fail(IPK_ERR_INVALID, "npoints out of range");
    if (monochrome) { ipk::srgb_d65_43(cm); mul[0] = mul[1] = mul[2] = mul[3] = 1.0f; }                     // colorspaces.rs:90-101
    else { std::memcpy(cm, cam_to_xyz_normalized, sizeof(cm)); ipk::normalize_wbs(wb_coeffs, mul); }
    f.mul4 = mul; f.cm12 = cm; f.rgbm9 = g_host.xyz_d65_33;
    auto sane = [](float v) { return std::fabs(v) <= 0x1p20f; };
    bool ok = true;
    for (int i = 0; i < 4; ++i) ok = ok && sane(mul[i]);
    for (int i = 0; i < 12; ++i) ok = ok && sane(cm[i]);
    f.fast_ok = ok ? 1 : 0;
    f.has_curve = !curve_is_noop(exposure, npoints);
    if (f.has_curve) {
      int rc = build_curve(exposure, points, npoints, sp); if (rc) return rc;
      for (int i = 0; i < sp.npoints; ++i) if (!(std::fabs(sp.px[i]) <= 0x1p20f && std::fabs(sp.py[i]) <= 0x1p20f && std::fabs(sp.c1[i]) <= 0x1p40f)) f.fast_ok = 0;
      for (int i = 0; i < sp.nseg; ++i) if (!(std::fabs(sp.c2[i]) <= 0x1p40f && std::fabs(sp.c3[i]) <= 0x1p40f)) f.fast_ok = 0;
    }
    f.spline = &sp;
    f.linear = linear;
    f.lab_table = cx().lut_plain[ipk::kLutXyzLab]; f.gam_table = cx().lut_plain[ipk::kLutGamma]; f.lab_pairs = cx().lut_pairs[ipk::kLutXyzLab]; f.gam_pairs = cx().lut_pairs[ipk::kLutGamma];
    f.num_cus = cx().num_cus; f.gam_q8 = cx().lut_q8;
    return IPK_OK;
  }
};
}  // namespace

// Generic-CFA cell records for a launch in rotated space: the record of rotated-space pixel (y', x') is the record of the sensor
// pixel it came from (its taps stay in the sensor's order; the kernel renames the window).  The rotated pattern has the sensor
// pattern's dimensions swapped (transposing orientations) and a phase that depends on the frame size through the flips.
static int get_rot_cells(const char *pat, const ipk::Cfa &cfa, int ori, size_t width, size_t height, const float **out) {
  bool t, fx, fy;
  ipk::orientation_to_flips(ori, t, fx, fy);
  const int pw = cfa.width, ph = cfa.height;
  char key[160];
  snprintf(key, sizeof(key), "%s|%d|%d|%d", pat, ori, (int)(width % (size_t)pw), (int)(height % (size_t)ph));
  std::lock_guard<std::mutex> lk(cx().mu);
  auto it = cx().rot_cells.find(key);
  if (it != cx().rot_cells.end()) { *out = it->second; return IPK_OK; }
  std::vector<float> cells;
  if (!cfa.three_colour() || !cfa.gen_cells(cells)) return fail(IPK_ERR_UNSUPPORTED, "CFA has a fourth colour");
  const int rpw = t ? ph : pw, rph = t ? pw : ph;          // rotated pattern: width follows the sensor rows when transposed
  std::vector<float> rot((size_t)rpw * rph * ipk::Cfa::kGenCellFloats);
  for (int y = 0; y < rph; ++y)
    for (int x = 0; x < rpw; ++x) {
      const int64_t ro = t ? (fy ? (int64_t)height - 1 - x : x) : (fy ? (int64_t)height - 1 - y : y);
      const int64_t co = t ? (fx ? (int64_t)width - 1 - y : y) : (fx ? (int64_t)width - 1 - x : x);
      const int sy = (int)(((ro % ph) + ph) % ph), sx = (int)(((co % pw) + pw) % pw);
      std::memcpy(&rot[((size_t)y * rpw + x) * ipk::Cfa::kGenCellFloats], &cells[((size_t)sy * pw + sx) * ipk::Cfa::kGenCellFloats], ipk::Cfa::kGenCellFloats * sizeof(float));
    }
  float *dev = nullptr;
  HIPCHK(hipMalloc(reinterpret_cast<void **>(&dev), rot.size() * sizeof(float)));
  HIPCHK(hipMemcpy(dev, rot.data(), rot.size() * sizeof(float), hipMemcpyHostToDevice));
  cx().rot_cells[key] = dev;
  *out = dev;
  return IPK_OK;
}

// ori = 0: the frame as it is.  ori = Rotate90 / Rotate270 (Bayer filters, whole frames): the mosaic is first permuted into the
// output orientation (1 channel: 2 or 4 bytes per pixel instead of the 12 of the result) and the kernel works in rotated space,
// so that dst receives OpTransform's output directly; IPK_ERR_UNSUPPORTED (nothing launched) when no such variant exists.
// nbatch > 0: the frames srcs[0..nbatch) -> dsts[0..nbatch), all with the geometry and parameters of *p (src / dst = the first pair)
// win_c1 > 0: a region -- only the columns [win_c0, win_c1) of the band's rows are computed and stored, packed, into dst (ori 0, one frame)
// four_ok: the entry point honours p->four_colour (ipk_raw_to_srgb, its batch and host forms, the region launch say so); every other caller, and any
// added later, refuses a fourth colour whatever the field says
struct FusedOpts {
  size_t nbatch = 0; const void *const *srcs = nullptr; void *const *dsts = nullptr;
  bool probe = false;
  size_t win_c0 = 0, win_c1 = 0;
  bool four_ok = false;
};
static int fused_impl(const ipk_fused_params *p, const void *src, void *dst, void *stream, int ori, const FusedOpts &o = FusedOpts()) {
  const size_t nbatch = o.nbatch, win_c0 = o.win_c0, win_c1 = o.win_c1;
  const void *const *const srcs = o.srcs; void *const *const dsts = o.dsts;
  const bool probe = o.probe, four_ok = o.four_ok;
  REQUIRE_INIT();
  if (!p || !src || !dst) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_fused_params, p)
  if (p->src_type != IPK_SRC_U16 && p->src_type != IPK_SRC_F32) return fail(IPK_ERR_INVALID, "fused path takes u16 or f32 CFA data");
  if (!dims_ok(p->width, p->height) || p->owidth < p->x + p->width) return fail(IPK_ERR_INVALID, "bad geometry");
  if (p->out_type < 0 || p->out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if (p->four_colour != 0 && p->four_colour != 1) return fail(IPK_ERR_INVALID, "four_colour must be 0 or 1 (got %d)", p->four_colour);
  ipk::Cfa cfa; DevCfa dev;
  { int rc = get_cfa(p->cfa, cfa, dev); if (rc) return rc; }
  int xoff = 0, yoff = 0;
  const bool bayer = cfa.bayer_phase(xoff, yoff);
  const bool four = !cfa.three_colour();
  if (four && !(four_ok && p->four_colour == 1 && ori == 0 && !probe && dev.gen_cells))
    return fail(IPK_ERR_UNSUPPORTED, (four_ok && ori == 0 && !probe) ? "CFA \"%s\" has a fourth colour; set four_colour = 1, or run the staged ops"
                                                                     : "CFA \"%s\" has a fourth colour; run the staged ops", p->cfa);
  if (!bayer && !dev.gen_cells) return fail(IPK_ERR_UNSUPPORTED, "CFA \"%s\": no cell records; run the staged ops", p->cfa);

  PointwisePrep pp;
  ipk::FusedLaunch &f = pp.f;
  const size_t esz = p->src_type == IPK_SRC_U16 ? 2 : 4;
  const bool band = p->band_out_rows != 0;
  f.row_off = band ? p->band_src_row0 : 0;
  f.out_r0 = band ? p->band_out_row0 : 0;
  f.out_r1 = band ? p->band_out_row0 + p->band_out_rows : p->height;
  if (f.out_r1 > p->height || f.out_r0 >= f.out_r1) return fail(IPK_ERR_INVALID, "band rows outside the frame");
  if (band) {
    const size_t need0 = f.out_r0 > 0 ? f.out_r0 - 1 : 0, need1 = std::min(p->height, f.out_r1 + 1);
    if (p->band_src_row0 > need0 || p->band_src_row0 + p->band_src_rows < need1)
      return fail(IPK_ERR_INVALID, "band source rows do not cover the 1-row halo");
  }
  // whole frame: src is sensor element (0,0) -> skip the top crop; band: src already starts at sensor row y+band_src_row0
  const char *base = static_cast<const char *>(src) + ((band ? 0 : p->y * p->owidth) + p->x) * esz;
  f.src = base; f.dst = dst;
  f.src_is_u16 = p->src_type == IPK_SRC_U16;
  f.src_aligned4 = (reinterpret_cast<uintptr_t>(base) % 4 == 0) && (p->owidth % 2 == 0);
  f.batch_n = 0; f.batch_src = nullptr; f.batch_dst = nullptr;
  std::vector<const void *> bases;
  if (nbatch) {
    const size_t off = static_cast<size_t>(base - static_cast<const char *>(src));
    for (size_t i = 0; i < nbatch; ++i) {
      if (!srcs[i] || !dsts[i]) return fail(IPK_ERR_INVALID, "null frame pointer in the batch");
      bases.push_back(static_cast<const char *>(srcs[i]) + off);
      f.src_aligned4 = f.src_aligned4 && reinterpret_cast<uintptr_t>(bases.back()) % 4 == 0;
    }
    f.batch_n = (int)nbatch; f.batch_src = bases.data(); f.batch_dst = dsts;
  }
  f.width = p->width; f.height = p->height; f.owidth = p->owidth;
  f.ori = 0; f.roles[0] = f.roles[1] = f.roles[2] = f.roles[3] = 0;
  Scratch rot(S(stream));
  if (ori != 0) {
    bool t, fx, fy;
    ipk::orientation_to_flips(ori, t, fx, fy);
    if (band || ori < 1 || ori > 7 || (t ? p->height : p->width) < 256 ||             // the rotated frame must be at least one 256-pixel strip wide
        (t && p->width > ipk::kRotate1MaxTransposedRows))                              // and no taller than the transposing permutation's grid
      return fail(IPK_ERR_UNSUPPORTED, "no rotated-space variant for this frame");
    // rotate_buffer's index walk (transform.rs:102-128) over the crop window of the pitched 1-channel source
    int64_t width = (int64_t)p->width, height = (int64_t)p->height, x_step = 1, y_step = (int64_t)p->owidth, off = 0;
    if (fx) { x_step = -x_step; off += width - 1; }
    if (fy) { y_step = -y_step; off += (int64_t)p->owidth * (height - 1); }
    if (t) { std::swap(width, height); std::swap(x_step, y_step); }
    void *m = nullptr;
    int rc = rot.get((size_t)width * (size_t)height * esz, &m); if (rc) return rc;
    if (f.src_is_u16) ipk::launch_rotate1<uint16_t>(reinterpret_cast<const uint16_t *>(base), (size_t)width, (size_t)height, off, x_step, y_step, static_cast<uint16_t *>(m), S(stream));
    else ipk::launch_rotate1<float>(reinterpret_cast<const float *>(base), (size_t)width, (size_t)height, off, x_step, y_step, static_cast<float *>(m), S(stream));
    HIPCHK(hipGetLastError());
    // the demosaic role of a rotated-space pixel = the role of the sensor pixel it came from: depends on the parities only
    for (int pr = 0; pr < 2; ++pr) for (int pc = 0; pc < 2; ++pc) {
      const int64_t ro = t ? (fy ? (int64_t)p->height - 1 - pc : pc) : (fy ? (int64_t)p->height - 1 - pr : pr);
      const int64_t co = t ? (fx ? (int64_t)p->width - 1 - pr : pr) : (fx ? (int64_t)p->width - 1 - pc : pc);
      f.roles[2 * pr + pc] = (int)((((ro + yoff) & 1) << 1) | ((co + xoff) & 1));
    }
    f.ori = ori;
    f.src = m; f.src_aligned4 = (width % 2 == 0);
    f.width = (size_t)width; f.height = (size_t)height; f.owidth = (size_t)width;
    f.out_r0 = 0; f.out_r1 = (size_t)height; f.row_off = 0;
    xoff = 0; yoff = 0;
  }
  f.black0 = p->black0; f.white0 = p->white0;
  f.exact_norm = validate_cdiv_for_range(p->black0, p->white0 - p->black0, f.src_is_u16) ? 0 : 1;
  f.xoff = xoff; f.yoff = yoff;
  f.gen_cells = bayer ? nullptr : dev.gen_cells; f.gen_pw = dev.gen_pw; f.gen_ph = dev.gen_ph;
  if (ori != 0 && !bayer) {                                // rotated space: the pattern's dimensions swap, the records follow the sensor pixels
    const float *rc_dev = nullptr;
    int rc = get_rot_cells(p->cfa, cfa, ori, p->width, p->height, &rc_dev); if (rc) return rc;
    bool tt, fxx, fyy; ipk::orientation_to_flips(ori, tt, fxx, fyy);
    f.gen_cells = rc_dev;
    if (tt) { f.gen_pw = dev.gen_ph; f.gen_ph = dev.gen_pw; }
  }
  // generic-CFA mode sums up to nine normalised samples and divides by a constant: u16 kernels check their samples only
  // when the levels allow one outside [2^-60, 2^60] (f32 kernels always check)
  f.gen_check = (!bayer && f.src_is_u16 && !gen_levels_ok_u16(p->black0, p->white0 - p->black0)) ? 1 : 0;
  f.four = four ? 1 : 0;                                   // a fourth colour: literal demosaic with a fourth bin, literal point-wise form (launch_fused_bayer)
  // the point-wise stages' share -- multipliers, matrix, curve, fast_ok, tables -- as every other launch of the chain prepares it
  { int rc = pp.prepare(0, p->wb_coeffs, p->cam_to_xyz_normalized, p->exposure, p->points, p->npoints, p->linear); if (rc) return rc; }
  {
    // when the samples (u16: all 65 536 walked here; f32: bounded below through the black level), the multipliers and the matrix
    // are ordinary (see pointwise4_fast in ipk_kernels.hip), the kernel variant without per-pixel input guards is legal
    const float range = p->white0 - p->black0;
    bool plain = bayer && range > 0.0f && std::fabs(pp.mul[3]) <= 0x1p20f;                               // (the fourth multiplier: finite and ordinary is enough)
    if (f.src_is_u16) plain = plain && gen_levels_ok_u16(p->black0, range);                       // every nonzero sample >= 2^-20 in magnitude
    else plain = plain && std::fabs(p->black0) >= range * 0x1p-6f && std::fabs(p->black0) <= 0x1p70f;   // every nonzero sample >= 2^-31
    for (int i = 0; i < 3; ++i) plain = plain && pp.mul[i] >= 0x1p-4f && pp.mul[i] <= 0x1p10f;
    for (int i = 0; i < 12; ++i) { const float c = std::fabs(pp.cm[i]); plain = plain && (c == 0.0f || (c >= 0x1p-12f && c <= 0x1p20f)); }
    f.px_guard = plain ? 0 : 1;
  }
  f.out_type = probe ? 4 : p->out_type;
  f.queues = cx().queues;
  if (p->schedule != IPK_SCHED_AUTO && p->schedule != IPK_SCHED_SPLIT) return fail(IPK_ERR_INVALID, "bad schedule");
  f.schedule = p->schedule;
  if (win_c1 != 0 && (ori != 0 || nbatch || probe || win_c0 >= win_c1 || win_c1 > p->width)) return fail(IPK_ERR_INVALID, "bad column window");
  f.win_c0 = win_c0; f.win_c1 = win_c1;
  { const int lrc = ipk::launch_fused_bayer(f, S(stream));
    if (lrc == -4) return fail(IPK_ERR_HIP, "kernel launch failed (nothing was enqueued; the stream's task queue is untouched)");
    if (lrc != 0) return fail(IPK_ERR_UNSUPPORTED, probe ? "the stream probe exists for Bayer frames of 256+ columns with validated levels" : "no rotated-space variant for these parameters"); }
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_raw_to_srgb(const ipk_fused_params *p, const void *src, void *dst, void *stream) { FusedOpts o; o.four_ok = true; return fused_impl(p, src, dst, stream, 0, o); }
// Measurement aid: the fused kernel's memory skeleton (its launch, task walk, row loads, OpGoFloat, demosaic::full, LDS staging, nontemporal stores) without
// the point-wise stages -- dst receives the demosaiced R, G, B as width*rows*3 f32.  bench.py times it next to ipk_raw_to_srgb (roofline.ceiling_ms).
int ipk_stream_probe(const ipk_fused_params *p, const void *src, void *dst, void *stream) {
  IPK_FOLD_CFA(ipk_fused_params, p)
  if (p && p->band_out_rows != 0) return fail(IPK_ERR_INVALID, "the stream probe takes whole frames");
  FusedOpts o; o.probe = true;
  return fused_impl(p, src, dst, stream, 0, o);
}
// A batch of same-shaped frames through one descriptor: Pipeline::run over a shoot.  One persistent launch per 64 frames where the
// kernel has a batch variant (ordinary Bayer parameters), one launch per frame otherwise -- the results are the single-frame ones.
int ipk_raw_to_srgb_batch(const ipk_fused_params *p, const void *const *srcs, void *const *dsts, size_t n, void *stream) {
  if (!p || (n && (!srcs || !dsts))) return fail(IPK_ERR_INVALID, "null argument");
  if (n == 0) return IPK_OK;
  if (n > (size_t)1 << 20) return fail(IPK_ERR_INVALID, "batch too large");
  IPK_FOLD_CFA(ipk_fused_params, p)
  if (p->band_out_rows != 0) return fail(IPK_ERR_INVALID, "a batch takes whole frames, not bands");
  FusedOpts o; o.nbatch = n; o.srcs = srcs; o.dsts = dsts; o.four_ok = true;
  return fused_impl(p, srcs[0], dsts[0], stream, 0, o);
}
int ipk_raw_to_srgb_oriented(const ipk_fused_params *p, const void *src, int orientation, void *dst, size_t *out_width, size_t *out_height, void *stream) {
  if (!p || !out_width || !out_height) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_fused_params, p)
  // (a fourth colour is refused here for every orientation: the rotated-space variants compile the fast point-wise form in, and callers with a Normal
  // orientation have ipk_raw_to_srgb)
  if (orientation == IPK_OR_NORMAL || orientation == IPK_OR_UNKNOWN) { *out_width = p->width; *out_height = p->height; return fused_impl(p, src, dst, stream, 0); }
  if (orientation < 0 || orientation > 8) return fail(IPK_ERR_INVALID, "bad orientation");
  { bool t, fx, fy; ipk::orientation_to_flips(orientation, t, fx, fy); *out_width = t ? p->height : p->width; *out_height = t ? p->width : p->height; }
  return fused_impl(p, src, dst, stream, orientation);
}

// OpToLab::run + OpBaseCurve::run + OpFromLab::run + OpGamma::run (colorspaces.rs:89-112, curves.rs:33-49, colorspaces.rs:127-137,
// gamma.rs:16-26) in one pass: what Pipeline::run computes between rotatecrop and transform when no cache needs the
// intermediate buffers.

int ipk_pointwise_chain(const float *src4, size_t width, size_t height, int monochrome, const float *wb_coeffs, const float *cam_to_xyz_normalized,
                        float exposure, const float *points, int npoints, int linear, float *dst3, void *stream) {
  REQUIRE_INIT();
  if (!src4 || !dst3 || !wb_coeffs || !cam_to_xyz_normalized || !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad pointwise_chain arguments");
  PointwisePrep pp;
  int rc = pp.prepare(monochrome, wb_coeffs, cam_to_xyz_normalized, exposure, points, npoints, linear); if (rc) return rc;
  pp.f.src = src4; pp.f.dst = dst3;
  ipk::launch_pointwise_chain(pp.f, width * height, S(stream));
  HIPCHK(hipGetLastError());
  return IPK_OK;
}

// the same followed by output8bit / output16bit (src/pipeline.rs:408-414, :455-461) in one pass: what output_8bit / output_16bit compute behind a staged
// demosaic (a preview under a size limit, an X-Trans or four-colour frame) without the f32 image in between
int ipk_pointwise_chain_out(const float *src4, size_t width, size_t height, int monochrome, const float *wb_coeffs, const float *cam_to_xyz_normalized,
                            float exposure, const float *points, int npoints, int linear, int out_type, void *dst, void *stream) {
  REQUIRE_INIT();
  if (!src4 || !dst || !wb_coeffs || !cam_to_xyz_normalized || !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad pointwise_chain_out arguments");
  if (out_type == IPK_OUT_F32) return ipk_pointwise_chain(src4, width, height, monochrome, wb_coeffs, cam_to_xyz_normalized, exposure, points, npoints, linear, static_cast<float *>(dst), stream);
  if (out_type != IPK_OUT_U8 && out_type != IPK_OUT_U16) return fail(IPK_ERR_INVALID, "bad out_type");
  if (width * height < 256) return fail(IPK_ERR_UNSUPPORTED, "pointwise_chain_out needs at least 256 pixels (use ipk_pointwise_chain + ipk_output8bit / 16bit)");
  PointwisePrep pp;
  int rc = pp.prepare(monochrome, wb_coeffs, cam_to_xyz_normalized, exposure, points, npoints, linear); if (rc) return rc;
  pp.f.src = src4; pp.f.dst = dst; pp.f.out_type = out_type;
  if (ipk::launch_chain_quantised(pp.f, width * height, S(stream)) != 0) return fail(IPK_ERR_UNSUPPORTED, "pointwise_chain_out: frame too small");
  HIPCHK(hipGetLastError());
  return IPK_OK;
}

int ipk_raster_to_srgb(const void *src, int src_type, size_t width, size_t height, const float *wb_coeffs, const float *cam_to_xyz_normalized,
                       float exposure, const float *points, int npoints, int linear, int out_type, void *dst, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst || !wb_coeffs || !cam_to_xyz_normalized || !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad raster_to_srgb arguments");
  if (src_type != IPK_SRC_RGB8 && src_type != IPK_SRC_RGB16) return fail(IPK_ERR_INVALID, "raster_to_srgb takes RGB8 or RGB16 sources");
  if (out_type < 0 || out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if (width * height < 256) return fail(IPK_ERR_UNSUPPORTED, "raster_to_srgb needs at least 256 pixels (use the staged ops)");
  PointwisePrep pp;
  int rc = pp.prepare(0, wb_coeffs, cam_to_xyz_normalized, exposure, points, npoints, linear); if (rc) return rc;
  pp.f.src = src; pp.f.dst = dst; pp.f.out_type = out_type;
  if (ipk::launch_raster_chain(pp.f, width * height, src_type == IPK_SRC_RGB16, cx().lut_pairs[ipk::kLutGammaReverse], S(stream)) != 0)
    return fail(IPK_ERR_UNSUPPORTED, "raster_to_srgb: frame too small");
  HIPCHK(hipGetLastError());
  return IPK_OK;
}

// The same launch over a rectangle of any source whose OpDemosaic is a pass-through: rasters, three-sample and monochrome u16 raws (runtime modes of
// k_raster_chain<uint8_t | uint16_t>; no kernel of its own, and none for f32 raws, which stay staged)
int ipk_plain_to_srgb(const void *src, int src_type, int kind, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                      const float *black4, const float *white4, const float *wb_coeffs, const float *cam_to_xyz_normalized,
                      float exposure, const float *points, int npoints, int linear, int out_type, void *dst, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst || !wb_coeffs || !cam_to_xyz_normalized || !dims_ok(width, height) || !dims_ok(owidth, 1) || y >= (1ull << 31))
    return fail(IPK_ERR_INVALID, "bad plain_to_srgb arguments");
  if (kind != IPK_PLAIN_RASTER && kind != IPK_PLAIN_RGB && kind != IPK_PLAIN_MONO) return fail(IPK_ERR_INVALID, "bad plain kind");
  if (out_type < 0 || out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if (x > owidth || width > owidth - x) return fail(IPK_ERR_INVALID, "the rectangle's columns [%zu, %zu) leave the %zu-wide source", x, x + width, owidth);
  if (src_type == IPK_SRC_F32) return fail(IPK_ERR_UNSUPPORTED, "plain_to_srgb has no f32 form (run the staged ops)");
  if (kind == IPK_PLAIN_RASTER ? (src_type != IPK_SRC_RGB8 && src_type != IPK_SRC_RGB16) : src_type != IPK_SRC_U16)
    return fail(IPK_ERR_INVALID, "plain_to_srgb takes RGB8 / RGB16 rasters and u16 three-sample / monochrome raws");
  if (kind != IPK_PLAIN_RASTER && (!black4 || !white4)) return fail(IPK_ERR_INVALID, "plain_to_srgb: a raw source needs its levels");
  if (width * height < 256) return fail(IPK_ERR_UNSUPPORTED, "plain_to_srgb needs at least 256 pixels (use the staged ops)");
  PointwisePrep pp;
  int rc = pp.prepare(kind == IPK_PLAIN_MONO, wb_coeffs, cam_to_xyz_normalized, exposure, points, npoints, linear); if (rc) return rc;
  const size_t spp = kind == IPK_PLAIN_MONO ? 1 : 3, esz = src_type == IPK_SRC_RGB8 ? 1 : 2;
  pp.f.src = static_cast<const char *>(src) + (y * owidth + x) * spp * esz;         // the rectangle's first sample
  pp.f.dst = dst; pp.f.out_type = out_type;
  ipk::PlainSource ps;
  ps.levels = kind; ps.owidth = owidth; ps.width = width;
  for (int c = 0; c < 3; ++c) { ps.black[c] = kind == IPK_PLAIN_RASTER ? 0.0f : black4[c]; ps.white[c] = kind == IPK_PLAIN_RASTER ? 0.0f : white4[c]; }
  if (ipk::launch_raster_chain(pp.f, width * height, src_type != IPK_SRC_RGB8, cx().lut_pairs[ipk::kLutGammaReverse], S(stream), &ps) != 0)
    return fail(IPK_ERR_UNSUPPORTED, "plain_to_srgb: the launch refused this rectangle");
  HIPCHK(hipGetLastError());
  return IPK_OK;
}

// The sensor-source half of a k_fused_resample set-up: the cropped frame's first sample and geometry, the levels, and whether gofloat's division must be a
// true one
static void fused_sensor_source(ipk::FusedLaunch &f, const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height,
                                float black0, float white0) {
  f.src_is_u16 = src_type == IPK_SRC_U16;
  f.src = static_cast<const char *>(src) + (y * owidth + x) * (f.src_is_u16 ? 2 : 4);
  f.width = width; f.height = height; f.owidth = owidth;
  f.black0 = black0; f.white0 = white0;
  f.exact_norm = validate_cdiv_for_range(black0, white0 - black0, f.src_is_u16) ? 0 : 1;
}
// The launch behind ipk_raw_to_srgb_resampled (corners: its six corner coordinates) and ipk_raw_to_srgb_scaled (corners == NULL: scale_down_opbuf's
// transform), k_fused_resample: the checks both share, then the plan from the cropped frame's sides, or the refusal (nothing is enqueued then)
// win (the window forms): the rectangle of the nwidth x nheight result the launch is laid over; dst then holds exactly its pixels
static int resampled_launch(const ipk_fused_params *p, const void *src, const int64_t *corners, size_t nwidth, size_t nheight, void *dst, void *stream,
                            const char *what, const char *refusal, const ipk::ResampleWindow *win = nullptr) {
  REQUIRE_INIT();
  if (!p || !src || !dst) return fail(IPK_ERR_INVALID, "null argument");
  if (win && (win->cols == 0 || win->rows == 0 || win->col0 > nwidth || win->cols > nwidth - win->col0 || win->row0 > nheight || win->rows > nheight - win->row0))
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", win->col0, win->row0, win->cols, win->rows, nwidth, nheight);
  IPK_FOLD_CFA(ipk_fused_params, p)
  if (p->src_type != IPK_SRC_U16 && p->src_type != IPK_SRC_F32) return fail(IPK_ERR_INVALID, "the %s fused path takes u16 or f32 CFA data", what);
  if (!dims_ok(p->width, p->height) || p->owidth < p->x + p->width) return fail(IPK_ERR_INVALID, "bad geometry");
  if (p->out_type < 0 || p->out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if (p->band_out_rows != 0) return fail(IPK_ERR_INVALID, "the %s fused path takes whole frames, not bands", what);
  if (p->four_colour != 0 && p->four_colour != 1) return fail(IPK_ERR_INVALID, "four_colour must be 0 or 1 (got %d)", p->four_colour);
  ipk::Cfa cfa; DevCfa dev;
  { int rc = get_cfa(p->cfa, cfa, dev); if (rc) return rc; }
  if (!cfa.three_colour()) return fail(IPK_ERR_UNSUPPORTED, "CFA \"%s\" has a fourth colour; run the staged ops", p->cfa);
  ipk::ResamplePlan plan;
  const bool admitted = corners ? ipk::resample_plan(p->width, p->height, corners[0], corners[1], corners[2], corners[3], corners[4], corners[5], nwidth, nheight, plan)
                                : ipk::scaledown_plan(p->width, p->height, nwidth, nheight, plan);
  if (!admitted) return fail(IPK_ERR_UNSUPPORTED, "%s", refusal);
  PointwisePrep pp;
  { int rc = pp.prepare(0, p->wb_coeffs, p->cam_to_xyz_normalized, p->exposure, p->points, p->npoints, p->linear); if (rc) return rc; }
  fused_sensor_source(pp.f, src, p->src_type, p->owidth, p->x, p->y, p->width, p->height, p->black0, p->white0);
  pp.f.dst = dst;
  pp.f.out_type = p->out_type;
  if (ipk::launch_fused_resample(pp.f, plan, nwidth, nheight, dev.lookups, S(stream), win) != 0)
    return fail(IPK_ERR_HIP, "kernel launch failed (nothing was enqueued)");
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
static const char *const kResampledRefusal =
    "not a transform the resampled fused path takes (output sides >= 2, finite skips whose magnitudes sum to less than 2 per axis, sides below 2^24); run the staged ops";
static const char *const kScaledRefusal =
    "not a size the scaled fused path takes (output sides >= 2, both skips (side - 1) / (new side - 1) at least 1 and below 3, sides below 2^24); run the staged ops";
// ipk_raw_to_srgb with scaling::transform_buffer (src/scaling.rs:51-130) between demosaic::full and OpToLab, the corner points being the three
// OpRotateCrop::run computes (src/ops/rotatecrop.rs:39-64): one launch (k_fused_resample).  Arguments as for ipk_transform_buffer_f32.
int ipk_raw_to_srgb_resampled(const ipk_fused_params *p, const void *src, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                              int64_t blx, int64_t bly, size_t nwidth, size_t nheight, void *dst, void *stream) {
  const int64_t corners[6] = {tlx, tly, trx, try_, blx, bly};
  return resampled_launch(p, src, corners, nwidth, nheight, dst, stream, "resampled", kResampledRefusal);
}
// ipk_raw_to_srgb with scale_down_opbuf(nwidth, nheight) (src/scaling.rs:35-48: transform_buffer with the corners (0, 0), (width - 1, 0), (0, height - 1))
// between demosaic::full and OpToLab -- OpDemosaic::run's last branch (src/ops/demosaic.rs:51-59) -- in the same launch, its axis-aligned mode
int ipk_raw_to_srgb_scaled(const ipk_fused_params *p, const void *src, size_t nwidth, size_t nheight, void *dst, void *stream) {
  return resampled_launch(p, src, nullptr, nwidth, nheight, dst, stream, "scaled", kScaledRefusal);
}
// the window forms of the two: the same launch laid over the rectangle [wx, wx + ww) x [wy, wy + wh) of the result (ResampleWindow)
int ipk_raw_to_srgb_resampled_window(const ipk_fused_params *p, const void *src, int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                     size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, void *dst, void *stream) {
  const int64_t corners[6] = {tlx, tly, trx, try_, blx, bly};
  const ipk::ResampleWindow win = {wy, wx, wh, ww};
  return resampled_launch(p, src, corners, nwidth, nheight, dst, stream, "resampled", kResampledRefusal, &win);
}
int ipk_raw_to_srgb_scaled_window(const ipk_fused_params *p, const void *src, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh,
                                  void *dst, void *stream) {
  const ipk::ResampleWindow win = {wy, wx, wh, ww};
  return resampled_launch(p, src, nullptr, nwidth, nheight, dst, stream, "scaled", kScaledRefusal, &win);
}
// OpGoFloat (CFA branch) + OpDemosaic::run's `full` + scale_down_opbuf branch (demosaic.rs:51-59) in one launch, into the nwidth x nheight 4-channel f32
// buffer ipk_gofloat_cfa_* -> ipk_demosaic_run write for such a frame, bit for bit: k_fused_resample's axis walk in its RGBE output mode (no chain, no
// quantiser).  The sibling of ipk_raw_scaled_demosaic for the scales below minscale; win: that rectangle of the result alone, packed.  A filter with a
// fourth colour (E is not +0.0 there) and geometry scaledown_plan refuses get IPK_ERR_UNSUPPORTED with nothing enqueued
static int raw_demosaic_scaled_impl(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, float black0, float white0,
                                    const char *cfa_pat, size_t nwidth, size_t nheight, const ipk::ResampleWindow *win, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst4 || !cfa_pat || !dims_ok(width, height) || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32) || owidth < x + width)
    return fail(IPK_ERR_INVALID, "bad raw_demosaic_scaled arguments");
  if (win && !window_ok(nwidth, nheight, win->col0, win->row0, win->cols, win->rows))
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", win->col0, win->row0, win->cols, win->rows, nwidth, nheight);
  ipk::Cfa cfa; DevCfa dev;
  { int rc = get_cfa(cfa_pat, cfa, dev); if (rc) return rc; }
  if (!cfa.three_colour()) return fail(IPK_ERR_UNSUPPORTED, "CFA \"%s\" has a fourth colour; run the staged ops", cfa_pat);
  ipk::ResamplePlan plan;
  if (!ipk::scaledown_plan(width, height, nwidth, nheight, plan)) return fail(IPK_ERR_UNSUPPORTED, "%s", kScaledRefusal);
  PointwisePrep pp;                                                          // the mode reads none of the point-wise parameters: any ordinary set
  { int rc = pp.prepare(1, nullptr, nullptr, 0.0f, nullptr, 0, 1); if (rc) return rc; }
  fused_sensor_source(pp.f, src, src_type, owidth, x, y, width, height, black0, white0);
  pp.f.dst = dst4;
  pp.f.out_type = IPK_OUT_F32;
  if (ipk::launch_fused_resample(pp.f, plan, nwidth, nheight, dev.lookups, S(stream), win, 0, 1) != 0)
    return fail(IPK_ERR_HIP, "kernel launch failed (nothing was enqueued)");
  HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_raw_demosaic_scaled(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, float black0, float white0,
                            const char *cfa_pat, size_t nwidth, size_t nheight, float *dst4, void *stream) {
  return raw_demosaic_scaled_impl(src, src_type, owidth, x, y, width, height, black0, white0, cfa_pat, nwidth, nheight, nullptr, dst4, stream);
}
int ipk_raw_demosaic_scaled_window(const void *src, int src_type, size_t owidth, size_t x, size_t y, size_t width, size_t height, float black0, float white0,
                                   const char *cfa_pat, size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, float *dst4, void *stream) {
  const ipk::ResampleWindow win = {wy, wx, wh, ww};
  return raw_demosaic_scaled_impl(src, src_type, owidth, x, y, width, height, black0, white0, cfa_pat, nwidth, nheight, &win, dst4, stream);
}
// what such a window reads of the cropped frame (host only): ipk::resample_footprint on the skips of the corners
int ipk_transform_window_footprint(size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_, int64_t blx, int64_t bly,
                                   size_t nwidth, size_t nheight, size_t wx, size_t wy, size_t ww, size_t wh, size_t *out4) {
  if (!out4) return fail(IPK_ERR_INVALID, "null argument");
  ipk::ResamplePlan plan;
  if (!ipk::resample_skips(width, height, tlx, tly, trx, try_, blx, bly, nwidth, nheight, plan))
    return fail(IPK_ERR_UNSUPPORTED, "not a transform the fused paths take (output sides >= 2, finite skips, sides below 2^24)");
  if (ww == 0 || wh == 0 || wx > nwidth || ww > nwidth - wx || wy > nheight || wh > nheight - wy)
    return fail(IPK_ERR_INVALID, "window (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", wx, wy, ww, wh, nwidth, nheight);
  const ipk::ResampleFootprint f = ipk::resample_footprint(plan, width, height, wy, wx, wh, ww);
  out4[0] = f.x; out4[1] = f.y; out4[2] = f.w; out4[3] = f.h;
  return IPK_OK;
}

// ------------------------------------------------------------------------------------------
// self-test hooks
// ------------------------------------------------------------------------------------------
static int selftest_collect(void *dev, uint64_t *n_bad, uint32_t *first_bad) {
  struct { unsigned long long bad; unsigned int first; unsigned int pad; } h;
  HIPCHK(hipMemcpy(&h, dev, sizeof(h), hipMemcpyDeviceToHost));
  (void)hipFree(dev);
  *n_bad = h.bad; if (first_bad) *first_bad = h.first;
  return IPK_OK;
}
static int selftest_alloc(void **dev) {
  struct { unsigned long long bad; unsigned int first; unsigned int pad; } h = {0, 0xFFFFFFFFu, 0};
  HIPCHK(hipMalloc(dev, sizeof(h)));
  HIPCHK(hipMemcpy(*dev, &h, sizeof(h), hipMemcpyHostToDevice));
  return IPK_OK;
}
int ipk_selftest_cdiv(float c, int variant, float lo, float hi, int include_special, uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  if (!(c > 0.0f) || variant < 0 || variant > 2 || !n_bad) return fail(IPK_ERR_INVALID, "bad selftest arguments");
  uint32_t lo_bits, hi_bits; std::memcpy(&lo_bits, &lo, 4); std::memcpy(&hi_bits, &hi, 4);
  void *dev; int rc = selftest_alloc(&dev); if (rc) return rc;
  ipk::launch_selftest_cdiv(c, variant, lo_bits, hi_bits, include_special, dev, nullptr);
  HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_selftest_lut_weight(uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  void *dev; int rc = selftest_alloc(&dev); if (rc) return rc;
  ipk::launch_selftest_fract(dev, nullptr); HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_selftest_clamp01(uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  void *dev; int rc = selftest_alloc(&dev); if (rc) return rc;
  ipk::launch_selftest_clamp(dev, nullptr); HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_copy_probe(const void *src, void *dst, size_t bytes, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst || (bytes & 15) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return fail(IPK_ERR_INVALID, "ipk_copy_probe wants 16-byte aligned buffers and a multiple of 16 bytes");
  ipk::launch_copy_probe(src, dst, bytes, cx().num_cus, S(stream)); HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_mix_probe(const void *src, void *dst, size_t src_bytes, void *stream) {
  REQUIRE_INIT();
  if (!src || !dst || (src_bytes & 4095) || ((uintptr_t)src & 15) || ((uintptr_t)dst & 15)) return fail(IPK_ERR_INVALID, "ipk_mix_probe wants 16-byte aligned buffers and a multiple of 4096 source bytes (whole blocks)");
  ipk::launch_mix_probe(src, dst, src_bytes, S(stream)); HIPCHK(hipGetLastError());
  return IPK_OK;
}
int ipk_clock_probe(uint64_t *out2_dev, uint32_t spin_us, void *stream) {
  REQUIRE_INIT();
  if (!out2_dev || spin_us == 0 || spin_us > 2000000u) return fail(IPK_ERR_INVALID, "ipk_clock_probe: null output or a spin outside (0, 2 s]");
  ipk::launch_clock_probe(out2_dev, (unsigned long long)spin_us * 100ull, S(stream)); HIPCHK(hipGetLastError());
  return IPK_OK;
}
// no REQUIRE_INIT: the log is host state, and an empty log needs no device
int ipk_selftest_launch_log(int enabled) { ipk::launch_log_enable(enabled != 0); return IPK_OK; }
size_t ipk_selftest_launch_log_read(char *buf, size_t cap) { return ipk::launch_log_read(buf, cap); }
int ipk_selftest_task_queue(int enabled) { REQUIRE_INIT(); ipk::selftest_task_queue(enabled != 0); return IPK_OK; }
int ipk_selftest_spline3(float exposure, const float *points, int npoints, uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  if (!n_bad || (npoints > 0 && !points)) return fail(IPK_ERR_INVALID, "bad selftest arguments");
  ipk::Spline sp; int rc = build_curve(exposure, points, npoints, sp); if (rc) return rc;
  void *dev; rc = selftest_alloc(&dev); if (rc) return rc;
  if (ipk::launch_selftest_spline3(sp, dev, nullptr) != 0) { (void)hipFree(dev); return fail(IPK_ERR_UNSUPPORTED, "the kernels keep the select form for this curve"); }
  HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_selftest_quant16(uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  if (!n_bad) return fail(IPK_ERR_INVALID, "bad selftest arguments");
  void *dev; int rc = selftest_alloc(&dev); if (rc) return rc;
  ipk::launch_selftest_quant16(dev, nullptr); HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_selftest_q8(uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  if (!n_bad) return fail(IPK_ERR_INVALID, "bad selftest arguments");
  void *dev; int rc = selftest_alloc(&dev); if (rc) return rc;
  ipk::launch_selftest_q8(cx().lut_pairs[ipk::kLutGamma], cx().lut_q8, dev, nullptr); HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_selftest_quant8(int variant, uint64_t *n_bad, uint32_t *first_bad_bits) {
  REQUIRE_INIT();
  void *dev; int rc = selftest_alloc(&dev); if (rc) return rc;
  ipk::launch_selftest_quant8(dev, variant, nullptr); HIPCHK(hipGetLastError());
  return selftest_collect(dev, n_bad, first_bad_bits);
}
int ipk_selftest_cbrtf(const float *in, float *out, size_t n, int variant, void *stream) {
  REQUIRE_INIT();
  // variants 3-5 (one XYZ -> Lab lookup per element, see k_selftest_lab_slot) run whole waves: n in multiples of 256
  if (!in || !out || variant < 0 || variant > 5 || (variant >= 3 && n % 256 != 0)) return fail(IPK_ERR_INVALID, "bad selftest arguments");
  ipk::launch_selftest_cbrt(in, out, n, variant, cx().lut_pairs[ipk::kLutXyzLab], S(stream)); HIPCHK(hipGetLastError());
  return IPK_OK;
}

// ------------------------------------------------------------------------------------------
// Pipeline::run (src/pipeline.rs:311-375) for one source, cache == None
// ------------------------------------------------------------------------------------------
// allow_fused as the switch it began as: any non-zero value means "on" -- except IPK_FUSED_CACHED_RESAMPLE standing alone, a bit younger than that rule,
// which no route, report or region plan may see (with it or without it they answer the same, for every mask); IPK_FUSED_SCALED_ROTATECROP, younger still,
// likewise counts beside IPK_FUSED_ON only and is nothing alone
static bool fused_on(const ipk_pipeline_desc *d) { return (d->allow_fused & ~(IPK_FUSED_CACHED_RESAMPLE | IPK_FUSED_SCALED_ROTATECROP)) != 0; }
static bool opted(const ipk_pipeline_desc *d, int bit) { return (d->allow_fused & (IPK_FUSED_ON | bit)) == (IPK_FUSED_ON | bit); }   // an opt-in bit counts beside IPK_FUSED_ON only
// the descriptor's OpRotateCrop in its reset() state (pipeline.rs:314-316)
static ipk::RotateCrop rotatecrop_of(const ipk_pipeline_desc *d) {
  ipk::RotateCrop rc;
  rc.crop_top = d->rotatecrop[0]; rc.crop_right = d->rotatecrop[1]; rc.crop_bottom = d->rotatecrop[2];
  rc.crop_left = d->rotatecrop[3]; rc.rotation = d->rotatecrop[4];
  return rc;
}
// rc_state (may be null): the OpRotateCrop as the two folds of the negotiation leave it (input_ratio, output size) -- the state
// its Serialize impl exposes to the hash chain (pipeline.rs:318-335, rotatecrop.rs:10-18)
static int pipeline_sizes_impl(const ipk_pipeline_desc *d, size_t *demosaic_w, size_t *demosaic_h, size_t *final_w, size_t *final_h,
                               ipk::RotateCrop *rc_state) {
  if (!d) return fail(IPK_ERR_INVALID, "null descriptor");
  if (d->rotation < 0 || d->rotation > 3) return fail(IPK_ERR_INVALID, "bad rotation");
  ipk::RotateCrop rc = rotatecrop_of(d);
  ipk::Rect r;
  if (!ipk::size_image(d->crop_top, d->crop_right, d->crop_bottom, d->crop_left, d->width, d->height, r))
    return fail(IPK_ERR_INVALID, "source smaller than 10x10");
  size_t w = r.width, h = r.height;
  rc.transform_forward(w, h, w, h);                                       // forward fold (pipeline.rs:318-324)
  ipk::transform_forward(d->rotation, w, h, w, h);
  const ipk::Scaling s = ipk::calculate_scaling_total(w, h, d->maxwidth, d->maxheight);   // :328-329
  w = s.width; h = s.height;
  ipk::transform_forward(d->rotation, w, h, w, h);                        // reverse fold (:331-335)
  rc.transform_reverse(w, h, w, h);
  if (rc_state) *rc_state = rc;
  *demosaic_w = w; *demosaic_h = h;
  // The size run() PRODUCES (what output_8bit reports and tests/maxsize_test.rs asserts on): every op sizes its output from
  // the buffer it is handed, not from the negotiation, so behind a rotatecrop the result can differ from the forward fold by a
  // pixel.  demosaic.rs:27-61: the demosaic size when it scales, else its input; rotatecrop.rs:39-64: calc_size of its input
  // unless it is a no-op or rejects its crops; transform.rs:56-73: sides swapped by the transposing orientations.
  size_t pw = r.width, ph = r.height;
  if (ipk::calculate_scaling_total(pw, ph, w, h).scale > 1.0f) { pw = w; ph = h; }
  {
    int64_t pts[6]; size_t nw, nh;
    if (rotatecrop_of(d).corners(pw, ph, pts, nw, nh)) { pw = nw; ph = nh; }
  }
  {
    bool transpose, fx, fy;
    ipk::orientation_to_flips(ipk::transform_orientation(d->rotation, d->fliph != 0, d->flipv != 0), transpose, fx, fy);
    if (transpose) std::swap(pw, ph);
  }
  *final_w = pw; *final_h = ph;
  return IPK_OK;
}
int ipk_pipeline_sizes(const ipk_pipeline_desc *d, size_t *demosaic_w, size_t *demosaic_h, size_t *final_w, size_t *final_h) {
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  return pipeline_sizes_impl(d, demosaic_w, demosaic_h, final_w, final_h, nullptr);
}

// Pipeline::default_ops (pipeline.rs:286-288) for a raster source: every user-visible op field equals PipelineOps::new(Other),
// bit for bit (the reference compares serialised bytes).  Its OpRotateCrop also serialises negotiated state that a previous
// slow-path run leaves behind; the descriptor is stateless, so that quirk is not reproduced.
static bool default_ops_other(const ipk_pipeline_desc *d) {
  auto same = [](float a, float b) { return std::memcmp(&a, &b, 4) == 0; };
  if (d->src_type != IPK_SRC_RGB8 && d->src_type != IPK_SRC_RGB16) return false;
  if (d->crop_top || d->crop_right || d->crop_bottom || d->crop_left || d->is_cfa || d->cfa[0]) return false;
  for (int i = 0; i < 4; ++i) if (!same(d->blacklevels[i], 0.0f) || !same(d->whitelevels[i], 0.0f)) return false;
  for (int i = 0; i < 5; ++i) if (!same(d->rotatecrop[i], 0.0f)) return false;
  float m[12]; ipk::srgb_d65_43(m);
  for (int i = 0; i < 12; ++i) if (!same(d->cam_to_xyz_normalized[i], m[i])) return false;
  const float wb[4] = {1.0f, 1.0f, 1.0f, 0.0f};
  for (int i = 0; i < 4; ++i) if (!same(d->wb_coeffs[i], wb[i])) return false;
  if (!same(d->exposure, 0.0f) || d->npoints != 0) return false;
  return d->rotation == 0 && !d->fliph && !d->flipv;
}
int ipk_pipeline_takes_fastpath(const ipk_pipeline_desc *d, int out_type) {
  if (!d) return fail(IPK_ERR_INVALID, "null descriptor");
  ipk_pipeline_desc taken;
  { const int rc = take_desc(d, taken); if (rc) return rc; }
  d = &taken;
  return (d->use_fastpath && (out_type == IPK_OUT_U8 || out_type == IPK_OUT_U16) && default_ops_other(d)) ? 1 : 0;
}
// output_8bit / output_16bit fast path (pipeline.rs:381-402, :428-449) on device buffers
static int run_fastpath(const ipk_pipeline_desc *d, const void *src, void *dst, int out_type, void *stream) {
  const size_t n = d->width * d->height * 3;
  const ipk::Scaling sc = ipk::calculate_scaling_total(d->width, d->height, d->maxwidth, d->maxheight);      // scaling_size
  const bool scaled = sc.width != d->width || sc.height != d->height;
  const bool want16 = out_type == IPK_OUT_U16, have16 = d->src_type == IPK_SRC_RGB16;
  const size_t esz = want16 ? 2 : 1;
  Scratch tmp(S(stream));
  const void *rgb = src;
  if (want16 != have16) {                                                  // to_rgb8 / to_rgb16
    void *conv = dst;
    if (scaled) { int rc = tmp.get(n * esz, &conv); if (rc) return rc; }
    if (want16) ipk::launch_chan_8_to_16(static_cast<const uint8_t *>(src), n, static_cast<uint16_t *>(conv), cx().num_cus, S(stream));
    else ipk::launch_chan_16_to_8(static_cast<const uint16_t *>(src), n, static_cast<uint8_t *>(conv), cx().num_cus, S(stream));
    HIPCHK(hipGetLastError());
    rgb = conv;
  }
  if (!scaled) {
    if (rgb != dst) HIPCHK(hipMemcpyAsync(dst, rgb, n * esz, hipMemcpyDeviceToDevice, S(stream)));
    return IPK_OK;
  }
  // scale_down_srgb / scale_down_srgb16 (scaling.rs:162-182)
  return want16
    ? ipk_transform_buffer_u16(static_cast<const uint16_t *>(rgb), d->width, d->height, 0, 0, (int64_t)d->width - 1, 0, 0, (int64_t)d->height - 1,
                               sc.width, sc.height, 3, nullptr, static_cast<uint16_t *>(dst), stream)
    : ipk_transform_buffer_u8(static_cast<const uint8_t *>(rgb), d->width, d->height, 0, 0, (int64_t)d->width - 1, 0, 0, (int64_t)d->height - 1,
                              sc.width, sc.height, 3, nullptr, static_cast<uint8_t *>(dst), stream);
}

// ---- do_timing! (src/pipeline.rs:68-80): per-stage times of the pipeline driver, hipEvents on the caller's stream ----------------
namespace {
struct TimingSession { bool active = false; std::vector<std::pair<std::string, hipEvent_t>> marks; };
thread_local TimingSession g_timing;
struct StageTimer {                    // marks are no-ops unless ipk_timing_begin() armed this thread
  hipStream_t s; bool on; const char *rest = nullptr;
  explicit StageTimer(hipStream_t st) : s(st), on(g_timing.active) { if (on) mark("(start)"); }
  void mark(const char *name) {
    if (!on) return;
    hipEvent_t e = nullptr;
    if (hipEventCreate(&e) != hipSuccess || hipEventRecord(e, s) != hipSuccess) { on = false; return; }
    g_timing.marks.emplace_back(name, e);
  }
  ~StageTimer() { if (rest) mark(rest); }
};
}  // namespace
int ipk_timing_begin(void) {
  for (auto &m : g_timing.marks) (void)hipEventDestroy(m.second);
  g_timing.marks.clear();
  g_timing.active = true;
  return IPK_OK;
}
int ipk_timing_end(ipk_stage_time *out, int max_stages, int *n_stages) {
  // the session ends whatever the arguments are: a bad call must not leave the thread armed with its events alive
  g_timing.active = false;
  auto &mk = g_timing.marks;
  if (!n_stages || (max_stages > 0 && !out)) {
    for (auto &m : mk) (void)hipEventDestroy(m.second);
    mk.clear();
    return fail(IPK_ERR_INVALID, "null argument");
  }
  int n = 0, rc = IPK_OK;
  if (!mk.empty() && hipEventSynchronize(mk.back().second) != hipSuccess) rc = fail(IPK_ERR_HIP, "hipEventSynchronize failed");
  for (size_t i = 1; i < mk.size() && rc == IPK_OK; ++i) {
    if (mk[i].first == "(start)") continue;                       // a second pipeline call inside one session starts a new sequence
    float ms = 0.0f;
    if (hipEventElapsedTime(&ms, mk[i - 1].second, mk[i].second) != hipSuccess) { rc = fail(IPK_ERR_HIP, "hipEventElapsedTime failed"); break; }
    if (n < max_stages) { std::snprintf(out[n].name, sizeof(out[n].name), "%s", mk[i].first.c_str()); out[n].ms = ms; }
    ++n;
  }
  for (auto &m : mk) (void)hipEventDestroy(m.second);
  mk.clear();
  *n_stages = n;
  return rc;
}

namespace {
// Everything a driver derives from a descriptor for one call, negotiated once
struct Negotiated {
  ipk::Rect r; size_t dw, dh, fw, fh; ipk::RotateCrop rc; int linear; int orientation; bool transform_noop;
  bool raw, cfa_branch;                  // a raw source, and one OpGoFloat treats as a CFA mosaic (gofloat.rs:95,109,121)
  float scale;                           // OpDemosaic's scale: the cropped source against the demosaic size
};
// The descriptor fields every driver checks before it reads them: out_type always, the two fuse flags and / or the curve's point count where the
// driver asks (a driver that leaves the curve to the launch that builds it -- ipk_pipeline_run -- does not ask for it)
enum { kCheckFuse = 1, kCheckCurve = 2 };
int validate_desc(const ipk_pipeline_desc *d, int out_type, int checks) {
  if (!d) return fail(IPK_ERR_INVALID, "null descriptor");
  if (out_type < 0 || out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if ((checks & kCheckCurve) && (d->npoints < 0 || d->npoints > 64)) return fail(IPK_ERR_INVALID, "npoints out of range");
  if ((checks & kCheckFuse) && d->fuse_rotatecrop != 0 && d->fuse_rotatecrop != 1) return fail(IPK_ERR_INVALID, "fuse_rotatecrop must be 0 or 1 (got %d)", d->fuse_rotatecrop);
  if ((checks & kCheckFuse) && d->fuse_scaledown != 0 && d->fuse_scaledown != 1) return fail(IPK_ERR_INVALID, "fuse_scaledown must be 0 or 1 (got %d)", d->fuse_scaledown);
  return IPK_OK;
}
int negotiate(const ipk_pipeline_desc *d, int out_type, Negotiated &n) {
  { const int vrc = validate_desc(d, out_type, kCheckFuse); if (vrc) return vrc; }
  // one negotiation: the sizes and the rotatecrop state both come from pipeline_sizes_impl's folds (the reverse fold is seeded
  // with scaling_size of the forward result, pipeline.rs:328-335 -- not with the size run() produces)
  int rc = pipeline_sizes_impl(d, &n.dw, &n.dh, &n.fw, &n.fh, &n.rc); if (rc) return rc;
  ipk::size_image(d->crop_top, d->crop_right, d->crop_bottom, d->crop_left, d->width, d->height, n.r);
  n.scale = ipk::calculate_scaling_total(n.r.width, n.r.height, n.dw, n.dh).scale;
  n.raw = d->src_type == IPK_SRC_U16 || d->src_type == IPK_SRC_F32;
  n.cfa_branch = n.raw && !(d->cpp == 1 && !d->is_cfa) && d->cpp != 3;
  // output_8bit forces linear=false (pipeline.rs:405), output_16bit linear=true (:452)
  n.linear = out_type == IPK_OUT_U8 ? 0 : (out_type == IPK_OUT_U16 ? 1 : (d->linear != 0));
  n.orientation = ipk::transform_orientation(d->rotation, d->fliph != 0, d->flipv != 0);
  n.transform_noop = n.orientation == IPK_OR_NORMAL || n.orientation == IPK_OR_UNKNOWN;
  return IPK_OK;
}
// the size run() produced against the negotiated one; the cached driver also states its OpBuffer's colours (0: not stated), which must be 3
int check_produced(const Negotiated &n, size_t w, size_t h, size_t colors = 0) {
  if (w == n.fw && h == n.fh && (colors == 0 || colors == 3)) return IPK_OK;
  return colors ? fail(IPK_ERR_INVALID, "internal: produced %zux%zux%zu, negotiated %zux%zu", w, h, colors, n.fw, n.fh)
                : fail(IPK_ERR_INVALID, "internal: produced %zux%zu, negotiated %zux%zu", w, h, n.fw, n.fh);
}
size_t out_elem_size(int t) { return t == IPK_OUT_F32 ? 4 : t == IPK_OUT_U8 ? 1 : 2; }

// the parameters of a one-launch route's launch (ipk_fused_params), from the descriptor and its negotiation
void fused_params_of(const ipk_pipeline_desc *d, const Negotiated &n, int out_type, ipk_fused_params &fp) {
  std::memset(&fp, 0, sizeof(fp));
  fp.struct_size = (uint32_t)sizeof(fp);
  fp.src_type = d->src_type; fp.owidth = d->width; fp.x = n.r.x; fp.y = n.r.y; fp.width = n.r.width; fp.height = n.r.height;
  fp.black0 = d->blacklevels[0]; fp.white0 = d->whitelevels[0];
  std::memcpy(fp.cfa, d->cfa, sizeof(fp.cfa));
  std::memcpy(fp.wb_coeffs, d->wb_coeffs, sizeof(fp.wb_coeffs));
  std::memcpy(fp.cam_to_xyz_normalized, d->cam_to_xyz_normalized, sizeof(fp.cam_to_xyz_normalized));
  fp.exposure = d->exposure; fp.npoints = d->npoints; std::memcpy(fp.points, d->points, sizeof(fp.points));
  fp.linear = n.linear; fp.out_type = out_type; fp.schedule = d->schedule;
}

// ---- The route of one frame, decided once (choose_route) and read by every driver and report.  fp: the launch's parameters (every one-launch kind; the
// raster kind reads the source type, the size and the point-wise parameters from it); rcp: what OpRotateCrop::run hands to transform_buffer (kFusedResample);
// pw x ph: the image the launch produces before OpTransform; four: kFusedRaw with a fourth colour in the launch (fp.four_colour = 1); label /
// region_label: the stage run_timed shows for a whole frame / a windowed region ----
enum RouteKind { kFastPath, kFusedRaw, kFusedResample, kFusedScaledown, kFusedRaster, kScaledRotateCrop, kStaged };
enum ScalingPass { kPassScaledDemosaic, kPassDemosaicScaled, kPassRasterScaleDown };   // raw_scaled_demosaic_impl, raw_demosaic_scaled_impl, raster_scale_down_impl
struct RotateCropPoints { int64_t pts[6]; size_t nw, nh; };
struct Route {
  RouteKind kind; ipk_fused_params fp; RotateCropPoints rcp; size_t pw, ph; bool four;
  // kScaledRotateCrop: the launch that writes the n.dw x n.dh RGBE buffer, and the plan of the resampling launch over that buffer (rcp: its corners)
  ScalingPass pass1; ipk::ResamplePlan plan2;
  const char *label, *region_label;
  // kFusedRaster: plain = the frame is on the link because of IPK_FUSED_PLAIN (a cropped raster, a u16 three-sample or monochrome raw) and its launch is
  // ipk_plain_to_srgb of plain_kind (ipk_plain_kind) over the crop rectangle with these levels; an uncropped raster has plain = false, plain_kind 0
  bool plain; int plain_kind; float black4[4], white4[4];
};
// The chain, in order: fast path, raw, resample, scaledown, raster, staged -- the first link that holds names the route.
//   raw        gofloat..gamma as the one raw->sRGB launch: a CFA mosaic, every op in between point-wise or demosaic::full (OpRotateCrop a no-op, OpDemosaic
//              not scaling).  A filter with a fourth colour (RGBE ...) only where the caller opted in: allow_fused bit 1 (IPK_FUSED_FOUR_COLOUR)
//   resample   the same with an ACTIVE OpRotateCrop between demosaic::full and OpToLab (ipk_raw_to_srgb_resampled), opted into with fuse_rotatecrop.
//              corners() fails for crops outside the image, where the op returns its input -- and the frame stays staged, as it does when OpDemosaic
//              scales (with an angle the reverse size fold often negotiates a demosaic size one pixel short of the source) or the transform is not one
//              the launch admits (resample_plan)
//   scaledown  OpDemosaic's `full` + scale_down_opbuf branch (demosaic.rs:51-59: 1 < scale < minscale, the near-full-size preview) inside the launch
//              (ipk_raw_to_srgb_scaled, to the negotiated n.dw x n.dh), opted into with fuse_scaledown.  An active OpRotateCrop behind a scaling
//              OpDemosaic would be a second resampling: such frames stay staged
//   raster     run_other + tolab..gamma (+ quantisation) as one launch when OpDemosaic (a 4-channel buffer at scale <= 1: pass-through,
//              demosaic.rs:39-44) and OpRotateCrop are no-ops: an uncropped RGB8 / RGB16 raster.  With IPK_FUSED_PLAIN beside IPK_FUSED_ON the link also
//              takes the other frames whose OpGoFloat writes that 4-channel buffer -- rasters with OpGoFloat crops, u16 raws with cpp == 3 and u16
//              monochrome raws (cpp == 1 without a filter) -- as ipk_plain_to_srgb over the crop rectangle.  Their f32 forms stay staged: the launch is
//              a mode of the RGB8 / RGB16 kernels and has no f32 instantiation
// OpTransform does not enter: run_route folds any orientation in.  The order matters less than it looks, because the links exclude each other, and the
// callers that ask for one link only (the ipk_pipeline_fuses_* reports, the batch driver, the region plan) rely on exactly that:
//   - the fast path needs a raster source (default_ops_other), the three raw links need n.cfa_branch, which implies a raw source, and the raster link
//     needs !n.cfa_branch (a raster, or under IPK_FUSED_PLAIN a raw OpGoFloat does not treat as a mosaic): a fast-path frame fails every raw link and
//     a frame on a raw link never takes the fast path or the raster link;
//   - raw and scaledown need n.rc.noop(), resample needs !n.rc.noop();
//   - raw and resample need n.scale <= 1, scaledown needs n.scale > 1.
// So at most one raw link holds for a descriptor, wherever the fast-path test sits.  Fast path against raster is the one pair the order decides.
// out_type enters through the fast path and fp.out_type alone: the cached driver, which produces f32 whatever the caller asked for, asks with
// IPK_OUT_F32 after it has tested the fast path on the caller's type itself.
bool plain_opted(const ipk_pipeline_desc *d) { return opted(d, IPK_FUSED_PLAIN); }
// IPK_FUSED_PLAIN_PREVIEWS: a monochrome or three-sample raw (u16 or f32: the raws OpGoFloat does not treat as a mosaic, negotiate) whose OpDemosaic
// scales its 4-channel buffer (demosaic.rs:44-46) runs gofloat + demosaic as the one launch ipk_plain_scale_down
bool scales_plain(const ipk_pipeline_desc *d, const Negotiated &n) {
  return opted(d, IPK_FUSED_PLAIN_PREVIEWS) && n.raw && !n.cfa_branch && n.scale > 1.0f;
}
// An ACTIVE OpRotateCrop as one resampling launch over the sw x sh 4-channel buffer OpDemosaic hands it: the op accepts its crops there (corners) and the
// transform is one k_fused_resample admits (resample_plan).  Shared by the cached region driver (cached_resample) and the two-launch route below
bool rotatecrop_resamples(const ipk_pipeline_desc *d, const Negotiated &n, size_t sw, size_t sh, RotateCropPoints &r, ipk::ResamplePlan &plan) {
  if (n.rc.noop() || !rotatecrop_of(d).corners(sw, sh, r.pts, r.nw, r.nh)) return false;
  return ipk::resample_plan(sw, sh, r.pts[0], r.pts[1], r.pts[2], r.pts[3], r.pts[4], r.pts[5], r.nw, r.nh, plan);
}
// IPK_FUSED_SCALED_ROTATECROP (tried where the chain below ends staged): an active OpRotateCrop behind an OpDemosaic that scales, as TWO launches -- the
// scaling gofloat + demosaic pass into the n.dw x n.dh RGBE buffer, then k_fused_resample's cached-buffer source mode over that buffer with the chain and
// the quantiser behind it.  Pass 1 exists as one launch for a cpp == 1 mosaic with a valid three-colour filter (scale >= minscale: the scaled_demosaic
// kernels; below it: k_fused_resample's RGBE output mode where scaledown_plan admits the geometry), for an RGB8 / RGB16 raster and, under
// IPK_FUSED_PLAIN_PREVIEWS, for a monochrome or three-sample raw (ipk_plain_scale_down).  A fourth colour (E is not +0.0 there), monochrome and
// three-sample raws without that bit, scale <= 1 (fuse_rotatecrop's ground) and a no-op rotatecrop stay where they were
bool scaled_rotatecrop(const ipk_pipeline_desc *d, const Negotiated &n, Route &rt) {
  if (!opted(d, IPK_FUSED_SCALED_ROTATECROP) || n.rc.noop() || !(n.scale > 1.0f)) return false;
  if (n.raw) {
    ipk::Cfa cfa; ipk::ResamplePlan p1;
    if (!n.cfa_branch) {                                                     // IPK_FUSED_PLAIN_PREVIEWS: ipk_plain_scale_down is pass 1 (E = +0.0)
      if (!scales_plain(d, n)) return false;
      rt.pass1 = kPassScaledDemosaic;
      return rotatecrop_resamples(d, n, n.dw, n.dh, rt.rcp, rt.plan2);
    }
    if (d->cpp != 1 || !ipk::Cfa::parse(d->cfa, cfa) || !cfa.valid() || !cfa.three_colour()) return false;
    if (n.scale >= ipk::demosaic_minscale(cfa.width)) rt.pass1 = kPassScaledDemosaic;
    else if (ipk::scaledown_plan(n.r.width, n.r.height, n.dw, n.dh, p1)) rt.pass1 = kPassDemosaicScaled;
    else return false;
  } else rt.pass1 = kPassRasterScaleDown;
  return rotatecrop_resamples(d, n, n.dw, n.dh, rt.rcp, rt.plan2);
}
void choose_route(const ipk_pipeline_desc *d, const Negotiated &n, int out_type, Route &rt) {
  rt.kind = kStaged; rt.four = false; rt.pw = n.r.width; rt.ph = n.r.height; rt.label = rt.region_label = "";
  rt.plain = false; rt.plain_kind = IPK_PLAIN_RASTER;
  const bool uncropped = n.r.x == 0 && n.r.y == 0 && n.r.width == d->width && n.r.height == d->height;
  const bool plain_raw = n.raw && !n.cfa_branch && d->src_type == IPK_SRC_U16;           // cpp == 3, or cpp == 1 without a filter (negotiate)
  if (ipk_pipeline_takes_fastpath(d, out_type) == 1) { rt.kind = kFastPath; return; }
  ipk::Cfa cfa; ipk::ResamplePlan plan; int xo, yo;
  const bool mosaic = fused_on(d) && n.cfa_branch && d->cpp == 1 && ipk::Cfa::parse(d->cfa, cfa);
  const bool three = mosaic && cfa.three_colour(), still = n.rc.noop();
  RotateCropPoints &r = rt.rcp;
  if (mosaic && still && n.scale <= 1.0f && cfa.valid() && (three || cfa.bayer_phase(xo, yo) || (d->allow_fused & IPK_FUSED_FOUR_COLOUR))) {
    rt.kind = kFusedRaw; rt.four = !(three || cfa.bayer_phase(xo, yo));
    rt.label = "fused gofloat+demosaic+to_lab+basecurve+from_lab+gamma(+transform)";
    rt.region_label = "fused region gofloat+demosaic+to_lab+basecurve+from_lab+gamma(+transform)";
  } else if (three && !still && n.scale <= 1.0f && d->fuse_rotatecrop == 1 && rotatecrop_of(d).corners(n.r.width, n.r.height, r.pts, r.nw, r.nh) &&
             ipk::resample_plan(n.r.width, n.r.height, r.pts[0], r.pts[1], r.pts[2], r.pts[3], r.pts[4], r.pts[5], r.nw, r.nh, plan)) {
    rt.kind = kFusedResample; rt.pw = r.nw; rt.ph = r.nh;
    rt.label = "fused gofloat+demosaic+rotatecrop+to_lab+basecurve+from_lab+gamma(+transform)";
    rt.region_label = "fused region gofloat+demosaic+rotatecrop+to_lab+basecurve+from_lab+gamma(+transform)";
  } else if (three && still && n.scale > 1.0f && d->fuse_scaledown == 1 && n.scale < ipk::demosaic_minscale(cfa.width) &&
             ipk::scaledown_plan(n.r.width, n.r.height, n.dw, n.dh, plan)) {
    rt.kind = kFusedScaledown; rt.pw = n.dw; rt.ph = n.dh;
    rt.label = "fused gofloat+demosaic(scaled)+to_lab+basecurve+from_lab+gamma";          // a whole frame marks "transform" as a stage of its own (run_route)
    rt.region_label = "fused region gofloat+demosaic(scaled)+to_lab+basecurve+from_lab+gamma(+transform)";
  } else if (fused_on(d) && still && n.r.width * n.r.height >= 256 && n.scale <= 1.0f &&
             ((!n.raw && uncropped) || (plain_opted(d) && (!n.raw || plain_raw)))) {
    rt.kind = kFusedRaster;
    rt.plain = n.raw || !uncropped;
    rt.plain_kind = !n.raw ? IPK_PLAIN_RASTER : d->cpp == 3 ? IPK_PLAIN_RGB : IPK_PLAIN_MONO;
    std::memcpy(rt.black4, d->blacklevels, sizeof(rt.black4)); std::memcpy(rt.white4, d->whitelevels, sizeof(rt.white4));
    rt.label = "fused gofloat+to_lab+basecurve+from_lab+gamma(+transform)";
    rt.region_label = "fused region gofloat+to_lab+basecurve+from_lab+gamma(+transform)";      // regions under IPK_FUSED_PLAIN (plan_region)
  }
  if (rt.kind == kStaged && scaled_rotatecrop(d, n, rt)) {
    rt.kind = kScaledRotateCrop; rt.pw = r.nw; rt.ph = r.nh;
    rt.label = "rotatecrop+to_lab+basecurve+from_lab+gamma";                                // behind "gofloat+demosaic" (run_scaled_rotatecrop)
    rt.region_label = "region rotatecrop+to_lab+basecurve+from_lab+gamma";
  }
  if (rt.kind == kStaged) return;
  fused_params_of(d, n, out_type, rt.fp);
  rt.fp.four_colour = rt.four ? 1 : 0;
}

// output8bit / output16bit (pipeline.rs:408-414 / :455-461): cnt f32 samples into the quantised output type
int quantise(const void *src, size_t cnt, int out_type, void *dst, void *stream) {
  return out_type == IPK_OUT_U8 ? ipk_output8bit(static_cast<const float *>(src), cnt, static_cast<uint8_t *>(dst), stream)
                                : ipk_output16bit(static_cast<const float *>(src), cnt, static_cast<uint16_t *>(dst), stream);
}
// OpTransform's permutation of a 3-sample image of the output type.  On the 8- and 16-bit outputs it runs after the quantisation: output8bit /
// output16bit act per sample, so the permutation commutes with them and then moves 3 or 6 bytes per pixel instead of 12
int orient(const void *src, size_t w, size_t h, int orientation, int out_type, void *dst, size_t *ow, size_t *oh, void *stream) {
  if (out_type == IPK_OUT_F32) return ipk_rotate_buffer(static_cast<const float *>(src), w, h, orientation, static_cast<float *>(dst), ow, oh, stream);
  if (out_type == IPK_OUT_U8) return ipk_rotate_image_u8(static_cast<const uint8_t *>(src), w, h, orientation, static_cast<uint8_t *>(dst), ow, oh, stream);
  return ipk_rotate_image_u16(static_cast<const uint16_t *>(src), w, h, orientation, static_cast<uint16_t *>(dst), ow, oh, stream);
}
// Crop-only shortcut.  Without an angle the corner points are integers, both skips are exactly 1.0 and the cross terms 0, so the
// window of output pixel (row, col) is the 2x2 block at (x + col, y + row) with the weights {1, 0, 0, 0}: the result is the demosaiced pixel
// itself PROVIDED its three zero-weight neighbours are finite (0 * inf is NaN) and it is not -0.0 ((-0) + (+0) is +0).  For a u16 source whose
// every normalised sample is zero or ordinary (gen_levels_ok_u16 walks all 65 536) both hold: the samples are finite and never -0.0, and a
// demosaic output is a sum that starts at +0.0 over a positive count.  The launch is then the fused kernel's window form over the rectangle
// (launch_route).  f32 sources can hold -inf and always take k_fused_resample.
bool crop_only_shortcut(const ipk_fused_params &fp, const RotateCropPoints &r) {
  const float range = fp.white0 - fp.black0;
  const size_t lim = size_t(1) << 22;                          // x + col + 0.5 is exact in f32 far beyond any frame this holds for
  if (fp.src_type != IPK_SRC_U16 || !(range > 0.0f) || !std::isfinite(fp.black0) || !std::isfinite(range) || !gen_levels_ok_u16(fp.black0, range)) return false;
  if (fp.width >= lim || fp.height >= lim || r.pts[0] < 0 || r.pts[1] < 0) return false;
  const int64_t x = r.pts[0], y = r.pts[1];
  return r.pts[2] == x + (int64_t)r.nw - 1 && r.pts[3] == y && r.pts[4] == x && r.pts[5] == y + (int64_t)r.nh - 1 &&    // skips 1, 0, 0, 1
         (size_t)x + r.nw <= fp.width && (size_t)y + r.nh <= fp.height;                                                 // the rectangle lies inside the frame
}
// The one launch of a route into `out`.  win == null: the whole pw x ph image, by the whole-frame entry point.  win: that rectangle of it, packed, by
// the window form of the same launch (the raster kind's is ipk_plain_to_srgb over the rectangle: plan_region asks for it under IPK_FUSED_PLAIN only).  Whole frames never go through the
// window forms -- those are other kernel variants -- except on the crop-only shortcut, which IS the window form: written once, the whole frame
// being the window (0, 0, nw, nh).
int launch_route(const Route &rt, const void *src, const ipk::ResampleWindow *win, void *out, void *stream) {
  const ipk_fused_params &fp = rt.fp;
  const RotateCropPoints &r = rt.rcp;
  // k_fused_bayer's window form: the rows are a band whose source is the whole cropped frame (src then starts at the crop's first row), the columns
  // the launch's window; both are the cropped frame's
  auto fused_window = [&](size_t col0, size_t row0, size_t cols, size_t rows, bool four_ok) {
    ipk_fused_params b = fp;
    b.band_src_row0 = 0; b.band_src_rows = fp.height; b.band_out_row0 = row0; b.band_out_rows = rows;
    const void *top = static_cast<const char *>(src) + fp.y * fp.owidth * (fp.src_type == IPK_SRC_U16 ? 2 : 4);
    FusedOpts fo; fo.win_c0 = col0; fo.win_c1 = col0 + cols; fo.four_ok = four_ok;
    return fused_impl(&b, top, out, stream, 0, fo);
  };
  switch (rt.kind) {
    case kFusedRaw:
      return win ? fused_window(win->col0, win->row0, win->cols, win->rows, true) : ipk_raw_to_srgb(&fp, src, out, stream);
    case kFusedResample: {
      const ipk::ResampleWindow whole = {0, 0, r.nh, r.nw};
      const ipk::ResampleWindow &w = win ? *win : whole;
      if (crop_only_shortcut(fp, r)) return fused_window((size_t)r.pts[0] + w.col0, (size_t)r.pts[1] + w.row0, w.cols, w.rows, false);
      return win ? ipk_raw_to_srgb_resampled_window(&fp, src, r.pts[0], r.pts[1], r.pts[2], r.pts[3], r.pts[4], r.pts[5], r.nw, r.nh, w.col0, w.row0, w.cols, w.rows, out, stream)
                 : ipk_raw_to_srgb_resampled(&fp, src, r.pts[0], r.pts[1], r.pts[2], r.pts[3], r.pts[4], r.pts[5], r.nw, r.nh, out, stream);
    }
    case kFusedScaledown:
      return win ? ipk_raw_to_srgb_scaled_window(&fp, src, rt.pw, rt.ph, win->col0, win->row0, win->cols, win->rows, out, stream)
                 : ipk_raw_to_srgb_scaled(&fp, src, rt.pw, rt.ph, out, stream);
    case kFusedRaster:
      if (!win && !rt.plain) return ipk_raster_to_srgb(src, fp.src_type, fp.width, fp.height, fp.wb_coeffs, fp.cam_to_xyz_normalized, fp.exposure, fp.points, fp.npoints,
                                                       fp.linear, fp.out_type, out, stream);
      // the point-wise ops have no halo: a window is the launch's rectangle moved and shrunk, the whole frame of a plain source the crop rectangle
      return ipk_plain_to_srgb(src, fp.src_type, rt.plain_kind, fp.owidth, fp.x + (win ? win->col0 : 0), fp.y + (win ? win->row0 : 0), win ? win->cols : fp.width,
                               win ? win->rows : fp.height, rt.black4, rt.white4, fp.wb_coeffs, fp.cam_to_xyz_normalized, fp.exposure, fp.points, fp.npoints,
                               fp.linear, fp.out_type, out, stream);
    default: break;
  }
  return fail(IPK_ERR_INVALID, "internal: no such launch for this route");
}
// The launch-then-orient step of every driver: `launch` enqueues the 3-sample pw x ph image in front of OpTransform into the pointer it is handed -- dst
// itself when there is nothing to permute (permute = false behind another orientation than Normal: the launch applies OpTransform itself), else a scratch
// image of the output type that orient() moves into dst.  want_w x want_h: what dst holds, checked against the result before anything is enqueued
extern "C++" template <typename Launch>
int launch_then_orient(size_t pw, size_t ph, int out_type, bool permute, int orientation, size_t want_w, size_t want_h, void *dst, void *stream, Launch launch) {
  bool t, fx, fy; ipk::orientation_to_flips(orientation, t, fx, fy);
  if ((t ? ph : pw) != want_w || (t ? pw : ph) != want_h)
    return fail(IPK_ERR_INVALID, "internal: the launch produces %zux%zu (orientation %d), wanted %zux%zu", pw, ph, orientation, want_w, want_h);
  if (!permute) return launch(dst);
  Scratch sc(S(stream));
  void *tmp = nullptr; size_t ow = 0, oh = 0;
  int rc = sc.get(pw * ph * 3 * out_elem_size(out_type), &tmp); if (rc) return rc;
  rc = launch(tmp); if (rc < 0) return rc;
  rc = orient(tmp, pw, ph, orientation, out_type, dst, &ow, &oh, stream);
  return rc < 0 ? rc : IPK_OK;
}
// Rectangle (x, y, w, h) of a 3-sample image full_width pixels wide, packed into dst: one 2-D copy
int cut_region(const void *full, size_t full_width, size_t elem_size, size_t x, size_t y, size_t w, size_t h, void *dst, void *stream) {
  const size_t px = 3 * elem_size;
  HIPCHK(hipMemcpy2DAsync(dst, w * px, static_cast<const char *>(full) + (y * full_width + x) * px, full_width * px, w * px, h, hipMemcpyDeviceToDevice, S(stream)));
  return IPK_OK;
}
// A one-launch route, then OpTransform (launch_then_orient): the launch writes the image of the output type (fp.out_type).  win: a region
// (launch_route); want_w x want_h: the size the caller's dst holds.
int run_route(const Route &rt, const Negotiated &n, const void *src, const ipk::ResampleWindow *win, size_t want_w, size_t want_h, void *dst, void *stream) {
  StageTimer tm(S(stream));
  tm.rest = win ? rt.region_label : rt.label;
  const size_t pw = win ? win->cols : rt.pw, ph = win ? win->rows : rt.ph;
  if (!n.transform_noop && rt.kind == kFusedRaw && !win) {
    // Whole frames of the raw route (every portrait shot): Rotate90 / Rotate270 of a Bayer frame permute the 1-channel mosaic and run the fused
    // kernel in rotated space -- no pass over the 3-channel result at all.  Where no such variant exists the launch below takes over.
    size_t ow = 0, oh = 0;
    const int rc = launch_then_orient(pw, ph, rt.fp.out_type, false, n.orientation, want_w, want_h, dst, stream,
                                      [&](void *out) { return ipk_raw_to_srgb_oriented(&rt.fp, src, n.orientation, out, &ow, &oh, stream); });
    if (rc != IPK_ERR_UNSUPPORTED) return rc;
  }
  return launch_then_orient(pw, ph, rt.fp.out_type, !n.transform_noop, n.orientation, want_w, want_h, dst, stream, [&](void *out) {
    const int rc = launch_route(rt, src, win, out, stream);
    if (rc >= 0 && !n.transform_noop && rt.kind == kFusedScaledown && !win) { tm.mark(tm.rest); tm.rest = "transform"; }
    return rc;
  });
}

// ---- OpGoFloat (gofloat.rs:95-130): what it produces for a descriptor, and the launch that writes it ----
int gofloat_shape(const ipk_pipeline_desc *d, const Negotiated &n, size_t &colors, int &monochrome) {
  colors = 4; monochrome = 0;
  if (!n.raw || d->cpp == 3) return IPK_OK;
  if (d->cpp == 1 && !d->is_cfa) { monochrome = 1; return IPK_OK; }
  if (d->cpp != 1) return fail(IPK_ERR_UNSUPPORTED, "cpp=%d sources are not supported", d->cpp);
  colors = 1;
  return IPK_OK;
}
int launch_gofloat(const ipk_pipeline_desc *d, const Negotiated &n, const void *src, float *dst, void *stream) {
  const size_t x = n.r.x, y = n.r.y, w = n.r.width, h = n.r.height;
  const bool u16 = d->src_type == IPK_SRC_U16;
  const uint16_t *s16 = static_cast<const uint16_t *>(src);
  const float *s32 = static_cast<const float *>(src);
  if (!n.raw)
    return d->src_type == IPK_SRC_RGB8 ? ipk_gofloat_other_u8(static_cast<const uint8_t *>(src), d->width, x, y, w, h, dst, stream)
                                       : ipk_gofloat_other_u16(s16, d->width, x, y, w, h, dst, stream);
  if (d->cpp == 1 && !d->is_cfa)
    return u16 ? ipk_gofloat_mono_u16(s16, d->width, x, y, w, h, d->blacklevels[0], d->whitelevels[0], dst, stream)
               : ipk_gofloat_mono_f32(s32, d->width, x, y, w, h, d->blacklevels[0], d->whitelevels[0], dst, stream);
  if (d->cpp == 3)
    return u16 ? ipk_gofloat_rgb_u16(s16, d->width, x, y, w, h, d->blacklevels, d->whitelevels, dst, stream)
               : ipk_gofloat_rgb_f32(s32, d->width, x, y, w, h, d->blacklevels, d->whitelevels, dst, stream);
  return u16 ? ipk_gofloat_cfa_u16(s16, d->width, x, y, w, h, d->blacklevels[0], d->whitelevels[0], dst, stream)
             : ipk_gofloat_cfa_f32(s32, d->width, x, y, w, h, d->blacklevels[0], d->whitelevels[0], dst, stream);
}
// the monochrome flag of the buffer the one pass writes: a monochrome raw's (gofloat.rs:95-108), which the tail reads with the sRGB matrix and unit
// multipliers; every other source of the pass writes colour
int one_pass_monochrome(const ipk_pipeline_desc *d, const Negotiated &n) { return (n.raw && !n.cfa_branch && d->cpp == 1) ? 1 : 0; }
// OpGoFloat + OpDemosaic in one pass, into a dw x dh 4-channel buffer, when OpDemosaic::run would scale: its scaled_demosaic branch for a
// mosaic (demosaic.rs:47-50), its scale_down_opbuf branch for a raster source under a size limit and, under IPK_FUSED_PLAIN_PREVIEWS, for a
// monochrome or three-sample raw (demosaic.rs:44-46)
bool gofloat_demosaic_one_pass(const ipk_pipeline_desc *d, const Negotiated &n) {
  if (!fused_on(d)) return false;
  if (!n.raw) return n.scale > 1.0f;
  if (!n.cfa_branch) return scales_plain(d, n);
  ipk::Cfa cfa;
  return n.cfa_branch && d->cpp == 1 && ipk::Cfa::parse(d->cfa, cfa) && cfa.valid() && n.scale >= ipk::demosaic_minscale(cfa.width);
}
// win: that rectangle of the n.dw x n.dh buffer alone, packed (regions under IPK_FUSED_WINDOW_PREVIEWS); null: the whole buffer
int launch_gofloat_demosaic(const ipk_pipeline_desc *d, const Negotiated &n, const void *src, const ipk::ResampleWindow *win, float *dst, void *stream) {
  if (!n.raw) return raster_scale_down_impl(src, d->src_type, d->width, n.r.x, n.r.y, n.r.width, n.r.height, n.dw, n.dh, win, dst, stream);
  if (!n.cfa_branch)
    return plain_scale_down_impl(src, d->src_type, d->cpp == 3 ? IPK_PLAIN_RGB : IPK_PLAIN_MONO, d->width, n.r.x, n.r.y, n.r.width, n.r.height, d->blacklevels,
                                 d->whitelevels, n.dw, n.dh, win, dst, stream);
  return raw_scaled_demosaic_impl(src, d->src_type, d->width, n.r.x, n.r.y, n.r.width, n.r.height, d->blacklevels[0], d->whitelevels[0], d->cfa,
                                  n.dw, n.dh, win, dst, stream);
}
// ---- The eight ops of Pipeline::run (pipeline.rs:155-164), each stated once: what it makes of its input's shape (plan_op: no GPU, nothing allocated) and
// the launch that writes it (launch_op).  The scratch driver (run_staged / run_tail) and the cache driver (run_cached_ops) are loops over the two ----
struct OpShape { size_t w, h, colors; int mono; int branch = 0; };         // branch: of op 1's output, the DemosaicBranch that writes it
const char *const kOpLabels[8] = {"gofloat", "demosaic", "rotatecrop", "to_lab", "basecurve", "from_lab", "gamma", "transform"};
// IPK_NOOP: the op hands its input on (out = in); IPK_OK: `out` is the shape of the buffer it writes.  Op 0 has no input: `in` is not read
int plan_op(int op, const ipk_pipeline_desc *d, const Negotiated &n, const OpShape &in, OpShape &out) {
  out = in;
  switch (op) {
    case 0: out.w = n.r.width; out.h = n.r.height; return gofloat_shape(d, n, out.colors, out.mono);
    case 1: {
      const int branch = demosaic_plan(in.w, in.h, in.colors, d->cfa, n.dw, n.dh, &out.w, &out.h);
      out.colors = 4; out.branch = branch;
      return branch < 0 ? branch : branch == kDemosaicNoop ? IPK_NOOP : IPK_OK;
    }
    case 2: return ipk_rotatecrop(nullptr, in.w, in.h, in.colors, d->rotatecrop, nullptr, &out.w, &out.h, nullptr);
    case 3: out.colors = 3; return IPK_OK;
    case 4: return curve_is_noop(d->exposure, d->npoints) ? IPK_NOOP : IPK_OK;
    case 5: return IPK_OK;
    case 6: return n.linear ? IPK_NOOP : IPK_OK;                            // gamma.rs:17-18
    default: {
      if (n.transform_noop) return IPK_NOOP;                               // transform.rs:68-69
      bool t, fx, fy; ipk::orientation_to_flips(n.orientation, t, fx, fy);
      if (t) std::swap(out.w, out.h);
      return IPK_OK;
    }
  }
}
// op `op` from the buffer `in` of shape `s` (op 0: from the source) into `out`, which holds `to`, the shape plan_op gave
int launch_op(int op, const ipk_pipeline_desc *d, const Negotiated &n, const void *src, const float *in, const OpShape &s, float *out, const OpShape &to,
              void *stream) {
  size_t ow, oh;
  switch (op) {
    case 0: return launch_gofloat(d, n, src, out, stream);
    case 1: return demosaic_launch(to.branch, in, s.w, s.h, d->cfa, n.dw, n.dh, out, stream);
    case 2: return ipk_rotatecrop(in, s.w, s.h, s.colors, d->rotatecrop, out, &ow, &oh, stream);
    case 3: return ipk_tolab(in, s.w, s.h, s.mono, d->wb_coeffs, d->cam_to_xyz_normalized, out, stream);
    case 4: return ipk_basecurve(in, s.w, s.h, d->exposure, d->points, d->npoints, out, stream);
    case 5: return ipk_fromlab(in, s.w, s.h, out, stream);
    case 6: return ipk_gamma(in, s.w, s.h, 3, 0, out, stream);
    default: return ipk_rotate_buffer(in, s.w, s.h, n.orientation, out, &ow, &oh, stream);
  }
}

// Window `win` of OpRotateCrop's nw x nh result, resampled from the dense RGBE f32 buffer in front of the op with the chain and the quantiser behind it,
// then OpTransform: k_fused_resample's cached-buffer source mode inside launch_then_orient.  b: the buffer -- w x h pixels, `pitch` pixels from row to
// row, E = +0.0 everywhere -- and its monochrome flag; label: the launch's stage
struct RgbeBuffer { const void *p; size_t pitch, w, h; int mono; };
int resample_rgbe_window(const ipk_pipeline_desc *d, const Negotiated &n, const RgbeBuffer &b, const ipk::ResamplePlan &plan, size_t nw, size_t nh,
                         const ipk::ResampleWindow &win, const char *label, StageTimer &tm, size_t want_w, size_t want_h, void *dst, int out_type, void *stream) {
  PointwisePrep pp;
  int rc = pp.prepare(b.mono, d->wb_coeffs, d->cam_to_xyz_normalized, d->exposure, d->points, d->npoints, n.linear); if (rc) return rc;
  pp.f.src = b.p; pp.f.src_is_u16 = false; pp.f.out_type = out_type;
  pp.f.width = b.w; pp.f.height = b.h; pp.f.owidth = b.pitch;
  pp.f.black0 = 0.0f; pp.f.white0 = 1.0f;                                  // not read in this mode
  return launch_then_orient(win.cols, win.rows, out_type, !n.transform_noop, n.orientation, want_w, want_h, dst, stream, [&](void *out) -> int {
    pp.f.dst = out;
    if (ipk::launch_fused_resample(pp.f, plan, nw, nh, nullptr, S(stream), &win, 1) != 0)
      return fail(IPK_ERR_HIP, "kernel launch failed (nothing was enqueued)");
    HIPCHK(hipGetLastError());
    tm.mark(label);
    if (!n.transform_noop) tm.rest = "transform";
    return IPK_OK;
  });
}

// ---- kScaledRotateCrop: the scaling pass into the n.dw x n.dh RGBE buffer, then the resampling launch over it (choose_route / scaled_rotatecrop) ----
// Every tile box of the resampling launch over window w2 -- the kernel's rs_box: the extremes of the windows at the tile's four corner pixels -- lies
// inside the rectangle F of the buffer (an empty F: every box is empty).  resample_footprint's header argues it; the launch below reads a scratch that
// holds F alone, so the host checks it tile by tile before anything is enqueued
bool tile_boxes_inside(const ipk::ResamplePlan &p, size_t W, size_t H, const ipk::ResampleWindow &w2, const ipk::ResampleFootprint &F) {
  for (size_t q0 = 0; q0 < w2.rows; q0 += p.tile_h) {
    for (size_t p0 = 0; p0 < w2.cols; p0 += p.tile_w) {
      const uint32_t r[2] = {(uint32_t)(w2.row0 + q0), (uint32_t)(w2.row0 + std::min<size_t>(q0 + p.tile_h, w2.rows) - 1)};
      const uint32_t c[2] = {(uint32_t)(w2.col0 + p0), (uint32_t)(w2.col0 + std::min<size_t>(p0 + p.tile_w, w2.cols) - 1)};
      uint32_t x0 = 0xFFFFFFFFu, x1 = 0u, y0 = 0xFFFFFFFFu, y1 = 0u;
      for (int i = 0; i < 4; ++i) {
        uint32_t w[4];
        ipk::resample_window_at(p, (uint32_t)W, (uint32_t)H, r[i >> 1], c[i & 1], w);
        x0 = std::min(x0, w[0]); x1 = std::max(x1, w[1]); y0 = std::min(y0, w[2]); y1 = std::max(y1, w[3]);
      }
      if (x1 < x0 || y1 < y0) continue;                                     // the kernel reads nothing for this tile
      if (F.w == 0 || x0 < F.x || y0 < F.y || x1 >= F.x + F.w || y1 >= F.y + F.h) return false;
    }
  }
  return true;
}
// the rectangle of the n.dw x n.dh buffer that window w2 of OpRotateCrop's result reads (w == 0: no pixel of it has a tap)
ipk::ResampleFootprint scaled_rotatecrop_footprint(const Route &rt, const Negotiated &n, const ipk::ResampleWindow &w2) {
  return ipk::resample_footprint(rt.plan2, n.dw, n.dh, w2.row0, w2.col0, w2.rows, w2.cols);
}
// win: the rectangle of OpRotateCrop's rt.pw x rt.ph result a region comes from (plan_region); null: the whole frame.  want_w x want_h: what dst holds
int run_scaled_rotatecrop(const ipk_pipeline_desc *d, const Negotiated &n, const Route &rt, const void *src, const ipk::ResampleWindow *win, size_t want_w,
                          size_t want_h, void *dst, void *stream) {
  StageTimer tm(S(stream));
  const ipk::ResampleWindow whole = {0, 0, rt.rcp.nh, rt.rcp.nw};
  const ipk::ResampleWindow &w2 = win ? *win : whole;
  // pass 1 writes F packed: the whole buffer for a whole frame, the region's footprint in it otherwise
  ipk::ResampleFootprint F = {0, 0, n.dw, n.dh};
  if (win) F = scaled_rotatecrop_footprint(rt, n, w2);
  if (!tile_boxes_inside(rt.plan2, n.dw, n.dh, w2, F)) return fail(IPK_ERR_INVALID, "internal: a tile of the resampling launch leaves the %zux%zu footprint", F.w, F.h);
  Scratch sc(S(stream));
  void *buf = nullptr;
  int rc = sc.get(std::max<size_t>(F.w * F.h, 1) * 4 * sizeof(float), &buf); if (rc) return rc;
  if (F.w != 0) {
    const ipk::ResampleWindow w1 = {F.y, F.x, F.h, F.w};
    const ipk::ResampleWindow *pw1 = win ? &w1 : nullptr;
    rc = rt.pass1 == kPassDemosaicScaled
             ? raw_demosaic_scaled_impl(src, d->src_type, d->width, n.r.x, n.r.y, n.r.width, n.r.height, d->blacklevels[0], d->whitelevels[0], d->cfa, n.dw, n.dh,
                                        pw1, static_cast<float *>(buf), stream)
             : launch_gofloat_demosaic(d, n, src, pw1, static_cast<float *>(buf), stream);
    if (rc < 0) return rc;
  }
  tm.mark(win ? "region gofloat+demosaic" : "gofloat+demosaic");
  // pass 2 addresses its source in the buffer's own coordinates: the pointer is moved back by F's origin and the pitch is F's width, so pixel (x, y) of
  // the buffer is pixel (x - F.x, y - F.y) of the scratch; the kernel reads tile boxes only, all inside F (above)
  const RgbeBuffer b = {reinterpret_cast<const void *>(reinterpret_cast<uintptr_t>(buf) - (uintptr_t)(F.y * F.w + F.x) * 4 * sizeof(float)), F.w, n.dw, n.dh,
                        one_pass_monochrome(d, n)};
  return resample_rgbe_window(d, n, b, rt.plan2, rt.rcp.nw, rt.rcp.nh, w2, win ? rt.region_label : rt.label, tm, want_w, want_h, dst, rt.fp.out_type, stream);
}

// ---- staged path: the eight ops in the reference's order (pipeline.rs:155-164) ----
// The scratch driver: ops [from, 8) and the quantisation, from the buffer `buf` of shape `shape` (op from - 1's, owned by sc; from == 0: none), into dst, which
// holds want_w x want_h pixels of out_type -- the negotiated result behind run_staged, the region behind a window launch (ipk_pipeline_run_region under
// IPK_FUSED_WINDOW_PREVIEWS: from = 3, where every op is point-wise or a permutation, so a rectangle of the buffer gives that rectangle of the result).
// A scratch buffer per executed op, its input released behind it; the shapes are planned before anything is enqueued, so the last executed op writes
// straight into dst when the caller wants f32
int run_tail(const ipk_pipeline_desc *d, const Negotiated &n, int out_type, Scratch &sc, const void *src, int from, void *buf, const OpShape &shape,
             size_t want_w, size_t want_h, void *dst, StageTimer &tm, void *stream) {
  int rc, last = -1;
  auto produced = [&](size_t pw, size_t ph) {
    return pw == want_w && ph == want_h ? IPK_OK : fail(IPK_ERR_INVALID, "internal: produced %zux%zu, negotiated %zux%zu", pw, ph, want_w, want_h);
  };
  OpShape shp[9]; bool runs[8];
  shp[from] = shape;
  for (int i = from; i < 8; ++i) {
    rc = plan_op(i, d, n, shp[i], shp[i + 1]); if (rc < 0) return rc;
    runs[i] = rc != IPK_NOOP;
    if (runs[i]) last = i;
  }
  const bool f32_out = out_type == IPK_OUT_F32;
  for (int i = from; i < 8; ++i) {
    const size_t w = shp[i].w, h = shp[i].h;
    if (i == 3 && fused_on(d) && shp[3].colors == 4) {
      // tolab + basecurve + fromlab + gamma in one pass (no cache wants the three intermediates) ...
      const float *in = static_cast<const float *>(buf);
      if (!f32_out && n.transform_noop && w * h >= 256) {
        // ... and with output8bit / output16bit in the same pass when the caller wants 8 or 16 bits and nothing follows: the f32 image never exists
        rc = produced(w, h); if (rc) return rc;
        rc = ipk_pointwise_chain_out(in, w, h, shp[3].mono, d->wb_coeffs, d->cam_to_xyz_normalized, d->exposure, d->points, d->npoints, n.linear, out_type, dst, stream);
        if (rc < 0) return rc;
        tm.rest = nullptr;
        tm.mark("to_lab+basecurve+from_lab+gamma+quantise");
        return IPK_OK;
      }
      void *o = dst;
      if (!(f32_out && n.transform_noop)) { rc = sc.get(w * h * 3 * sizeof(float), &o); if (rc) return rc; }
      rc = ipk_pointwise_chain(in, w, h, shp[3].mono, d->wb_coeffs, d->cam_to_xyz_normalized, d->exposure, d->points, d->npoints, n.linear, static_cast<float *>(o), stream);
      if (rc < 0) return rc;
      sc.release(buf); buf = o;
      tm.mark("to_lab+basecurve+from_lab+gamma");
      i = 6;                                                               // on to OpTransform
      continue;
    }
    if (i == 7 && runs[7] && !f32_out) {
      // transform -- for the 8- and 16-bit outputs after the quantise loop instead of before it (orient)
      tm.rest = "quantise+transform";
      return launch_then_orient(w, h, out_type, true, n.orientation, want_w, want_h, dst, stream, [&](void *q) { return quantise(buf, w * h * 3, out_type, q, stream); });
    }
    if (runs[i]) {
      void *o = dst;
      if (!(f32_out && i == last)) { rc = sc.get(shp[i + 1].w * shp[i + 1].h * shp[i + 1].colors * sizeof(float), &o); if (rc) return rc; }
      rc = launch_op(i, d, n, src, static_cast<const float *>(buf), shp[i], static_cast<float *>(o), shp[i + 1], stream); if (rc < 0) return rc;
      sc.release(buf); buf = o;
    }
    if (runs[i] || i < 6) tm.mark(kOpLabels[i]);                           // (gamma and transform show as stages only where they run)
  }
  rc = produced(shp[8].w, shp[8].h); if (rc) return rc;
  if (!f32_out) { tm.rest = "quantise"; rc = quantise(buf, shp[8].w * shp[8].h * 3, out_type, dst, stream); }
  return rc < 0 ? rc : IPK_OK;
}
int run_staged(const ipk_pipeline_desc *d, const Negotiated &n, int out_type, const void *src, void *dst, StageTimer &tm, void *stream) {
  Scratch sc(S(stream));
  void *buf = nullptr;
  if (!gofloat_demosaic_one_pass(d, n)) return run_tail(d, n, out_type, sc, src, 0, nullptr, OpShape{}, n.fw, n.fh, dst, tm, stream);
  // gofloat + demosaic as one pass over the source where OpDemosaic::run would scale: op 0's buffer never exists
  int rc = sc.get(n.dw * n.dh * 4 * sizeof(float), &buf); if (rc) return rc;
  rc = launch_gofloat_demosaic(d, n, src, nullptr, static_cast<float *>(buf), stream); if (rc < 0) return rc;
  tm.mark("gofloat+demosaic");
  return run_tail(d, n, out_type, sc, src, 2, buf, OpShape{n.dw, n.dh, 4, one_pass_monochrome(d, n)}, n.fw, n.fh, dst, tm, stream);
}
}  // namespace

int ipk_pipeline_run(const ipk_pipeline_desc *d, const void *src, void *dst, int out_type, int *used_fused, void *stream) {
  REQUIRE_INIT();
  if (!d || !src || !dst) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  int rc = validate_desc(d, out_type, kCheckFuse); if (rc) return rc;      // (the curve's point count is left to the launch that builds the curve)
  // the fast path is tested before the negotiation, not through choose_route: it takes frames the negotiation refuses (a side under 10 pixels)
  if (ipk_pipeline_takes_fastpath(d, out_type) == 1) {
    if (used_fused) *used_fused = 0;
    if (d->width < 1 || d->height < 1) return fail(IPK_ERR_INVALID, "empty source");
    StageTimer tmf(S(stream)); tmf.rest = "fastpath";
    return run_fastpath(d, src, dst, out_type, stream);
  }
  Negotiated n; rc = negotiate(d, out_type, n); if (rc) return rc;
  if (used_fused) *used_fused = 0;
  Route rt; choose_route(d, n, out_type, rt);
  if (rt.kind == kStaged) { StageTimer tm(S(stream)); return run_staged(d, n, out_type, src, dst, tm, stream); }
  rc = rt.kind == kScaledRotateCrop ? run_scaled_rotatecrop(d, n, rt, src, nullptr, n.fw, n.fh, dst, stream)
                                    : run_route(rt, n, src, nullptr, n.fw, n.fh, dst, stream);
  if (rc == IPK_OK && used_fused) *used_fused = 1;
  return rc;
}
// Which route a descriptor takes, for callers and CPU tests: the drivers' own choose_route on the drivers' own negotiation (no GPU)
// r.d: the descriptor as the drivers read it (taken and folded), for the reports that go on to ask a driver's own test with r.n and r.rt
namespace { struct RouteReport { ipk_pipeline_desc d; Negotiated n; Route rt; }; }
static int report_route(const ipk_pipeline_desc *d, int out_type, RouteReport &r) {
  if (!d) return fail(IPK_ERR_INVALID, "null descriptor");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  const int rc = negotiate(d, out_type, r.n); if (rc) return rc;
  choose_route(d, r.n, out_type, r.rt);
  r.d = *d;
  return IPK_OK;
}
// does an active rotatecrop run inside the one launch (fuse_rotatecrop)?
int ipk_pipeline_fuses_rotatecrop(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : r.rt.kind == kFusedResample;
}
// allow_fused's IPK_FUSED_FOUR_COLOUR bit: does a frame whose filter has a fourth colour run as the one raw->sRGB launch?
int ipk_pipeline_fuses_four_colour(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : r.rt.kind == kFusedRaw && r.rt.four;
}
// fuse_scaledown: does OpDemosaic's full + scale_down_opbuf branch run inside the one launch?
int ipk_pipeline_fuses_scaledown(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : r.rt.kind == kFusedScaledown;
}
// IPK_FUSED_SCALED_ROTATECROP: does an active OpRotateCrop behind a scaling OpDemosaic run as the two launches of scaled_rotatecrop()?
int ipk_pipeline_fuses_scaled_rotatecrop(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : r.rt.kind == kScaledRotateCrop;
}
// IPK_FUSED_PLAIN_PREVIEWS: do OpGoFloat and a scaling OpDemosaic of a monochrome / three-sample raw run as the one launch ipk_plain_scale_down?
int ipk_pipeline_scales_plain(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : (r.rt.kind != kFastPath && scales_plain(&r.d, r.n)) ? 1 : 0;
}
// IPK_FUSED_PLAIN: does a cropped raster / a u16 three-sample or monochrome raw run as the one launch ipk_plain_to_srgb (the whole-frame half of the bit)?
int ipk_pipeline_fuses_plain(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : r.rt.kind == kFusedRaster && r.rt.plain;
}

// ------------------------------------------------------------------------------------------
// A region of ipk_pipeline_run's result (a viewer's viewport, one tile of a tiled render)
// ------------------------------------------------------------------------------------------
namespace {
// windowed = 1 on kFusedRaw: the region comes from the unrotated rectangle `win` of the cropped frame, which the window launch computes and
// OpTransform's permutation (dihedral: rectangles map to rectangles) turns into the region.  On kFusedResample / kFusedScaledown where allow_fused
// has IPK_FUSED_WINDOW_REGIONS: the same with the rectangle taken of the resampled rt.pw x rt.ph image that launch produces; the window launch of
// k_fused_resample computes it.  preview = 1 (windowed too), where allow_fused has IPK_FUSED_WINDOW_PREVIEWS beside IPK_FUSED_ON: a staged frame whose
// gofloat + demosaic is the one scaling pass (gofloat_demosaic_one_pass) and whose OpRotateCrop is a no-op -- everything behind that pass is point-wise
// or OpTransform's permutation, so the rectangle is taken of the n.dw x n.dh preview, the pass runs as a window launch and run_tail finishes the
// rectangle.  On kFusedRaster where allow_fused has IPK_FUSED_PLAIN beside IPK_FUSED_ON and the region has at least 256 pixels (the launch's floor): the
// rectangle of the cropped frame, which ipk_plain_to_srgb computes from its own samples alone (point-wise: no halo).  Every other route: windowed = 0, the
// region is cut from the whole result
struct RegionPlan { int windowed, preview; ipk::ResampleWindow win; };
bool windows_preview(const ipk_pipeline_desc *d, const Negotiated &n, const Route &rt) {
  return opted(d, IPK_FUSED_WINDOW_PREVIEWS) && rt.kind == kStaged && gofloat_demosaic_one_pass(d, n) && n.rc.noop();
}
// the descriptor's negotiation and the region against its result: what every region entry point checks first
int negotiate_region(const ipk_pipeline_desc *d, int out_type, size_t x, size_t y, size_t w, size_t h, Negotiated &n) {
  int rc = negotiate(d, out_type, n); if (rc) return rc;
  rc = validate_desc(d, out_type, kCheckCurve); if (rc) return rc;
  if (n.fw == 0 || n.fh == 0) return fail(IPK_ERR_INVALID, "the result is empty");
  if (w == 0 || h == 0 || x > n.fw || w > n.fw - x || y > n.fh || h > n.fh - y)
    return fail(IPK_ERR_INVALID, "region (%zu, %zu) %zux%zu is empty or outside the %zux%zu result", x, y, w, h, n.fw, n.fh);
  return IPK_OK;
}
// The rectangle of the W x H image in front of OpTransform that region (x, y, w, h) of the result comes from, and the flips that take one to the other.
// rotate_buffer's walk (transform.rs:102-128): result pixel (ox, oy) is source pixel (fx ? W-1-u : u, fy ? H-1-v : v) with (u, v) = t ? (oy, ox) : (ox, oy)
int region_window(const Negotiated &n, size_t W, size_t H, size_t x, size_t y, size_t w, size_t h, ipk::ResampleWindow &win, bool &t, bool &fx, bool &fy) {
  t = fx = fy = false;
  if (!n.transform_noop) ipk::orientation_to_flips(n.orientation, t, fx, fy);
  if ((t ? H : W) != n.fw || (t ? W : H) != n.fh) return fail(IPK_ERR_INVALID, "internal: fused result %zux%zu, negotiated %zux%zu", W, H, n.fw, n.fh);
  const size_t u0 = t ? y : x, un = t ? h : w, v0 = t ? x : y, vn = t ? w : h;
  win.col0 = fx ? W - u0 - un : u0; win.cols = un;
  win.row0 = fy ? H - v0 - vn : v0; win.rows = vn;
  return IPK_OK;
}
int plan_region(const ipk_pipeline_desc *d, int out_type, size_t x, size_t y, size_t w, size_t h, Negotiated &n, Route &rt, RegionPlan &pl) {
  int rc = negotiate_region(d, out_type, x, y, w, h, n); if (rc) return rc;
  choose_route(d, n, out_type, rt);
  const bool opted = (d->allow_fused & IPK_FUSED_WINDOW_REGIONS) != 0;
  pl.preview = windows_preview(d, n, rt) ? 1 : 0;
  pl.windowed = (pl.preview || rt.kind == kFusedRaw || rt.kind == kScaledRotateCrop || (opted && (rt.kind == kFusedResample || rt.kind == kFusedScaledown)) ||
                 (rt.kind == kFusedRaster && plain_opted(d) && w * h >= 256)) ? 1 : 0;
  if (!pl.windowed) return IPK_OK;
  bool t, fx, fy;
  return region_window(n, pl.preview ? n.dw : rt.pw, pl.preview ? n.dh : rt.ph, x, y, w, h, pl.win, t, fx, fy);
}
// Where region (x, y, w, h) of the result lies in the bw x bh buffer Pipeline::run hands from OpRotateCrop to OpToLab: region pixel (i, j) is the buffer's
// pixel g.base + i * g.x_step + j * g.y_step.  The buffer's size is the one whose transform is the negotiated result (check_produced's rule: what the
// ops produce is held against n.fw x n.fh), not the forward fold's
// win: the unrotated rectangle of the buffer the region comes from; transposed: the orientation swaps rows and columns (g.x_step is then +-bw)
struct RegionGather { size_t bw, bh; ipk::GatherSource g; ipk::ResampleWindow win; bool transposed; };
// the walk itself: the w-wide region behind rectangle win of a buffer bw pixels wide, under the flips of the orientation.  The region's pixel (0, 0) is
// the window's corner the flips name; a step along u moves one column, along v one row of the buffer
ipk::GatherSource gather_walk(size_t bw, const ipk::ResampleWindow &win, bool t, bool fx, bool fy, size_t w) {
  const int64_t W = (int64_t)bw, du = fx ? -1 : 1, dv = fy ? -W : W;
  const int64_t col = (int64_t)(fx ? win.col0 + win.cols - 1 : win.col0), row = (int64_t)(fy ? win.row0 + win.rows - 1 : win.row0);
  ipk::GatherSource g;
  g.base = row * W + col;
  g.x_step = t ? dv : du; g.y_step = t ? du : dv;
  g.width = w;
  return g;
}
// the whole-frame case: a bw x bh buffer read as its orientation's image (bh wide where the orientation transposes), every index inside the buffer
ipk::GatherSource frame_gather(size_t bw, size_t bh, int orientation) {
  bool t, fx, fy; ipk::orientation_to_flips(orientation, t, fx, fy);
  ipk::ResampleWindow win; win.row0 = 0; win.col0 = 0; win.rows = bh; win.cols = bw;
  return gather_walk(bw, win, t, fx, fy, t ? bh : bw);
}
int region_gather(const Negotiated &n, size_t x, size_t y, size_t w, size_t h, RegionGather &rg) {
  bool t = false, fx = false, fy = false;
  if (!n.transform_noop) ipk::orientation_to_flips(n.orientation, t, fx, fy);
  rg.bw = t ? n.fh : n.fw; rg.bh = t ? n.fw : n.fh;
  ipk::ResampleWindow &win = rg.win;
  const int rc = region_window(n, rg.bw, rg.bh, x, y, w, h, win, t, fx, fy); if (rc) return rc;
  rg.transposed = t;
  rg.g = gather_walk(rg.bw, win, t, fx, fy, w);
  const int64_t W = (int64_t)rg.bw;
  const int64_t far = rg.g.base + (int64_t)(w - 1) * rg.g.x_step + (int64_t)(h - 1) * rg.g.y_step, cnt = W * (int64_t)rg.bh;
  const int64_t cx1 = rg.g.base + (int64_t)(w - 1) * rg.g.x_step, cy1 = rg.g.base + (int64_t)(h - 1) * rg.g.y_step;
  for (int64_t c : {rg.g.base, far, cx1, cy1}) if (c < 0 || c >= cnt) return fail(IPK_ERR_INVALID, "internal: the region's gather leaves the %zux%zu buffer", rg.bw, rg.bh);
  return IPK_OK;
}
}  // namespace

// IPK_FUSED_WINDOW_PREVIEWS: does a region of this descriptor run as a window of its scaling gofloat + demosaic pass?
int ipk_pipeline_windows_preview(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  return rc ? rc : windows_preview(&r.d, r.n, r.rt) ? 1 : 0;
}

int ipk_pipeline_region(const ipk_pipeline_desc *d, int out_type, size_t x, size_t y, size_t w, size_t h, size_t *src_x, size_t *src_y, size_t *src_w,
                        size_t *src_h) {
  if (!d || !src_x || !src_y || !src_w || !src_h) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  Negotiated n; Route rt; RegionPlan pl;
  const int rc = plan_region(d, out_type, x, y, w, h, n, rt, pl); if (rc) return rc;
  if (!pl.windowed) { *src_x = n.r.x; *src_y = n.r.y; *src_w = n.r.width; *src_h = n.r.height; return 0; }
  const ipk::ResampleWindow &win = pl.win;
  if (pl.preview) {
    const ipk::ResampleFootprint f = ipk::scaled_window_footprint(n.r.width, n.r.height, n.dw, n.dh, win.row0, win.col0, win.rows, win.cols);
    *src_x = n.r.x + f.x; *src_y = n.r.y + f.y; *src_w = f.w; *src_h = f.h;
    return 1;
  }
  if (rt.kind == kScaledRotateCrop) {
    // what pass 1's window launch over F -- the rectangle's footprint in the n.dw x n.dh buffer -- reads, in sensor coordinates; empty where F is
    const ipk::ResampleFootprint F = scaled_rotatecrop_footprint(rt, n, win);
    ipk::ResampleFootprint f = {0, 0, 0, 0};
    ipk::ResamplePlan p1;
    if (F.w != 0 && rt.pass1 == kPassDemosaicScaled) {
      if (!ipk::scaledown_plan(n.r.width, n.r.height, n.dw, n.dh, p1)) return fail(IPK_ERR_INVALID, "internal: the route's plan was refused");
      f = ipk::resample_footprint(p1, n.r.width, n.r.height, F.y, F.x, F.h, F.w);
    } else if (F.w != 0) f = ipk::scaled_window_footprint(n.r.width, n.r.height, n.dw, n.dh, F.y, F.x, F.h, F.w);
    *src_x = n.r.x + f.x; *src_y = n.r.y + f.y; *src_w = f.w; *src_h = f.h;
    return 1;
  }
  if (rt.kind == kFusedRaster) {                                  // point-wise from the sensor samples: the rectangle itself, in sensor coordinates
    *src_x = n.r.x + win.col0; *src_y = n.r.y + win.row0; *src_w = win.cols; *src_h = win.rows;
    return 1;
  }
  if (rt.kind != kFusedRaw) {
    // the window launch's footprint (ipk_transform_window_footprint) in sensor coordinates; empty where no pixel of the rectangle has a tap
    const int64_t *pts = rt.rcp.pts;
    ipk::ResamplePlan plan;
    const bool ok = rt.kind == kFusedResample ? ipk::resample_plan(n.r.width, n.r.height, pts[0], pts[1], pts[2], pts[3], pts[4], pts[5], rt.pw, rt.ph, plan)
                                              : ipk::scaledown_plan(n.r.width, n.r.height, rt.pw, rt.ph, plan);
    if (!ok) return fail(IPK_ERR_INVALID, "internal: the route's plan was refused");
    const ipk::ResampleFootprint f = ipk::resample_footprint(plan, n.r.width, n.r.height, win.row0, win.col0, win.rows, win.cols);
    *src_x = n.r.x + f.x; *src_y = n.r.y + f.y; *src_w = f.w; *src_h = f.h;
    return 1;
  }
  // demosaic::full's one-pixel halo, clipped to the crop window, in sensor coordinates
  const size_t c0 = win.col0 > 0 ? win.col0 - 1 : 0, c1 = std::min(n.r.width, win.col0 + win.cols + 1);
  const size_t r0 = win.row0 > 0 ? win.row0 - 1 : 0, r1 = std::min(n.r.height, win.row0 + win.rows + 1);
  *src_x = n.r.x + c0; *src_y = n.r.y + r0; *src_w = c1 - c0; *src_h = r1 - r0;
  return 1;
}

int ipk_pipeline_run_region(const ipk_pipeline_desc *d, const void *src, size_t x, size_t y, size_t w, size_t h, void *dst, int out_type, int *windowed,
                            void *stream) {
  REQUIRE_INIT();
  if (!d || !src || !dst) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  Negotiated n; Route rt; RegionPlan pl;
  int rc = plan_region(d, out_type, x, y, w, h, n, rt, pl); if (rc) return rc;
  if (windowed) *windowed = pl.windowed;
  if (!pl.windowed) {
    const size_t esz = out_elem_size(out_type);
    // every other route: the whole result into scratch, then the region's rows in one 2-D copy
    Scratch sc(S(stream));
    void *full = nullptr;
    rc = sc.get(n.fw * n.fh * 3 * esz, &full); if (rc) return rc;
    rc = ipk_pipeline_run(d, src, full, out_type, nullptr, stream); if (rc < 0) return rc;
    StageTimer tc(S(stream)); tc.rest = "region copy";
    return cut_region(full, n.fw, esz, x, y, w, h, dst, stream);
  }
  if (pl.preview) {
    // the scaling pass over the rectangle of the preview, then what run_staged runs behind it, on the rectangle
    StageTimer tm(S(stream));
    Scratch sc(S(stream));
    void *buf = nullptr;
    rc = sc.get(pl.win.cols * pl.win.rows * 4 * sizeof(float), &buf); if (rc) return rc;
    rc = launch_gofloat_demosaic(d, n, src, &pl.win, static_cast<float *>(buf), stream); if (rc < 0) return rc;
    tm.mark("region gofloat+demosaic");
    return run_tail(d, n, out_type, sc, src, 3, buf, OpShape{pl.win.cols, pl.win.rows, 4, one_pass_monochrome(d, n)}, w, h, dst, tm, stream);
  }
  // the one-launch routes: the window launch writes the rectangle into dst, or into scratch for OpTransform's permutation
  if (rt.kind == kScaledRotateCrop) return run_scaled_rotatecrop(d, n, rt, src, &pl.win, w, h, dst, stream);
  return run_route(rt, n, src, &pl.win, w, h, dst, stream);
}

// ------------------------------------------------------------------------------------------
// Pipeline::run with a cache (src/pipeline.rs:341-372): hash chain + memoised device OpBuffers
// ------------------------------------------------------------------------------------------
namespace {
// ophashes[0..7] of pipeline.rs:342-361.  Field order follows the reference structs.
void hash_chain(const ipk_pipeline_desc *d, const Negotiated &n, uint64_t source_id, ipk::BufHash out[8]) {
  ipk::BufHasher h;
  // PipelineSettings (pipeline.rs:110-137)
  h.usize(d->maxwidth); h.usize(d->maxheight); h.usize(n.dw); h.usize(n.dh); h.boolean(n.linear != 0); h.boolean(d->use_fastpath != 0);
  // gofloat (gofloat.rs:4-12).  The reference hashes no identity of the image at all (a PipelineCache is only
  // valid for one source); source_id + the source geometry make one cache safe across several resident frames.
  h.str_raw("gofloat");
  h.usize(d->crop_top); h.usize(d->crop_right); h.usize(d->crop_bottom); h.usize(d->crop_left); h.boolean(d->is_cfa != 0);
  h.f32s(d->blacklevels, 4); h.f32s(d->whitelevels, 4);
  h.u64(source_id); h.u64(uint64_t(d->src_type)); h.usize(d->width); h.usize(d->height); h.u64(uint64_t(d->cpp));
  out[0] = h.result();
  h.str_raw("demosaic"); h.string(d->cfa);                                               // demosaic.rs:4-6
  out[1] = h.result();
  h.str_raw("rotatecrop");                                                               // rotatecrop.rs:10-18
  h.f32(n.rc.crop_top); h.f32(n.rc.crop_right); h.f32(n.rc.crop_bottom); h.f32(n.rc.crop_left); h.f32(n.rc.rotation);
  h.f32(n.rc.input_ratio); h.boolean(n.rc.has_output); if (n.rc.has_output) { h.usize(n.rc.out_w); h.usize(n.rc.out_h); }
  out[2] = h.result();
  h.str_raw("to_lab"); h.f32s(d->cam_to_xyz_normalized, 12); h.f32s(d->wb_coeffs, 4);   // colorspaces.rs:5-10 (the fields run() reads)
  out[3] = h.result();
  h.str_raw("basecurve"); h.f32(d->exposure); h.u64(uint64_t(d->npoints)); h.f32s(d->points, size_t(2 * std::max(0, d->npoints)));   // curves.rs:6-9
  out[4] = h.result();
  h.str_raw("from_lab"); out[5] = h.result();
  h.str_raw("gamma"); out[6] = h.result();
  h.str_raw("transform"); h.u64(uint64_t(d->rotation)); h.boolean(d->fliph != 0); h.boolean(d->flipv != 0);                          // transform.rs:15-19
  out[7] = h.result();
}
ipk::BufHash key_of(const uint8_t *k) { ipk::BufHash b; std::memcpy(b.data(), k, 32); return b; }
}  // namespace

int ipk_pipeline_hashes(const ipk_pipeline_desc *d, int out_type, uint64_t source_id, uint8_t *out256) {
  if (!out256) return fail(IPK_ERR_INVALID, "null output");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  Negotiated n; int rc = negotiate(d, out_type, n); if (rc) return rc;
  rc = validate_desc(d, out_type, kCheckCurve); if (rc) return rc;
  ipk::BufHash hs[8]; hash_chain(d, n, source_id, hs);
  for (int i = 0; i < 8; ++i) std::memcpy(out256 + 32 * i, hs[i].data(), 32);
  return IPK_OK;
}

// the cached buffers' users run on the owner's device: drain THAT device (whatever context the calling thread has current) before they are freed
static void cache_drain(ipk_cache *c) {
  ipk_ctx *o = c->owner ? c->owner : ipk_ctx_current();
  if (!o || !o->ready) return;
  int prev = -1; (void)hipGetDevice(&prev);
  if (prev != o->device) (void)hipSetDevice(o->device);
  (void)hipDeviceSynchronize();
  if (prev >= 0 && prev != o->device) (void)hipSetDevice(prev);
}
int ipk_cache_new(size_t max_bytes, ipk_cache **out) {
  if (!out) return fail(IPK_ERR_INVALID, "null output");
  *out = new ipk_cache(max_bytes, ipk_ctx_current());
  return IPK_OK;
}
int ipk_cache_free(ipk_cache *c) {
  if (c) { cache_drain(c); delete c; }
  return IPK_OK;
}
int ipk_cache_clear(ipk_cache *c) {
  if (!c) return fail(IPK_ERR_INVALID, "null cache");
  cache_drain(c);
  c->lru.clear();
  return IPK_OK;
}
int ipk_cache_contains(const ipk_cache *c, const uint8_t *key32) {
  if (!c || !key32) return fail(IPK_ERR_INVALID, "null argument");
  return c->lru.contains(key_of(key32)) ? 1 : 0;
}
int ipk_cache_stats(const ipk_cache *c, size_t *bytes, size_t *entries, uint64_t *hits, uint64_t *misses, uint64_t *evictions) {
  if (!c) return fail(IPK_ERR_INVALID, "null cache");
  size_t b, e; uint64_t hi, mi, ev; c->lru.stats(b, e, hi, mi, ev);
  if (bytes) *bytes = b; if (entries) *entries = e; if (hits) *hits = hi; if (misses) *misses = mi; if (evictions) *evictions = ev;
  return IPK_OK;
}
int ipk_cache_get(ipk_cache *c, const uint8_t *key32, const float **data, size_t *width, size_t *height, size_t *colors, int *monochrome) {
  if (!c || !key32) return fail(IPK_ERR_INVALID, "null argument");
  CBufP b = c->lru.get(key_of(key32));
  if (!b) return IPK_NOOP;
  if (data) *data = static_cast<const float *>(b->p);
  if (width) *width = b->w; if (height) *height = b->h; if (colors) *colors = b->colors; if (monochrome) *monochrome = b->mono;
  return IPK_OK;
}
int ipk_selftest_cache_put(ipk_cache *c, const uint8_t *key32, size_t bytes) {   // LRU bookkeeping without device memory (CPU tests)
  if (!c || !key32) return fail(IPK_ERR_INVALID, "null argument");
  c->lru.put(key_of(key32), std::make_shared<CBuf>(), bytes);
  return IPK_OK;
}
int ipk_selftest_sha256(const void *data, size_t n, uint8_t *out32) {
  ipk::Sha256 s; s.update(data, n); const auto r = s.result(); std::memcpy(out32, r.data(), 32); return IPK_OK;
}

namespace {
int claim_cache(ipk_cache *cache) {
  if (!cache->owner) cache->owner = ipk_ctx_current();                   // a cache made before ipk_init belongs to the first context that fills it
  if (cache->owner != ipk_ctx_current()) return fail(IPK_ERR_INVALID, "the cache belongs to another context (its buffers live on that context's device)");
  return IPK_OK;
}
// the latest op among [0, upto) whose output is memoised (pipeline.rs:352-361: every hash is looked up, the last hit wins) into buf; the op to resume at
int cache_resume(ipk_cache *cache, const ipk::BufHash hs[8], int upto, CBufP &buf) {
  int startpos = 0;
  for (int i = 0; i < upto; ++i) { CBufP hit = cache->lru.get(hs[i]); if (hit) { buf = hit; startpos = i + 1; } }
  return startpos;
}
// ops_run bits 3..7 of a launch that runs the point-wise tail with OpTransform: to_lab and from_lab always, the no-ops of the reference not counted
int pointwise_ops_mask(bool has_curve, const Negotiated &n) { return 0x28 | (has_curve ? 1 << 4 : 0) | (n.linear ? 0 : 1 << 6) | (n.transform_noop ? 0 : 1 << 7); }
// Ops [from, to) of Pipeline::run(Some(cache)) from `buf` (op from - 1's buffer; unused for from == 0): every buffer materialised enters the cache under
// its op's hash, a no-op stores its input under its own key, `mask` gains bit i for every op executed and `buf` ends as op to - 1's buffer.  Shared by
// ipk_pipeline_run_cached (to = 8) and ipk_pipeline_run_cached_region (to = 3: the RGBE buffer its gather launch reads)
int run_cached_ops(const ipk_pipeline_desc *d, const Negotiated &n, const ipk::BufHash hs[8], const void *src, ipk_cache *cache, int from, int to,
                   CBufP &buf, int &mask, void *stream) {
  for (int i = from; i < to; ++i) {
    CBufP o;
    if (i == 0 && gofloat_demosaic_one_pass(d, n) && !cache->lru.contains(hs[1])) {   // gofloat + demosaic in the same pass when it would scale
      int rc = cbuf_new(n.dw, n.dh, 4, one_pass_monochrome(d, n), o); if (rc) return rc;
      rc = launch_gofloat_demosaic(d, n, src, nullptr, static_cast<float *>(o->p), stream); if (rc < 0) return rc;
      mask |= 3; buf = o; cache->lru.put(hs[1], o, o->bytes()); i = 1;     // op 1's output; op 0's is never materialised
      continue;
    }
    const OpShape in = buf ? OpShape{buf->w, buf->h, buf->colors, buf->mono} : OpShape{};
    OpShape out;
    int rc = plan_op(i, d, n, in, out); if (rc < 0) return rc;
    if (rc != IPK_NOOP) {                                                  // a no-op hands its input on (the same Arc under a second key)
      rc = cbuf_new(out.w, out.h, out.colors, out.mono, o); if (rc) return rc;
      rc = launch_op(i, d, n, src, static_cast<const float *>(buf ? buf->p : nullptr), in, static_cast<float *>(o->p), out, stream); if (rc < 0) return rc;
      buf = o;
    }
    mask |= 1 << i;
    cache->lru.put(hs[i], buf, buf->bytes());
  }
  return IPK_OK;
}
}  // namespace

int ipk_pipeline_run_cached(const ipk_pipeline_desc *d, const void *src, uint64_t source_id, ipk_cache *cache, int out_type, void *dst,
                            int *ops_run, int *used_fused, void *stream) {
  REQUIRE_INIT();
  if (!d || !src || !dst || !cache) return fail(IPK_ERR_INVALID, "null argument");
  int rc = claim_cache(cache); if (rc) return rc;
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  rc = validate_desc(d, out_type, kCheckCurve | kCheckFuse); if (rc) return rc;
  if (ipk_pipeline_takes_fastpath(d, out_type) == 1) {                    // returns before the cache is consulted (pipeline.rs:381-402), and before the negotiation
    if (ops_run) *ops_run = 0;
    if (used_fused) *used_fused = 0;
    return run_fastpath(d, src, dst, out_type, stream);
  }
  Negotiated n; rc = negotiate(d, out_type, n); if (rc) return rc;
  ipk::BufHash hs[8]; hash_chain(d, n, source_id, hs);
  if (ops_run) *ops_run = 0;
  if (used_fused) *used_fused = 0;
  hipStream_t st = S(stream);

  CBufP buf;
  int startpos = cache_resume(cache, hs, 8, buf), mask = 0;

  // Nothing memoised and gofloat..transform is one launch on a raw source (any orientation: run_route folds OpTransform in): cheaper on this machine
  // than materialising seven intermediates; only the final buffer enters the cache.  The buffer is f32 whatever the caller wants,
  // so the route is asked for IPK_OUT_F32; a raster source's one launch is not taken here (its staged ops fill the cache)
  Route rt;
  if (startpos == 0) choose_route(d, n, IPK_OUT_F32, rt);
  if (startpos == 0 && (rt.kind == kFusedRaw || rt.kind == kFusedResample || rt.kind == kFusedScaledown)) {
    CBufP o; rc = cbuf_new(n.fw, n.fh, 3, 0, o); if (rc) return rc;
    rc = run_route(rt, n, src, nullptr, n.fw, n.fh, o->p, stream);
    if (rc < 0) return rc;
    cache->lru.put(hs[7], o, o->bytes());
    buf = o; startpos = 8; mask = 0xFF;
    if (used_fused) *used_fused = rc == IPK_OK;
  }

  rc = run_cached_ops(d, n, hs, src, cache, startpos, 8, buf, mask, stream); if (rc < 0) return rc;
  if (ops_run) *ops_run = mask;
  rc = check_produced(n, buf->w, buf->h, buf->colors); if (rc) return rc;
  const size_t cnt = buf->w * buf->h * 3;
  if (out_type != IPK_OUT_F32) rc = quantise(buf->p, cnt, out_type, dst, stream);
  else { HIPCHK(hipMemcpyAsync(dst, buf->p, cnt * sizeof(float), hipMemcpyDeviceToDevice, st)); rc = IPK_OK; }
  if (rc < 0) return rc;
  // `buf` may be evicted (and its memory freed) as soon as we return; hipFree waits for the device, so the copy above is safe
  return IPK_OK;
}

// ------------------------------------------------------------------------------------------
// A region from the cache: the buffer behind OpRotateCrop is all a region needs (everything after it is point-wise or OpTransform's permutation)
// ------------------------------------------------------------------------------------------
namespace {
// IPK_FUSED_CACHED_RESAMPLE: may a region be resampled straight from the demosaic buffer (hash 1)?  The bit beside IPK_FUSED_ON, off the fast path, an
// OpRotateCrop that is active and accepts its crops on the sw x sh buffer OpDemosaic hands it (pipeline_sizes_impl's rule: the negotiated size where it
// scales, else the cropped source), no fourth colour -- the one 4-channel buffer whose E is not +0.0 everywhere --, and a transform the launch admits
struct CachedResample { size_t sw, sh; RotateCropPoints r; ipk::ResamplePlan plan; };
bool cached_resample(const ipk_pipeline_desc *d, const Negotiated &n, int out_type, CachedResample &c) {
  if (!opted(d, IPK_FUSED_CACHED_RESAMPLE) || ipk_pipeline_takes_fastpath(d, out_type) == 1) return false;
  if (n.cfa_branch) { ipk::Cfa cfa; if (!ipk::Cfa::parse(d->cfa, cfa) || !cfa.valid() || !cfa.three_colour()) return false; }
  c.sw = n.scale > 1.0f ? n.dw : n.r.width; c.sh = n.scale > 1.0f ? n.dh : n.r.height;
  return rotatecrop_resamples(d, n, c.sw, c.sh, c.r, c.plan);
}
}  // namespace
int ipk_pipeline_resamples_cached_region(const ipk_pipeline_desc *d, int out_type) {
  RouteReport r; const int rc = report_route(d, out_type, r);
  CachedResample c;
  return rc ? rc : cached_resample(&r.d, r.n, out_type, c) ? 1 : 0;
}

int ipk_pipeline_region_gather(const ipk_pipeline_desc *d, int out_type, size_t x, size_t y, size_t w, size_t h, size_t *buf_w, size_t *buf_h,
                               int64_t *base, int64_t *x_step, int64_t *y_step) {
  if (!d || !buf_w || !buf_h || !base || !x_step || !y_step) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  Negotiated n; RegionGather rg;
  int rc = negotiate_region(d, out_type, x, y, w, h, n); if (rc) return rc;
  rc = region_gather(n, x, y, w, h, rg); if (rc) return rc;
  *buf_w = rg.bw; *buf_h = rg.bh; *base = rg.g.base; *x_step = rg.g.x_step; *y_step = rg.g.y_step;
  return IPK_OK;
}

namespace {
// One ipk_pipeline_run_cached_region call behind its checks -- arguments, negotiation, the region's place in the buffer behind OpRotateCrop, hash chain --
// and the four forms that serve it, one per state of descriptor and cache.  `mask` gains the bit of every op a form executed
struct CachedRegion {
  const ipk_pipeline_desc *d; const void *src; ipk_cache *cache; size_t x, y, w, h; void *dst; int out_type; void *stream;
  Negotiated n; RegionGather rg; ipk::BufHash hs[8];
  // a fast-path descriptor: the reference returns before it consults the cache: the whole result, then the rectangle
  int cut_fastpath() const {
    const size_t esz = out_elem_size(out_type);
    Scratch sc(S(stream));
    void *full = nullptr;
    int rc = sc.get(n.fw * n.fh * 3 * esz, &full); if (rc) return rc;
    rc = run_fastpath(d, src, full, out_type, stream); if (rc < 0) return rc;
    return cut_region(full, n.fw, esz, x, y, w, h, dst, stream);
  }
  // the final buffer is memoised: the region is cut from it (8- / 16-bit output: the f32 rectangle into scratch, then the quantiser)
  int cut_final(const CBufP &fin) const {
    StageTimer tm(S(stream));
    int rc = check_produced(n, fin->w, fin->h, fin->colors); if (rc) return rc;
    tm.rest = "region copy";
    Scratch sc(S(stream));
    void *rect = dst;
    if (out_type != IPK_OUT_F32) { rc = sc.get(w * h * 3 * sizeof(float), &rect); if (rc) return rc; }
    rc = cut_region(fin->p, n.fw, sizeof(float), x, y, w, h, rect, stream);
    if (rc || out_type == IPK_OUT_F32) return rc;
    tm.mark(tm.rest); tm.rest = "quantise";
    rc = quantise(rect, w * h * 3, out_type, dst, stream);
    return rc < 0 ? rc : IPK_OK;
  }
  // IPK_FUSED_CACHED_RESAMPLE with the rotatecrop buffer missing (a crop or straighten edit): the cache is brought up to op 1 only, and ONE launch resamples
  // the region's rectangle of OpRotateCrop's rg.bw x rg.bh result from that buffer, chain and quantiser behind it (k_fused_resample's cached-buffer
  // source mode).  Nothing enters the cache under hash 2.  Every orientation but Normal: the plain rectangle into scratch, then orient()
  int resample(const CachedResample &cr, int &mask) const {
    StageTimer tm(S(stream));
    CBufP buf;
    const int startpos = cache_resume(cache, hs, 2, buf);
    int rc = run_cached_ops(d, n, hs, src, cache, startpos, 2, buf, mask, stream); if (rc < 0) return rc;
    if (buf->w != cr.sw || buf->h != cr.sh || buf->colors != 4 || cr.r.nw != rg.bw || cr.r.nh != rg.bh)
      return fail(IPK_ERR_INVALID, "internal: produced %zux%zux%zu in front of rotatecrop (negotiated %zux%zu), rotatecrop to %zux%zu (negotiated %zux%zu)",
                  buf->w, buf->h, buf->colors, cr.sw, cr.sh, cr.r.nw, cr.r.nh, rg.bw, rg.bh);
    if (mask) tm.mark("gofloat..demosaic");
    const RgbeBuffer b = {buf->p, buf->w, buf->w, buf->h, buf->mono};
    rc = resample_rgbe_window(d, n, b, cr.plan, rg.bw, rg.bh, rg.win, "region rotatecrop+to_lab+basecurve+from_lab+gamma", tm, w, h, dst, out_type, stream);
    if (rc < 0) return rc;
    mask |= (1 << 2) | pointwise_ops_mask(!curve_is_noop(d->exposure, d->npoints), n);
    // `buf` may be evicted (and its memory freed) as soon as we return; hipFree waits for the device, so the launch above is safe
    return rc;
  }
  // Bring the cache up to op 2: the latest hit among gofloat, demosaic and rotatecrop, then the missing ones as ipk_pipeline_run_cached runs them.  Its
  // whole-frame one-launch shortcut is not taken (the next edit is to find the RGBE buffer), and hits behind op 2 are not used: entering at the RGBE
  // buffer is one launch either way
  int gather(int &mask) const {
    StageTimer tm(S(stream));
    CBufP buf;
    const int startpos = cache_resume(cache, hs, 3, buf);
    int rc = run_cached_ops(d, n, hs, src, cache, startpos, 3, buf, mask, stream); if (rc < 0) return rc;
    if (buf->w != rg.bw || buf->h != rg.bh || buf->colors != 4)
      return fail(IPK_ERR_INVALID, "internal: produced %zux%zux%zu in front of to_lab, negotiated %zux%zu", buf->w, buf->h, buf->colors, rg.bw, rg.bh);
    if (mask) tm.mark("gofloat..rotatecrop");
    // ONE launch over the rectangle: to_lab..gamma with OpTransform folded into the load (and the quantisation where the region has the launch's 256 pixels).
    // The transposing orientations are the exception from 256 pixels up: there a wave's 64 loads of the folded form lie a buffer row apart, one cache line
    // each, and the launch measured 3.3x the plain rectangle's time at 24 MP (0.68 against 0.20 ms, profiles/r15_cached_region.txt) -- more than orient()
    // costs on the rectangle.  They take the plain-rectangle gather launch into scratch and orient() behind it, the two-launch form run_tail uses
    PointwisePrep pp;
    rc = pp.prepare(buf->mono, d->wb_coeffs, d->cam_to_xyz_normalized, d->exposure, d->points, d->npoints, n.linear); if (rc) return rc;
    const size_t npix = w * h;
    const bool direct = out_type == IPK_OUT_F32 || npix >= 256;
    const bool two = rg.transposed && npix >= 256;
    const ipk::GatherSource g = two ? ipk::GatherSource{(int64_t)(rg.win.row0 * rg.bw + rg.win.col0), 1, (int64_t)rg.bw, rg.win.cols} : rg.g;
    pp.f.src = buf->p; pp.f.out_type = direct ? out_type : IPK_OUT_F32;
    rc = launch_then_orient(rg.win.cols, rg.win.rows, out_type, two, n.orientation, w, h, dst, stream, [&](void *out) -> int {
      Scratch sc(S(stream));                                               // under 256 pixels an 8- / 16-bit region is the f32 launch and the quantiser
      void *o = out;
      if (!direct) { const int grc = sc.get(npix * 3 * sizeof(float), &o); if (grc) return grc; }
      pp.f.dst = o;
      const int lrc = pp.f.out_type == IPK_OUT_F32 ? ipk::launch_pointwise_chain(pp.f, npix, S(stream), &g) : ipk::launch_chain_quantised(pp.f, npix, S(stream), &g);
      if (lrc != 0) return fail(IPK_ERR_INVALID, "internal: the gather launch refused a %zux%zu region", w, h);
      HIPCHK(hipGetLastError());
      tm.mark(two ? "region to_lab+basecurve+from_lab+gamma" : "region to_lab+basecurve+from_lab+gamma+transform");
      if (two) tm.rest = "transform";
      if (direct) return IPK_OK;
      tm.rest = "quantise";
      return quantise(o, npix * 3, out_type, out, stream);
    });
    mask |= pointwise_ops_mask(pp.f.has_curve, n);
    // `buf` may be evicted (and its memory freed) as soon as we return; hipFree waits for the device, so the launch above is safe
    return rc;
  }
};
}  // namespace

int ipk_pipeline_run_cached_region(const ipk_pipeline_desc *d, const void *src, uint64_t source_id, ipk_cache *cache, size_t x, size_t y, size_t w, size_t h,
                                   void *dst, int out_type, int *ops_run, int *windowed, void *stream) {
  if (!d || !src || !dst || !cache) return fail(IPK_ERR_INVALID, "null argument");
  REQUIRE_INIT();
  int rc = claim_cache(cache); if (rc) return rc;
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  rc = validate_desc(d, out_type, kCheckCurve | kCheckFuse); if (rc) return rc;
  CachedRegion c = {d, src, cache, x, y, w, h, dst, out_type, stream, {}, {}, {}};
  rc = negotiate_region(d, out_type, x, y, w, h, c.n); if (rc) return rc;
  rc = region_gather(c.n, x, y, w, h, c.rg); if (rc) return rc;
  if (ops_run) *ops_run = 0; if (windowed) *windowed = 0;
  // the form, in order of precedence: a fast-path descriptor, the final buffer memoised, IPK_FUSED_CACHED_RESAMPLE without the rotatecrop buffer, the gather
  if (ipk_pipeline_takes_fastpath(d, out_type) == 1) return c.cut_fastpath();
  hash_chain(d, c.n, source_id, c.hs);
  if (CBufP fin = cache->lru.get(c.hs[7])) return c.cut_final(fin);
  CachedResample cr; int mask = 0;
  rc = cached_resample(d, c.n, out_type, cr) && !cache->lru.contains(c.hs[2]) ? c.resample(cr, mask) : c.gather(mask);
  if (rc < 0) return rc;
  if (ops_run) *ops_run = mask; if (windowed) *windowed = 1;
  return IPK_OK;
}

// ------------------------------------------------------------------------------------------
// host-pointer forms
// ------------------------------------------------------------------------------------------
namespace {
struct DevBuf {
  void *p = nullptr;
  ~DevBuf() { if (p) (void)hipFree(p); }
  int alloc(size_t bytes) { return hipMalloc(&p, bytes ? bytes : 1) == hipSuccess ? IPK_OK : fail(IPK_ERR_NOMEM, "hipMalloc(%zu) failed", bytes); }
  int upload(const void *h, size_t bytes) { int rc = alloc(bytes); if (rc) return rc; HIPCHK(hipMemcpy(p, h, bytes, hipMemcpyHostToDevice)); return IPK_OK; }
  int download(void *h, size_t bytes) { HIPCHK(hipMemcpy(h, p, bytes, hipMemcpyDeviceToHost)); return IPK_OK; }
};
size_t src_elem_size(int t) { return t == IPK_SRC_U16 ? 2 : t == IPK_SRC_F32 ? 4 : t == IPK_SRC_RGB8 ? 1 : 2; }
}  // namespace

#define HOST_TRY(expr) do { int rc_ = (expr); if (rc_ < 0) return rc_; } while (0)

int ipk_host_pipeline_run(const ipk_pipeline_desc *d, const void *src, void *dst, int out_type, int *used_fused) {
  if (!src || !dst) { REQUIRE_INIT(); return fail(IPK_ERR_INVALID, "null argument"); }
  return ipk_host_pipeline_run_batch(d, &src, &dst, 1, out_type, used_fused);
}
void *ipk_host_alloc(size_t bytes) {
  void *p = nullptr;
  if (hipHostMalloc(&p, bytes ? bytes : 1, hipHostMallocPortable) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
  return p;
}
void ipk_host_free(void *p) { if (p) (void)hipHostFree(p); }

namespace {
int HostLanes::ensure(size_t in_bytes, size_t out_bytes) {
  if (!made) {
    for (hipStream_t *s : {&up, &run, &down}) HIPCHK(hipStreamCreateWithFlags(s, hipStreamNonBlocking));
    for (int i = 0; i < kSlots; ++i)
      for (hipEvent_t *e : {&up_done[i], &run_done[i], &down_done[i]}) HIPCHK(hipEventCreateWithFlags(e, hipEventDisableTiming));
    made = true;
  }
  if (in_bytes > in_cap) {
    for (int i = 0; i < kSlots; ++i) { if (in[i]) (void)hipFree(in[i]); in[i] = nullptr; }
    in_cap = 0;
    for (int i = 0; i < kSlots; ++i) if (hipMalloc(&in[i], in_bytes) != hipSuccess) return fail(IPK_ERR_NOMEM, "hipMalloc(%zu) failed", in_bytes);
    in_cap = in_bytes;
  }
  if (out_bytes > out_cap) {
    for (int i = 0; i < kSlots; ++i) { if (out[i]) (void)hipFree(out[i]); out[i] = nullptr; }
    out_cap = 0;
    for (int i = 0; i < kSlots; ++i) if (hipMalloc(&out[i], out_bytes) != hipSuccess) return fail(IPK_ERR_NOMEM, "hipMalloc(%zu) failed", out_bytes);
    out_cap = out_bytes;
  }
  return IPK_OK;
}
void HostLanes::release() {
  for (hipStream_t *s : {&up, &run, &down}) if (*s) { (void)hipStreamSynchronize(*s); (void)hipStreamDestroy(*s); *s = nullptr; }
  for (int i = 0; i < kSlots; ++i) {
    for (hipEvent_t *e : {&up_done[i], &run_done[i], &down_done[i]}) if (*e) { (void)hipEventDestroy(*e); *e = nullptr; }
    if (in[i]) (void)hipFree(in[i]); if (out[i]) (void)hipFree(out[i]);
    in[i] = out[i] = nullptr;
  }
  in_cap = out_cap = 0; made = false;
}
}  // namespace

// ------------------------------------------------------------------------------------------
// A caller looping Pipeline::run over the frames of a shoot (src/pipeline.rs:246-249: frames are independent), device pointers
// ------------------------------------------------------------------------------------------
// In order: the two frame-table primitives, the comparisons of two descriptors, the admission of one, the plan of n, the chunk walk, the drivers
namespace {
// ---- the two frame-table primitives ----
// ipk_scaled_demosaic_batch_each: every frame validated and admitted (its filter's device table fetched) before anything is enqueued, then one frame-table
// launch per 64 frames (launch_raw_scaled_demosaic_each), its table in the scratch pool.  stage: the name marked behind every launch
// sizes (optional, 2n values: nwidth_i, nheight_i; ipk_scaled_demosaic_batch_sized): frame i's own result size -- nwidth and nheight are not read, slice i
// lies behind the earlier slices, and each group of 64 is one sized launch.  Equal sizes throughout are the call without them
int scaled_batch_each_impl(const void *const *srcs, const ipk_scaled_frame *frames, size_t n, int src_type, int kind, size_t nwidth, size_t nheight, float *dst4,
                           void *stream, StageTimer &tm, const char *stage, const size_t *sizes = nullptr) {
  if (n == 0) return IPK_OK;
  if (kind == IPK_PLAIN_RASTER) return fail(IPK_ERR_UNSUPPORTED, "scaled_demosaic_batch_each: the raster scaler has no frame-table mode");
  if (kind != -1 && kind != IPK_PLAIN_RGB && kind != IPK_PLAIN_MONO) return fail(IPK_ERR_INVALID, "bad kind");
  if (n > (size_t)1 << 20) return fail(IPK_ERR_INVALID, "batch too large");
  if (sizes) {
    bool equal = true;
    for (size_t i = 0; i < n; ++i) {
      if (!dims_ok(sizes[2 * i], sizes[2 * i + 1])) return fail(IPK_ERR_INVALID, "sizes[%zu]: bad dimensions %zux%zu", i, sizes[2 * i], sizes[2 * i + 1]);
      equal = equal && sizes[2 * i] == sizes[0] && sizes[2 * i + 1] == sizes[1];
    }
    nwidth = sizes[0]; nheight = sizes[1];                                   // equal throughout: the call without sizes
    if (equal) sizes = nullptr;
  }
  if (!srcs || !frames || !dst4 || !dims_ok(nwidth, nheight) || (src_type != IPK_SRC_U16 && src_type != IPK_SRC_F32))
    return fail(IPK_ERR_INVALID, "bad scaled_demosaic_batch_each arguments");
  const bool plain = kind != -1;
  std::vector<ipk::ScaledFrameLaunch> fl(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t nw_i = sizes ? sizes[2 * i] : nwidth, nh_i = sizes ? sizes[2 * i + 1] : nheight;      // the frame's own result
    const ipk_scaled_frame &f = frames[i];
    if (!srcs[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
    if (f.struct_size != sizeof(ipk_scaled_frame))
      return fail(IPK_ERR_INVALID, "frames[%zu].struct_size is %u, not sizeof(ipk_scaled_frame) = %zu", i, f.struct_size, sizeof(ipk_scaled_frame));
    if (!dims_ok(f.width, f.height)) return fail(IPK_ERR_INVALID, "frames[%zu]: bad dimensions", i);
    if (f.x > f.owidth || f.width > f.owidth - f.x) return fail(IPK_ERR_INVALID, "frames[%zu]: window wider than the source pitch", i);
    ipk::ScaledFrameLaunch &l = fl[i];
    l.src = srcs[i]; l.owidth = f.owidth; l.x = f.x; l.y = f.y; l.width = f.width; l.height = f.height; l.cfa48_dev = nullptr;
    for (int c = 0; c < 3; ++c) { l.black[c] = f.black4[plain ? c : 0]; l.white[c] = f.white4[plain ? c : 0]; }
    if (!plain) {
      char pat[sizeof(f.cfa)]; std::memcpy(pat, f.cfa, sizeof(pat)); pat[sizeof(pat) - 1] = 0;
      ipk::Cfa cfa; DevCfa dev;
      const int rc = get_cfa(pat, cfa, dev);
      if (rc) { const std::string why = g_err; return fail(rc, "frames[%zu]: %s", i, why.c_str()); }
      l.cfa48_dev = dev.cfa48;
    }
    if (!ipk::raw_scaled_demosaic_general(f.width, f.height, nw_i, nh_i, true, plain))
      return fail(IPK_ERR_UNSUPPORTED, "frames[%zu]: %zux%zu -> %zux%zu selects a window-8 kernel, which has no frame-table mode", i, f.width, f.height, nw_i, nh_i);
  }
  const size_t slice = nwidth * nheight * 4;                                 // one size for all: the slices are this far apart
  size_t off = 0;                                                            // sized: where the group's first slice begins
  for (size_t i0 = 0; i0 < n; i0 += ipk::kScaledEachMax) {
    const size_t m = std::min(ipk::kScaledEachMax, n - i0);
    Scratch sc(S(stream));
    void *table = nullptr;
    { const int rc = sc.get(ipk::scaled_each_table_bytes(m), &table); if (rc) return rc; }
    const int lrc = ipk::launch_raw_scaled_demosaic_each(fl.data() + i0, m, src_type == IPK_SRC_U16, plain ? (kind == IPK_PLAIN_MONO ? 1 : 3) : 0, nwidth, nheight,
                                                         dst4 + (sizes ? off : i0 * slice), table, S(stream), sizes ? sizes + 2 * i0 : nullptr);
    if (sizes) for (size_t i = i0; i < i0 + m; ++i) off += sizes[2 * i] * sizes[2 * i + 1] * 4;
    if (lrc == -4) return fail(IPK_ERR_HIP, "scaled_demosaic_batch_each: the table upload or the launch could not be enqueued");
    if (lrc != 0) return fail(IPK_ERR_INVALID, "scaled_demosaic_batch_each: the launcher refused the frames");
    tm.mark(stage);
  }
  return IPK_OK;
}
// ipk_pointwise_chain_out_batch: every frame's parameters through PointwisePrep::prepare (so normalize_wbs, the spline, has_curve and fast_ok are the single
// form's, per frame) before anything is enqueued, then one frame-table launch per 64 frames (launch_chain_batch), its table in the scratch pool.  stage: the
// name marked behind every launch
// orientations (optional, n ipk_orientation values): frame i leaves as OpTransform's image of its result -- its record gathers through frame_gather, the
// permutation folded into the loads -- height wide where the orientation transposes.  Null, or Normal / Unknown throughout: the launches of old.
// stage_oriented (optional): the name behind a launch with at least one oriented frame, where it differs
// sizes (optional, 2n values: width_i, height_i; ipk_pointwise_chain_out_batch_sized): frame i's own size -- width and height are not read, every frame is
// held to the bounds of a call of its own, and each group of 64 is one sized launch.  Equal sizes throughout are the call without them
int chain_out_batch_impl(const float *const *srcs4, size_t width, size_t height, int monochrome, const ipk_chain_params *params, const int *orientations, size_t n,
                         int linear, int out_type, void *const *dsts, void *stream, StageTimer &tm, const char *stage, const char *stage_oriented = nullptr,
                         const size_t *sizes = nullptr) {
  if (out_type < 0 || out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if (sizes && n != 0) {
    if (n > (size_t)1 << 20) return fail(IPK_ERR_INVALID, "batch too large");
    bool equal = true;
    for (size_t i = 0; i < n; ++i) {
      if (!dims_ok(sizes[2 * i], sizes[2 * i + 1])) return fail(IPK_ERR_INVALID, "sizes[%zu]: bad dimensions %zux%zu", i, sizes[2 * i], sizes[2 * i + 1]);
      if (out_type != IPK_OUT_F32 && sizes[2 * i] * sizes[2 * i + 1] < 256)
        return fail(IPK_ERR_UNSUPPORTED, "sizes[%zu]: pointwise_chain_out_batch needs at least 256 pixels per frame for 8- and 16-bit outputs", i);
      equal = equal && sizes[2 * i] == sizes[0] && sizes[2 * i + 1] == sizes[1];
    }
    width = sizes[0]; height = sizes[1];
    if (equal) sizes = nullptr;
  }
  if (!sizes && !dims_ok(width, height)) return fail(IPK_ERR_INVALID, "bad pointwise_chain_out_batch arguments");
  if (n == 0) return IPK_OK;
  if (!srcs4 || !dsts || !params) return fail(IPK_ERR_INVALID, "null argument");
  if (n > (size_t)1 << 20) return fail(IPK_ERR_INVALID, "batch too large");
  const size_t npix = width * height, dalign = out_elem_size(out_type);
  if (!sizes && out_type != IPK_OUT_F32 && npix < 256)
    return fail(IPK_ERR_UNSUPPORTED, "pointwise_chain_out_batch needs at least 256 pixels per frame for 8- and 16-bit outputs");
  std::vector<PointwisePrep> pps(n);
  for (size_t i = 0; i < n; ++i) {
    if (!srcs4[i] || !dsts[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
    if (reinterpret_cast<uintptr_t>(srcs4[i]) % 16 != 0 || reinterpret_cast<uintptr_t>(dsts[i]) % dalign != 0)
      return fail(IPK_ERR_INVALID, "frame %zu: the source needs 16-byte alignment, the destination its element's", i);
    if (params[i].struct_size != sizeof(ipk_chain_params))
      return fail(IPK_ERR_INVALID, "params[%zu].struct_size is %u, not sizeof(ipk_chain_params) = %zu", i, params[i].struct_size, sizeof(ipk_chain_params));
    if (orientations && (orientations[i] < 0 || orientations[i] > 8)) return fail(IPK_ERR_INVALID, "orientations[%zu] is %d, not an ipk_orientation", i, orientations[i]);
    const ipk_chain_params &p = params[i];
    const int rc = pps[i].prepare(monochrome, p.wb_coeffs, p.cam_to_xyz_normalized, p.exposure, p.points, p.npoints, linear);
    if (rc) { const std::string why = g_err; return fail(rc, "params[%zu]: %s", i, why.c_str()); }
    pps[i].f.src = srcs4[i]; pps[i].f.dst = dsts[i]; pps[i].f.out_type = out_type;
  }
  std::vector<ipk::FusedLaunch> fl;
  std::vector<ipk::GatherSource> gs;
  std::vector<size_t> np;
  for (size_t i0 = 0; i0 < n; i0 += ipk::kChainBatchMax) {
    const size_t m = std::min(ipk::kChainBatchMax, n - i0);
    fl.clear(); gs.clear(); np.clear();
    bool oriented = false;
    for (size_t i = 0; i < m; ++i) {
      fl.push_back(pps[i0 + i].f);
      const size_t wi = sizes ? sizes[2 * (i0 + i)] : width, hi = sizes ? sizes[2 * (i0 + i) + 1] : height;
      const int o = orientations ? orientations[i0 + i] : IPK_OR_NORMAL;
      ipk::GatherSource g = {0, 0, 0, 0};                                  // width 0: the flat walk
      if (o != IPK_OR_NORMAL && o != IPK_OR_UNKNOWN) { g = frame_gather(wi, hi, o); oriented = true; }
      gs.push_back(g);
      np.push_back(wi * hi);
    }
    Scratch sc(S(stream));
    void *table = nullptr;
    { const int rc = sc.get(ipk::chain_batch_table_bytes(m), &table); if (rc) return rc; }
    const int lrc = ipk::launch_chain_batch(fl.data(), m, npix, out_type, table, S(stream), oriented ? gs.data() : nullptr, sizes ? np.data() : nullptr);
    if (lrc == -4) return fail(IPK_ERR_HIP, "pointwise_chain_out_batch: the table upload or the launch could not be enqueued");
    if (lrc != 0) return fail(IPK_ERR_UNSUPPORTED, "pointwise_chain_out_batch: frame too small");
    tm.mark(oriented && stage_oriented ? stage_oriented : stage);
  }
  return IPK_OK;
}

// ---- two descriptors compared.  Floats compare by their bits, cfa as the folded string the drivers read, padding never ----
bool same_bits(const float *a, const float *b, size_t n) { return std::memcmp(a, b, n * sizeof(float)) == 0; }
// the five fields OpToLab and OpBaseCurve read: what every run lets differ
bool same_pointwise(const ipk_pipeline_desc &a, const ipk_pipeline_desc &b) {
  return same_bits(a.wb_coeffs, b.wb_coeffs, 4) && same_bits(a.cam_to_xyz_normalized, b.cam_to_xyz_normalized, 12) && same_bits(&a.exposure, &b.exposure, 1) &&
         a.npoints == b.npoints && same_bits(a.points, b.points, 128);
}
// the three OpTransform reads: what IPK_FUSED_BATCH_ORIENTED lets differ inside a run
bool same_orientation(const ipk_pipeline_desc &a, const ipk_pipeline_desc &b) { return a.rotation == b.rotation && a.fliph == b.fliph && a.flipv == b.flipv; }
// the eleven sensor fields: what IPK_FUSED_BATCH_SENSOR lets differ inside a run (cfa_width / cfa_height are folded into cfa)
bool same_sensor(const ipk_pipeline_desc &a, const ipk_pipeline_desc &b) {
  return a.width == b.width && a.height == b.height && std::strcmp(a.cfa, b.cfa) == 0 && a.cfa_width == b.cfa_width && a.cfa_height == b.cfa_height &&
         a.crop_top == b.crop_top && a.crop_right == b.crop_right && a.crop_bottom == b.crop_bottom && a.crop_left == b.crop_left &&
         same_bits(a.blacklevels, b.blacklevels, 4) && same_bits(a.whitelevels, b.whitelevels, 4);
}
// equal in the five, the three and the eleven: same-shaped descriptors that are one descriptor to the uniform batch (ipk_pipeline_run_batch)
bool same_settings(const ipk_pipeline_desc &a, const ipk_pipeline_desc &b) { return same_pointwise(a, b) && same_orientation(a, b) && same_sensor(a, b); }
// Same-shaped: every field equal but the five -- and but the three where oriented_ok, but the eleven where sensor_ok (plan_each says when a pair may).
// a and b are taken and folded; sa / sb are the struct_size values the callers wrote
bool same_shape(const ipk_pipeline_desc &a, uint32_t sa, const ipk_pipeline_desc &b, uint32_t sb, bool oriented_ok, bool sensor_ok) {
  return sa == sb && a.src_type == b.src_type && a.cpp == b.cpp && a.is_cfa == b.is_cfa && (sensor_ok || same_sensor(a, b)) &&
         same_bits(a.rotatecrop, b.rotatecrop, 5) && (oriented_ok || same_orientation(a, b)) && a.maxwidth == b.maxwidth &&
         a.maxheight == b.maxheight && a.linear == b.linear && a.allow_fused == b.allow_fused && a.use_fastpath == b.use_fastpath &&
         a.schedule == b.schedule && a.fuse_rotatecrop == b.fuse_rotatecrop &&
         a.reserved1 == b.reserved1 && a.fuse_scaledown == b.fuse_scaledown;
}

// ---- one descriptor admitted ----
// IPK_FUSED_BATCH_PREVIEWS: a batch of staged frames whose gofloat + demosaic is the one scaling pass (gofloat_demosaic_one_pass) and whose every later op
// is point-wise (OpRotateCrop a no-op; OpTransform too, or a permutation under IPK_FUSED_BATCH_ORIENTED) runs chunk by chunk as one scaling launch group into one RGBE scratch, then the chain over the
// previews lying one after another.  dw * dh >= 256 is the one-pass chain's own floor, kept per frame: the batch uses the kernels a single frame would.
// chunk: frames per scratch (at most 64, at most 256 MiB of RGBE); pass1_batched: pass 1 is the general scaling kernel's batch launch (the scratch slices
// are 16-byte aligned), else one launch per frame of the kernel the frame selects
struct BatchPreviews { size_t chunk; bool pass1_batched; };
bool batches_previews(const ipk_pipeline_desc *d, const Negotiated &n, const Route &rt, size_t frames, BatchPreviews &bp) {
  bp.chunk = 0; bp.pass1_batched = false;
  if (!opted(d, IPK_FUSED_BATCH_PREVIEWS) || frames <= 1 || rt.kind != kStaged || !gofloat_demosaic_one_pass(d, n) || !n.rc.noop() || n.dw * n.dh < 256) return false;
  if (!n.transform_noop) {
    // IPK_FUSED_BATCH_ORIENTED: OpTransform rides in pass 2's loads (chain_out_batch_impl), where its image of the preview is the negotiated result
    bool t, fx, fy; ipk::orientation_to_flips(n.orientation, t, fx, fy);
    if (!opted(d, IPK_FUSED_BATCH_ORIENTED) || (t ? n.dh : n.dw) != n.fw || (t ? n.dw : n.dh) != n.fh) return false;
  }
  // (a descriptor no launch would take -- a preview of 2^24 pixels and more, whose byte count may wrap to 0, or a sensor side of 2^31 and more, which the
  // kernel selection cannot convert -- still gets an answer here: a frame per chunk, no batch launch)
  const size_t cap_px = (size_t)1 << 24;                                    // 256 MiB of RGBE
  bp.chunk = n.dw > cap_px / n.dh ? 1 : std::min<size_t>(64, std::max<size_t>(1, ((size_t)256 << 20) / (n.dw * n.dh * 16)));
  bp.pass1_batched = n.raw && dims_ok(n.r.width, n.r.height) && ipk::raw_scaled_demosaic_general(n.r.width, n.r.height, n.dw, n.dh, true, !n.cfa_branch);
  return true;
}
int take_folded(const ipk_pipeline_desc *d, ipk_pipeline_desc &out) {
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  out = *d;
  return IPK_OK;
}
// What the plan needs to know about one descriptor, derived in one pass (admit) and only read from there on; what a frame does not fill stays zero.
//   fast     the frame takes the raster fast path.  It is never negotiated, and nothing else is filled
//   ng       its negotiation; ng.dw x ng.dh is the demosaic size the frames of a run share
//   rt, bp, batches   its route, and whether it would batch its own previews: batches_previews asked for two frames (the frame count enters that function
//            through frames <= 1 alone, so one answer serves every run longer than one).  Under IPK_FUSED_BATCH_PREVIEWS only: without the bit the
//            answer is no whatever the route, and none is chosen
//   four     under IPK_FUSED_BATCH_SENSOR: the filter of a frame whose pass 1 is the batch launch has a fourth colour
struct Admitted { bool fast, batches, four; Negotiated ng; Route rt; BatchPreviews bp; };
int admit(const ipk_pipeline_desc &d, int out_type, Admitted &a) {
  a.fast = ipk_pipeline_takes_fastpath(&d, out_type) == 1;
  if (a.fast) { if (d.width < 1 || d.height < 1) return fail(IPK_ERR_INVALID, "empty source"); return IPK_OK; }
  { const int rc = negotiate(&d, out_type, a.ng); if (rc) return rc; }
  if (!opted(&d, IPK_FUSED_BATCH_PREVIEWS)) return IPK_OK;
  choose_route(&d, a.ng, out_type, a.rt);
  a.batches = batches_previews(&d, a.ng, a.rt, 2, a.bp);
  if (a.batches && a.bp.pass1_batched && a.ng.cfa_branch && opted(&d, IPK_FUSED_BATCH_SENSOR)) {
    ipk::Cfa cfa; a.four = ipk::Cfa::parse(d.cfa, cfa) && cfa.valid() && !cfa.three_colour();
  }
  return IPK_OK;
}

// ---- n frames, n descriptors (ipk_pipeline_run_batch_each): the plan ----
enum { kEachSingle = 0, kEachUniform = 1, kEachVaried = 2 };
// segs: what is executed, in order.  first, count: the segment's frames (a single segment is one frame); route: what runs them; run_first: the first frame
// of the run of same-shaped descriptors the segment lies in (ipk_pipeline_batch_each_plan reports it).  A varied segment is its whole run: bp chunks it,
// sensor says whether its frames differ in a sensor field (IPK_FUSED_BATCH_SENSOR)
struct EachPlan {
  std::vector<ipk_pipeline_desc> d;                  // taken and folded
  std::vector<Admitted> adm;
  struct Segment { size_t first, count; int route; size_t run_first; BatchPreviews bp; bool sensor; };
  std::vector<Segment> segs;
};
// validates every descriptor as ipk_pipeline_run does (and the curve's point count, as the batch driver does), then cuts the runs
int plan_each(const ipk_pipeline_desc *const *descs, size_t n, int out_type, EachPlan &p) {
  if (out_type < 0 || out_type > 2) return fail(IPK_ERR_INVALID, "bad out_type");
  if (n && !descs) return fail(IPK_ERR_INVALID, "null argument");
  if (n > (size_t)1 << 20) return fail(IPK_ERR_INVALID, "batch too large");
  p.d.resize(n); p.adm.assign(n, Admitted{}); p.segs.clear();
  std::vector<uint32_t> sizes(n);
  for (size_t i = 0; i < n; ++i) {
    if (!descs[i]) return fail(IPK_ERR_INVALID, "null descriptor at index %zu", i);
    sizes[i] = descs[i]->struct_size;
    int rc = take_folded(descs[i], p.d[i]);
    if (!rc) rc = validate_desc(&p.d[i], out_type, kCheckFuse | kCheckCurve);
    if (!rc) rc = admit(p.d[i], out_type, p.adm[i]);
    if (rc) { const std::string why = g_err; return fail(rc, "descriptor %zu: %s", i, why.c_str()); }
  }
  // A frame that would batch its own previews and carries `bit` may differ from its run's first frame in that bit's fields, where the first frame does
  // too and both negotiate one demosaic size (the scaling pass's filter).  IPK_FUSED_BATCH_ORIENTED folds OpTransform into pass 2.  IPK_FUSED_BATCH_SENSOR
  // needs pass 1 to be the general kernel's batch launch for both, and both to agree in whether the filter has a fourth colour (src_type, cpp and is_cfa,
  // hence the kernel's layout and the chain's monochrome flag, count as shape anyway)
  const auto frees = [&](size_t i, int bit) { return p.adm[i].batches && opted(&p.d[i], bit); };
  for (size_t a = 0, b; a < n; a = b) {
    const Admitted &A = p.adm[a];
    for (b = a + 1; b < n; ++b) {
      const Admitted &B = p.adm[b];
      // IPK_FUSED_BATCH_SIZES waives the one demosaic size where pass 1 of both is the general kernel's batch launch: the sized launches take such a chunk
      const bool one_size = (A.ng.dw == B.ng.dw && A.ng.dh == B.ng.dh) ||
                            (frees(a, IPK_FUSED_BATCH_SIZES) && frees(b, IPK_FUSED_BATCH_SIZES) && A.bp.pass1_batched && B.bp.pass1_batched);
      const bool oriented_ok = one_size && frees(a, IPK_FUSED_BATCH_ORIENTED) && frees(b, IPK_FUSED_BATCH_ORIENTED);
      const bool sensor_ok = one_size && frees(a, IPK_FUSED_BATCH_SENSOR) && frees(b, IPK_FUSED_BATCH_SENSOR) && A.bp.pass1_batched && B.bp.pass1_batched &&
                             A.four == B.four;
      // the raster fast path is decided by the five point-wise fields themselves (default_ops_other): a frame that takes it shares no run with one that
      // does not, so every frame of a run is on the route ipk_pipeline_run would choose for it
      if (A.fast != B.fast || !same_shape(p.d[a], sizes[a], p.d[b], sizes[b], oriented_ok, sensor_ok)) break;
    }
    bool all_equal = true;
    for (size_t i = a + 1; i < b; ++i) all_equal = all_equal && same_settings(p.d[a], p.d[i]);
    if (b - a > 1 && !all_equal && A.batches) {
      bool sensor = false;
      for (size_t i = a + 1; i < b; ++i) sensor = sensor || !same_sensor(p.d[a], p.d[i]);
      p.segs.push_back({a, b - a, kEachVaried, a, A.bp, sensor});
    } else {
      for (size_t j = a, k; j < b; j = k) {          // maximal sub-runs of equal descriptors: the uniform batch, which keeps its own routes
        for (k = j + 1; k < b && same_settings(p.d[j], p.d[k]); ++k) {}
        p.segs.push_back({j, k - j, k - j > 1 ? (int)kEachUniform : (int)kEachSingle, a, BatchPreviews{0, false}, false});
      }
    }
  }
  return IPK_OK;
}

// ---- the chunk walk ----
// a frame as the walk sees it: its descriptor and its negotiation
struct FrameRef { const ipk_pipeline_desc *d; const Negotiated *ng; };
// The chunks of n frames, cut greedily in order: a chunk grows while it has fewer than 64 frames and its RGBE previews sum to at most 256 MiB, and a frame
// that alone is larger (or whose byte count would wrap) is a chunk of its own.  For frames of one demosaic size that is batches_previews' chunk,
// min(64, max(1, 256 MiB / slice)), from the first frame on.  Returns the length of the chunk that begins at frame i0
extern "C++" template <typename Frame>
size_t preview_chunk_len(Frame frame, size_t i0, size_t n) {
  const size_t cap_px = (size_t)1 << 24;                                    // 256 MiB of RGBE
  size_t m = 0, px = 0;
  while (i0 + m < n && m < 64) {
    const Negotiated &ng = *frame(i0 + m).ng;
    const size_t own = ng.dh == 0 || ng.dw > cap_px / ng.dh ? cap_px + 1 : ng.dw * ng.dh;
    if (m != 0 && own > cap_px - px) break;
    px += std::min(own, cap_px); ++m;
    if (own > cap_px) break;
  }
  return m;
}
// The chunk walk both preview batches share: frame(i) is frame i of n -- the same pair for every i in a uniform batch (run_batch_previews), the plan's
// records in a varied run, whose frames negotiate one demosaic size unless IPK_FUSED_BATCH_SIZES let them differ.  A chunk (preview_chunk_len) of one frame is
// single(i); a longer one gets its scratch, pass 1 -- the chunk's RGBE previews one after another, frame i0 + i at offs[i] floats -- and then
// pass2(i0, m, rgbe, offs, sized, tm), which enqueues the point-wise work of frames i0 .. i0 + m and marks its stages.  Pass 1 of a chunk whose frames
// differ in a sensor field is ONE frame-table launch (scaled_batch_each_impl: frame
// i's levels, crops and filter from its descriptor, its window from its negotiation), marked "batch-each gofloat+demosaic"; the plan lets them differ
// only where bp.pass1_batched holds for every one.  A chunk whose frames differ in demosaic size (sized) is the same call with every frame's own size: ONE
// sized launch under the same name.  Any other chunk is the uniform launch on the chunk's first descriptor.
// sensor_varies: false where no two of the n frames differ in a sensor field (none is compared then)
extern "C++" template <typename Frame, typename Single, typename Pass2>
int run_preview_chunks(Frame frame, const BatchPreviews &bp, bool sensor_varies, const void *const *srcs, size_t n, void *stream, Single single, Pass2 pass2) {
  std::vector<ipk_scaled_frame> sf;
  std::vector<size_t> offs, sizes;
  for (size_t i0 = 0, m; i0 < n; i0 += m) {
    m = preview_chunk_len(frame, i0, n);
    if (m == 1) { const int rc = single(i0); if (rc < 0) return rc; continue; }
    // The chunk's first frame states what the chunk shares.  In a varied run that is not the run's first frame: without a table the chunk's frames have
    // its sensor fields, and everything else pass 1 reads -- src_type, cpp, is_cfa, the demosaic size -- is equal throughout the chunk
    const FrameRef c = frame(i0);
    const ipk_pipeline_desc *const dc = c.d; const Negotiated &nc = *c.ng;
    const size_t slice = nc.dw * nc.dh * 4;
    offs.assign(m, 0); sizes.assign(2 * m, 0);
    size_t total = 0;
    bool sized = false;
    for (size_t i = 0; i < m; ++i) {
      const Negotiated &ni = *frame(i0 + i).ng;
      offs[i] = total; sizes[2 * i] = ni.dw; sizes[2 * i + 1] = ni.dh; total += ni.dw * ni.dh * 4;
      sized = sized || ni.dw != nc.dw || ni.dh != nc.dh;
    }
    StageTimer tm(S(stream));
    Scratch sc(S(stream));
    void *buf = nullptr;
    int rc = sc.get(total * sizeof(float), &buf); if (rc) return rc;
    float *rgbe = static_cast<float *>(buf);
    bool table = sized;
    if (sensor_varies) for (size_t i = 1; i < m; ++i) table = table || !same_sensor(*dc, *frame(i0 + i).d);
    if (table) {
      if (sized && !bp.pass1_batched) return fail(IPK_ERR_INVALID, "internal: a chunk of differing demosaic sizes outside the general kernel's batch launch");
      sf.assign(m, ipk_scaled_frame{});
      for (size_t i = 0; i < m; ++i) {
        const ipk_pipeline_desc &di = *frame(i0 + i).d; const Negotiated &ni = *frame(i0 + i).ng;
        ipk_scaled_frame &f = sf[i];
        f.struct_size = (uint32_t)sizeof(f);
        f.owidth = di.width; f.x = ni.r.x; f.y = ni.r.y; f.width = ni.r.width; f.height = ni.r.height;
        std::memcpy(f.black4, di.blacklevels, sizeof(f.black4)); std::memcpy(f.white4, di.whitelevels, sizeof(f.white4));
        std::memcpy(f.cfa, di.cfa, sizeof(f.cfa));
      }
      rc = scaled_batch_each_impl(srcs + i0, sf.data(), m, dc->src_type, nc.cfa_branch ? -1 : (dc->cpp == 3 ? IPK_PLAIN_RGB : IPK_PLAIN_MONO), nc.dw, nc.dh, rgbe,
                                  stream, tm, "batch-each gofloat+demosaic", sized ? sizes.data() : nullptr);
      if (rc < 0) return rc;
    } else if (bp.pass1_batched) {
      rc = nc.cfa_branch ? raw_scaled_demosaic_batch_impl(srcs + i0, m, dc->src_type, dc->width, nc.r.x, nc.r.y, nc.r.width, nc.r.height, dc->blacklevels[0],
                                                          dc->whitelevels[0], dc->cfa, nc.dw, nc.dh, rgbe, stream)
                         : plain_scale_down_batch_impl(srcs + i0, m, dc->src_type, dc->cpp == 3 ? IPK_PLAIN_RGB : IPK_PLAIN_MONO, dc->width, nc.r.x, nc.r.y, nc.r.width,
                                                       nc.r.height, dc->blacklevels, dc->whitelevels, nc.dw, nc.dh, rgbe, stream);
      if (rc < 0) return rc;
    } else {
      for (size_t i = 0; i < m; ++i) { rc = launch_gofloat_demosaic(dc, nc, srcs[i0 + i], nullptr, rgbe + i * slice, stream); if (rc < 0) return rc; }
    }
    if (!table) tm.mark("batch gofloat+demosaic");
    rc = pass2(i0, m, rgbe, offs.data(), sized, tm); if (rc < 0) return rc;
  }
  return IPK_OK;
}
void chain_params_of(const ipk_pipeline_desc &d, ipk_chain_params &c) {
  c.struct_size = (uint32_t)sizeof(c);
  std::memcpy(c.wb_coeffs, d.wb_coeffs, sizeof(c.wb_coeffs));
  std::memcpy(c.cam_to_xyz_normalized, d.cam_to_xyz_normalized, sizeof(c.cam_to_xyz_normalized));
  c.exposure = d.exposure; c.npoints = d.npoints; std::memcpy(c.points, d.points, sizeof(c.points));
}
// Pass 2 of a chunk as ONE frame-table launch (chain_out_batch_impl): frame i's record from its own descriptor and negotiation -- its point-wise
// parameters, its composed orientation -- its source the scratch's slice i, its destination dsts[i] wherever it lies (a destination is not a slice of one
// flat image here, so frames following each other in memory gain nothing).  The stage is prefix + "to_lab+basecurve+from_lab+gamma", "+transform" behind a
// launch with at least one oriented frame, "+quantise" for the 8- and 16-bit outputs.  sized: the chunk's frames differ in demosaic size, and the launch
// is the sized one on every frame's own
extern "C++" template <typename Frame>
int chain_pass2_each(Frame frame, size_t i0, size_t m, const float *rgbe, const size_t *offs, bool sized, int out_type, void *const *dsts, int *used_fused,
                     void *stream, StageTimer &tm, const char *prefix) {
  std::vector<ipk_chain_params> cp(m); std::vector<const float *> s4(m); std::vector<int> ori(m); std::vector<size_t> sizes(sized ? 2 * m : 0);
  for (size_t i = 0; i < m; ++i) {
    const FrameRef f = frame(i0 + i);
    chain_params_of(*f.d, cp[i]); s4[i] = rgbe + offs[i]; ori[i] = f.ng->orientation;
    if (sized) { sizes[2 * i] = f.ng->dw; sizes[2 * i + 1] = f.ng->dh; }
  }
  if (used_fused) *used_fused = 0;
  const std::string chain = std::string(prefix) + "to_lab+basecurve+from_lab+gamma", quantise = out_type == IPK_OUT_F32 ? "" : "+quantise";
  const std::string stage = chain + quantise, stage_oriented = chain + "+transform" + quantise;
  const FrameRef c = frame(i0);
  return chain_out_batch_impl(s4.data(), c.ng->dw, c.ng->dh, one_pass_monochrome(c.d, *c.ng), cp.data(), ori.data(), m, c.ng->linear, out_type, dsts + i0, stream,
                              tm, stage.c_str(), stage_oriented.c_str(), sized ? sizes.data() : nullptr);
}

// ---- the drivers ----
// n frames of one descriptor as batched previews.  Pass 2 is the chain over the previews lying one after another -- or, where OpTransform is not a no-op
// (IPK_FUSED_BATCH_ORIENTED), the frame-table launch, every record with the descriptor's orientation
int run_batch_previews(const ipk_pipeline_desc *d, const Negotiated &ng, const BatchPreviews &bp, const void *const *srcs, void *const *dsts, size_t n,
                       int out_type, int *used_fused, void *stream) {
  const size_t out_bytes = ng.dw * ng.dh * 3 * out_elem_size(out_type);
  const bool f32_out = out_type == IPK_OUT_F32;
  const int monochrome = one_pass_monochrome(d, ng);
  const auto frame = [&](size_t) { return FrameRef{d, &ng}; };
  return run_preview_chunks(frame, bp, false, srcs, n, stream,
    [&](size_t i) { return ipk_pipeline_run(d, srcs[i], dsts[i], out_type, used_fused, stream); },
    [&](size_t i0, size_t m, float *rgbe, const size_t *offs, bool sized, StageTimer &tm) {
      if (!ng.transform_noop) return chain_pass2_each(frame, i0, m, rgbe, offs, sized, out_type, dsts, used_fused, stream, tm, "batch ");
      // the chain once per maximal run of frames whose destinations follow each other in memory
      for (size_t j = 0; j < m;) {
        size_t k = j + 1;
        while (k < m && dsts[i0 + k] == static_cast<char *>(dsts[i0 + k - 1]) + out_bytes) ++k;
        const int rc = ipk_pointwise_chain_out(rgbe + offs[j], ng.dw, (k - j) * ng.dh, monochrome, d->wb_coeffs, d->cam_to_xyz_normalized, d->exposure, d->points,
                                               d->npoints, ng.linear, out_type, dsts[i0 + j], stream);
        if (rc < 0) return rc;
        tm.mark(f32_out ? "batch to_lab+basecurve+from_lab+gamma" : "batch to_lab+basecurve+from_lab+gamma+quantise");
        j = k;
      }
      return (int)IPK_OK;
    });
}
// a varied segment of the plan: the chunks and pass 1 of run_batch_previews, frame i with descriptor i's own sensor settings where they differ, then the
// frame-table launch per chunk, frame i's record from descriptor i
int run_batch_each_varied(const EachPlan &p, const EachPlan::Segment &s, const void *const *srcs, void *const *dsts, int out_type, int *used_fused, void *stream) {
  const size_t a = s.first;
  const auto frame = [&](size_t i) { return FrameRef{&p.d[a + i], &p.adm[a + i].ng}; };
  return run_preview_chunks(frame, s.bp, s.sensor, srcs + a, s.count, stream,
    [&](size_t i) { return ipk_pipeline_run(&p.d[a + i], srcs[a + i], dsts[a + i], out_type, used_fused, stream); },
    [&](size_t i0, size_t m, float *rgbe, const size_t *offs, bool sized, StageTimer &tm) {
      return chain_pass2_each(frame, i0, m, rgbe, offs, sized, out_type, dsts + a, used_fused, stream, tm, "batch-each ");
    });
}
}  // namespace

// IPK_FUSED_BATCH_PREVIEWS: does a batch of n frames of this descriptor run as batched previews (1) or frame by frame (0)?  The driver's own test (no GPU)
int ipk_pipeline_batches_previews(const ipk_pipeline_desc *d, int out_type, size_t n, size_t *chunk, int *pass1_batched) {
  if (chunk) *chunk = 0;
  if (pass1_batched) *pass1_batched = 0;
  RouteReport r; const int rc = report_route(d, out_type, r); if (rc) return rc;
  BatchPreviews bp;
  if (!batches_previews(&r.d, r.n, r.rt, n, bp)) return 0;
  if (chunk) *chunk = bp.chunk;
  if (pass1_batched) *pass1_batched = bp.pass1_batched ? 1 : 0;
  return 1;
}

int ipk_pipeline_run_batch(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n, int out_type, int *used_fused, void *stream) {
  REQUIRE_INIT();
  if (!d || (n && (!srcs || !dsts))) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  { const int rc = validate_desc(d, out_type, kCheckCurve); if (rc) return rc; }      // (the fuse flags: where a frame is run, so an empty batch passes)
  for (size_t i = 0; i < n; ++i) if (!srcs[i] || !dsts[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
  if (used_fused) *used_fused = 0;
  if (n == 0) return IPK_OK;
  Negotiated ng; Route rt; BatchPreviews bp;
  if (n > 1 && negotiate(d, out_type, ng) == IPK_OK) {
    choose_route(d, ng, out_type, rt);
    // Is Pipeline::run for each frame exactly the fused raw launch with nothing behind it (OpTransform a no-op)?  Then the batch is one
    // persistent launch per 64 frames (ipk_raw_to_srgb_batch).
    if (ng.transform_noop && rt.kind == kFusedRaw) {
      const int rc = ipk_raw_to_srgb_batch(&rt.fp, srcs, dsts, n, stream);
      if (rc == IPK_OK && used_fused) *used_fused = 1;
      return rc;
    }
    // Or a batch of previews under IPK_FUSED_BATCH_PREVIEWS: a scaling launch group and the chain per chunk (run_batch_previews)
    if (batches_previews(d, ng, rt, n, bp)) return run_batch_previews(d, ng, bp, srcs, dsts, n, out_type, used_fused, stream);
  }
  for (size_t i = 0; i < n; ++i) { const int rc = ipk_pipeline_run(d, srcs[i], dsts[i], out_type, used_fused, stream); if (rc < 0) return rc; }
  return IPK_OK;
}

// ipk_pointwise_chain_out for n same-sized buffers, each with its own parameters and destination: one frame-table launch per 64 frames
int ipk_pointwise_chain_out_batch(const float *const *srcs4, size_t width, size_t height, int monochrome, const void *params, size_t n, int linear,
                                  int out_type, void *const *dsts, void *stream) {
  REQUIRE_INIT();
  StageTimer tm(S(stream));
  return chain_out_batch_impl(srcs4, width, height, monochrome, static_cast<const ipk_chain_params *>(params), nullptr, n, linear, out_type, dsts, stream, tm,
                              "pointwise_chain_out_batch");
}
// the same with an orientation per frame: OpTransform's permutation folded into each frame's loads
int ipk_pointwise_chain_out_batch_oriented(const float *const *srcs4, size_t width, size_t height, int monochrome, const void *params, const int *orientations,
                                           size_t n, int linear, int out_type, void *const *dsts, void *stream) {
  REQUIRE_INIT();
  StageTimer tm(S(stream));
  return chain_out_batch_impl(srcs4, width, height, monochrome, static_cast<const ipk_chain_params *>(params), orientations, n, linear, out_type, dsts, stream,
                              tm, "pointwise_chain_out_batch_oriented");
}
// ipk_raw_scaled_demosaic / ipk_plain_scale_down for n frames with their own windows, levels and filters into one result size: one frame-table launch per 64
int ipk_scaled_demosaic_batch_each(const void *const *srcs, const void *frames, size_t n, int src_type, int kind, size_t nwidth, size_t nheight, float *dst4,
                                   void *stream) {
  REQUIRE_INIT();
  StageTimer tm(S(stream));
  return scaled_batch_each_impl(srcs, static_cast<const ipk_scaled_frame *>(frames), n, src_type, kind, nwidth, nheight, dst4, stream, tm,
                                "scaled_demosaic_batch_each");
}
// the same with a result size per frame, the slices packed one behind another: one sized frame-table launch per 64
int ipk_scaled_demosaic_batch_sized(const void *const *srcs, const void *frames, const size_t *sizes, size_t n, int src_type, int kind, float *dst4, void *stream) {
  REQUIRE_INIT();
  if (n && !sizes) return fail(IPK_ERR_INVALID, "null argument");
  StageTimer tm(S(stream));
  return scaled_batch_each_impl(srcs, static_cast<const ipk_scaled_frame *>(frames), n, src_type, kind, 0, 0, dst4, stream, tm, "scaled_demosaic_batch_sized", sizes);
}
// ipk_pointwise_chain_out_batch_oriented with a size per frame: one sized frame-table launch per 64
int ipk_pointwise_chain_out_batch_sized(const float *const *srcs4, const size_t *sizes, int monochrome, const void *params, const int *orientations, size_t n,
                                        int linear, int out_type, void *const *dsts, void *stream) {
  REQUIRE_INIT();
  if (n && !sizes) return fail(IPK_ERR_INVALID, "null argument");
  StageTimer tm(S(stream));
  return chain_out_batch_impl(srcs4, 1, 1, monochrome, static_cast<const ipk_chain_params *>(params), orientations, n, linear, out_type, dsts, stream, tm,
                              "pointwise_chain_out_batch_sized", nullptr, sizes);
}
// The plan of ipk_pipeline_run_batch_each, for callers and CPU tests (no GPU)
int ipk_pipeline_batch_each_plan(const ipk_pipeline_desc *const *descs, size_t n, int out_type, int *route, size_t *run_first) {
  EachPlan p;
  { const int rc = plan_each(descs, n, out_type, p); if (rc) return rc; }
  for (const EachPlan::Segment &s : p.segs)
    for (size_t i = s.first; i < s.first + s.count; ++i) { if (route) route[i] = s.route; if (run_first) run_first[i] = s.run_first; }
  return IPK_OK;
}
// The chunks that plan is executed in (no GPU): chunk_first[i] is the first frame of the chunk frame i runs in.  A varied run's chunks are the walk's own
// (preview_chunk_len); a run of equal descriptors that batches its previews is cut by the same rule from its first frame on; every other frame -- a
// single one, or one of a uniform batch on another route, which has no scratch to share -- is its own
int ipk_pipeline_batch_each_chunks(const ipk_pipeline_desc *const *descs, size_t n, int out_type, size_t *chunk_first) {
  EachPlan p;
  { const int rc = plan_each(descs, n, out_type, p); if (rc) return rc; }
  if (!chunk_first) return IPK_OK;
  for (const EachPlan::Segment &s : p.segs) {
    const size_t a = s.first;
    const auto frame = [&](size_t i) { return FrameRef{&p.d[a + i], &p.adm[a + i].ng}; };
    const bool chunked = s.route == kEachVaried || (s.route == kEachUniform && p.adm[a].batches);
    for (size_t i = 0, m; i < s.count; i += m) {
      m = chunked ? preview_chunk_len(frame, i, s.count) : 1;
      for (size_t j = i; j < i + m; ++j) chunk_first[a + j] = a + i;
    }
  }
  return IPK_OK;
}
// n frames, n descriptors: the plan's runs in order -- a varied run as one scaling launch group and one frame-table launch per chunk, runs of equal
// descriptors through ipk_pipeline_run_batch, every other frame through ipk_pipeline_run
int ipk_pipeline_run_batch_each(const ipk_pipeline_desc *const *descs, const void *const *srcs, void *const *dsts, size_t n, int out_type, int *used_fused,
                                void *stream) {
  REQUIRE_INIT();
  if (n && (!descs || !srcs || !dsts)) return fail(IPK_ERR_INVALID, "null argument");
  EachPlan p;
  { const int rc = plan_each(descs, n, out_type, p); if (rc) return rc; }
  for (size_t i = 0; i < n; ++i) {
    if (!srcs[i] || !dsts[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
    // a curve the launches would refuse, before anything is enqueued (every route but the fast path builds it)
    const ipk_pipeline_desc &d = p.d[i];
    if (!curve_is_noop(d.exposure, d.npoints) && !p.adm[i].fast) {
      ipk::Spline sp;
      const int rc = build_curve(d.exposure, d.points, d.npoints, sp);
      if (rc) { const std::string why = g_err; return fail(rc, "descriptor %zu: %s", i, why.c_str()); }
    }
  }
  if (used_fused) *used_fused = 0;
  for (const EachPlan::Segment &s : p.segs) {
    const size_t a = s.first;
    const int rc = s.route == kEachVaried ? run_batch_each_varied(p, s, srcs, dsts, out_type, used_fused, stream)
                 : s.route == kEachUniform ? ipk_pipeline_run_batch(&p.d[a], srcs + a, dsts + a, s.count, out_type, used_fused, stream)
                                           : ipk_pipeline_run(&p.d[a], srcs[a], dsts[a], out_type, used_fused, stream);
    if (rc < 0) return rc;
  }
  return IPK_OK;
}

// ---- the same over the process's device set: frame i -> set member i mod N, from ONE host thread (launches are asynchronous) -------------
namespace {
void devset_snapshot(std::vector<Context *> &v) {
  std::lock_guard<std::mutex> lk(g_reg_mu);
  v = g_devset;
  if (v.empty() && cx().ready) v.push_back(&cx());      // no set: the current context alone
}
struct CurrentGuard {                                    // puts the calling thread's current context (and its device) back
  Context *saved = t_current;
  ~CurrentGuard() { t_current = saved; if (cx().ready) (void)hipSetDevice(cx().device); }
};
}  // namespace

int ipk_pipeline_run_batch_multi(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n, int out_type, int *used_fused) {
  REQUIRE_INIT();
  if (!d || (n && (!srcs || !dsts))) return fail(IPK_ERR_INVALID, "null argument");
  std::vector<Context *> set; devset_snapshot(set);
  const size_t nd = set.size();
  CurrentGuard guard;
  int fused_all = 1;
  for (size_t k = 0; k < nd; ++k) {
    std::vector<const void *> s; std::vector<void *> o;
    for (size_t i = k; i < n; i += nd) { s.push_back(srcs[i]); o.push_back(dsts[i]); }
    if (s.empty()) continue;
    if (!set[k]->ready) return fail(IPK_ERR_NOT_INIT, "device-set member %zu has been destroyed", k);
    t_current = set[k];
    { int rc = bind_device(set[k]->device); if (rc) return rc; }
    if (!set[k]->multi_stream) HIPCHK(hipStreamCreateWithFlags(&set[k]->multi_stream, hipStreamNonBlocking));
    int fused = 0;
    const int rc = ipk_pipeline_run_batch(d, s.data(), o.data(), s.size(), out_type, &fused, set[k]->multi_stream);
    if (rc < 0) return rc;
    fused_all = fused_all && fused;
  }
  if (used_fused) *used_fused = n ? fused_all : 0;
  return IPK_OK;
}
int ipk_devices_sync(void) {
  REQUIRE_INIT();
  std::vector<Context *> set; devset_snapshot(set);
  CurrentGuard guard;
  int rc = IPK_OK;
  for (Context *c : set) {
    if (!c->ready || !c->multi_stream) continue;
    if (hipSetDevice(c->device) != hipSuccess || hipStreamSynchronize(c->multi_stream) != hipSuccess) {
      rc = fail(IPK_ERR_HIP, "synchronising device %d failed: %s", c->device, hipGetErrorString(hipGetLastError()));
    }
  }
  return rc;
}

// Host buffers in, host buffers out, over the device set: one host thread per member runs ipk_host_pipeline_run_batch on the frames dealt
// to it (its own three streams and two device slots), so every GPU uploads, computes and downloads at the same time.  Synchronous at return,
// like every ipk_host_* entry point.  The buffers should come from ipk_host_alloc (page-locked, visible to every device).
int ipk_host_pipeline_run_batch_multi(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n, int out_type, int *used_fused) {
  REQUIRE_INIT();
  if (!d || (n && (!srcs || !dsts))) return fail(IPK_ERR_INVALID, "null argument");
  std::vector<Context *> set; devset_snapshot(set);
  const size_t nd = set.size();
  if (nd == 1) {
    CurrentGuard guard;
    t_current = set[0];
    return ipk_host_pipeline_run_batch(d, srcs, dsts, n, out_type, used_fused);
  }
  struct Share { int rc = IPK_OK; int fused = 0; size_t frames = 0; std::string err; };
  std::vector<Share> res(nd);
  auto work = [&](size_t k) {
    std::vector<const void *> s; std::vector<void *> o;
    for (size_t i = k; i < n; i += nd) { s.push_back(srcs[i]); o.push_back(dsts[i]); }
    res[k].frames = s.size();
    if (s.empty()) return;
    t_current = set[k];                                  // this worker thread's current context
    res[k].rc = ipk_host_pipeline_run_batch(d, s.data(), o.data(), s.size(), out_type, &res[k].fused);
    if (res[k].rc < 0) res[k].err = g_err;               // ipk_last_error() is per thread: hand the text to the caller's
    t_current = nullptr;
  };
  {
    std::vector<std::thread> th;
    for (size_t k = 1; k < nd; ++k) th.emplace_back(work, k);
    { CurrentGuard guard; work(0); }                     // the caller's thread takes the first share
    for (auto &t : th) t.join();
  }
  int fused_all = 1;
  for (size_t k = 0; k < nd; ++k) {
    if (res[k].rc < 0) return fail(res[k].rc, "device-set member %zu (device %d): %s", k, set[k]->device, res[k].err.c_str());
    if (res[k].frames) fused_all = fused_all && res[k].fused;
  }
  if (used_fused) *used_fused = n ? fused_all : 0;
  return IPK_OK;
}

int ipk_host_pipeline_run_batch(const ipk_pipeline_desc *d, const void *const *srcs, void *const *dsts, size_t n, int out_type, int *used_fused) {
  REQUIRE_INIT();
  if (!d || (n && (!srcs || !dsts))) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  for (size_t i = 0; i < n; ++i) if (!srcs[i] || !dsts[i]) return fail(IPK_ERR_INVALID, "null frame pointer at index %zu", i);
  size_t dw, dh, fw, fh;
  HOST_TRY(ipk_pipeline_sizes(d, &dw, &dh, &fw, &fh));
  if (n == 0) return IPK_OK;
  const bool raw = d->src_type == IPK_SRC_U16 || d->src_type == IPK_SRC_F32;
  const size_t in_bytes = d->width * d->height * (raw ? (size_t)d->cpp : 3) * src_elem_size(d->src_type);
  const size_t out_bytes = fw * fh * 3 * out_elem_size(out_type);
  HostLanes &L = cx().lanes;
  std::lock_guard<std::mutex> lk(L.mu);
  HIPCHK(hipDeviceSynchronize());   // the lanes are non-blocking streams: nothing enqueued earlier (scratch-pool users on other streams) may still be running
  HOST_TRY(L.ensure(in_bytes, out_bytes));
  // one frame's enqueues; any failure stops the batch, and the lanes are drained in every case before the return (the
  // caller's buffers must not be touched afterwards)
  auto enqueue = [&](size_t i) -> int {
    const int s = (int)(i % HostLanes::kSlots);
    const bool reused = i >= (size_t)HostLanes::kSlots;
    // upload i into slot s once the kernels of frame i - kSlots have consumed it
    if (reused) HIPCHK(hipStreamWaitEvent(L.up, L.run_done[s], 0));
    HIPCHK(hipMemcpyAsync(L.in[s], srcs[i], in_bytes, hipMemcpyHostToDevice, L.up));
    HIPCHK(hipEventRecord(L.up_done[s], L.up));
    // compute once the upload has landed and the slot's previous output has left
    HIPCHK(hipStreamWaitEvent(L.run, L.up_done[s], 0));
    if (reused) HIPCHK(hipStreamWaitEvent(L.run, L.down_done[s], 0));
    const int rc = ipk_pipeline_run(d, L.in[s], L.out[s], out_type, used_fused, L.run);
    if (rc < 0) return rc;
    HIPCHK(hipEventRecord(L.run_done[s], L.run));
    // download
    HIPCHK(hipStreamWaitEvent(L.down, L.run_done[s], 0));
    HIPCHK(hipMemcpyAsync(dsts[i], L.out[s], out_bytes, hipMemcpyDeviceToHost, L.down));
    HIPCHK(hipEventRecord(L.down_done[s], L.down));
    return IPK_OK;
  };
  int rc = IPK_OK;
  for (size_t i = 0; i < n && rc == IPK_OK; ++i) rc = enqueue(i);
  const hipError_t e0 = hipStreamSynchronize(L.up), e1 = hipStreamSynchronize(L.run), e2 = hipStreamSynchronize(L.down);
  if (rc < 0) return rc;
  HIPCHK(e0); HIPCHK(e1); HIPCHK(e2);
  return IPK_OK;
}

// A region from a HOST frame into a HOST buffer: on the windowed route only the sensor window ipk_pipeline_region reports crosses the link (one pitched
// copy into its place in a frame-sized device buffer -- the launch reads nothing else), and only the region comes back.
int ipk_host_pipeline_run_region(const ipk_pipeline_desc *d, const void *src, size_t x, size_t y, size_t w, size_t h, void *dst, int out_type,
                                 int *windowed) {
  REQUIRE_INIT();
  if (!d || !src || !dst) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_pipeline_desc, d)
  size_t sx, sy, sw, sh;
  const int route = ipk_pipeline_region(d, out_type, x, y, w, h, &sx, &sy, &sw, &sh);
  if (route < 0) return route;
  const bool raw = d->src_type == IPK_SRC_U16 || d->src_type == IPK_SRC_F32;
  const size_t px = (raw ? (size_t)d->cpp : 3) * src_elem_size(d->src_type), pitch = d->width * px;
  const size_t in_bytes = d->height * pitch, out_bytes = w * h * 3 * out_elem_size(out_type);
  HostLanes &L = cx().lanes;
  std::lock_guard<std::mutex> lk(L.mu);
  HIPCHK(hipDeviceSynchronize());   // as ipk_host_pipeline_run_batch: nothing enqueued earlier may still use the lanes
  HOST_TRY(L.ensure(in_bytes, out_bytes));
  int rc = IPK_OK;
  if (route == 1) {
    // the window's rows, widened to 64-byte boundaries inside the frame's rows (at most 126 bytes more per row): pitched copies whose rows start at an
    // odd u16 sample or hold an odd number of them measured 4-5 times slower than widened ones (profiles/r12_region_windows.txt)
    const size_t b0 = sx * px / 64 * 64, b1 = std::min(pitch, (sx * px + sw * px + 63) / 64 * 64);
    const size_t off = sy * pitch + b0;
    if (sw != 0 && sh != 0 &&                                  // an empty window (no pixel of the region has a tap): the launch reads nothing
        hipMemcpy2DAsync(static_cast<char *>(L.in[0]) + off, pitch, static_cast<const char *>(src) + off, pitch, b1 - b0, sh, hipMemcpyHostToDevice, L.run) != hipSuccess)
      rc = fail(IPK_ERR_HIP, "window upload failed");
  } else if (hipMemcpyAsync(L.in[0], src, in_bytes, hipMemcpyHostToDevice, L.run) != hipSuccess) {
    rc = fail(IPK_ERR_HIP, "frame upload failed");
  }
  if (rc == IPK_OK) rc = ipk_pipeline_run_region(d, L.in[0], x, y, w, h, L.out[0], out_type, windowed, L.run);
  if (rc >= 0 && hipMemcpyAsync(dst, L.out[0], out_bytes, hipMemcpyDeviceToHost, L.run) != hipSuccess) rc = fail(IPK_ERR_HIP, "region download failed");
  const hipError_t e = hipStreamSynchronize(L.run);   // the caller's buffers are not touched after the return
  if (rc < 0) return rc;
  HIPCHK(e);
  return IPK_OK;
}

int ipk_host_gofloat_cfa_u16(const uint16_t *src, size_t owidth, size_t oheight, size_t x, size_t y, size_t width, size_t height,
                             float black0, float white0, float *dst) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src, owidth * oheight * 2)); HOST_TRY(b.alloc(width * height * 4));
  HOST_TRY(ipk_gofloat_cfa_u16(static_cast<const uint16_t *>(a.p), owidth, x, y, width, height, black0, white0, static_cast<float *>(b.p), nullptr));
  return b.download(dst, width * height * 4);
}
int ipk_host_gofloat_cfa_f32(const float *src, size_t owidth, size_t oheight, size_t x, size_t y, size_t width, size_t height,
                             float black0, float white0, float *dst) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src, owidth * oheight * 4)); HOST_TRY(b.alloc(width * height * 4));
  HOST_TRY(ipk_gofloat_cfa_f32(static_cast<const float *>(a.p), owidth, x, y, width, height, black0, white0, static_cast<float *>(b.p), nullptr));
  return b.download(dst, width * height * 4);
}
int ipk_host_demosaic_full(const float *src, size_t width, size_t height, const char *cfa, float *dst4) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src, width * height * 4)); HOST_TRY(b.alloc(width * height * 16));
  HOST_TRY(ipk_demosaic_full(static_cast<const float *>(a.p), width, height, cfa, static_cast<float *>(b.p), nullptr));
  return b.download(dst4, width * height * 16);
}
int ipk_host_transform_buffer_f32(const float *src, size_t width, size_t height, int64_t tlx, int64_t tly, int64_t trx, int64_t try_,
                                  int64_t blx, int64_t bly, size_t nwidth, size_t nheight, size_t components, const char *cfa, float *dst) {
  REQUIRE_INIT(); DevBuf a, b;
  const size_t in_comps = cfa ? 1 : components;
  HOST_TRY(a.upload(src, width * height * in_comps * 4)); HOST_TRY(b.alloc(nwidth * nheight * components * 4));
  HOST_TRY(ipk_transform_buffer_f32(static_cast<const float *>(a.p), width, height, tlx, tly, trx, try_, blx, bly, nwidth, nheight, components, cfa,
                                    static_cast<float *>(b.p), nullptr));
  return b.download(dst, nwidth * nheight * components * 4);
}
int ipk_host_tolab(const float *src4, size_t width, size_t height, int monochrome, const float *wb, const float *cm, float *dst3) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src4, width * height * 16)); HOST_TRY(b.alloc(width * height * 12));
  HOST_TRY(ipk_tolab(static_cast<const float *>(a.p), width, height, monochrome, wb, cm, static_cast<float *>(b.p), nullptr));
  return b.download(dst3, width * height * 12);
}
int ipk_host_basecurve(const float *src3, size_t width, size_t height, float exposure, const float *points, int npoints, float *dst3) {
  REQUIRE_INIT();
  if (curve_is_noop(exposure, npoints)) return IPK_NOOP;
  DevBuf a, b;
  HOST_TRY(a.upload(src3, width * height * 12)); HOST_TRY(b.alloc(width * height * 12));
  HOST_TRY(ipk_basecurve(static_cast<const float *>(a.p), width, height, exposure, points, npoints, static_cast<float *>(b.p), nullptr));
  return b.download(dst3, width * height * 12);
}
int ipk_host_fromlab(const float *src3, size_t width, size_t height, float *dst3) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src3, width * height * 12)); HOST_TRY(b.alloc(width * height * 12));
  HOST_TRY(ipk_fromlab(static_cast<const float *>(a.p), width, height, static_cast<float *>(b.p), nullptr));
  return b.download(dst3, width * height * 12);
}
int ipk_host_gamma(const float *src, size_t width, size_t height, size_t colors, int linear, float *dst) {
  REQUIRE_INIT();
  if (linear) return IPK_NOOP;
  DevBuf a, b;
  const size_t bytes = width * height * colors * 4;
  HOST_TRY(a.upload(src, bytes)); HOST_TRY(b.alloc(bytes));
  HOST_TRY(ipk_gamma(static_cast<const float *>(a.p), width, height, colors, 0, static_cast<float *>(b.p), nullptr));
  return b.download(dst, bytes);
}
int ipk_host_rotate_buffer(const float *src3, size_t width, size_t height, int orientation, float *dst3, size_t *ow, size_t *oh) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src3, width * height * 12)); HOST_TRY(b.alloc(width * height * 12));
  HOST_TRY(ipk_rotate_buffer(static_cast<const float *>(a.p), width, height, orientation, static_cast<float *>(b.p), ow, oh, nullptr));
  return b.download(dst3, width * height * 12);
}
int ipk_host_output8bit(const float *src, size_t n, uint8_t *dst) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src, n * 4)); HOST_TRY(b.alloc(n));
  HOST_TRY(ipk_output8bit(static_cast<const float *>(a.p), n, static_cast<uint8_t *>(b.p), nullptr));
  return b.download(dst, n);
}
int ipk_host_output16bit(const float *src, size_t n, uint16_t *dst) {
  REQUIRE_INIT(); DevBuf a, b;
  HOST_TRY(a.upload(src, n * 4)); HOST_TRY(b.alloc(n * 2));
  HOST_TRY(ipk_output16bit(static_cast<const float *>(a.p), n, static_cast<uint16_t *>(b.p), nullptr));
  return b.download(dst, n * 2);
}
int ipk_host_raw_to_srgb(const ipk_fused_params *p, const void *src, void *dst) {
  REQUIRE_INIT();
  if (!p || !src || !dst) return fail(IPK_ERR_INVALID, "null argument");
  IPK_FOLD_CFA(ipk_fused_params, p)
  const size_t esz = p->src_type == IPK_SRC_U16 ? 2 : 4;
  const bool band = p->band_out_rows != 0;
  const size_t src_rows = band ? p->band_src_rows : p->y + p->height;
  const size_t out_rows = band ? p->band_out_rows : p->height;
  DevBuf a, b;
  HOST_TRY(a.upload(src, src_rows * p->owidth * esz));
  HOST_TRY(b.alloc(out_rows * p->width * 3 * out_elem_size(p->out_type)));
  HOST_TRY(ipk_raw_to_srgb(p, a.p, b.p, nullptr));
  return b.download(dst, out_rows * p->width * 3 * out_elem_size(p->out_type));
}

}  // extern "C"
