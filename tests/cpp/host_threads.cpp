// Eight threads on the entry points that need no device and may be called from any thread (every entry point works on the calling
// thread's current context, ipk_last_error() is thread-local) -- the ThreadSanitizer target of `make san`, also built with AddressSanitizer + UBSan
// and plain.  The threads
//   - ask for the size / route / hash reports of DIFFERING descriptors and shift CFA patterns, all at once (the thread_local memos, the shared
//     host tables and their locks are under them);
//   - provoke failures whose message names the thread, and must read their OWN message back from ipk_last_error();
//   - walk the context calls' failure paths: ipk_ctx_current() without a context, ipk_ctx_make_current(NULL) and of a handle that is no context;
//   - share ONE ipk_cache through put / contains / stats / get (documented as safe in include/imagepipe_amd.h); what a thread sees there depends on
//     the interleaving, so only invariants are checked and only the final state enters the digest.
// No device is opened: the program ends by checking ipk_is_initialized() == 0.     host_threads [iterations per thread]   (default 400)
#include <atomic>
#include <string>
#include <thread>
#include <vector>
#include <cmath>
#include "san_common.hpp"

using san::Exact; using san::Rng; using san::Section;

namespace {
constexpr int kThreads = 8;
const char *const XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG";
const char *const CFAS[6] = {"RGGB", "GBRG", XT, "RGBE", "8x2:RGBGRBGGGBGRGRBG", ""};
const float RC[4][5] = {{0, 0, 0, 0, 0}, {0.1f, 0.05f, 0.2f, 0, 0}, {0.1f, 0, 0, 0, 0.2f}, {0.07f, 0.11f, 0.05f, 0.02f, 0.04f}};
std::atomic<int> g_bad{0};
#define T_EXPECT(cond, ...) do { if (!(cond)) { std::fprintf(stderr, "CONTRACT thread %d %s:%d: %s: ", tid, __FILE__, __LINE__, #cond); std::fprintf(stderr, __VA_ARGS__); std::fprintf(stderr, "\n"); ++g_bad; } } while (0)

ipk_pipeline_desc desc_for(Rng &r) {
  ipk_pipeline_desc d = IPK_PIPELINE_DESC_INIT;
  const char *cfa = CFAS[r.below(6)];
  d.src_type = (int)r.below(2); d.width = 40 + r.below(300); d.height = 40 + r.below(200); d.cpp = 1; d.is_cfa = cfa[0] ? 1 : 0;
  std::strcpy(d.cfa, cfa);
  d.crop_top = r.below(6); d.crop_right = r.below(6); d.crop_bottom = r.below(6); d.crop_left = r.below(6);
  for (int i = 0; i < 4; ++i) { d.blacklevels[i] = 512.0f; d.whitelevels[i] = 16383.0f + (float)r.below(4); }
  d.wb_coeffs[0] = 2.0f; d.wb_coeffs[1] = 1.0f; d.wb_coeffs[2] = 1.5f; d.wb_coeffs[3] = NAN;
  ipk_const_matrix(2, d.cam_to_xyz_normalized);
  std::memcpy(d.rotatecrop, RC[r.below(4)], sizeof d.rotatecrop);
  d.npoints = (int)r.below(3); for (int i = 0; i < 2 * d.npoints; ++i) d.points[i] = 0.2f + 0.3f * (float)(i / 2) + 0.1f * r.unit();
  d.rotation = (int)r.below(4); d.fliph = (int)r.below(2);
  d.maxwidth = r.below(3) ? 0 : 20 + r.below(200);
  d.allow_fused = (int)r.below(8); d.fuse_rotatecrop = (int)r.below(2); d.fuse_scaledown = (int)r.below(2);
  return d;
}

struct PerThread { Section reports{"threads_reports"}, errors{"threads_errors"}, cache{"threads_cache"}; };

void worker(int tid, int iters, ipk_cache *shared, PerThread &out) {
  Rng r(0x7EAD0000ull + (uint64_t)tid);
  uint8_t key[32];
  for (int it = 0; it < iters; ++it) {
    // reports on this thread's own descriptor
    { Section &S = out.reports;
      ipk_pipeline_desc d = desc_for(r);
      const int out_type = (int)r.below(3);
      size_t s[4] = {0, 0, 0, 0}, o[4] = {0, 0, 0, 0};
      const int rc = S.rc(ipk_pipeline_sizes(&d, &s[0], &s[1], &s[2], &s[3])); S.bytes(s, sizeof s);
      S.rc(ipk_pipeline_takes_fastpath(&d, out_type)); S.rc(ipk_pipeline_fuses_rotatecrop(&d, out_type));
      S.rc(ipk_pipeline_fuses_scaledown(&d, out_type)); S.rc(ipk_pipeline_fuses_four_colour(&d, out_type));
      uint8_t h[256];
      if (S.rc(ipk_pipeline_hashes(&d, out_type, (uint64_t)tid, h)) == IPK_OK) S.bytes(h, sizeof h);
      if (rc == IPK_OK && s[2] && s[3]) { S.rc(ipk_pipeline_region(&d, out_type, 0, 0, s[2], s[3], &o[0], &o[1], &o[2], &o[3])); S.bytes(o, sizeof o); }
      const std::string pat = CFAS[r.below(5)];
      Exact<char> shifted(pat.size() + 1);
      T_EXPECT(S.rc(ipk_cfa_shift(pat.c_str(), r.range(-50, 50), r.range(-50, 50), shifted)) == IPK_OK, "%s", ipk_last_error());
      S.str(shifted);
      ++S.cases; }
    // a failure whose message names this thread; other threads fail in between
    { Section &S = out.errors;
      const int n_devices = 1000 + tid, index = n_devices + it;
      T_EXPECT(S.rc(ipk_deal_frames(5, n_devices, index, nullptr, nullptr, nullptr)) == IPK_ERR_INVALID, "accepted");
      std::this_thread::yield();
      char want[64]; std::snprintf(want, sizeof want, "bad device index %d of %d", index, n_devices);
      T_EXPECT(std::strcmp(ipk_last_error(), want) == 0, "read '%s', expected '%s'", ipk_last_error(), want);
      // the context calls without a context
      T_EXPECT(ipk_ctx_current() == nullptr, "a context exists");
      T_EXPECT(S.rc(ipk_ctx_make_current(nullptr)) == IPK_OK, "%s", ipk_last_error());
      alignas(16) static char not_a_context[64];
      T_EXPECT(S.rc(ipk_ctx_make_current(reinterpret_cast<ipk_ctx *>(not_a_context))) == IPK_ERR_INVALID, "a stray handle became current");
      T_EXPECT(ipk_ctx_device(nullptr) == -1 && ipk_device_ctx(tid) == nullptr && ipk_device_set_size() == 0, "a device set exists");
      ++S.cases; }
    // the shared cache
    { Section &S = out.cache;
      Rng k(0xCAC4Eull + r.below(64)); for (int j = 0; j < 4; ++j) { const uint64_t v = k.next(); std::memcpy(key + 8 * j, &v, 8); }
      T_EXPECT(ipk_selftest_cache_put(shared, key, 100) == IPK_OK, "%s", ipk_last_error());
      const int has = ipk_cache_contains(shared, key);
      T_EXPECT(has == 0 || has == 1, "contains -> %d", has);
      size_t bytes = 0, entries = 0; uint64_t hits = 0, misses = 0, ev = 0;
      T_EXPECT(ipk_cache_stats(shared, &bytes, &entries, &hits, &misses, &ev) == IPK_OK && bytes <= 1000 && bytes == entries * 100, "%zu bytes in %zu entries", bytes, entries);
      const float *data = nullptr; size_t w, h, c; int mono;
      const int g = ipk_cache_get(shared, key, &data, &w, &h, &c, &mono);
      T_EXPECT(g == IPK_OK || g == IPK_NOOP, "get -> %d", g);
      ++S.cases; }
  }
}
}  // namespace

int main(int argc, char **argv) {
  const int iters = argc > 1 ? std::atoi(argv[1]) : 400;
  ipk_cache *shared = nullptr;
  if (ipk_cache_new(1000, &shared) != IPK_OK) return 3;
  std::vector<PerThread> per((size_t)kThreads);
  std::vector<std::thread> th;
  for (int t = 0; t < kThreads; ++t) th.emplace_back(worker, t, iters, shared, std::ref(per[(size_t)t]));
  for (auto &t : th) t.join();
  Section reports("threads_reports"), errors("threads_errors"), cache("threads_cache");
  for (const PerThread &p : per) {
    reports.u64(p.reports.h); reports.cases += p.reports.cases; errors.u64(p.errors.h); errors.cases += p.errors.cases; cache.cases += p.cache.cases;
  }
  // the cache's final state does not depend on the interleaving: every put was 100 bytes into a budget of 1000 and there were more than ten
  size_t bytes = 0, entries = 0; uint64_t hits = 0, misses = 0, ev = 0;
  cache.rc(ipk_cache_stats(shared, &bytes, &entries, &hits, &misses, &ev));
  cache.u64(bytes); cache.u64(entries); cache.u64(hits + misses);
  if (kThreads * iters > 10 && (bytes != 1000 || entries != 10 || hits + misses != (uint64_t)kThreads * (uint64_t)iters)) {
    std::fprintf(stderr, "CONTRACT the shared cache ends with %zu bytes, %zu entries, %llu gets\n", bytes, entries, (unsigned long long)(hits + misses)); ++g_bad;
  }
  ipk_cache_free(shared);
  reports.done(); errors.done(); cache.done();
  if (ipk_is_initialized() != 0) { std::fprintf(stderr, "CONTRACT the library was initialised\n"); return 1; }
  if (g_bad.load()) { std::fprintf(stderr, "%d contract failures\n", g_bad.load()); return 1; }
  std::printf("HOST_THREADS_OK\n");
  return 0;
}
