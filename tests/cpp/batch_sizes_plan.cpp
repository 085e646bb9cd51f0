// The plan and the chunk report of ipk_pipeline_run_batch_each under IPK_FUSED_BATCH_SIZES (ipk_pipeline_batch_each_plan, ipk_pipeline_batch_each_chunks:
// no GPU) as a stand-alone program, built with and without AddressSanitizer + UBSan by tests/cpp/Makefile's rules for such programs
// (make build/san/asan/batch_sizes_plan build/san/plain/batch_sizes_plan; tests/test_batch_sizes_sanitizers.py asks for both, runs both and compares the
// digests).  Two parts:
//   contract -- batches of the route tests' thumbnail under maxwidth 19 (Normal 19x14, Rotate90 25x19) and of a 200x160 body (19x15), alternating, with
//               every mask of bits 0, 8, 9, 10 and 11 the route tests name; the outputs are fresh heap blocks of exactly n entries;
//   hostile  -- seeded batches whose descriptors carry huge sizes, crops and size limits under the five bits: previews whose byte counts wrap, sums that
//               cross the 256 MiB cut.  Any status is acceptable there; a sanitizer report, a crash, a hang or an allocation by frame size is not.
// It never initialises the library and ends by checking that.      batch_sizes_plan [hostile-batches]      (default 20000)
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>
#include "san_common.hpp"

using san::Exact; using san::Rng; using san::Section;

namespace {
enum { ON = 1, BATCH = 256, ORIENTED = 512, SENSOR = 1024, SIZES = 2048 };

ipk_pipeline_desc thumb(int mask, int rotation) {
  ipk_pipeline_desc d = IPK_PIPELINE_DESC_INIT;
  d.src_type = 0; d.width = 211; d.height = 157; d.cpp = 1; d.is_cfa = 1;
  std::strncpy(d.cfa, "RGGB", sizeof(d.cfa) - 1);
  d.crop_top = 2; d.crop_right = 3; d.crop_bottom = 4; d.crop_left = 5;
  for (int i = 0; i < 4; ++i) { d.blacklevels[i] = 512.0f; d.whitelevels[i] = 16383.0f; }
  d.wb_coeffs[0] = 2.0f; d.wb_coeffs[1] = 1.0f; d.wb_coeffs[2] = 1.5f; d.wb_coeffs[3] = NAN;
  const float m[12] = {0.4124564f, 0.3575761f, 0.1804375f, 0.0f, 0.2126729f, 0.7151522f, 0.0721750f, 0.0f, 0.0193339f, 0.1191920f, 0.9503041f, 0.0f};
  std::memcpy(d.cam_to_xyz_normalized, m, sizeof m);
  d.npoints = 1; d.points[0] = 0.5f; d.points[1] = 0.6f;
  d.maxwidth = 19; d.allow_fused = mask; d.rotation = rotation;
  return d;
}
ipk_pipeline_desc body(int mask, int rotation) {
  ipk_pipeline_desc d = thumb(mask, rotation);
  d.width = 200; d.height = 160; d.crop_top = d.crop_right = d.crop_bottom = d.crop_left = 0;
  return d;
}
// one call of each report: outputs of exactly n entries; the chunk report must agree with the plan it cuts
void plan_call(Section &S, const std::vector<ipk_pipeline_desc> &ds, int out_type) {
  const size_t n = ds.size();
  Exact<const ipk_pipeline_desc *> ptrs(n);
  for (size_t i = 0; i < n; ++i) ptrs[i] = &ds[i];
  Exact<int> route(n, 0x77); Exact<size_t> first(n, 0x77), chunk(n, 0x77);
  const int rc = S.rc(ipk_pipeline_batch_each_plan(ptrs, n, out_type, route, first));
  const int rc2 = S.rc(ipk_pipeline_batch_each_chunks(ptrs, n, out_type, chunk));
  SAN_EXPECT(rc == rc2, "plan %d, chunks %d", rc, rc2);
  if (rc == IPK_OK && rc2 == IPK_OK)
    for (size_t i = 0; i < n; ++i) {
      S.i32(route[i]); S.u64(first[i]); S.u64(chunk[i]);
      SAN_EXPECT(route[i] >= 0 && route[i] <= 2 && first[i] <= i && chunk[i] <= i && chunk[i] >= first[i] && i - chunk[i] < 64 &&
                 (route[i] != 0 || chunk[i] == i) && (i == 0 || chunk[i] == i || chunk[i] == chunk[i - 1]),
                 "frame %zu: route %d, run_first %zu, chunk_first %zu", i, route[i], first[i], chunk[i]);
    }
  ++S.cases;
}
void sec_contract() {
  Section S("sizes_contract");
  const int masks[8] = {ON | BATCH | ORIENTED | SIZES, ON | BATCH | SENSOR | SIZES, ON | BATCH | ORIENTED | SENSOR | SIZES, ON | BATCH | SIZES,
                        ON | BATCH | ORIENTED, ON | ORIENTED | SIZES, BATCH | SENSOR | SIZES, SIZES};
  for (int mask : masks)
    for (int out_type = 0; out_type < 3; ++out_type)
      for (int n : {0, 1, 2, 5, 67, 130})
        for (int kind = 0; kind < 3; ++kind) {
          std::vector<ipk_pipeline_desc> ds;
          for (int i = 0; i < n; ++i) {
            ds.push_back(kind == 0 ? thumb(mask, i % 2) : kind == 1 ? (i % 2 ? body(mask, 0) : thumb(mask, 0)) : (i % 3 ? body(mask, i % 4) : thumb(mask, i % 4)));
            ds.back().wb_coeffs[0] = 2.0f + 0.03125f * (float)(i % 7);
          }
          plan_call(S, ds, out_type);
        }
  // the header's example: Normal and Rotate90 alternating are one varied run and one chunk
  for (int n : {2, 3, 5}) {
    std::vector<ipk_pipeline_desc> ds;
    for (int i = 0; i < n; ++i) ds.push_back(thumb(ON | BATCH | ORIENTED | SIZES, i % 2));
    Exact<const ipk_pipeline_desc *> p(n);
    for (int i = 0; i < n; ++i) p[i] = &ds[i];
    Exact<int> route(n, 0x77); Exact<size_t> first(n, 0x77), chunk(n, 0x77);
    const int rc = ipk_pipeline_batch_each_plan(p, n, 1, route, first), rc2 = ipk_pipeline_batch_each_chunks(p, n, 1, chunk);
    bool ok = rc == IPK_OK && rc2 == IPK_OK;
    for (int i = 0; ok && i < n; ++i) ok = route[i] == 2 && first[i] == 0 && chunk[i] == 0;
    SAN_EXPECT(ok, "n = %d: rc %d %d", n, rc, rc2);
  }
  S.done();
}
void sec_hostile(uint64_t count) {
  Section S("sizes_hostile");
  Rng r(0x512E5);
  const size_t huge[8] = {0, 1, 7, 60000, (size_t)1 << 24, (size_t)1 << 31, ((size_t)1 << 63) + 5, ~(size_t)0};
  const size_t limits[8] = {0, 1, 19, 3000, 4096, (size_t)1 << 24, (size_t)1 << 36, ~(size_t)0};
  for (uint64_t c = 0; c < count; ++c) {
    const int n = r.range(1, 9);
    const int mask = r.below(8) ? (ON | BATCH | SIZES | (r.below(2) ? ORIENTED : 0) | (r.below(2) ? SENSOR : 0)) : (int)r.next();
    // one hostile shape per batch, so that its frames stay same-shaped and the chunk cut sees them
    ipk_pipeline_desc base = thumb(mask, 0);
    for (int m = r.range(0, 3); m > 0; --m)
      switch (r.below(5)) {
        case 0: base.width = huge[r.below(8)]; base.crop_left = base.crop_right = 0; break;
        case 1: base.height = huge[r.below(8)]; base.crop_top = base.crop_bottom = 0; break;
        case 2: base.maxwidth = limits[r.below(8)]; break;
        case 3: base.maxheight = limits[r.below(8)]; break;
        default: base.width = 60000; base.height = 40000; base.maxwidth = 3000; break;
      }
    std::vector<ipk_pipeline_desc> ds;
    for (int i = 0; i < n; ++i) {
      ipk_pipeline_desc d = base;
      d.rotation = r.range(0, 3); d.fliph = r.below(2);
      if (r.below(4) == 0) { d.width = huge[r.below(8)]; d.height = huge[r.below(8)]; }
      if (r.below(16) == 0) d.allow_fused = (int)r.next();
      d.wb_coeffs[0] = 2.0f + 0.03125f * (float)i;
      ds.push_back(d);
    }
    plan_call(S, ds, r.range(0, 2));
  }
  S.done();
}
}  // namespace

int main(int argc, char **argv) {
  const uint64_t n = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 20000;
  sec_contract(); sec_hostile(n);
  if (ipk_is_initialized() != 0) { std::fprintf(stderr, "CONTRACT the library was initialised\n"); return 1; }
  if (san::g_failures) { std::fprintf(stderr, "%d contract failures\n", san::g_failures); return 1; }
  std::printf("BATCH_SIZES_PLAN_OK\n");
  return 0;
}
