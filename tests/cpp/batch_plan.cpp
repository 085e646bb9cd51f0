// The plan of ipk_pipeline_run_batch_each (ipk_pipeline_batch_each_plan: no GPU) as a stand-alone program, built with and without AddressSanitizer +
// UBSan by tests/cpp/Makefile's rules for such programs (make build/san/asan/batch_plan build/san/plain/batch_plan; tests/test_batch_sensor_sanitizers.py
// asks for both, runs both and compares the digests).  Two parts:
//   contract -- batches of the route tests' thumbnail (211x157 RGGB, crops 2 3 4 5, maxwidth 23) whose frames differ in the sensor fields that
//               IPK_FUSED_BATCH_SENSOR lets vary, in orientation and in colour, with every mask of bits 0, 8, 9 and 10; the outputs are fresh heap blocks
//               of exactly n entries and every descriptor is a heap block of exactly its struct_size;
//   hostile  -- seeded batches whose descriptors carry huge sizes and crops, NaN / inf levels, unterminated filters, contradicting cfa_width /
//               cfa_height and struct_size values of older and newer layouts.  Any status is acceptable there; a sanitizer report, a crash or a hang
//               is not.
// It never initialises the library and ends by checking that.      batch_plan [hostile-batches]      (default 20000)
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <vector>
#include "san_common.hpp"

using san::Exact; using san::Rng; using san::Section;

namespace {
const char *XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG";
enum { ON = 1, BATCH = 256, ORIENTED = 512, SENSOR = 1024 };

ipk_pipeline_desc thumb(int mask) {
  ipk_pipeline_desc d = IPK_PIPELINE_DESC_INIT;
  d.src_type = 0; d.width = 211; d.height = 157; d.cpp = 1; d.is_cfa = 1;
  std::strncpy(d.cfa, "RGGB", sizeof(d.cfa) - 1);
  d.crop_top = 2; d.crop_right = 3; d.crop_bottom = 4; d.crop_left = 5;
  for (int i = 0; i < 4; ++i) { d.blacklevels[i] = 512.0f; d.whitelevels[i] = 16383.0f; }
  d.wb_coeffs[0] = 2.0f; d.wb_coeffs[1] = 1.0f; d.wb_coeffs[2] = 1.5f; d.wb_coeffs[3] = NAN;
  const float m[12] = {0.4124564f, 0.3575761f, 0.1804375f, 0.0f, 0.2126729f, 0.7151522f, 0.0721750f, 0.0f, 0.0193339f, 0.1191920f, 0.9503041f, 0.0f};
  std::memcpy(d.cam_to_xyz_normalized, m, sizeof m);
  d.npoints = 1; d.points[0] = 0.5f; d.points[1] = 0.6f;
  d.maxwidth = 23; d.allow_fused = mask;
  return d;
}
// frame k's variation of the thumbnail: what the route tests vary
void vary(ipk_pipeline_desc &d, int k) {
  switch (k % 12) {
    case 0: break;
    case 1: d.blacklevels[0] = 513.0f; break;
    case 2: for (int i = 0; i < 4; ++i) d.whitelevels[i] = 16000.0f; break;
    case 3: d.crop_top = 1; break;
    case 4: d.crop_right = 4; d.crop_left = 4; std::strncpy(d.cfa, "GRBG", sizeof(d.cfa) - 1); break;
    case 5: d.width = 216; d.height = 162; d.crop_top = d.crop_right = d.crop_bottom = d.crop_left = 0; std::strncpy(d.cfa, XT, sizeof(d.cfa) - 1); break;
    case 6: d.width = 230; d.height = 170; d.crop_top = d.crop_right = d.crop_bottom = d.crop_left = 0; break;
    case 7: d.width = 204; d.height = 150; d.crop_top = d.crop_right = d.crop_bottom = d.crop_left = 0; break;     // 23 x 16: cuts
    case 8: d.maxwidth = 60; break;                                                                                // a window-8 kernel: cuts
    case 9: std::strncpy(d.cfa, "RGBE", sizeof(d.cfa) - 1); break;                                                 // a fourth colour: cuts
    case 10: d.cfa_width = 2; d.cfa_height = 2; std::strncpy(d.cfa, "BGGR", sizeof(d.cfa) - 1); break;
    default: d.wb_coeffs[0] = 2.25f; d.exposure = 0.5f; break;
  }
}
// one call: descriptors as exact heap objects of their own struct_size, outputs of exactly n entries
void plan_call(Section &S, const std::vector<ipk_pipeline_desc> &ds, int out_type) {
  const size_t n = ds.size();
  std::vector<Exact<unsigned char> *> blocks;
  Exact<const ipk_pipeline_desc *> ptrs(n);
  for (size_t i = 0; i < n; ++i) {
    const size_t have = std::min<size_t>(std::max<size_t>(ds[i].struct_size, sizeof(uint32_t)), sizeof(ipk_pipeline_desc));
    blocks.push_back(new Exact<unsigned char>(have));
    std::memcpy(blocks.back()->p, &ds[i], have);
    ptrs[i] = reinterpret_cast<const ipk_pipeline_desc *>(blocks.back()->p);
  }
  Exact<int> route(n, 0x77); Exact<size_t> first(n, 0x77);
  if (S.rc(ipk_pipeline_batch_each_plan(ptrs, n, out_type, route, first)) == IPK_OK)
    for (size_t i = 0; i < n; ++i) { S.i32(route[i]); S.u64(first[i]); SAN_EXPECT(route[i] >= 0 && route[i] <= 2 && first[i] <= i, "frame %zu: route %d, run_first %zu", i, route[i], first[i]); }
  ++S.cases;
  for (auto *b : blocks) delete b;
}
void sec_contract() {
  Section S("plan_contract");
  const int masks[7] = {ON | BATCH | SENSOR, ON | BATCH | SENSOR | ORIENTED, ON | BATCH, ON | SENSOR, BATCH | SENSOR, SENSOR, 0};
  for (int mask : masks)
    for (int out_type = 0; out_type < 3; ++out_type)
      for (int n : {0, 1, 2, 5, 12, 65})
        for (int stride : {1, 5, 7}) {
          std::vector<ipk_pipeline_desc> ds;
          for (int i = 0; i < n; ++i) {
            ds.push_back(thumb(mask));
            vary(ds.back(), i * stride);
            if (mask & ORIENTED) { ds.back().maxheight = 23; ds.back().rotation = i % 4; ds.back().fliph = (i / 4) % 2; }
          }
          plan_call(S, ds, out_type);
        }
  // the header's example: each sensor field alone keeps one varied run under the three bits
  for (int k = 1; k <= 6; ++k) {
    std::vector<ipk_pipeline_desc> ds(3, thumb(ON | BATCH | SENSOR));
    vary(ds[1], k);
    Exact<int> route(3, 0x77); Exact<size_t> first(3, 0x77);
    const ipk_pipeline_desc *p[3] = {&ds[0], &ds[1], &ds[2]};
    const int rc = ipk_pipeline_batch_each_plan(p, 3, 1, route, first);
    SAN_EXPECT(rc == IPK_OK && route[0] == 2 && route[1] == 2 && route[2] == 2 && first[1] == 0 && first[2] == 0, "variation %d: rc %d, routes %d %d %d", k, rc, route[0], route[1], route[2]);
  }
  S.done();
}
void sec_hostile(uint64_t count) {
  Section S("plan_hostile");
  Rng r(0x5E2502);
  const float odd[8] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1e-42f, 3.0e38f, -512.0f};
  const size_t huge[6] = {0, 1, 7, (size_t)1 << 31, ((size_t)1 << 63) + 5, ~(size_t)0};
  for (uint64_t c = 0; c < count; ++c) {
    const int n = r.range(1, 6);
    std::vector<ipk_pipeline_desc> ds;
    for (int i = 0; i < n; ++i) {
      ipk_pipeline_desc d = thumb(r.below(4) ? (ON | BATCH | SENSOR | (r.below(2) ? ORIENTED : 0)) : (int)r.next());
      vary(d, (int)r.below(12));
      for (int m = r.range(0, 3); m > 0; --m)
        switch (r.below(10)) {
          case 0: d.width = huge[r.below(6)]; break;
          case 1: d.height = huge[r.below(6)]; break;
          case 2: { size_t *const crops[4] = {&d.crop_top, &d.crop_right, &d.crop_bottom, &d.crop_left}; *crops[r.below(4)] = r.below(2) ? huge[r.below(6)] : r.below(300); break; }
          case 3: d.blacklevels[r.below(4)] = odd[r.below(8)]; break;
          case 4: d.whitelevels[r.below(4)] = odd[r.below(8)]; break;
          case 5: for (size_t j = 0; j < sizeof(d.cfa); ++j) d.cfa[j] = "RGBEX:x3"[r.below(8)]; break;          // no terminator
          case 6: d.cfa_width = r.range(-2, 50); d.cfa_height = r.range(-2, 50); break;
          case 7: d.struct_size = r.below(2) ? (uint32_t)r.below(sizeof(d) + 16) : (uint32_t)offsetof(ipk_pipeline_desc, schedule); break;
          case 8: d.maxwidth = huge[r.below(6)]; d.maxheight = r.below(2) ? 0 : huge[r.below(6)]; break;
          default: d.cpp = r.range(-1, 4); d.is_cfa = r.range(-1, 2); d.src_type = r.range(-1, 4); break;
        }
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
  std::printf("BATCH_PLAN_OK\n");
  return 0;
}
