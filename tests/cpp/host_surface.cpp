// The no-GPU surface of include/imagepipe_amd.h as a stand-alone program, built with and without AddressSanitizer + UBSan by `make san`
// (tests/test_host_sanitizers.py runs both and compares the digests).  Two parts:
//   contract -- valid inputs; every output buffer is a fresh heap block of EXACTLY the size the header documents, so a byte too many is reported;
//   hostile  -- seeded descriptors and arguments with NaN / inf / denormal / huge floats, size_t up to 2^64-1, negative and oversized counts, an
//               unterminated cfa[160], unknown enum values and struct_size values of older and newer layouts.  Any status is acceptable there; a
//               sanitizer report, a crash or a hang is not.
// It never initialises the library (no ipk_init, ipk_ctx_create, ipk_init_devices, no device entry point) and ends by checking that.
//   host_surface [hostile-descriptors [hostile-argument-sets [trace]]]       (defaults 200000 200000)
//
// What the hostile generator does NOT produce, each next to the header sentence that makes it invalid to pass (there is no other filtering):
//   - null descriptors, null output pointers and null strings where the header documents a buffer ("out4 = x, y, width, height", "bands[nranks]",
//     "out256", "char *out >= strlen(pattern) + 1 bytes"): a documented buffer is one the caller has.  Where the header says a pointer MAY be NULL
//     (ipk_deal_frames' outputs, ipk_cache_stats' outputs) NULL is passed.
//   - a `pts` array shorter than npts pairs: "pts = npts (x,y) pairs; arrays sized >= npts+2" (ipk_spline_new).  The arrays are exactly that size;
//     for npts < 0 they are empty.
//   - a `bands` array shorter than nranks: "bands[nranks]" (ipk_band_plan, ipk_band_plan_scaled).  nranks is drawn from [-3, 256] and the array has
//     exactly max(nranks, 0) entries.
//   - a descriptor object shorter than its own struct_size: "the leading struct_size says how many bytes of it the caller's object really has".  The
//     object is a heap block of exactly min(struct_size, sizeof) bytes (at least the struct_size field itself), so a read past it is reported.
//   - a pattern string without a terminator for ipk_cfa_shift ("Pattern strings").  Inside a descriptor cfa[160] MAY be unterminated, and is.
#include <cfloat>
#include <climits>
#include <cmath>
#include <string>
#include <vector>
#include "san_common.hpp"

using san::Exact; using san::Rng; using san::Section;

namespace {
const char *const XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG";
std::string w12() {                                        // the 12x12 filter of tests/test_rotatecrop_route.py
  const std::string x = XT;
  auto s = [&](int a) { return x.substr((size_t)a, 6); };
  std::string a = s(0) + s(18) + s(6) + s(24) + s(12) + s(30), b = s(18) + s(0) + s(24) + s(6) + s(30) + s(12);
  std::string w = a + a + b + b;
  return (w + w).substr(0, 144);
}
const int DIV48[10] = {1, 2, 3, 4, 6, 8, 12, 16, 24, 48};

// ---------------------------------------------------------------------------------------------------------------------------------
// ipk_cfa_shift
// ---------------------------------------------------------------------------------------------------------------------------------
std::string stated(int w, int h, const char *wfmt = "%d", const char *hfmt = "%d") {
  char pre[32], a[8], b[8];
  std::snprintf(a, sizeof a, wfmt, w); std::snprintf(b, sizeof b, hfmt, h);
  std::snprintf(pre, sizeof pre, "%sx%s:", a, b);
  std::string s = pre;
  static const char L[] = "RGBEMY";
  for (int i = 0; i < w * h; ++i) s.push_back(L[(i * 7 + (i / w) * 3 + w + h) % 6]);
  return s;
}
std::vector<std::string> shift_patterns() {
  std::vector<std::string> p = {"", "RGGB", "GBRG", "GRBG", "BGGR", "RGBE", XT, w12()};   // the empty pattern (no filter) first: one byte of output
  for (int w : DIV48) for (int h : DIV48) p.push_back(stated(w, h));
  p.push_back("2x2:RGGB"); p.push_back(std::string("6x6:") + XT); p.push_back("12x12:" + w12());          // a stated shape that is also an inferable one
  p.push_back(stated(2, 8, "%02d", "%02d")); p.push_back(stated(8, 2, "%02d", "%d")); p.push_back("02x02:RGGB");   // leading zeros
  return p;
}
int shift_exact(Section &S, const std::string &pat, int x, int y, std::string &got) {
  Exact<char> out(pat.size() + 1);                         // "at most strlen(pattern) characters"
  const int rc = S.rc(ipk_cfa_shift(pat.c_str(), x, y, out));
  ++S.cases;
  if (rc == IPK_OK) {
    const void *nul = std::memchr(out.p, 0, out.n);
    SAN_EXPECT(nul != nullptr, "'%s' shifted by (%d, %d) is not terminated within strlen + 1 bytes", pat.c_str(), x, y);
    got.assign(out.p, nul ? (size_t)(static_cast<const char *>(nul) - out.p) : out.n);
    S.bytes(got.c_str(), got.size() + 1);
  } else {
    got.clear();
    for (size_t i = 0; i < out.n; ++i) SAN_EXPECT((unsigned char)out.p[i] == 0x55, "a refused pattern '%s' wrote its output", pat.c_str());
  }
  return rc;
}
const int NEG[8][2] = {{-1, 0}, {0, -1}, {-1, -1}, {-5, -7}, {-48, -48}, {-49, 3}, {INT_MIN, INT_MAX}, {-2147483647, -96}};
int mod48(int v) { const long long m = (long long)v % 48; return (int)(m < 0 ? m + 48 : m); }
void sec_cfa_shift() {
  Section S("cfa_shift");
  std::string got;
  for (const std::string &pat : shift_patterns()) {
    std::vector<std::string> grid(48 * 48);
    for (int y = 0; y < 48; ++y)
      for (int x = 0; x < 48; ++x) {
        SAN_EXPECT(shift_exact(S, pat, x, y, got) == IPK_OK, "'%s' refused: %s", pat.c_str(), ipk_last_error());
        SAN_EXPECT(got.size() <= pat.size(), "'%s' -> '%s' is longer than the pattern", pat.c_str(), got.c_str());
        if (pat.empty()) SAN_EXPECT(got.empty(), "the empty pattern shifted to '%s'", got.c_str());
        grid[(size_t)y * 48 + x] = got;
      }
    // the identity comes back in canonical notation, and shifting it again by nothing changes nothing
    SAN_EXPECT(ipk_cfa_shift(grid[0].c_str(), 0, 0, Exact<char>(grid[0].size() + 1)) == IPK_OK, "the result '%s' is not a pattern", grid[0].c_str());
    // negative shifts count modulo the 48 x 48 tiling
    for (const auto &n : NEG) {
      SAN_EXPECT(shift_exact(S, pat, n[0], n[1], got) == IPK_OK, "'%s' by (%d, %d) refused", pat.c_str(), n[0], n[1]);
      SAN_EXPECT(got == grid[(size_t)mod48(n[1]) * 48 + mod48(n[0])], "'%s' by (%d, %d) is '%s', not the shift by (%d, %d)", pat.c_str(), n[0], n[1],
                 got.c_str(), mod48(n[0]), mod48(n[1]));
    }
  }
  S.done();
  Section R("cfa_shift_refused");
  const char *bad[] = {"RGXB", "RGGBGRBGGBRGBGGR", "5x2:RGBGRGBGRG", "2x8:RGGB", "x8:RGGBGRBGGBRGBGGR", "2x:RGGB", "2x8RGGB", "0x4:", "2x8:RGBGRBGGGBGRGRBX",
                       "R", "2x2:", ":", "002x2:RGGB", "2x2:RGGB:", "96x1:R"};
  for (const char *b : bad) SAN_EXPECT(shift_exact(R, b, 1, 1, got) < 0, "'%s' was accepted", b);
  R.done();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// curves, tables
// ---------------------------------------------------------------------------------------------------------------------------------
void spline_call(Section &S, const float *pts, int npts, size_t cap) {
  Exact<float> px(cap), py(cap), c1(cap), c2(cap), c3(cap);
  const int k = S.rc(ipk_spline_new(pts, npts, px, py, c1, c2, c3));
  ++S.cases;
  if (k >= 2) {
    SAN_EXPECT((size_t)k <= cap, "%d knots from %d points", k, npts);
    S.f32s(px.p, (size_t)k); S.f32s(py.p, (size_t)k); S.f32s(c1.p, (size_t)k); S.f32s(c2.p, (size_t)(k - 1)); S.f32s(c3.p, (size_t)(k - 1));
  }
}
void sec_spline() {
  Section S("spline_new");
  Rng r(0x5911E);
  for (int npts = 0; npts <= 64; ++npts)
    for (int variant = 0; variant < 3; ++variant) {
      Exact<float> pts((size_t)npts * 2);
      for (int i = 0; i < npts; ++i) {
        float x = ((float)i + 0.25f + 0.5f * r.unit()) / (float)npts, y = r.unit();
        if (variant == 1) { if (i == 0) x = y = 0.0f; if (i == npts - 1 && npts > 1) x = y = 1.0f; }     // the end knots are the caller's own
        if (variant == 2) x = r.unit();                                                                   // unsorted, repeated abscissae
        pts[(size_t)i * 2] = x; pts[(size_t)i * 2 + 1] = y;
      }
      spline_call(S, pts, npts, (size_t)npts + 2);
    }
  S.done();
}
void sec_tables() {
  Section S("tables");
  for (int which = -1; which <= 3; ++which) {
    Exact<float> t(8193);
    if (S.rc(ipk_lut_table(which, t)) == IPK_OK) S.bytes(t.p, t.size_bytes());
    ++S.cases;
  }
  for (int which = 0; which <= 4; ++which) {
    Exact<float> m(which < 2 ? 9 : 12);
    if (S.rc(ipk_const_matrix(which, m)) == IPK_OK) S.bytes(m.p, m.size_bytes());
    ++S.cases;
  }
  S.done();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the descriptor grid of tools/make_route_table.py, restated
// ---------------------------------------------------------------------------------------------------------------------------------
struct Frame { size_t w, h; size_t crops[4]; };
const Frame FRAMES[4] = {{47, 61, {0, 0, 0, 0}}, {96, 120, {3, 1, 2, 5}}, {131, 97, {0, 0, 0, 0}}, {300, 20, {0, 0, 0, 0}}};
struct Source { const char *cfa; int src_type, cpp, is_cfa; };
const Source SOURCES[10] = {{"RGGB", 0, 1, 1}, {"RGGB", 1, 1, 1}, {XT, 0, 1, 1}, {XT, 1, 1, 1}, {"RGBE", 0, 1, 1}, {"RGBE", 1, 1, 1},
                            {"", 0, 1, 0}, {"", 0, 3, 0}, {"", 2, 3, 0}, {"", 3, 3, 0}};
const size_t MAXWIDTHS[3] = {0, 87, 20};
const int ALLOW_FUSED[5] = {0, 1, 3, 5, 7};
const int FUSE_FLAGS[4][2] = {{0, 0}, {1, 0}, {0, 1}, {1, 1}};
const int ORIENTATIONS[3][2] = {{0, 0}, {1, 0}, {2, 1}};
const float R9[9][5] = {{0.05f, 0.05f, 0.05f, 0.05f, 0}, {0.1f, 0.05f, 0.2f, 0, 0}, {0, 0, 0, 0, 0.04f}, {0.1f, 0, 0, 0, 0.2f}, {0, 0, 0, 0, 0.5f},
                        {0.02f, 0.03f, 0.01f, 0.02f, 0.77f}, {0, 0, 0, 0, 1.0f}, {0, 0, 0, 0, 1.3f}, {0.07f, 0.11f, 0.05f, 0.02f, 0.04f}};
const int GRID_RC[4] = {-1, 1, 3, 8};                      // off, and R9[1], R9[3], R9[8]

void cam_matrix(float *m12) {                              // tests/util.py cam_matrix(): SRGB_D65_43 with scaled rows, in f32
  const float m[12] = {0.4124564f, 0.3575761f, 0.1804375f, 0.0f, 0.2126729f, 0.7151522f, 0.0721750f, 0.0f, 0.0193339f, 0.1191920f, 0.9503041f, 0.0f};
  const float s[3] = {1.10f, 1.05f, 1.20f};
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 4; ++c) m12[r * 4 + c] = m[r * 4 + c] * s[r];
}
ipk_pipeline_desc base_desc(size_t w, size_t h, const char *cfa, const size_t *crops, int src_type, int cpp, int is_cfa) {
  ipk_pipeline_desc d = IPK_PIPELINE_DESC_INIT;
  d.src_type = src_type; d.width = w; d.height = h; d.cpp = cpp; d.is_cfa = is_cfa;
  std::strncpy(d.cfa, cfa, sizeof(d.cfa) - 1);
  d.crop_top = crops[0]; d.crop_right = crops[1]; d.crop_bottom = crops[2]; d.crop_left = crops[3];
  for (int i = 0; i < 4; ++i) { d.blacklevels[i] = 512.0f; d.whitelevels[i] = 16383.0f; }
  d.wb_coeffs[0] = 2.0f; d.wb_coeffs[1] = 1.0f; d.wb_coeffs[2] = 1.5f; d.wb_coeffs[3] = NAN;
  cam_matrix(d.cam_to_xyz_normalized);
  d.allow_fused = 1;
  return d;
}
const size_t UNTOUCHED = ~(size_t)0;
int32_t col(size_t v) { return v == UNTOUCHED ? -1 : (int32_t)v; }
// one row of the recording (make_route_table.py _row): 19 int32
void route_row(const ipk_pipeline_desc *d, int out_type, int32_t *row) {
  row[0] = ipk_pipeline_takes_fastpath(d, out_type); row[1] = ipk_pipeline_fuses_rotatecrop(d, out_type);
  row[2] = ipk_pipeline_fuses_scaledown(d, out_type); row[3] = ipk_pipeline_fuses_four_colour(d, out_type);
  Exact<size_t> s(4, 0xFF);
  const int rc = ipk_pipeline_sizes(d, &s[0], &s[1], &s[2], &s[3]);
  const size_t fw = s[2], fh = s[3];
  row[4] = rc; for (int i = 0; i < 4; ++i) row[5 + i] = col(s[(size_t)i]);
  const size_t regions[2][4] = {{1, 2, 5, 3}, {0, 0, rc == 0 ? fw : 0, rc == 0 ? fh : 0}};
  for (int k = 0; k < 2; ++k) {
    Exact<size_t> o(4, 0xFF);
    row[9 + 5 * k] = ipk_pipeline_region(d, out_type, regions[k][0], regions[k][1], regions[k][2], regions[k][3], &o[0], &o[1], &o[2], &o[3]);
    for (int i = 0; i < 4; ++i) row[10 + 5 * k + i] = col(o[(size_t)i]);
  }
}
void fold_row(Section &S, const int32_t *row, int n) { for (int i = 0; i < n; ++i) S.i32(row[i]); ++S.cases; }
void hashes_call(Section &H, const ipk_pipeline_desc *d, int out_type, uint64_t id) {
  Exact<uint8_t> out(256);
  if (H.rc(ipk_pipeline_hashes(d, out_type, id, out)) == IPK_OK) H.bytes(out.p, 256);
  ++H.cases;
}
void sec_routes() {
  Section G("route_grid"), H("route_hashes"), I("route_invalid"), F("route_fast");
  int32_t row[19];
  for (const Frame &f : FRAMES)
    for (const Source &s : SOURCES) {
      ipk_pipeline_desc d = base_desc(f.w, f.h, s.cfa, f.crops, s.src_type, s.cpp, s.is_cfa);
      d.fuse_rotatecrop = 0;
      for (int k : GRID_RC) for (size_t mw : MAXWIDTHS) for (int allow : ALLOW_FUSED) for (const auto &ff : FUSE_FLAGS) for (const auto &o : ORIENTATIONS) {
        for (int i = 0; i < 5; ++i) d.rotatecrop[i] = k < 0 ? 0.0f : R9[k][i];
        d.maxwidth = mw; d.allow_fused = allow; d.fuse_rotatecrop = ff[0]; d.fuse_scaledown = ff[1]; d.rotation = o[0]; d.fliph = o[1];
        for (int out_type = 0; out_type < 2; ++out_type) {
          // the descriptor itself is an exact heap object too
          Exact<ipk_pipeline_desc> hd(1); std::memcpy(hd.p, &d, sizeof d);
          route_row(hd, out_type, row); fold_row(G, row, 19);
          hashes_call(H, hd, out_type, 7);
        }
      }
      for (int kind = 0; kind < 2; ++kind)
        for (int out_type = 0; out_type < 2; ++out_type) {
          ipk_pipeline_desc bad = base_desc(f.w, f.h, s.cfa, f.crops, s.src_type, s.cpp, s.is_cfa);
          bad.fuse_rotatecrop = 1; bad.fuse_scaledown = 1; bad.allow_fused = 7;
          if (kind == 0) bad.fuse_rotatecrop = 2; else bad.npoints = 65;
          route_row(&bad, out_type, row);
          Exact<uint8_t> h256(256);
          const int32_t inv[7] = {row[0], row[1], row[2], row[3], row[4], row[9], ipk_pipeline_hashes(&bad, out_type, 7, h256)};
          fold_row(I, inv, 7);
        }
    }
  Exact<float> m(12); ipk_const_matrix(2, m);
  const size_t fast_frames[4][2] = {{47, 61}, {96, 120}, {300, 20}, {5, 5}}, none[4] = {0, 0, 0, 0};
  for (const auto &fr : fast_frames) for (int src_type = 2; src_type <= 3; ++src_type) for (size_t mw : MAXWIDTHS) for (int use = 1; use >= 0; --use) for (int fliph = 0; fliph < 2; ++fliph) {
    ipk_pipeline_desc d = base_desc(fr[0], fr[1], "", none, src_type, 3, 0);
    d.fuse_rotatecrop = 1; d.fuse_scaledown = 1; d.maxwidth = mw; d.use_fastpath = use; d.fliph = fliph;
    for (int i = 0; i < 4; ++i) { d.blacklevels[i] = 0.0f; d.whitelevels[i] = 0.0f; }
    std::memcpy(d.cam_to_xyz_normalized, m.p, 48);
    d.wb_coeffs[0] = d.wb_coeffs[1] = d.wb_coeffs[2] = 1.0f; d.wb_coeffs[3] = 0.0f;
    for (int out_type = 0; out_type < 3; ++out_type) { route_row(&d, out_type, row); fold_row(F, row, 19); }
  }
  G.done(); H.done(); I.done(); F.done();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// windows: ipk_transform_window_footprint and the regions of the windowed routes (tests/test_region_windows_route.py)
// ---------------------------------------------------------------------------------------------------------------------------------
struct Win { size_t x, y, w, h; };
std::vector<Win> windows_of(size_t nw, size_t nh) {
  auto mn = [](size_t a, size_t b) { return a < b ? a : b; };
  const size_t x3 = mn(3, nw - 1), y5 = mn(5, nh - 1);
  return {{0, 0, 1, 1}, {nw - 1, 0, 1, 1}, {0, nh - 1, 1, 1}, {nw - 1, nh - 1, 1, 1}, {x3, y5, mn(17, nw - x3), mn(9, nh - y5)}, {0, nh / 2, nw, 1}, {nw / 3, 0, 1, nh}, {0, 0, nw, nh}};
}
void footprint_call(Section &S, size_t W, size_t H, const int64_t *c6, size_t nw, size_t nh, const Win &w, bool expect_ok) {
  Exact<size_t> out(4, 0xFF);
  const int rc = S.rc(ipk_transform_window_footprint(W, H, c6[0], c6[1], c6[2], c6[3], c6[4], c6[5], nw, nh, w.x, w.y, w.w, w.h, out));
  ++S.cases;
  if (expect_ok) SAN_EXPECT(rc == IPK_OK, "footprint refused: %s", ipk_last_error());
  if (rc == IPK_OK) {
    SAN_EXPECT(out[0] + out[2] <= W && out[1] + out[3] <= H, "the footprint leaves the frame");
    S.bytes(out.p, out.size_bytes());
  } else for (int i = 0; i < 4; ++i) SAN_EXPECT(out[(size_t)i] == UNTOUCHED, "a refused footprint wrote its output");
}
void sec_windows() {
  Section S("window_footprint");
  struct T { int64_t c[6]; size_t nw, nh; };
  const T fixed[4] = {{{-4, -3, 58, 5, -9, 49}, 57, 44}, {{5, 40, 6, 39, 30, 44}, 2, 31}, {{50, 3, 4, 3, 50, 40}, 47, 38}, {{3, 7, 3, 7, 3, 7}, 9, 6}};
  for (const T &t : fixed) for (const Win &w : windows_of(t.nw, t.nh)) footprint_call(S, 61, 47, t.c, t.nw, t.nh, w, true);
  // the scaled form: scale_down_opbuf's corners and the demosaic size the library negotiates under a width limit
  const size_t scaled[3][3] = {{131, 97, 87}, {101, 103, 51}, {150, 100, 60}}, none[4] = {0, 0, 0, 0};
  for (const auto &sc : scaled) {
    ipk_pipeline_desc d = base_desc(sc[0], sc[1], "RGGB", none, 0, 1, 1);
    d.maxwidth = sc[2];
    size_t dw = 0, dh = 0, fw = 0, fh = 0;
    SAN_EXPECT(ipk_pipeline_sizes(&d, &dw, &dh, &fw, &fh) == IPK_OK && dw >= 2 && dh >= 2, "sizes: %s", ipk_last_error());
    const int64_t c[6] = {0, 0, (int64_t)sc[0] - 1, 0, 0, (int64_t)sc[1] - 1};
    for (const Win &w : windows_of(dw, dh)) footprint_call(S, sc[0], sc[1], c, dw, dh, w, true);
  }
  const int64_t c[6] = {0, 0, 60, 0, 0, 46};
  const Win refused[6] = {{0, 0, 0, 1}, {0, 0, 1, 0}, {40, 0, 2, 1}, {0, 30, 1, 2}, {41, 0, 1, 1}, {UNTOUCHED, 0, 2, 1}};
  for (const Win &w : refused) footprint_call(S, 61, 47, c, 41, 31, w, false);
  footprint_call(S, 61, 47, c, 1, 31, Win{0, 0, 1, 1}, false); footprint_call(S, 61, 47, c, 41, 1, Win{0, 0, 1, 1}, false);
  S.done();

  // regions of the taken descriptors, with and without IPK_FUSED_WINDOW_REGIONS
  Section R("regions");
  struct Taken { size_t w, h; const size_t *crops; int rc; size_t maxwidth; };
  static const size_t sensor[4] = {3, 1, 2, 5};
  std::vector<Taken> taken;
  for (int k = 0; k < 9; ++k) taken.push_back({96, 120, sensor, k, 0});
  for (int k = 0; k < 9; ++k) taken.push_back({47, 61, none, k, 0});
  taken.push_back({131, 97, none, -1, 87}); taken.push_back({101, 103, none, -1, 51});
  const struct { const char *cfa; int src_type, out_type; } forms[4] = {{"RGGB", 0, 0}, {"RGGB", 1, 1}, {XT, 0, 2}, {XT, 1, 0}};
  for (const Taken &t : taken) for (const auto &f : forms) {
    ipk_pipeline_desc d = base_desc(t.w, t.h, f.cfa, t.crops, f.src_type, 1, 1);
    if (t.rc >= 0) { d.fuse_rotatecrop = 1; std::memcpy(d.rotatecrop, R9[t.rc], sizeof d.rotatecrop); } else { d.fuse_scaledown = 1; d.maxwidth = t.maxwidth; }
    size_t dw, dh, fw = 0, fh = 0;
    SAN_EXPECT(ipk_pipeline_sizes(&d, &dw, &dh, &fw, &fh) == IPK_OK && fw >= 1 && fh >= 1, "sizes: %s", ipk_last_error());
    for (int bit = 0; bit < 2; ++bit) {
      d.allow_fused = bit ? (IPK_FUSED_ON | IPK_FUSED_WINDOW_REGIONS) : IPK_FUSED_ON;
      for (const Win &w : windows_of(fw, fh)) {
        Exact<size_t> o(4, 0xFF);
        const int route = R.rc(ipk_pipeline_region(&d, f.out_type, w.x, w.y, w.w, w.h, &o[0], &o[1], &o[2], &o[3]));
        ++R.cases;
        SAN_EXPECT(route == bit, "route %d with allow_fused %d: %s", route, d.allow_fused, route < 0 ? ipk_last_error() : "");
        SAN_EXPECT(o[0] + o[2] <= t.w && o[1] + o[3] <= t.h, "the sensor window leaves the sensor");
        R.bytes(o.p, o.size_bytes());
      }
    }
  }
  R.done();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// band plans, the dealing rule, the cache's bookkeeping
// ---------------------------------------------------------------------------------------------------------------------------------
void sec_bands() {
  Section S("band_plan");
  const size_t heights[11] = {1, 2, 5, 11, 12, 13, 37, 64, 100, 1000, 4001};
  const int periods[3] = {2, 6, 12};
  for (int n = 1; n <= 64; ++n) for (int p : periods) for (size_t h : heights) {
    Exact<ipk_band> b((size_t)n);
    SAN_EXPECT(S.rc(ipk_band_plan(h, n, p, b)) == IPK_OK, "band_plan(%zu, %d, %d): %s", h, n, p, ipk_last_error());
    ++S.cases;
    size_t rows = 0;
    for (int k = 0; k < n; ++k) {
      SAN_EXPECT(b[(size_t)k].out_row0 == rows && b[(size_t)k].src_row0 + b[(size_t)k].src_rows <= h, "band %d of %d leaves the %zu-row frame", k, n, h);
      if (k) SAN_EXPECT(b[(size_t)k].out_row0 % (size_t)p == 0 || b[(size_t)k].out_rows == 0, "band %d starts off the CFA period", k);
      rows += b[(size_t)k].out_rows;
    }
    SAN_EXPECT(rows == h, "the bands cover %zu of %zu rows", rows, h);
    S.bytes(b.p, b.size_bytes());
  }
  S.done();
  Section T("band_plan_scaled");
  const size_t pairs[6][2] = {{5760, 1440}, {100, 37}, {37, 36}, {12, 2}, {97, 65}, {4000, 3}};
  for (int n = 1; n <= 64; ++n) for (const auto &hp : pairs) {
    Exact<ipk_band> b((size_t)n);
    SAN_EXPECT(T.rc(ipk_band_plan_scaled(hp[0], hp[1], n, b)) == IPK_OK, "band_plan_scaled: %s", ipk_last_error());
    ++T.cases;
    size_t rows = 0;
    for (int k = 0; k < n; ++k) { SAN_EXPECT(b[(size_t)k].src_row0 + b[(size_t)k].src_rows <= hp[0], "scaled band %d leaves the frame", k); rows += b[(size_t)k].out_rows; }
    SAN_EXPECT(rows == hp[1], "the bands cover %zu of %zu rows", rows, hp[1]);
    T.bytes(b.p, b.size_bytes());
  }
  T.done();
}
void sec_deal() {
  Section S("deal_frames");
  const size_t frames[6] = {0, 1, 7, 64, 1000, UNTOUCHED};
  for (size_t nf : frames) for (int nd = 1; nd <= 8; ++nd) {
    size_t total = 0;
    for (int ix = 0; ix < nd; ++ix) {
      Exact<size_t> o(3, 0xFF);
      SAN_EXPECT(S.rc(ipk_deal_frames(nf, nd, ix, &o[0], &o[1], &o[2])) == IPK_OK, "deal_frames: %s", ipk_last_error());
      ++S.cases; S.bytes(o.p, o.size_bytes()); total += o[2];
    }
    SAN_EXPECT(total == nf, "%zu of %zu frames dealt to %d devices", total, nf, nd);
  }
  const int bad[3][2] = {{0, 0}, {4, -1}, {4, 4}};
  for (const auto &b : bad) { SAN_EXPECT(S.rc(ipk_deal_frames(10, b[0], b[1], nullptr, nullptr, nullptr)) < 0, "accepted"); ++S.cases; }
  S.done();
}
void key_of(uint64_t i, uint8_t *k32) { Rng r(0xCAC4E + i); for (int j = 0; j < 4; ++j) { const uint64_t v = r.next(); std::memcpy(k32 + 8 * j, &v, 8); } }
void sec_cache() {
  Section S("cache");
  auto stats = [&](ipk_cache *c, size_t want_bytes, size_t want_entries) {
    Exact<size_t> be(2, 0xFF); Exact<uint64_t> hme(3, 0xFF);
    S.rc(ipk_cache_stats(c, &be[0], &be[1], &hme[0], &hme[1], &hme[2])); ++S.cases;
    S.bytes(be.p, be.size_bytes()); S.bytes(hme.p, hme.size_bytes());
    SAN_EXPECT(be[0] == want_bytes && be[1] == want_entries, "cache holds %zu bytes in %zu entries, expected %zu in %zu", be[0], be[1], want_bytes, want_entries);
  };
  ipk_cache *c = nullptr;
  SAN_EXPECT(S.rc(ipk_cache_new(1000, &c)) == IPK_OK && c, "cache_new"); ++S.cases;
  Exact<uint8_t> key(32);
  for (uint64_t i = 0; i < 40; ++i) { key_of(i, key); S.rc(ipk_selftest_cache_put(c, key, 100)); ++S.cases; }       // past the budget: 30 evictions
  for (uint64_t i = 0; i < 40; ++i) { key_of(i, key); SAN_EXPECT(S.rc(ipk_cache_contains(c, key)) == (i >= 30 ? 1 : 0), "entry %d", (int)i); ++S.cases; }
  stats(c, 1000, 10);
  for (uint64_t i : {0ull, 39ull}) {                                                                             // a missing key, a present one
    const float *data = reinterpret_cast<const float *>(16); Exact<size_t> whc(3); int mono = 7;
    key_of(i, key);
    SAN_EXPECT(S.rc(ipk_cache_get(c, key, &data, &whc[0], &whc[1], &whc[2], &mono)) == (i ? IPK_OK : IPK_NOOP), "get %d", (int)i); ++S.cases;
  }
  S.rc(ipk_cache_clear(c)); ++S.cases;
  stats(c, 0, 0);
  for (uint64_t i = 0; i < 5; ++i) { key_of(100 + i, key); S.rc(ipk_selftest_cache_put(c, key, 100)); ++S.cases; }
  S.rc(ipk_cache_free(c)); ++S.cases;                                                                           // freeing a non-empty cache
  SAN_EXPECT(S.rc(ipk_cache_new(1000, &c)) == IPK_OK, "cache_new"); ++S.cases;
  key_of(1, key); S.rc(ipk_selftest_cache_put(c, key, 5000)); ++S.cases;                                        // larger than the whole budget: ends up alone
  key_of(2, key); S.rc(ipk_selftest_cache_put(c, key, 10)); ++S.cases;
  stats(c, 10, 1);
  S.rc(ipk_cache_free(c)); ++S.cases;
  S.done();
}

// ---------------------------------------------------------------------------------------------------------------------------------
// hostile
// ---------------------------------------------------------------------------------------------------------------------------------
float hostile_f(Rng &r) {
  static const float sp[] = {NAN, INFINITY, -INFINITY, 0.0f, -0.0f, 1e-45f, -1e-40f, FLT_MIN, FLT_MAX, -FLT_MAX, 1e30f, -1e30f, 9.223372e18f, 1.8446744e19f,
                             2147483648.0f, 4294967296.0f, -2147483904.0f, 1.0f, -1.0f, 0.5f, 0.99999994f, 1.0000001f, 16777216.0f, 65535.0f, 512.0f, 16383.0f};
  switch (r.below(4)) {
    case 0: return sp[r.below(sizeof sp / sizeof sp[0])];
    case 1: { const uint32_t b = (uint32_t)r.next(); float f; std::memcpy(&f, &b, 4); return f; }
    case 2: return r.unit();
    default: return (r.unit() - 0.5f) * 4.0f;
  }
}
size_t hostile_z(Rng &r) {
  static const uint64_t sp[] = {0, 1, 2, 9, 10, 11, 47, 48, 255, 256, 0x7FFFFFFFull, 0x80000000ull, 0xFFFFFFFFull, 0x100000000ull, 0x100000001ull, 1ull << 24,
                                (1ull << 24) - 1, 1ull << 62, 1ull << 63, (1ull << 63) - 1, ~0ull, ~0ull - 1, ~0ull - 47};
  switch (r.below(4)) {
    case 0: return (size_t)sp[r.below(sizeof sp / sizeof sp[0])];
    case 1: return (size_t)r.next();
    case 2: return (size_t)r.below(400);
    default: return (size_t)r.below(20000);
  }
}
int hostile_i(Rng &r) {
  static const int sp[] = {0, 1, -1, 2, 3, 4, 5, 7, 8, 9, 64, 65, 66, -3, INT_MAX, INT_MIN, 255, 256, 65536};
  switch (r.below(3)) { case 0: return sp[r.below(sizeof sp / sizeof sp[0])]; case 1: return (int)r.next(); default: return r.range(-3, 8); }
}
int64_t hostile_i64(Rng &r) {
  switch (r.below(4)) { case 0: return (int64_t)r.next(); case 1: return (int64_t)hostile_z(r); case 2: return -(int64_t)r.below(300); default: return (int64_t)r.below(300); }
}
void hostile_cfa(Rng &r, char *cfa160) {
  static const char *good[] = {"RGGB", "GBRG", "RGBE", "", XT, "8x2:RGBGRBGGGBGRGRBG", "2x8:RGBGRBGGGBGRGRBG", "RGGBGRBGGBRGBGGR", "1x1:R", "48x1:RGBGRBGGGBGRGRBGRGBGRBGGGBGRGRBGRGBGRBGGGBGRGRBG"};
  static const char alphabet[] = "RGBEMYx:0123456789 Z\xff";
  std::memset(cfa160, 0, 160);
  switch (r.below(5)) {
    case 0: case 1: std::strcpy(cfa160, good[r.below(sizeof good / sizeof good[0])]); break;
    case 2: { std::string w = w12(); if (r.below(2)) w = "12x12:" + w; std::memcpy(cfa160, w.c_str(), w.size()); break; }
    case 3: { const size_t n = r.below(161); for (size_t i = 0; i < n; ++i) cfa160[i] = alphabet[r.below(sizeof alphabet - 1)]; break; }      // n = 160: no terminator
    default: for (int i = 0; i < 160; ++i) cfa160[i] = "RGB"[r.below(3)]; break;                                                                 // unterminated letters
  }
  if (r.below(8) == 0 && cfa160[0]) cfa160[r.below(strnlen(cfa160, 160))] = alphabet[r.below(sizeof alphabet - 1)];
}
bool g_trace = false;                                       // a fourth argument "trace": the running digest after every hostile case, to find where two builds part
void sec_hostile_desc(uint64_t count) {
  Section S("hostile_desc");
  Rng r(0xD35C);
  const size_t sizes[] = {sizeof(ipk_pipeline_desc), ipk_abi_sizeof(17), ipk_abi_sizeof(21), ipk_abi_sizeof(19), 0, 4, 8, sizeof(ipk_pipeline_desc) + 8,
                          sizeof(ipk_pipeline_desc) - 4, ipk_abi_sizeof(17) + 4, ipk_abi_sizeof(17) - 1, 0xFFFFFFFFu};
  for (uint64_t it = 0; it < count; ++it) {
    const Frame &f = FRAMES[r.below(4)]; const Source &s = SOURCES[r.below(10)];
    ipk_pipeline_desc d = base_desc(f.w, f.h, s.cfa, f.crops, s.src_type, s.cpp, s.is_cfa);
    // every field is hostile with probability 1/3; the rest keeps a descriptor the drivers would take, so that the deep paths are reached too
    auto H = [&] { return r.below(3) == 0; };
    if (H()) d.src_type = hostile_i(r);
    if (H()) d.width = hostile_z(r);
    if (H()) d.height = hostile_z(r);
    if (H()) d.cpp = hostile_i(r);
    if (H()) d.is_cfa = hostile_i(r);
    if (H()) hostile_cfa(r, d.cfa);
    if (H()) { d.crop_top = hostile_z(r); d.crop_right = hostile_z(r); d.crop_bottom = hostile_z(r); d.crop_left = hostile_z(r); }
    if (H()) for (int i = 0; i < 4; ++i) { d.blacklevels[i] = hostile_f(r); d.whitelevels[i] = hostile_f(r); }
    if (H()) for (int i = 0; i < 5; ++i) d.rotatecrop[i] = r.below(2) ? hostile_f(r) : R9[r.below(9)][i];
    if (H()) for (int i = 0; i < 12; ++i) d.cam_to_xyz_normalized[i] = hostile_f(r);
    if (H()) for (int i = 0; i < 4; ++i) d.wb_coeffs[i] = hostile_f(r);
    if (H()) d.exposure = hostile_f(r);
    if (H()) { d.npoints = r.range(-3, 66); for (int i = 0; i < 128; ++i) d.points[i] = r.below(4) ? r.unit() : hostile_f(r); }
    if (H()) { d.rotation = hostile_i(r); d.fliph = hostile_i(r); d.flipv = hostile_i(r); }
    if (H()) { d.maxwidth = hostile_z(r); d.maxheight = hostile_z(r); }
    if (H()) d.linear = hostile_i(r);
    d.allow_fused = H() ? hostile_i(r) : ALLOW_FUSED[r.below(5)];
    if (H()) d.use_fastpath = hostile_i(r);
    if (H()) { d.cfa_width = hostile_i(r); d.cfa_height = hostile_i(r); }
    if (H()) d.schedule = hostile_i(r);
    d.fuse_rotatecrop = H() ? hostile_i(r) : (int)r.below(2);
    if (H()) d.reserved1 = hostile_i(r);
    d.fuse_scaledown = H() ? hostile_i(r) : (int)r.below(2);
    if (r.below(4) == 0) d.struct_size = (uint32_t)sizes[r.below(sizeof sizes / sizeof sizes[0])];
    // the caller's object: exactly as many bytes as it says it has (never more than this header's struct, never less than the size field)
    size_t have = d.struct_size; if (have > sizeof d) have = sizeof d; if (have < 4) have = 4;
    Exact<unsigned char> obj(have); std::memcpy(obj.p, &d, have);
    const ipk_pipeline_desc *p = reinterpret_cast<const ipk_pipeline_desc *>(obj.p);
    const int out_type = r.below(6) ? (int)r.below(3) : hostile_i(r);
    Exact<size_t> sz(4, 0xFF);
    S.rc(ipk_pipeline_sizes(p, &sz[0], &sz[1], &sz[2], &sz[3])); S.bytes(sz.p, sz.size_bytes());
    S.rc(ipk_pipeline_takes_fastpath(p, out_type)); S.rc(ipk_pipeline_fuses_rotatecrop(p, out_type));
    S.rc(ipk_pipeline_fuses_scaledown(p, out_type)); S.rc(ipk_pipeline_fuses_four_colour(p, out_type));
    Exact<uint8_t> h256(256);
    if (S.rc(ipk_pipeline_hashes(p, out_type, r.below(2) ? 0 : r.next(), h256)) == IPK_OK) S.bytes(h256.p, 256);
    Exact<size_t> o(4, 0xFF);
    const bool inside = r.below(2) && sz[2] != UNTOUCHED && sz[2] && sz[3];
    const size_t x = inside ? r.below(sz[2]) : hostile_z(r), y = inside ? r.below(sz[3]) : hostile_z(r);
    const size_t w = inside ? 1 + r.below(sz[2] - x) : hostile_z(r), h = inside ? 1 + r.below(sz[3] - y) : hostile_z(r);
    S.rc(ipk_pipeline_region(p, out_type, x, y, w, h, &o[0], &o[1], &o[2], &o[3])); S.bytes(o.p, o.size_bytes());
    ++S.cases;
    if (g_trace) std::fprintf(stderr, "TRACE hostile_desc %llu %016llx\n", (unsigned long long)it, (unsigned long long)S.h);
  }
  S.done();
}
void sec_hostile_args(uint64_t count) {
  Section S("hostile_args");
  Rng r(0xA465);
  for (uint64_t it = 0; it < count; ++it) {
    switch (it % 12) {
      case 0: {
        const int npts = r.range(-3, 66); const size_t n = npts > 0 ? (size_t)npts : 0;
        Exact<float> pts(n * 2);
        for (size_t i = 0; i < n * 2; ++i) pts[i] = r.below(3) ? r.unit() : hostile_f(r);
        spline_call(S, pts, npts, n + 2); --S.cases;
        break; }
      case 1: {
        Exact<float> p5(5); for (int i = 0; i < 5; ++i) p5[(size_t)i] = r.below(2) ? hostile_f(r) : r.unit() * 0.6f;
        Exact<size_t> o(2, 0xFF);
        S.rc(ipk_rotatecrop_calc_size(p5, hostile_f(r), hostile_z(r), hostile_z(r), hostile_i(r), &o[0], &o[1])); S.bytes(o.p, o.size_bytes());
        break; }
      case 2: {
        Exact<size_t> o(4, 0xFF);
        if (S.rc(ipk_size_image(hostile_z(r), hostile_z(r), hostile_z(r), hostile_z(r), hostile_z(r), hostile_z(r), o)) == IPK_OK) S.bytes(o.p, o.size_bytes());
        break; }
      case 3: {
        Exact<float> sc(1); Exact<size_t> o(2, 0xFF);
        S.rc(ipk_calculate_scaling_total(hostile_z(r), hostile_z(r), hostile_z(r), hostile_z(r), sc, &o[0], &o[1])); S.f32s(sc.p, 1); S.bytes(o.p, o.size_bytes());
        break; }
      case 4: {
        Exact<size_t> o(4, 0xFF);
        const size_t W = r.below(2) ? 1 + r.below(300) : hostile_z(r), H = r.below(2) ? 1 + r.below(300) : hostile_z(r);
        const size_t nw = r.below(2) ? 2 + r.below(300) : hostile_z(r), nh = r.below(2) ? 2 + r.below(300) : hostile_z(r);
        int64_t c[6]; for (auto &v : c) v = hostile_i64(r);
        if (S.rc(ipk_transform_window_footprint(W, H, c[0], c[1], c[2], c[3], c[4], c[5], nw, nh, r.below(2) ? r.below(nw ? nw : 1) : hostile_z(r),
                                                r.below(2) ? r.below(nh ? nh : 1) : hostile_z(r), r.below(2) ? 1 : hostile_z(r), r.below(2) ? 1 : hostile_z(r), o)) == IPK_OK)
          S.bytes(o.p, o.size_bytes());
        break; }
      case 5: case 6: {
        const int n = r.range(-3, 256);
        Exact<ipk_band> b(n > 0 ? (size_t)n : 0);
        const int rc = it % 12 == 5 ? ipk_band_plan(hostile_z(r), n, hostile_i(r), b) : ipk_band_plan_scaled(hostile_z(r), hostile_z(r), n, b);
        if (S.rc(rc) == IPK_OK) S.bytes(b.p, b.size_bytes());
        break; }
      case 7: {
        Exact<float> a3(3), b3(3), tt(2), m(12), wb(4);
        for (size_t i = 0; i < 3; ++i) b3[i] = hostile_f(r);
        for (size_t i = 0; i < 12; ++i) m[i] = r.below(2) ? hostile_f(r) : r.unit();
        S.rc(ipk_temp_to_xyz(r.below(2) ? hostile_f(r) : 1000.0f + 30000.0f * r.unit(), a3)); S.f32s(a3.p, 3);
        S.rc(ipk_xyz_to_temp(r.below(2) ? b3.p : a3.p, &tt[0], &tt[1])); S.f32s(tt.p, 2);
        S.rc(ipk_tolab_set_temp(m, hostile_f(r), hostile_f(r), wb)); S.f32s(wb.p, 4);
        for (size_t i = 0; i < 4; ++i) if (r.below(2)) wb[i] = hostile_f(r);
        S.rc(ipk_tolab_get_temp(m, wb, &tt[0], &tt[1])); S.f32s(tt.p, 2);
        break; }
      case 8: {
        char cfa[161]; hostile_cfa(r, cfa); cfa[160] = 0;
        std::string pat = cfa, got;
        if (r.below(4) == 0) pat = stated(DIV48[r.below(10)], DIV48[r.below(10)]);
        shift_exact(S, pat, hostile_i(r), hostile_i(r), got); --S.cases;
        SAN_EXPECT(got.size() <= pat.size(), "'%s' -> '%s' is longer than the pattern", pat.c_str(), got.c_str());
        break; }
      case 9: {
        Exact<size_t> o(3, 0xFF);
        const bool nul = r.below(4) == 0;
        S.rc(ipk_deal_frames(hostile_z(r), hostile_i(r), hostile_i(r), nul ? nullptr : &o[0], nul ? nullptr : &o[1], nul ? nullptr : &o[2])); S.bytes(o.p, o.size_bytes());
        break; }
      case 10: {
        Exact<float> a(4), o(4); for (size_t i = 0; i < 4; ++i) a[i] = hostile_f(r);
        S.rc(ipk_normalize_wbs(a, o)); S.f32s(o.p, 4);
        Exact<int> f3(3); S.rc(ipk_orientation_to_flips(hostile_i(r), f3)); S.bytes(f3.p, 12);
        S.rc(ipk_orientation_from_flips(hostile_i(r), hostile_i(r), hostile_i(r)));
        S.rc(ipk_transform_orientation(hostile_i(r), hostile_i(r), hostile_i(r)));
        S.u64(ipk_abi_sizeof(hostile_i(r)));
        break; }
      default: {
        Exact<float> m(12); if (S.rc(ipk_const_matrix(hostile_i(r), m)) == IPK_OK) S.bytes(m.p, 48);
        if (it % 48 == 11) { Exact<float> t(8193); if (S.rc(ipk_lut_table(hostile_i(r), t)) == IPK_OK) S.bytes(t.p, t.size_bytes()); }
        Exact<uint8_t> d(r.below(300)), h(32); for (size_t i = 0; i < d.n; ++i) d[i] = (uint8_t)r.next();
        S.rc(ipk_selftest_sha256(d, d.n, h)); S.bytes(h.p, 32);
        break; }
    }
    ++S.cases;
    if (g_trace) std::fprintf(stderr, "TRACE hostile_args %llu %016llx\n", (unsigned long long)it, (unsigned long long)S.h);
  }
  S.done();
}
}  // namespace

int main(int argc, char **argv) {
  const uint64_t n_desc = argc > 1 ? std::strtoull(argv[1], nullptr, 10) : 200000, n_args = argc > 2 ? std::strtoull(argv[2], nullptr, 10) : 200000;
  g_trace = argc > 3 && std::strcmp(argv[3], "trace") == 0;
  sec_cfa_shift(); sec_spline(); sec_tables(); sec_routes(); sec_windows(); sec_bands(); sec_deal(); sec_cache();
  sec_hostile_desc(n_desc); sec_hostile_args(n_args);
  if (ipk_is_initialized() != 0) { std::fprintf(stderr, "CONTRACT the library was initialised\n"); return 1; }
  if (san::g_failures) { std::fprintf(stderr, "%d contract failures\n", san::g_failures); return 1; }
  std::printf("HOST_SURFACE_OK\n");
  return 0;
}
