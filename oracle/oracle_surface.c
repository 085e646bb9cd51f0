/* Every ORC_API function of imagepipe_oracle.c from a stand-alone C program, linked with the oracle's source directly (`make san`): once under
 * AddressSanitizer + UBSan (float-cast-overflow included -- a float-to-integer cast outside the target's range is where C parts from Rust's
 * saturating `as`) and once plain.  tests/test_host_sanitizers.py runs both with OMP_NUM_THREADS=1 and 4; all four digests of a section must agree.
 * Output buffers are heap blocks of exactly the size the call needs.  One line per section:  SECTION <name> cases=<n> digest=<fnv1a-64>
 *   oracle_surface <directory of tests/golden/pin>                                                                                         */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

/* the oracle's C surface (it has no header: Python binds it by name) */
typedef struct {
  int source_kind; const void *data; size_t width, height; int cpp; int is_cfa; char cfa[160];
  size_t crop_top, crop_right, crop_bottom, crop_left; float blacklevels[4], whitelevels[4];
  float rc[5]; float cam_to_xyz_normalized[12]; float wb_coeffs[4];
  float exposure; int npoints; float points[2 * 64];
  int rotation, fliph, flipv; size_t maxwidth, maxheight; int linear; int use_fastpath;
} orc_pipeline;
void orc_set_num_threads(int n); int orc_get_max_threads(void);
void orc_const_srgb_d65_33(float *); void orc_const_xyz_d65_33(float *); void orc_const_srgb_d65_43(float *); void orc_inverse33(const float *, float *);
void orc_luts_init(void); const float *orc_lut_table(int); int orc_lut_len(void);
void orc_lookup(int, const float *, float *, size_t);
void orc_input8bit(const uint8_t *, float *, size_t); void orc_input16bit(const uint16_t *, float *, size_t);
void orc_output8bit(const float *, uint8_t *, size_t); void orc_output16bit(const float *, uint16_t *, size_t);
void orc_xyz_to_lab(const float *, float *, size_t); void orc_lab_to_xyz(const float *, float *, size_t);
void orc_camera_to_lab(const float *, const float *, const float *, float *, size_t); void orc_lab_to_rgb(const float *, const float *, float *, size_t);
int orc_cfa_shift(const char *, int, int, char *); int orc_cfa_pattern(const char *, int *);
int orc_size_image(size_t, size_t, size_t, size_t, size_t, size_t, size_t *);
void orc_gofloat_cfa_u16(const uint16_t *, size_t, size_t, size_t, size_t, size_t, float, float, float *);
void orc_gofloat_cfa_f32(const float *, size_t, size_t, size_t, size_t, size_t, float, float, float *);
void orc_gofloat_mono_u16(const uint16_t *, size_t, size_t, size_t, size_t, size_t, float, float, float *);
void orc_gofloat_mono_f32(const float *, size_t, size_t, size_t, size_t, size_t, float, float, float *);
void orc_gofloat_rgb_u16(const uint16_t *, size_t, size_t, size_t, size_t, size_t, const float *, const float *, float *);
void orc_gofloat_rgb_f32(const float *, size_t, size_t, size_t, size_t, size_t, const float *, const float *, float *);
void orc_gofloat_other_u8(const uint8_t *, size_t, size_t, size_t, size_t, size_t, float *);
void orc_gofloat_other_u16(const uint16_t *, size_t, size_t, size_t, size_t, size_t, float *);
int orc_demosaic_full(const char *, const float *, size_t, size_t, float *);
void orc_calculate_scaling_total(size_t, size_t, size_t, size_t, float *, size_t *, size_t *);
int orc_transform_buffer_f32(const float *, size_t, size_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, size_t, size_t, size_t, const char *, float *);
int orc_transform_buffer_u8(const uint8_t *, size_t, size_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, size_t, size_t, size_t, const char *, uint8_t *);
int orc_transform_buffer_u16(const uint16_t *, size_t, size_t, int64_t, int64_t, int64_t, int64_t, int64_t, int64_t, size_t, size_t, size_t, const char *, uint16_t *);
int orc_scaled_demosaic(const char *, const float *, size_t, size_t, size_t, size_t, float *);
int orc_scale_down_opbuf(const float *, size_t, size_t, size_t, size_t, float *);
int orc_scale_down_srgb(const uint8_t *, size_t, size_t, size_t, size_t, uint8_t *); int orc_scale_down_srgb16(const uint16_t *, size_t, size_t, size_t, size_t, uint16_t *);
int orc_demosaic_run(const char *, const float *, size_t, size_t, size_t, size_t, size_t, float *, size_t *, size_t *);
void orc_normalize_wbs(const float *, float *);
void orc_tolab(const float *, size_t, size_t, int, const float *, const float *, float *); void orc_fromlab(const float *, size_t, size_t, float *);
void orc_temp_to_xyz(float, float *); void orc_xyz_to_temp(const float *, float *);
void orc_tolab_set_temp(const float *, float, float, float *); void orc_tolab_get_temp(const float *, const float *, float *);
int orc_spline_new(const float *, int, float *, float *, float *, float *, float *); int orc_spline_interpolate(const float *, int, const float *, float *, size_t);
int orc_basecurve(const float *, size_t, size_t, float, const float *, int, float *); int orc_gamma(const float *, size_t, size_t, size_t, int, float *);
void orc_orientation_to_flips(int, int *); int orc_orientation_from_flips(int, int, int); void orc_transform_new(int, int *); int orc_transform_orientation(int, int, int);
int orc_rotate_buffer(const float *, size_t, size_t, int, float *, size_t *, size_t *); void orc_transform_forward(int, size_t, size_t, size_t *, size_t *);
void orc_rotatecrop_calc_size(const float *, float, size_t, size_t, int, size_t *, size_t *);
int orc_rotatecrop_run(const float *, const float *, size_t, size_t, size_t, float *, size_t *, size_t *);
int orc_rotatecrop_corners(const float *, size_t, size_t, int64_t *, size_t *, size_t *);
uint64_t orc_selftest_rotatecrop_roundtrip_transform(void); uint64_t orc_selftest_rotatecrop_roundtrip_rotation(void);
size_t orc_pipeline_sizeof(void); int orc_pipeline_sizes(const orc_pipeline *, size_t *, size_t *, size_t *, size_t *);
float *orc_pipeline_run(const orc_pipeline *, size_t *, size_t *); void orc_free(void *); int orc_pipeline_default_ops_other(const orc_pipeline *);
uint8_t *orc_pipeline_output_8bit(orc_pipeline *, size_t *, size_t *); uint16_t *orc_pipeline_output_16bit(orc_pipeline *, size_t *, size_t *);

/* ---- digest, generator, exact buffers ---------------------------------------------------------------------------------------------- */
typedef struct { const char *name; uint64_t h, cases; } section;
static section sec(const char *name) { section s = {name, 0xcbf29ce484222325ull, 0}; return s; }
static void fold(section *s, const void *p, size_t n) { const unsigned char *b = p; for (size_t i = 0; i < n; i++) { s->h ^= b[i]; s->h *= 0x100000001b3ull; } }
static void fold_i(section *s, int64_t v) { unsigned char b[8]; for (int i = 0; i < 8; i++) b[i] = (unsigned char)((uint64_t)v >> (8 * i)); fold(s, b, 8); }
/* floats enter with every NaN as one canonical NaN: IEEE 754 arithmetic does not define a NaN's sign or payload, so two correct builds may differ there */
static void fold_f(section *s, const float *v, size_t n) {
  for (size_t i = 0; i < n; i++) { uint32_t u; memcpy(&u, &v[i], 4); if ((u & 0x7fffffffu) > 0x7f800000u) u = 0x7fc00000u; fold(s, &u, 4); }
}
static void done(const section *s) { printf("SECTION %s cases=%llu digest=%016llx\n", s->name, (unsigned long long)s->cases, (unsigned long long)s->h); fflush(stdout); }
static uint64_t g_rng = 0x0AC1E5EEDull;
static uint64_t rnd(void) { uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull); z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull; z = (z ^ (z >> 27)) * 0x94D049BB133111EBull; return z ^ (z >> 31); }
static float unitf(void) { return (float)(rnd() >> 40) / 16777216.0f; }
static void *exact(size_t bytes) { void *p = malloc(bytes); if (!p) { fprintf(stderr, "out of memory\n"); exit(3); } memset(p, 0x55, bytes); return p; }
static int g_fail = 0;
#define EXPECT(c, ...) do { if (!(c)) { fprintf(stderr, "CONTRACT %s:%d: %s: ", __FILE__, __LINE__, #c); fprintf(stderr, __VA_ARGS__); fprintf(stderr, "\n"); g_fail++; } } while (0)

/* tests/util.py SPECIALS */
static const float SP[37] = {0.0f, -0.0f, 1.0f, -1.0f, 0.5f, 1.5f, 2.0f, 8.0f, 1e-3f, -1e-3f, 0.008856452f, 0.0088564521f, 0.04045f, 0.0031308f, 1e-30f, -1e-30f, 1e-40f, -1e-40f,
                             1e30f, -1e30f, INFINITY, -INFINITY, NAN, 0.99999994f, 1.0000001f, 3.4e38f, 1.17549435e-38f, 0.9504700f, 1.08883f, 0.95047f, 255.0f, 65535.0f,
                             0.33333334f, 0.6f, 0.5f, 0.49999997f, 0.50000006f};
#define NSP 37
static const char *XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG";
static char W12[145];
static void make_w12(void) {
  static const int a[6] = {0, 18, 6, 24, 12, 30}, b[6] = {18, 0, 24, 6, 30, 12};
  char w[289]; size_t n = 0;
  for (int rep = 0; rep < 2; rep++) for (int k = 0; k < 6; k++) { memcpy(w + n, XT + a[k], 6); n += 6; }
  for (int rep = 0; rep < 2; rep++) for (int k = 0; k < 6; k++) { memcpy(w + n, XT + b[k], 6); n += 6; }
  memcpy(w + 144, w, 144); memcpy(W12, w, 144); W12[144] = 0;
}
static const float WB[4] = {2.0f, 1.0f, 1.5f, NAN};
static void cam_matrix(float *m12) {
  static const float m[12] = {0.4124564f, 0.3575761f, 0.1804375f, 0.0f, 0.2126729f, 0.7151522f, 0.0721750f, 0.0f, 0.0193339f, 0.1191920f, 0.9503041f, 0.0f};
  static const float s[3] = {1.10f, 1.05f, 1.20f};
  for (int r = 0; r < 3; r++) for (int c = 0; c < 4; c++) m12[r * 4 + c] = m[r * 4 + c] * s[r];
}

/* ---- demosaic: the pinned frames from disk, seeded frames at odd sizes, eight filters ------------------------------------------------- */
static void demosaic_frame(section *S, const char *cfa, const uint16_t *raw, size_t w, size_t h, float black, float white, size_t dw, size_t dh) {
  float *mosaic = exact(w * h * 4);
  orc_gofloat_cfa_u16(raw, w, 0, 0, w, h, black, white, mosaic); fold_f(S, mosaic, w * h);
  float *full = exact(w * h * 16);
  EXPECT(orc_demosaic_full(cfa, mosaic, w, h, full) == 0, "demosaic_full %s %zux%zu", cfa, w, h); fold_f(S, full, w * h * 4);
  /* OpDemosaic::run towards the given size, then scaled_demosaic on both sides of every filter's minscale (1.5 and 4) */
  const size_t big = (dw * dh > w * h ? dw * dh : w * h);
  float *run = exact(big * 16); size_t ow = 0, oh = 0;
  const int kind = orc_demosaic_run(cfa, mosaic, w, h, 1, dw, dh, run, &ow, &oh);
  EXPECT(kind >= 2 && ow * oh <= big, "demosaic_run -> %d", kind); fold_i(S, kind); fold_i(S, (int64_t)ow); fold_i(S, (int64_t)oh); fold_f(S, run, ow * oh * 4);
  const size_t sizes[2][2] = {{w * 2 / 3, h * 2 / 3}, {w / 4 < 2 ? 2 : w / 4, h / 4 < 2 ? 2 : h / 4}};
  for (int k = 0; k < 2; k++) {
    float *sd = exact(sizes[k][0] * sizes[k][1] * 16);
    EXPECT(orc_scaled_demosaic(cfa, mosaic, w, h, sizes[k][0], sizes[k][1], sd) == 0, "scaled_demosaic"); fold_f(S, sd, sizes[k][0] * sizes[k][1] * 4);
    free(sd);
  }
  free(run); free(full); free(mosaic);
  S->cases++;
}
static void sec_demosaic(const char *pin_dir) {
  section S = sec("demosaic");
  char path[1024], line[512];
  snprintf(path, sizeof path, "%s/cases.txt", pin_dir);
  FILE *f = fopen(path, "r");
  if (!f) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
  while (fgets(line, sizeof line, f)) {
    char name[64], cfa[160]; size_t w, h, dw, dh; float black, white;
    if (line[0] == '#' || sscanf(line, "%63s %159s %zu %zu %f %f %zu %zu", name, cfa, &w, &h, &black, &white, &dw, &dh) != 8) continue;
    snprintf(path, sizeof path, "%s/%s.raw.u16", pin_dir, name);
    FILE *r = fopen(path, "rb");
    if (!r) { fprintf(stderr, "cannot open %s\n", path); exit(2); }
    uint16_t *raw = exact(w * h * 2);
    if (fread(raw, 2, w * h, r) != w * h) { fprintf(stderr, "%s is short\n", path); exit(2); }
    fclose(r);
    demosaic_frame(&S, cfa, raw, w, h, black, white, dw, dh);
    free(raw);
  }
  fclose(f);
  const size_t sizes[4][2] = {{10, 10}, {11, 13}, {17, 10}, {23, 19}};
  const char *filters[8] = {"RGGB", "GRBG", "GBRG", "BGGR", XT, W12, "RGBE", "8x2:RGBGRBGGGBGRGRBG"};
  for (int s = 0; s < 4; s++) for (int k = 0; k < 8; k++) {
    const size_t w = sizes[s][0], h = sizes[s][1];
    uint16_t *raw = exact(w * h * 2);
    for (size_t i = 0; i < w * h; i++) raw[i] = (uint16_t)(rnd() % 16384);
    demosaic_frame(&S, filters[k], raw, w, h, 512.0f, 16383.0f, w - 3, h - 3);
    free(raw);
  }
  done(&S);
}

/* ---- transform_buffer: three element types, corners inside and outside the frame, special samples --------------------------------------- */
static void sec_transform(void) {
  section S = sec("transform");
  const size_t w = 31, h = 23, nw = 17, nh = 13;
  const int64_t corners[4][6] = {{2, 3, 27, 2, 3, 19}, {-4, -3, 36, 5, -9, 30}, {28, 3, 4, 3, 28, 20}, {3, 7, 3, 7, 3, 7}};
  const size_t comps[3] = {1, 3, 4};
  for (int c = 0; c < 4; c++) for (int k = 0; k < 3; k++) {
    const size_t n = w * h * comps[k], m = nw * nh * comps[k];
    const char *cfa = comps[k] == 1 ? "RGGB" : NULL;
    const int64_t *p = corners[c];
    float *sf = exact(n * 4), *of = exact(m * 4);
    for (size_t i = 0; i < n; i++) sf[i] = (i % 5 == 0) ? SP[(i / 5) % NSP] : unitf();
    fold_i(&S, orc_transform_buffer_f32(sf, w, h, p[0], p[1], p[2], p[3], p[4], p[5], nw, nh, comps[k], cfa, of)); fold_f(&S, of, m); S.cases++;
    uint8_t *s8 = exact(n), *o8 = exact(m);
    for (size_t i = 0; i < n; i++) s8[i] = (uint8_t)rnd();
    fold_i(&S, orc_transform_buffer_u8(s8, w, h, p[0], p[1], p[2], p[3], p[4], p[5], nw, nh, comps[k], cfa, o8)); fold(&S, o8, m); S.cases++;
    uint16_t *s16 = exact(n * 2), *o16 = exact(m * 2);
    for (size_t i = 0; i < n; i++) s16[i] = (uint16_t)rnd();
    fold_i(&S, orc_transform_buffer_u16(s16, w, h, p[0], p[1], p[2], p[3], p[4], p[5], nw, nh, comps[k], cfa, o16)); fold(&S, o16, m * 2); S.cases++;
    free(sf); free(of); free(s8); free(o8); free(s16); free(o16);
  }
  { float *s4 = exact(w * h * 16), *o4 = exact(nw * nh * 16); for (size_t i = 0; i < w * h * 4; i++) s4[i] = (i % 7 == 0) ? SP[(i / 7) % NSP] : unitf();
    fold_i(&S, orc_scale_down_opbuf(s4, w, h, nw, nh, o4)); fold_f(&S, o4, nw * nh * 4); S.cases++; free(s4); free(o4);
    uint8_t *s8 = exact(w * h * 3), *o8 = exact(nw * nh * 3); for (size_t i = 0; i < w * h * 3; i++) s8[i] = (uint8_t)rnd();
    fold_i(&S, orc_scale_down_srgb(s8, w, h, nw, nh, o8)); fold(&S, o8, nw * nh * 3); S.cases++; free(s8); free(o8);
    uint16_t *s16 = exact(w * h * 6), *o16 = exact(nw * nh * 6); for (size_t i = 0; i < w * h * 3; i++) s16[i] = (uint16_t)rnd();
    fold_i(&S, orc_scale_down_srgb16(s16, w, h, nw, nh, o16)); fold(&S, o16, nw * nh * 6); S.cases++; free(s16); free(o16); }
  done(&S);
}

/* ---- every gofloat form, whole and cropped; float sources carry the specials ------------------------------------------------------------- */
static void sec_gofloat(void) {
  section S = sec("gofloat");
  const size_t ow = 20, oh = 14;
  const size_t crops[2][4] = {{0, 0, 20, 14}, {3, 2, 15, 10}};             /* x, y, width, height */
  const float b4[4] = {512.0f, 500.0f, 520.0f, 512.0f}, w4[4] = {16383.0f, 16000.0f, 16383.0f, 15000.0f};
  uint16_t *u1 = exact(ow * oh * 2), *u3 = exact(ow * oh * 6); uint8_t *b3 = exact(ow * oh * 3);
  float *f1 = exact(ow * oh * 4), *f3 = exact(ow * oh * 12);
  for (size_t i = 0; i < ow * oh; i++) { u1[i] = (uint16_t)(rnd() % 16500); f1[i] = (i % 3 == 0) ? SP[(i / 3) % NSP] * 1000.0f : (float)(rnd() % 16500); }
  for (size_t i = 0; i < ow * oh * 3; i++) { u3[i] = (uint16_t)rnd(); b3[i] = (uint8_t)rnd(); f3[i] = (i % 4 == 0) ? SP[(i / 4) % NSP] * 1000.0f : (float)(rnd() % 16500); }
  for (int k = 0; k < 2; k++) {
    const size_t x = crops[k][0], y = crops[k][1], w = crops[k][2], h = crops[k][3];
    float *o1 = exact(w * h * 4), *o4 = exact(w * h * 16);
    size_t sz[4];
    EXPECT(orc_size_image(y, ow - x - w, oh - y - h, x, ow, oh, sz) == 0 && sz[0] == x && sz[1] == y && sz[2] == w && sz[3] == h, "size_image");
    orc_gofloat_cfa_u16(u1, ow, x, y, w, h, 512.0f, 16383.0f, o1); fold_f(&S, o1, w * h); S.cases++;
    orc_gofloat_cfa_f32(f1, ow, x, y, w, h, 512.0f, 16383.0f, o1); fold_f(&S, o1, w * h); S.cases++;
    orc_gofloat_mono_u16(u1, ow, x, y, w, h, 512.0f, 16383.0f, o4); fold_f(&S, o4, w * h * 4); S.cases++;
    orc_gofloat_mono_f32(f1, ow, x, y, w, h, 512.0f, 16383.0f, o4); fold_f(&S, o4, w * h * 4); S.cases++;
    orc_gofloat_rgb_u16(u3, ow, x, y, w, h, b4, w4, o4); fold_f(&S, o4, w * h * 4); S.cases++;
    orc_gofloat_rgb_f32(f3, ow, x, y, w, h, b4, w4, o4); fold_f(&S, o4, w * h * 4); S.cases++;
    orc_gofloat_other_u8(b3, ow, x, y, w, h, o4); fold_f(&S, o4, w * h * 4); S.cases++;
    orc_gofloat_other_u16(u3, ow, x, y, w, h, o4); fold_f(&S, o4, w * h * 4); S.cases++;
    free(o1); free(o4);
  }
  free(u1); free(u3); free(b3); free(f1); free(f3);
  done(&S);
}

/* ---- the point-wise functions on the specials -------------------------------------------------------------------------------------------- */
static void sec_pointwise(void) {
  section S = sec("pointwise");
  const size_t n = NSP * NSP;                                              /* pixels: every pair of specials in the first two channels */
  float *in3 = exact(n * 12), *in4 = exact(n * 16), *o3 = exact(n * 12), *o4 = exact(n * 16);
  for (size_t i = 0; i < n; i++) {
    const float a = SP[i % NSP], b = SP[i / NSP], c = SP[(i * 7 + 3) % NSP], e = SP[(i * 11 + 5) % NSP];
    in3[3 * i] = a; in3[3 * i + 1] = b; in3[3 * i + 2] = c; in4[4 * i] = a; in4[4 * i + 1] = b; in4[4 * i + 2] = c; in4[4 * i + 3] = e;
  }
  float cm[12], m9[9]; cam_matrix(cm); orc_const_xyz_d65_33(m9);
  for (int which = 0; which < 3; which++) { orc_lookup(which, in3, o3, n * 3); fold_f(&S, o3, n * 3); S.cases++; }
  { uint8_t *q8 = exact(n * 3); uint16_t *q16 = exact(n * 6);
    orc_output8bit(in3, q8, n * 3); fold(&S, q8, n * 3); S.cases++;
    orc_output16bit(in3, q16, n * 3); fold(&S, q16, n * 6); S.cases++;
    orc_input8bit(q8, o3, n * 3); fold_f(&S, o3, n * 3); S.cases++;
    orc_input16bit(q16, o3, n * 3); fold_f(&S, o3, n * 3); S.cases++;
    free(q8); free(q16); }
  orc_xyz_to_lab(in3, o3, n); fold_f(&S, o3, n * 3); S.cases++;
  orc_lab_to_xyz(in3, o3, n); fold_f(&S, o3, n * 3); S.cases++;
  orc_camera_to_lab(WB, cm, in4, o3, n); fold_f(&S, o3, n * 3); S.cases++;
  orc_lab_to_rgb(m9, in3, o3, n); fold_f(&S, o3, n * 3); S.cases++;
  for (int mono = 0; mono < 2; mono++) { orc_tolab(in4, NSP, NSP, mono, WB, cm, o3); fold_f(&S, o3, n * 3); S.cases++; }
  orc_fromlab(in3, NSP, NSP, o3); fold_f(&S, o3, n * 3); S.cases++;
  { const float pts[6] = {0.25f, 0.2f, 0.5f, 0.6f, 0.75f, 0.8f};
    fold_i(&S, orc_basecurve(in3, NSP, NSP, 0.0f, pts, 0, o3)); S.cases++;                                  /* the early-out: out untouched */
    fold_i(&S, orc_basecurve(in3, NSP, NSP, 0.5f, pts, 3, o3)); fold_f(&S, o3, n * 3); S.cases++;
    fold_i(&S, orc_basecurve(in3, NSP, NSP, -1.0f, pts, 1, o3)); fold_f(&S, o3, n * 3); S.cases++; }
  fold_i(&S, orc_gamma(in3, NSP, NSP, 3, 1, o3)); S.cases++;
  fold_i(&S, orc_gamma(in3, NSP, NSP, 3, 0, o3)); fold_f(&S, o3, n * 3); S.cases++;
  fold_i(&S, orc_gamma(in4, NSP, NSP, 4, 0, o4)); fold_f(&S, o4, n * 4); S.cases++;
  for (size_t i = 0; i + 4 <= NSP; i += 3) { float o[4]; orc_normalize_wbs(SP + i, o); fold_f(&S, o, 4); S.cases++; }
  free(in3); free(in4); free(o3); free(o4);
  done(&S);
}

/* ---- curves with 0..64 knots -------------------------------------------------------------------------------------------------------------- */
static void sec_spline(void) {
  section S = sec("spline");
  for (int npts = 0; npts <= 64; npts++) for (int variant = 0; variant < 2; variant++) {
    float *pts = exact((size_t)npts * 8);
    for (int i = 0; i < npts; i++) {
      float x = ((float)i + 0.25f + 0.5f * unitf()) / (float)npts, y = unitf();
      if (variant == 1) { if (i == 0) x = y = 0.0f; if (i == npts - 1 && npts > 1) x = y = 1.0f; }
      pts[2 * i] = x; pts[2 * i + 1] = y;
    }
    const size_t cap = (size_t)npts + 2;
    float *px = exact(cap * 4), *py = exact(cap * 4), *c1 = exact(cap * 4), *c2 = exact(cap * 4), *c3 = exact(cap * 4), *out = exact(NSP * 4);
    const int k = orc_spline_new(pts, npts, px, py, c1, c2, c3);
    fold_i(&S, k);
    if (k >= 2) { EXPECT((size_t)k <= cap, "%d knots", k); fold_f(&S, px, (size_t)k); fold_f(&S, py, (size_t)k); fold_f(&S, c1, (size_t)k); fold_f(&S, c2, (size_t)k - 1); fold_f(&S, c3, (size_t)k - 1); }
    if (orc_spline_interpolate(pts, npts, SP, out, NSP) == 0) fold_f(&S, out, NSP);
    free(pts); free(px); free(py); free(c1); free(c2); free(c3); free(out);
    S.cases++;
  }
  done(&S);
}

/* ---- rotatecrop, the size negotiation and the orientation helpers, with NaN, negative and > 1 parameters ------------------------------------- */
static const float R9[9][5] = {{0.05f, 0.05f, 0.05f, 0.05f, 0}, {0.1f, 0.05f, 0.2f, 0, 0}, {0, 0, 0, 0, 0.04f}, {0.1f, 0, 0, 0, 0.2f}, {0, 0, 0, 0, 0.5f},
                               {0.02f, 0.03f, 0.01f, 0.02f, 0.77f}, {0, 0, 0, 0, 1.0f}, {0, 0, 0, 0, 1.3f}, {0.07f, 0.11f, 0.05f, 0.02f, 0.04f}};
static void sec_rotatecrop(void) {
  section S = sec("rotatecrop");
  const float bad[8][5] = {{NAN, 0, 0, 0, 0}, {0, 0, 0, 0, NAN}, {-0.5f, 0, 0, 0, 0.1f}, {1.5f, 0, 0, 0, 0}, {0.6f, 0.6f, 0.6f, 0.6f, 0}, {0, 2.0f, 0, -1.0f, 3.0f},
                           {INFINITY, 0, 0, 0, 0}, {0, 0, 0, 0, -INFINITY}};
  const size_t sizes[3][2] = {{47, 61}, {300, 20}, {6000, 4000}};
  for (int k = 0; k < 17; k++) for (int s = 0; s < 3; s++) for (int rev = 0; rev < 2; rev++) {
    const float *p = k < 9 ? R9[k] : bad[k - 9];
    size_t ow = 0, oh = 0;
    orc_rotatecrop_calc_size(p, (float)sizes[s][0] / (float)sizes[s][1], sizes[s][0], sizes[s][1], rev, &ow, &oh);
    fold_i(&S, (int64_t)ow); fold_i(&S, (int64_t)oh); S.cases++;
  }
  const size_t w = 24, h = 18;
  float *src = exact(w * h * 16); for (size_t i = 0; i < w * h * 4; i++) src[i] = (i % 6 == 0) ? SP[(i / 6) % NSP] : unitf();
  for (int k = 0; k < 17; k++) {
    const float *p = k < 9 ? R9[k] : bad[k - 9];
    size_t ow = 0, oh = 0, cw = 0, ch = 0; int64_t pts[6] = {0, 0, 0, 0, 0, 0};
    const int q = orc_rotatecrop_run(p, src, w, h, 4, NULL, &ow, &oh);     /* size query */
    fold_i(&S, q); fold_i(&S, (int64_t)ow); fold_i(&S, (int64_t)oh);
    if (q == 1 && ow * oh > 0 && ow * oh <= 4096) { float *out = exact(ow * oh * 16); fold_i(&S, orc_rotatecrop_run(p, src, w, h, 4, out, &ow, &oh)); fold_f(&S, out, ow * oh * 4); free(out); }
    if (orc_rotatecrop_corners(p, w, h, pts, &cw, &ch) == 1) { fold(&S, pts, sizeof pts); fold_i(&S, (int64_t)cw); fold_i(&S, (int64_t)ch); }
    S.cases++;
  }
  free(src);
  EXPECT(orc_selftest_rotatecrop_roundtrip_transform() == 0 && orc_selftest_rotatecrop_roundtrip_rotation() == 0, "the reference's round-trip loops fail"); S.cases += 2;
  float *s3 = exact(7 * 5 * 12), *o3 = exact(7 * 5 * 12); for (size_t i = 0; i < 7 * 5 * 3; i++) s3[i] = unitf();
  for (int o = 0; o < 9; o++) {
    int f[3], t[3]; size_t ow = 0, oh = 0, fw, fh;
    orc_orientation_to_flips(o, f); fold(&S, f, sizeof f); fold_i(&S, orc_orientation_from_flips(f[0], f[1], f[2]));
    orc_transform_new(o, t); fold(&S, t, sizeof t);
    if (t[0] >= 0 && t[0] <= 3) { fold_i(&S, orc_transform_orientation(t[0], t[1], t[2])); orc_transform_forward(t[0], 7, 5, &fw, &fh); fold_i(&S, (int64_t)fw); fold_i(&S, (int64_t)fh); }
    fold_i(&S, orc_rotate_buffer(s3, 7, 5, o, o3, &ow, &oh)); fold_i(&S, (int64_t)ow); fold_i(&S, (int64_t)oh);
    if (ow * oh == 35) fold_f(&S, o3, 105);
    S.cases++;
  }
  free(s3); free(o3);
  done(&S);
}

/* ---- the pipeline driver: a CFA, a mono, a three-sample and a raster source, whole and under a size limit ------------------------------------ */
static void sec_pipeline(void) {
  section S = sec("pipeline");
  EXPECT(orc_pipeline_sizeof() == sizeof(orc_pipeline), "orc_pipeline differs: %zu here, %zu in the oracle", sizeof(orc_pipeline), orc_pipeline_sizeof());
  const size_t w = 37, h = 29;
  uint16_t *u1 = exact(w * h * 2), *u3 = exact(w * h * 6); uint8_t *b3 = exact(w * h * 3);
  for (size_t i = 0; i < w * h; i++) u1[i] = (uint16_t)(rnd() % 16384);
  for (size_t i = 0; i < w * h * 3; i++) { u3[i] = (uint16_t)(rnd() % 16384); b3[i] = (uint8_t)rnd(); }
  const struct { int kind; const void *data; int cpp, is_cfa; const char *cfa; } src[4] = {{0, u1, 1, 1, "GRBG"}, {0, u1, 1, 0, ""}, {0, u3, 3, 0, ""}, {2, b3, 3, 0, ""}};
  for (int k = 0; k < 4; k++) for (int limited = 0; limited < 2; limited++) {
    orc_pipeline p; memset(&p, 0, sizeof p);
    p.source_kind = src[k].kind; p.data = src[k].data; p.width = w; p.height = h; p.cpp = src[k].cpp; p.is_cfa = src[k].is_cfa; strcpy(p.cfa, src[k].cfa);
    p.crop_top = 1; p.crop_left = 2;
    for (int i = 0; i < 4; i++) { p.blacklevels[i] = 512.0f; p.whitelevels[i] = 16383.0f; }
    memcpy(p.rc, R9[limited ? 3 : 0], sizeof p.rc);
    cam_matrix(p.cam_to_xyz_normalized); memcpy(p.wb_coeffs, WB, sizeof WB);
    p.exposure = 0.3f; p.npoints = 2; p.points[0] = 0.3f; p.points[1] = 0.25f; p.points[2] = 0.7f; p.points[3] = 0.8f;
    p.rotation = limited ? 1 : 0; p.fliph = limited; p.maxwidth = limited ? 20 : 0; p.use_fastpath = 1;
    size_t dw, dh, fw = 0, fh = 0, ow = 0, oh = 0;
    fold_i(&S, orc_pipeline_sizes(&p, &dw, &dh, &fw, &fh)); fold_i(&S, (int64_t)dw); fold_i(&S, (int64_t)dh); fold_i(&S, (int64_t)fw); fold_i(&S, (int64_t)fh);
    fold_i(&S, orc_pipeline_default_ops_other(&p));
    float *f = orc_pipeline_run(&p, &ow, &oh);
    EXPECT(f && ow == fw && oh == fh, "pipeline_run %d/%d: %zux%zu, negotiated %zux%zu", k, limited, ow, oh, fw, fh);
    if (f) { fold_f(&S, f, ow * oh * 3); orc_free(f); }
    uint8_t *q8 = orc_pipeline_output_8bit(&p, &ow, &oh); if (q8) { fold(&S, q8, ow * oh * 3); orc_free(q8); }
    uint16_t *q16 = orc_pipeline_output_16bit(&p, &ow, &oh); if (q16) { fold(&S, q16, ow * oh * 6); orc_free(q16); }
    EXPECT(q8 && q16, "quantised outputs");
    S.cases++;
  }
  /* the raster fast path: default ops on an RGB8 source */
  { orc_pipeline p; memset(&p, 0, sizeof p);
    p.source_kind = 2; p.data = b3; p.width = w; p.height = h; p.cpp = 3; p.use_fastpath = 1; p.maxwidth = 20;
    orc_const_srgb_d65_43(p.cam_to_xyz_normalized); p.wb_coeffs[0] = p.wb_coeffs[1] = p.wb_coeffs[2] = 1.0f;
    size_t ow = 0, oh = 0;
    fold_i(&S, orc_pipeline_default_ops_other(&p));
    uint8_t *q8 = orc_pipeline_output_8bit(&p, &ow, &oh); if (q8) { fold(&S, q8, ow * oh * 3); orc_free(q8); }
    uint16_t *q16 = orc_pipeline_output_16bit(&p, &ow, &oh); if (q16) { fold(&S, q16, ow * oh * 6); orc_free(q16); }
    EXPECT(q8 && q16, "fast path outputs");
    S.cases++; }
  free(u1); free(u3); free(b3);
  done(&S);
}

/* ---- constants, tables, CFA strings, sizes, temperatures ------------------------------------------------------------------------------------- */
static void sec_misc(void) {
  section S = sec("misc");
  orc_set_num_threads(orc_get_max_threads());                              /* the caller's OMP_NUM_THREADS stays in force */
  float m9[9], i9[9], m12[12];
  orc_const_srgb_d65_33(m9); fold_f(&S, m9, 9); orc_const_xyz_d65_33(i9); fold_f(&S, i9, 9); orc_const_srgb_d65_43(m12); fold_f(&S, m12, 12);
  orc_inverse33(i9, m9); fold_f(&S, m9, 9); S.cases += 4;
  orc_luts_init(); EXPECT(orc_lut_len() == 8193, "lut_len %d", orc_lut_len());
  for (int which = 0; which < 3; which++) { fold_f(&S, orc_lut_table(which), (size_t)orc_lut_len()); S.cases++; }
  const char *pats[10] = {"RGGB", "", XT, W12, "8x2:RGBGRBGGGBGRGRBG", "2x2:RGGB", "02x08:RGBGRBGGGBGRGRBG", "RGGBGRBGGBRGBGGR", "RGXB", "5x2:RGBGRGBGRG"};
  const int shifts[5][2] = {{0, 0}, {1, 0}, {5, 7}, {-1, -1}, {-49, 96}};
  for (int k = 0; k < 10; k++) {
    for (int s = 0; s < 5; s++) {
      char *out = exact(strlen(pats[k]) + 1);
      const int rc = orc_cfa_shift(pats[k], shifts[s][0], shifts[s][1], out);
      fold_i(&S, rc);
      if (rc == 0) { EXPECT(memchr(out, 0, strlen(pats[k]) + 1) != NULL, "'%s' shifted is longer than the pattern", pats[k]); fold(&S, out, strlen(out) + 1); }
      free(out); S.cases++;
    }
    int *p48 = exact(48 * 48 * sizeof(int));
    const int cw = orc_cfa_pattern(pats[k], p48); fold_i(&S, cw); if (cw > 0) fold(&S, p48, 48 * 48 * sizeof(int));
    free(p48); S.cases++;
  }
  const size_t zs[7] = {0, 1, 9, 10, 300, 6000, SIZE_MAX};
  for (int a = 0; a < 7; a++) for (int b = 0; b < 7; b++) {
    size_t o4[4] = {0, 0, 0, 0}, nw = 0, nh = 0; float scale = 0;
    fold_i(&S, orc_size_image(zs[a], zs[b], zs[(a + b) % 7], zs[(a * 3 + b) % 7], zs[(a + 3) % 7], zs[(b + 4) % 7], o4)); fold(&S, o4, sizeof o4);
    orc_calculate_scaling_total(zs[a] + 1 ? zs[a] + 1 : 1, zs[b] + 1 ? zs[b] + 1 : 1, zs[(a + b) % 7], zs[(a * 3 + b) % 7], &scale, &nw, &nh);
    fold_f(&S, &scale, 1); fold_i(&S, (int64_t)nw); fold_i(&S, (int64_t)nh);
    S.cases++;
  }
  const float temps[8] = {1000.0f, 2500.0f, 5003.0f, 6504.0f, 40000.0f, 0.0f, NAN, INFINITY};
  float x2c[12], c2x[12]; cam_matrix(c2x); for (int i = 0; i < 12; i++) x2c[i] = 0.1f + 0.07f * (float)i;
  for (int k = 0; k < 8; k++) {
    float xyz[3], tt[2], wb[4];
    orc_temp_to_xyz(temps[k], xyz); fold_f(&S, xyz, 3);
    orc_xyz_to_temp(xyz, tt); fold_f(&S, tt, 2);
    orc_tolab_set_temp(x2c, temps[k], k % 2 ? 1.1f : SP[k * 3], wb); fold_f(&S, wb, 4);
    orc_tolab_get_temp(c2x, wb, tt); fold_f(&S, tt, 2);
    S.cases++;
  }
  done(&S);
}

int main(int argc, char **argv) {
  if (argc < 2) { fprintf(stderr, "usage: oracle_surface <tests/golden/pin>\n"); return 2; }
  make_w12();
  sec_misc(); sec_demosaic(argv[1]); sec_transform(); sec_gofloat(); sec_pointwise(); sec_spline(); sec_rotatecrop(); sec_pipeline();
  if (g_fail) { fprintf(stderr, "%d contract failures\n", g_fail); return 1; }
  printf("ORACLE_SURFACE_OK\n");
  return 0;
}
