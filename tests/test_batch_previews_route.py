"""Batches of previews (no GPU): which descriptors ipk_pipeline_batches_previews sends to the route of IPK_FUSED_BATCH_PREVIEWS (allow_fused bit 8), the
chunk size and the kind of pass 1 it reports, and that the bit moves nothing else -- no size, no hash, no other report, no region plan -- over ten
sources x seven geometries of tests/test_switch_matrix_route.py's kind (rebuilt here: this module imports no helper of another test).  Every expectation
is written down from include/imagepipe_amd.h; sizes come from ipk_pipeline_sizes and are asserted, not trusted."""
import ctypes as C

import numpy as np
import pytest

import util

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
L16 = "8x2:RGBGRBGGGBGRGRBG"
ON, PLAIN_PREVIEWS, BATCH = 1, 128, 256
U16, F32, RGB8, RGB16 = 0, 1, 2, 3                                        # ipk_src_type
OUT_F32, OUT_U8, OUT_U16 = 0, 1, 2
MINSCALE = {2: 2.0, 6: 3.0, 8: 2.0, 12: 12.0}                             # src/ops/demosaic.rs:33-39 by the filter's width


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def make_desc(w, h, cfa="RGGB", crops=(0, 0, 0, 0), src_type=U16, cpp=1, is_cfa=None, allow_fused=ON | BATCH, **kw):
    """a descriptor of the synthetic camera (util), the reference's default curve, every flag off"""
    from imagepipe_amd._lib import PipelineDesc
    d = PipelineDesc()
    d.src_type, d.width, d.height, d.cpp = src_type, w, h, cpp
    d.is_cfa = int(bool(cfa)) if is_cfa is None else is_cfa
    d.cfa = cfa.encode()
    d.crop_top, d.crop_right, d.crop_bottom, d.crop_left = crops
    d.blacklevels[:] = [util.BLACK] * 4
    d.whitelevels[:] = [util.WHITE] * 4
    d.wb_coeffs[:] = util.WB
    d.cam_to_xyz_normalized[:] = [float(v) for v in util.cam_matrix().ravel()]
    d.npoints = 1
    d.points[0], d.points[1] = 0.5, 0.6
    d.allow_fused = allow_fused
    for k, v in kw.items():
        if k in ("rotatecrop", "blacklevels", "whitelevels"):
            getattr(d, k)[:] = v
        else:
            setattr(d, k, v)
    return d


def sizes(L, d):
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
    return tuple(v.value for v in a)


def report(L, d, n, out_type=OUT_U8):
    """(answer, chunk, pass1_batched)"""
    chunk, p1 = C.c_size_t(77), C.c_int(77)
    rc = L.ipk_pipeline_batches_previews(C.byref(d), out_type, n, C.byref(chunk), C.byref(p1))
    return rc, chunk.value, p1.value


def cropped(d):
    return d.width - d.crop_left - d.crop_right, d.height - d.crop_top - d.crop_bottom


def general_kernel(w, h, nw, nh, plain=False):
    """the launcher's rule for the general kernel on a 16-byte aligned destination (include/imagepipe_amd.h, ipk_raw_scaled_demosaic_batch): a skip above 7
    or below 1, a frame under 8 samples wide, every plain layout -- with the f32 skips of src/scaling.rs:69-72"""
    f = np.float32
    sx, sy = (f(w - 1) - f(0)) / f(nw - 1), (f(h - 1) - f(0)) / f(nh - 1)
    return bool(plain or not (1.0 <= sx <= 7.0 and 1.0 <= sy <= 7.0 and w >= 8))


def chunk_of(dw, dh):
    return min(64, max(1, (256 << 20) // (dw * dh * 16)))


# ---------------------------------------------------------------------------------------------
# admission
# ---------------------------------------------------------------------------------------------
def thumb(**kw):
    """the GPU module's mosaic: 211x157 u16 RGGB, sensor crops (2, 3, 4, 5) -> 203x151, under maxwidth 23 -> 23x17"""
    args = dict(crops=(2, 3, 4, 5), maxwidth=23)
    args.update(kw)
    return make_desc(211, 157, "RGGB", **args)


def test_the_thumbnail_is_taken(L):
    d = thumb()
    assert sizes(L, d) == (23, 17, 23, 17) and cropped(d) == (203, 151)
    assert general_kernel(203, 151, 23, 17)
    for out_type in (OUT_F32, OUT_U8, OUT_U16):
        for n in (2, 3, 64, 65, 1000):
            assert report(L, d, n, out_type) == (1, 64, 1), (out_type, n)
    # the outputs are optional
    assert L.ipk_pipeline_batches_previews(C.byref(d), OUT_U8, 2, None, None) == 1
    assert L.ipk_pipeline_batches_previews(None, OUT_U8, 2, None, None) < 0


def test_refusals(L):
    """n <= 1, an active rotatecrop, each non-Normal orientation, a preview under 256 pixels, scale < minscale: 0, with chunk and pass1_batched zeroed"""
    no = (0, 0, 0)
    for n in (0, 1):
        assert report(L, thumb(), n) == no, n
    for rc in ((0.1, 0.05, 0.08, 0.12, 0.0), (0.0, 0.0, 0.0, 0.0, 0.03)):
        assert report(L, thumb(rotatecrop=[float(np.float32(v)) for v in rc]), 4) == no, rc
    seen = set()
    for rotation in range(4):
        for fliph in (0, 1):
            for flipv in (0, 1):
                ori = L.ipk_transform_orientation(rotation, fliph, flipv)
                seen.add(ori)
                got = report(L, thumb(rotation=rotation, fliph=fliph, flipv=flipv, maxwidth=23, maxheight=23), 4)
                assert (got[0] == 1) == (ori == 0), (rotation, fliph, flipv, ori, got)
                assert got == no or got[1:] == (64, 1)
    assert seen == set(range(8)), seen                                      # Normal and the seven others
    d = thumb(maxwidth=15)
    dw, dh = sizes(L, d)[:2]
    assert dw * dh < 256 and report(L, d, 4) == no, (dw, dh)
    d = thumb(maxwidth=19)                                                  # the floor is >=: 19 x 14 = 266 is in
    dw, dh = sizes(L, d)[:2]
    assert dw * dh >= 256 and report(L, d, 4)[0] == 1, (dw, dh)
    for mw in (0, 203, 150, 110):                                           # no scaling; scale 1.35 and 1.85 < minscale 2 (demosaic::full + scale_down_opbuf)
        assert report(L, thumb(maxwidth=mw), 4) == no, mw
    assert report(L, make_desc(300, 240, XT, maxwidth=120), 4) == no        # X-Trans at 2.5 < 3
    assert report(L, make_desc(300, 240, XT, maxwidth=100), 4)[0] == 1      # and at 3.0


def test_plain_raws_need_bit_7(L):
    for cpp, src_type in ((1, U16), (1, F32), (3, U16), (3, F32)):
        kw = dict(cfa="", cpp=cpp, src_type=src_type, is_cfa=0, maxwidth=30)
        assert report(L, make_desc(131, 113, **kw), 4) == (0, 0, 0), (cpp, src_type)
        d = make_desc(131, 113, allow_fused=ON | BATCH | PLAIN_PREVIEWS, **kw)
        dw, dh = sizes(L, d)[:2]
        assert report(L, d, 4) == (1, chunk_of(dw, dh), 1), (cpp, src_type)


def test_rasters(L):
    """a raster under a size limit is taken, pass 1 a launch per frame (the raster scaler has no batch form); on the fast path nothing changes"""
    for src_type in (RGB8, RGB16):
        d = make_desc(131, 113, "", src_type=src_type, cpp=3, is_cfa=0, exposure=0.25, maxwidth=40)
        dw, dh = sizes(L, d)[:2]
        assert report(L, d, 4) == (1, chunk_of(dw, dh), 0), src_type
    from imagepipe_amd._lib import PipelineDesc
    d = PipelineDesc()                                                      # Pipeline::default_ops of a raster: the fast path under output_8bit
    d.src_type, d.width, d.height, d.cpp, d.maxwidth, d.use_fastpath, d.allow_fused = RGB8, 131, 113, 3, 40, 1, ON | BATCH
    d.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    m = (C.c_float * 12)()
    assert L.ipk_const_matrix(2, m) == 0                                    # SRGB_D65_43
    d.cam_to_xyz_normalized[:] = list(m)
    assert L.ipk_pipeline_takes_fastpath(C.byref(d), OUT_U8) == 1
    assert report(L, d, 4, OUT_U8) == (0, 0, 0)
    assert L.ipk_pipeline_takes_fastpath(C.byref(d), OUT_F32) == 0 and report(L, d, 4, OUT_F32)[0] == 1    # run() has no fast path


# (width, height, filter, maxwidth): skips of 9.2; 4.0 (X-Trans, the GPU module's per-frame case); exactly 7.0 in x; just above 7; 2.0
SHAPES = [(203, 151, "RGGB", 23), (300, 200, XT, 75), (701, 470, "RGGB", 101), (711, 470, "RGGB", 101), (2048, 1366, "RGGB", 1024),
          (300, 240, XT, 30), (150, 100, XT, 30)]


def test_pass1_follows_the_launchers_rule(L):
    outcomes = set()
    for w, h, cfa, mw in SHAPES:
        d = make_desc(w, h, cfa, maxwidth=mw)
        dw, dh = sizes(L, d)[:2]
        got = report(L, d, 4)
        if dw * dh < 256:
            assert got == (0, 0, 0), (w, h, mw)
            continue
        want = general_kernel(w, h, dw, dh)
        assert got == (1, chunk_of(dw, dh), int(want)), (w, h, cfa, mw, dw, dh, got)
        outcomes.add(want)
    assert outcomes == {True, False}
    f = np.float32
    assert float((f(700) - f(0)) / f(100)) == 7.0 and float((f(710) - f(0)) / f(100)) > 7.0


def test_chunk_follows_the_formula(L):
    cases = [(make_desc(8640, 5760, XT, maxwidth=2160), (2160, 1440), 5), (make_desc(2048, 1366, "RGGB", maxwidth=1024), (1024, 683), 23),
             (thumb(), (23, 17), 64)]
    for d, want_size, want_chunk in cases:
        assert sizes(L, d)[:2] == want_size
        assert chunk_of(*want_size) == want_chunk
        got = report(L, d, 100)
        assert got[0] == 1 and got[1] == want_chunk, (want_size, got)


# ---------------------------------------------------------------------------------------------
# the bit moves nothing else: ten sources x seven geometries
# ---------------------------------------------------------------------------------------------
W, H = 131, 113
# name -> (filter, cpp, src_type)
SOURCES = {"mono_u16": ("", 1, U16), "mono_f32": ("", 1, F32), "rgb3_u16": ("", 3, U16), "rgb3_f32": ("", 3, F32), "bayer": ("GRBG", 1, U16),
           "xtrans": (XT, 1, F32), "rgbe": ("RGBE", 1, U16), "l16": (L16, 1, U16), "rgb8": ("", 3, RGB8), "rgb16": ("", 3, RGB16)}
ANGLE = lambda a: (0.0, 0.0, 0.0, 0.0, a)
SENSOR_CROPS = (3, 2, 1, 5)
# name -> (sensor crops, rotatecrop, branch of OpDemosaic: scale <= 1, 1 < scale < minscale, scale >= minscale); odd-numbered ones are transposed
GEOMETRIES = [("G0", (0, 0, 0, 0), None, "le1"), ("G1", SENSOR_CROPS, (0.1, 0.05, 0.08, 0.12, 0.0), "le1"), ("G2", (0, 0, 0, 0), ANGLE(0.03), "le1"),
              ("G3", (0, 0, 0, 0), None, "mid"), ("G4", (0, 0, 0, 0), None, "ge"), ("G5", (0, 0, 0, 0), ANGLE(0.03), "mid"),
              ("G6", SENSOR_CROPS, ANGLE(0.3), "ge")]
REPORTS = ["takes_fastpath", "fuses_rotatecrop", "fuses_scaledown", "fuses_four_colour", "windows_preview", "fuses_plain", "scales_plain",
           "fuses_scaled_rotatecrop", "resamples_cached_region"]


def cfa_width(cfa):
    return int(cfa.split("x")[0]) if ":" in cfa else {0: 2, 4: 2, 36: 6, 144: 12}[len(cfa)]


def scale_of(L, d):
    dw, dh = sizes(L, d)[:2]
    s, nw, nh = C.c_float(), C.c_size_t(), C.c_size_t()
    cw, ch = cropped(d)
    assert L.ipk_calculate_scaling_total(cw, ch, dw, dh, C.byref(s), C.byref(nw), C.byref(nh)) == 0
    return s.value


def case_desc(L, name, j):
    cfa, cpp, src_type = SOURCES[name]
    _, crops, rc, branch = GEOMETRIES[j]
    kw = {}
    if rc is not None:
        kw["rotatecrop"] = [float(np.float32(v)) for v in rc]
    if j % 2:
        kw.update(rotation=1, fliph=1)
    if src_type in (RGB8, RGB16):
        kw["exposure"] = 0.25                                               # not the default ops: no fast path
    shifted = cfa
    if cfa:
        out = C.create_string_buffer(160)
        assert L.ipk_cfa_shift(cfa.encode(), crops[3], crops[0], out) == 0
        shifted = out.value.decode()
    d = make_desc(W, H, shifted, crops, src_type=src_type, cpp=cpp, is_cfa=int(bool(cfa)), allow_fused=0, **kw)
    if branch != "le1":
        ms = MINSCALE[cfa_width(cfa)]
        lo, hi = (1.0, ms) if branch == "mid" else (ms, ms * 4)
        target = (lo + hi) / 2 if branch == "mid" else ms + 0.6
        fw = sizes(L, d)[2]
        for mw in sorted(range(2, fw), key=lambda m: abs(fw / m - target)):
            d.maxwidth = mw
            if lo < scale_of(L, d) < hi or (branch == "ge" and scale_of(L, d) == lo):
                break
        else:
            raise AssertionError("no maxwidth reaches the %s branch" % branch)
    return d


def popcount(v):
    return bin(v).count("1")


# the masks of bits 0..7 with at most two bits set or at most two clear: every pair of older switches, both ways; the two flags both off and both on
MASKS = [m for m in range(256) if popcount(m) <= 2 or popcount(m) >= 6]
FLAGS = [(0, 0), (1, 1)]


def everything_else(L, d, out_type, regions):
    row = [getattr(L, "ipk_pipeline_" + r)(C.byref(d), out_type) for r in REPORTS]
    row.append(sizes(L, d))
    for t in (0, 1, 2):
        buf = C.create_string_buffer(256)
        row.append((L.ipk_pipeline_hashes(C.byref(d), t, 5, buf), buf.raw))
    for reg in regions:
        s = [C.c_size_t(0) for _ in range(4)]
        row.append((L.ipk_pipeline_region(C.byref(d), out_type, *reg, *[C.byref(v) for v in s]),) + tuple(v.value for v in s))
    return row


def expected_taken(L, d, name):
    """the header's conditions, from the descriptor and ipk_pipeline_sizes, for a mask that has bits 0 and 8"""
    cfa, cpp, src_type = SOURCES[name]
    dw, dh = sizes(L, d)[:2]
    if any(d.rotatecrop[k] != 0.0 for k in range(5)) or L.ipk_transform_orientation(d.rotation, d.fliph, d.flipv) != 0 or dw * dh < 256:
        return False
    s = scale_of(L, d)
    if src_type in (RGB8, RGB16):
        return s > 1.0
    if not cfa:
        return bool(d.allow_fused & PLAIN_PREVIEWS) and s > 1.0
    return s >= MINSCALE[cfa_width(cfa)]


@pytest.mark.parametrize("name", list(SOURCES))
def test_bit_8_moves_nothing_else(L, name):
    taken = 0
    for j in range(len(GEOMETRIES)):
        d = case_desc(L, name, j)
        out_type = (list(SOURCES).index(name) + j) % 3
        fw, fh = sizes(L, d)[2:]
        bw = min(fw, 20)
        bh = -(-256 // bw)
        regions = [(5, 3, min(13, fw - 7), min(9, fh - 5)), (fw - bw, fh - bh, bw, bh)]
        for fr, fs in FLAGS:
            d.fuse_rotatecrop, d.fuse_scaledown = fr, fs
            for m in MASKS:
                d.allow_fused = m
                before = everything_else(L, d, out_type, regions)
                assert report(L, d, 4, out_type) == (0, 0, 0), (name, j, m)          # without bit 8: never
                if not m & ON:
                    # without bit 0 the new bit is what bits 3, 4 and 7 are: a non-zero value, so "on" for every older route -- with bits 1 and 2, which
                    # count without bit 0, and without bits 3..7, which do not
                    d.allow_fused = ON | (m & 6)
                    before = everything_else(L, d, out_type, regions)
                d.allow_fused = m | BATCH
                assert everything_else(L, d, out_type, regions) == before, (name, GEOMETRIES[j][0], m, fr, fs)
                got = report(L, d, 4, out_type)
                if not m & ON:
                    assert got == (0, 0, 0), (name, j, m)                            # bit 8 counts beside bit 0 only
                else:
                    want = expected_taken(L, d, name)
                    assert got[0] == int(want), (name, GEOMETRIES[j][0], m, got)
                    taken += want
                    if want:
                        dw, dh = sizes(L, d)[:2]
                        plain = not SOURCES[name][0]
                        raster = SOURCES[name][2] in (RGB8, RGB16)
                        assert got[1:] == (chunk_of(dw, dh), int(not raster and general_kernel(*cropped(d), dw, dh, plain))), (name, j, m, got)
    assert taken, name + ": no geometry of this source is taken under any mask"
