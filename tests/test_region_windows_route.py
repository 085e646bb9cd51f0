"""Regions of the one-launch rotatecrop and scaledown routes as a window of that launch (no GPU): which descriptors ipk_pipeline_region sends there
under IPK_FUSED_WINDOW_REGIONS (bit 2 of allow_fused), that nothing else depends on the bit, and the sensor footprint the window launch reports
(ipk_transform_window_footprint) against a numpy-float32 restatement of the reference's window expressions (src/scaling.rs:77-87) over EVERY pixel
of the window.

What "the exact box" is here.  Output pixel (row, col) reads the taps from_x ..= to_x by from_y ..= to_y; a pixel whose from exceeds its to (a
negative skip, or an angle near a right one) has no tap.  The launch, however, stages per tile the box [min from, max to] of its pixels' window ENDS
(rs_box in ipk_kernels.hip), whether or not the individual windows are empty, so the footprint is measured against that box: x from the smallest
from_x to the largest to_x over all pixels of the window, likewise y, empty when the largest to lies below the smallest from (no pixel can have a tap
then), plus demosaic::full's one-pixel halo clipped to the frame.  It contains the union of the taps actually read, which is asserted too."""
import ctypes as C

import numpy as np
import pytest

import util
import test_rotatecrop_route as rr
import test_scaledown_route as sr
from test_rotatecrop_route import R9, XT, W12, SENSOR_CROPS, INVALID

WIN = 4                                                                   # IPK_FUSED_WINDOW_REGIONS
NOCROP = (0, 0, 0, 0)
R9_IDS = ["crop5", "crop-uneven", "rot.04", "rot.2", "rot.5", "rot.77", "rot1.0", "rot1.3", "crop+rot.04"]
# the taken descriptors of the two route tests: (name, builder, width, height, sensor crops, keywords)
TAKEN = [("rc-96x120c-%s" % R9_IDS[k], rr._desc, 96, 120, SENSOR_CROPS, dict(rotatecrop=R9[k])) for k in range(len(R9))] + \
        [("rc-47x61-%s" % R9_IDS[k], rr._desc, 47, 61, NOCROP, dict(rotatecrop=R9[k])) for k in range(len(R9))] + \
        [("sd-131x97@87", sr._desc, 131, 97, NOCROP, dict(maxwidth=87)), ("sd-101x103@51", sr._desc, 101, 103, NOCROP, dict(maxwidth=51))]


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _region(L, d, x, y, w, h, out_type=0):
    s = [C.c_size_t(12345) for _ in range(4)]
    rc = L.ipk_pipeline_region(C.byref(d), out_type, x, y, w, h, *[C.byref(v) for v in s])
    return rc, tuple(v.value for v in s)


def _footprint(L, W, H, corners, window):
    tl, tr, bl, nw, nh = corners
    out = (C.c_size_t * 4)()
    rc = L.ipk_transform_window_footprint(W, H, tl[0], tl[1], tr[0], tr[1], bl[0], bl[1], nw, nh, *window, out)
    assert rc == 0, (rc, L.ipk_last_error())
    return tuple(out)


def _windows_of(nw, nh):
    """the issue's windows: one pixel at each corner, (3, 5, 17, 9) (cut to the image where it is smaller), a full row, a full column, the image"""
    w17 = (min(3, nw - 1), min(5, nh - 1), min(17, nw - min(3, nw - 1)), min(9, nh - min(5, nh - 1)))
    return [(0, 0, 1, 1), (nw - 1, 0, 1, 1), (0, nh - 1, 1, 1), (nw - 1, nh - 1, 1, 1), w17, (0, nh // 2, nw, 1), (nw // 3, 0, 1, nh), (0, 0, nw, nh)]


def _usize(v):
    """Rust's `f32 as usize`: NaN and negative values give 0, large ones saturate"""
    return np.where(v > 0, np.minimum(v, np.float32(2 ** 40)), np.float32(0)).astype(np.int64)


def _pixel_windows(W, H, corners):
    """scaling.rs:69-72 and :77-87 in numpy float32, every operation rounded on its own: (from_x, to_x, from_y, to_y), each nheight x nwidth"""
    tl, tr, bl, nw, nh = corners
    f = np.float32
    with np.errstate(all="ignore"):
        sxx, sxy = (f(tr[0]) - f(tl[0])) / f(nw - 1), (f(tr[1]) - f(tl[1])) / f(nw - 1)
        syx, syy = (f(bl[0]) - f(tl[0])) / f(nh - 1), (f(bl[1]) - f(tl[1])) / f(nh - 1)
        row, col = np.arange(nh, dtype=f)[:, None], np.arange(nw, dtype=f)[None, :]
        row1, col1 = np.arange(1, nh + 1, dtype=f)[:, None], np.arange(1, nw + 1, dtype=f)[None, :]
        from_x, to_x = f(tl[0]) + syx * row, f(tl[0]) + syx * row1
        from_y, to_y = f(tl[1]) + syy * row, f(tl[1]) + syy * row1
        for a in (from_x, to_x, from_y, to_y, sxx * col):
            assert a.dtype == np.float32
        fx = np.minimum(W - 1, _usize(np.floor(from_x + (sxx * col))))
        tx = np.minimum(W - 1, _usize(np.floor(to_x + (sxx * col1))))
        fy = np.minimum(H - 1, _usize(np.floor(from_y + (sxy * col))))
        ty = np.minimum(H - 1, _usize(np.floor(to_y + (sxy * col1))))
    return fx, tx, fy, ty


def _check_footprints(L, W, H, corners, tag):
    tl, tr, bl, nw, nh = corners
    fx, tx, fy, ty = _pixel_windows(W, H, corners)
    seen_empty = seen_full = False
    for win in _windows_of(nw, nh):
        wx, wy, ww, wh = win
        sl = (slice(wy, wy + wh), slice(wx, wx + ww))
        x0, x1, y0, y1 = int(fx[sl].min()), int(tx[sl].max()), int(fy[sl].min()), int(ty[sl].max())
        gx, gy, gw, gh = _footprint(L, W, H, corners, win)
        assert (gw == 0) == (gh == 0), (tag, win)
        assert gx + gw <= W and gy + gh <= H, "%s %r: the footprint %r leaves the %dx%d frame" % (tag, win, (gx, gy, gw, gh), W, H)
        # the taps actually read (pixels whose window is not empty), with the halo
        has = (fx[sl] <= tx[sl]) & (fy[sl] <= ty[sl])
        if has.any():
            ux0, ux1 = int(fx[sl][has].min()), int(tx[sl][has].max())
            uy0, uy1 = int(fy[sl][has].min()), int(ty[sl][has].max())
            assert gw > 0 and gx <= max(ux0 - 1, 0) and gx + gw - 1 >= min(ux1 + 1, W - 1) and gy <= max(uy0 - 1, 0) and gy + gh - 1 >= min(uy1 + 1, H - 1), \
                "%s %r: the footprint %r misses taps of [%d, %d] x [%d, %d] or their halo" % (tag, win, (gx, gy, gw, gh), ux0, ux1, uy0, uy1)
        if x1 < x0 or y1 < y0:
            assert not has.any()
            assert (gw, gh) == (0, 0), "%s %r: no window end lies past a window start, yet the footprint is %r" % (tag, win, (gx, gy, gw, gh))
            seen_empty = True
            continue
        ex0, ex1, ey0, ey1 = max(x0 - 1, 0), min(x1 + 1, W - 1), max(y0 - 1, 0), min(y1 + 1, H - 1)    # the exact box and its halo
        assert gw > 0 and gx <= ex0 and gx + gw - 1 >= ex1 and gy <= ey0 and gy + gh - 1 >= ey1, \
            "%s %r: the footprint %r does not contain [%d, %d] x [%d, %d]" % (tag, win, (gx, gy, gw, gh), ex0, ex1, ey0, ey1)
        assert ex0 - gx <= 2 and gx + gw - 1 - ex1 <= 2 and ey0 - gy <= 2 and gy + gh - 1 - ey1 <= 2, \
            "%s %r: the footprint %r exceeds [%d, %d] x [%d, %d] by more than 2" % (tag, win, (gx, gy, gw, gh), ex0, ex1, ey0, ey1)
        seen_full = True
    return seen_empty, seen_full


# ---------------------------------------------------------------------------------------------
# the footprint helper
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", range(len(R9)), ids=R9_IDS)
def test_footprint_of_the_r9_transforms(L, orc, k):
    for w, h, crops in ((96, 120, SENSOR_CROPS), (47, 61, NOCROP)):
        _, _, cw, ch = orc.size_image(*crops, w, h)
        corners = orc.rotatecrop_corners(R9[k], cw, ch)
        assert corners is not None
        _, full = _check_footprints(L, cw, ch, corners, "%s %dx%d" % (R9_IDS[k], cw, ch))
        assert full


@pytest.mark.parametrize("name,corners", [
    ("outside", ((-4, -3), (58, 5), (-9, 49), 57, 44)), ("narrow", ((5, 40), (6, 39), (30, 44), 2, 31)),
    ("mirror", ((50, 3), (4, 3), (50, 40), 47, 38)), ("flat", ((3, 7), (3, 7), (3, 7), 9, 6))], ids=["outside", "narrow", "mirror", "flat"])
def test_footprint_of_clamped_and_degenerate_transforms(L, name, corners):
    _check_footprints(L, 61, 47, corners, name)


def test_footprint_is_empty_where_no_window_has_a_tap(L):
    """a mirrored single column: every to_x lies left of its from_x"""
    corners = ((50, 3), (4, 3), (50, 40), 47, 38)
    fx, tx, _, _ = _pixel_windows(61, 47, corners)
    assert (tx[:, 7] < fx[:, 7]).all()
    assert _footprint(L, 61, 47, corners, (7, 0, 1, 38)) == (0, 0, 0, 0)
    assert _footprint(L, 61, 47, corners, (7, 5, 1, 1)) == (0, 0, 0, 0)


@pytest.mark.parametrize("case", ["131x97@87", "101x103@51", "150x100xt@60"])
def test_footprint_of_the_scaled_form(L, orc, case):
    """skips 1.5, 2.0 and 2.53 with scale_down_opbuf's corners (0, 0), (width - 1, 0), (0, height - 1)"""
    w, h, crops, mw, mh, _ = sr.SMALL_TAKEN[case]
    _, sx, sy, dw, dh = sr._negotiated(orc, w, h, crops, mw, mh)
    assert {"131x97@87": 1.5 < sx < 1.52, "101x103@51": sx == 2.0 and sy == 2.0, "150x100xt@60": 2.5 < sx < 2.56}[case]
    empty, full = _check_footprints(L, w, h, ((0, 0), (w - 1, 0), (0, h - 1), dw, dh), case)
    assert full and not empty


def test_footprint_refusals(L):
    out = (C.c_size_t * 4)(7, 7, 7, 7)
    fp = lambda *a: L.ipk_transform_window_footprint(61, 47, 0, 0, 60, 0, 0, 46, *a)
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (40, 0, 2, 1), (0, 30, 1, 2), (41, 0, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        assert fp(41, 31, *win, out) == INVALID, win
    assert fp(41, 31, 0, 0, 1, 1, None) == INVALID
    assert fp(1, 31, 0, 0, 1, 1, out) == -5 and fp(41, 1, 0, 0, 1, 1, out) == -5        # IPK_ERR_UNSUPPORTED: output sides below 2
    assert tuple(out) == (7, 7, 7, 7)
    assert fp(41, 31, 40, 30, 1, 1, out) == 0 and tuple(out) != (7, 7, 7, 7)


# ---------------------------------------------------------------------------------------------
# the route report
# ---------------------------------------------------------------------------------------------
def _expected_corners(orc, name, w, h, crops, kw):
    _, _, cw, ch = orc.size_image(*crops, w, h)
    if name.startswith("rc-"):
        return cw, ch, orc.rotatecrop_corners(kw["rotatecrop"], cw, ch)
    _, _, _, dw, dh = sr._negotiated(orc, w, h, crops, kw.get("maxwidth", 0), kw.get("maxheight", 0))
    return cw, ch, ((0, 0), (cw - 1, 0), (0, ch - 1), dw, dh)


@pytest.mark.parametrize("case", TAKEN, ids=[c[0] for c in TAKEN])
def test_taken_descriptors_are_windowed_with_the_bit_only(L, orc, case):
    name, build, w, h, crops, kw = case
    x0, y0, cw, ch = orc.size_image(*crops, w, h)
    cw, ch, corners = _expected_corners(orc, name, w, h, crops, kw)
    nw, nh = corners[3], corners[4]
    for cfa, src_type, out_type in (("RGGB", 0, 0), ("RGGB", 1, 1), (XT, 0, 2), (XT, 1, 0)):
        d0, d1 = build(w, h, cfa, crops, src_type=src_type, **kw), build(w, h, cfa, crops, src_type=src_type, **kw)
        d1.allow_fused = 1 | WIN
        a = [C.c_size_t() for _ in range(4)]
        assert L.ipk_pipeline_sizes(C.byref(d1), *[C.byref(v) for v in a]) == 0 and (a[2].value, a[3].value) == (nw, nh), name
        for fuses in (L.ipk_pipeline_fuses_rotatecrop, L.ipk_pipeline_fuses_scaledown, L.ipk_pipeline_fuses_four_colour):
            assert fuses(C.byref(d0), out_type) == fuses(C.byref(d1), out_type)
        assert (L.ipk_pipeline_fuses_rotatecrop if name.startswith("rc-") else L.ipk_pipeline_fuses_scaledown)(C.byref(d1), out_type) == 1
        for win in _windows_of(nw, nh):
            assert _region(L, d0, *win, out_type) == (0, (x0, y0, cw, ch)), "%s %r: without the bit the route is 0 and the window the crop window" % (name, win)
            gx, gy, gw, gh = _footprint(L, cw, ch, corners, win)
            assert _region(L, d1, *win, out_type) == (1, (x0 + gx, y0 + gy, gw, gh)), "%s %r" % (name, win)
        # the hashes do not see the bit
        ha, hb = C.create_string_buffer(256), C.create_string_buffer(256)
        assert L.ipk_pipeline_hashes(C.byref(d0), out_type, 5, ha) == 0 and L.ipk_pipeline_hashes(C.byref(d1), out_type, 5, hb) == 0
        assert ha.raw == hb.raw


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (0, 1)])
def test_every_orientation_is_windowed(L, orc, rot, fh):
    """the region is mapped back through OpTransform: still route 1, and a one-pixel region at a corner of the result comes from a corner of the
    resampled image -- its footprint is one of the four corner footprints"""
    w, h, crops, rc = 96, 120, SENSOR_CROPS, R9[3]
    d = rr._desc(w, h, "GRBG", crops, rotatecrop=rc, rotation=rot, fliph=fh)
    d.allow_fused = 1 | WIN
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
    fw, fhh = a[2].value, a[3].value
    x0, y0, cw, ch = orc.size_image(*crops, w, h)
    corners = orc.rotatecrop_corners(rc, cw, ch)
    nw, nh = corners[3], corners[4]
    assert {fw, fhh} == {nw, nh}
    corner_fps = {(x0 + f[0], y0 + f[1], f[2], f[3]) for f in (_footprint(L, cw, ch, corners, win) for win in _windows_of(nw, nh)[:4])}
    for x, y in ((0, 0), (fw - 1, 0), (0, fhh - 1), (fw - 1, fhh - 1)):
        route, fp = _region(L, d, x, y, 1, 1)
        assert route == 1 and fp in corner_fps, (x, y, fp)
    whole = _footprint(L, cw, ch, corners, (0, 0, nw, nh))
    assert _region(L, d, 0, 0, fw, fhh) == (1, (x0 + whole[0], y0 + whole[1], whole[2], whole[3]))


def test_plain_fused_frames_answer_the_same_with_and_without_the_bit(L):
    for cfa, crops in (("RGGB", NOCROP), (XT, SENSOR_CROPS)):
        d0, d1 = rr._desc(96, 120, cfa, crops), rr._desc(96, 120, cfa, crops)
        d1.allow_fused = 1 | WIN
        for win in ((0, 0, 1, 1), (3, 5, 17, 9), (0, 7, 90, 1), (0, 0, 90, 115)):
            a, b = _region(L, d0, *win), _region(L, d1, *win)
            assert a == b and a[0] == 1, (cfa[:6], win, a, b)


def test_refused_descriptors_stay_whole_frame_with_the_bit(L, orc):
    rc = R9[3]
    x0, y0, cw, ch = orc.size_image(*NOCROP, 47, 61)
    cases = [rr._desc(47, 61, "RGBE", rotatecrop=rc),                                       # a fourth colour
             rr._desc(47, 61, rotatecrop=rc, fuse=0),                                       # fuse_rotatecrop = 0
             rr._desc(47, 61, rotatecrop=rc, maxwidth=20),                                  # rotatecrop under a scaling demosaic
             rr._desc(47, 61, rotatecrop=rc, maxwidth=20, fuse_scaledown=1),
             sr._desc(131, 97, maxwidth=87, fuse=0),                                        # fuse_scaledown = 0
             sr._desc(131, 97, "RGBE", maxwidth=87),
             sr._desc(131, 97, maxwidth=80, rotatecrop=R9[0], fuse_rotatecrop=1),           # the same, from the other side
             sr._desc(131, 97, maxwidth=40)]                                                # the scaled_demosaic preview branch
    for i, d in enumerate(cases):
        d.allow_fused = 1 | WIN
        route, fp = _region(L, d, 0, 0, 2, 2)
        assert route == 0, i
        assert fp == ((0, 0, 47, 61) if d.width == 47 else (0, 0, 131, 97)), (i, fp)
    d = rr._desc(47, 61, rotatecrop=rc, allow_fused=0)
    assert _region(L, d, 0, 0, 2, 2)[0] == 0


def test_invalid_regions(L, orc):
    for d in (rr._desc(47, 61, rotatecrop=R9[3]), sr._desc(131, 97, maxwidth=87)):
        d.allow_fused = 1 | WIN
        a = [C.c_size_t() for _ in range(4)]
        assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
        fw, fh = a[2].value, a[3].value
        assert _region(L, d, 0, 0, fw, fh)[0] == 1
        for win in ((0, 0, 0, 1), (0, 0, 1, 0), (fw - 1, 0, 2, 1), (0, fh - 1, 1, 2), (fw, 0, 1, 1), (0, fh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
            rc, fp = _region(L, d, *win)
            assert rc == INVALID and fp == (12345,) * 4, (win, rc, fp)
        assert _region(L, d, 0, 0, 1, 1, out_type=3)[0] == INVALID


def test_bindings_carry_the_bit():
    import inspect
    import imagepipe_amd
    from imagepipe_amd import _lib
    assert _lib.FUSED_WINDOW_REGIONS == WIN
    src = inspect.getsource(imagepipe_amd.Pipeline)
    assert "self.window_regions = False" in src and "d.allow_fused |= _lib.FUSED_WINDOW_REGIONS" in src
    for name in ("raw_to_srgb_resampled_window", "raw_to_srgb_scaled_window", "transform_window_footprint"):
        assert callable(getattr(imagepipe_amd, name)) and name in imagepipe_amd.__all__
    assert imagepipe_amd.transform_window_footprint(61, 47, (0, 0, 60, 0, 0, 46), 61, 47, (10, 10, 1, 1)) == (9, 9, 4, 4)
