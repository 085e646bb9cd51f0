"""Regions of downscaled previews as a window of the scaling gofloat + demosaic pass (no GPU): which descriptors ipk_pipeline_region sends there under
IPK_FUSED_WINDOW_PREVIEWS (bit 3 of allow_fused), that bit 2 and every other mask leave them whole-frame, and the sensor footprint the window launch
reports (ipk_scaled_window_footprint) against a numpy-float32 restatement of the reference's window expressions (src/scaling.rs:84-87 with
scale_down_buffer's corners) over EVERY pixel of the window, widened by the 8-sample row loads of the window-8 kernels."""
import ctypes as C

import numpy as np
import pytest

import util
import test_scaledown_route as sr
from test_scaledown_route import XT, INVALID, SENSOR_CROPS, NOCROP, MINSCALE
from test_region_windows_route import _windows_of, _usize

ON, FOUR, REGIONS, PREVIEWS = 1, 2, 4, 8
RC = [float(np.float32(v)) for v in (0.1, 0, 0, 0, 0.2)]


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _raster(w, h, **kw):
    """an edited raster (the levels, white balance and matrix of sr._desc are not the defaults: no fast path)"""
    return sr._desc(w, h, "", src_type=2, cpp=3, is_cfa=0, **kw)


# name -> (builder of a fresh descriptor, width, height, crops, filter width for minscale or None for a raster)
TAKEN = {
    "bayer-131x97@40": (lambda: sr._desc(131, 97, "RGGB", maxwidth=40), 131, 97, NOCROP, 2),
    "bayer-scale2-200x120@100": (lambda: sr._desc(200, 120, "GRBG", maxwidth=100), 200, 120, NOCROP, 2),
    "bayer-f32-crops-96x120@h30": (lambda: sr._desc(96, 120, "RGGB", SENSOR_CROPS, src_type=1, maxheight=30), 96, 120, SENSOR_CROPS, 2),
    "xtrans-150x100@40": (lambda: sr._desc(150, 100, XT, maxwidth=40), 150, 100, NOCROP, 6),
    "xtrans-scale3-150x100@50": (lambda: sr._desc(150, 100, XT, maxwidth=50), 150, 100, NOCROP, 6),
    "rgbe-131x97@40": (lambda: sr._desc(131, 97, "RGBE", maxwidth=40), 131, 97, NOCROP, 2),
    "raster-rgb8-128x64@64": (lambda: _raster(128, 64, maxwidth=64, exposure=0.1), 128, 64, NOCROP, None),
    "raster-rgb16-83x57@29": (lambda: sr._desc(83, 57, "", src_type=3, cpp=3, is_cfa=0, maxwidth=29), 83, 57, NOCROP, None),
}


def _region(L, d, x, y, w, h, out_type=0):
    s = [C.c_size_t(12345) for _ in range(4)]
    rc = L.ipk_pipeline_region(C.byref(d), out_type, x, y, w, h, *[C.byref(v) for v in s])
    return rc, tuple(v.value for v in s)


def _sizes(L, d):
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
    return tuple(v.value for v in a)


def _footprint(L, W, H, nw, nh, window):
    out = (C.c_size_t * 4)()
    rc = L.ipk_scaled_window_footprint(W, H, nw, nh, *window, out)
    assert rc == 0, (rc, L.ipk_last_error())
    return tuple(out)


def _taps(W, H, nw, nh):
    """scaling.rs:69-72 and :84-87 for scale_down_buffer's corners in numpy float32, each operation rounded on its own: from_x, to_x (per column) and
    from_y, to_y (per row), plus lx = min(from_x, W - 8), the first sample of the window-8 kernels' row load (frames of 8 columns and more)"""
    f = np.float32
    with np.errstate(all="ignore"):
        sx, sy = (f(W - 1) - f(0)) / f(nw - 1), (f(H - 1) - f(0)) / f(nh - 1)
        col, col1 = np.arange(nw, dtype=f), np.arange(1, nw + 1, dtype=f)
        row, row1 = np.arange(nh, dtype=f), np.arange(1, nh + 1, dtype=f)
        fx, tx = np.minimum(W - 1, _usize(np.floor(f(0) + sx * col))), np.minimum(W - 1, _usize(np.floor(f(0) + sx * col1)))
        fy, ty = np.minimum(H - 1, _usize(np.floor(f(0) + sy * row))), np.minimum(H - 1, _usize(np.floor(f(0) + sy * row1)))
    assert (sx * col).dtype == np.float32
    lx = np.minimum(fx, W - 8) if W >= 8 else None
    return float(sx), float(sy), fx, tx, fy, ty, lx


def _check_footprints(L, W, H, nw, nh, tag):
    _, _, fx, tx, fy, ty, lx = _taps(W, H, nw, nh)
    assert (fx <= tx).all() and (fy <= ty).all()
    for win in _windows_of(nw, nh):
        wx, wy, ww, wh = win
        x0, x1 = int(fx[wx:wx + ww].min()), int(tx[wx:wx + ww].max())
        y0, y1 = int(fy[wy:wy + wh].min()), int(ty[wy:wy + wh].max())
        gx, gy, gw, gh = _footprint(L, W, H, nw, nh, win)
        t = "%s %r: footprint %r, taps [%d, %d] x [%d, %d]" % (tag, win, (gx, gy, gw, gh), x0, x1, y0, y1)
        assert gw > 0 and gh > 0 and gx + gw <= W and gy + gh <= H, t + ": empty or outside the frame"
        assert gx <= x0 and gx + gw - 1 >= x1 and gy <= y0 and gy + gh - 1 >= y1, t + ": a tap is outside"
        if lx is not None:
            assert gx <= int(lx[wx:wx + ww].min()) and gx + gw >= int(lx[wx:wx + ww].max()) + 8, t + ": an 8-sample load is outside"
        assert x0 - gx <= 7 and gx + gw - 1 - x1 <= 7, t + ": more than 7 columns beyond the taps"
        assert (gy, gy + gh - 1) == (y0, y1), t + ": rows beyond the taps"


# (width, height, nwidth, nheight): skips in (1, 2), [2, 4), [4, 7] and above 7, frames under 8 columns, the shapes of the GPU cases
FOOTPRINT_SHAPES = [(131, 97, 87, 64), (150, 100, 100, 40), (150, 100, 50, 40), (101, 103, 51, 52), (150, 100, 30, 40), (150, 100, 22, 15),
                    (150, 100, 15, 40), (7, 30, 3, 10), (83, 57, 29, 19), (8, 9, 2, 3), (700, 30, 330, 12), (2400, 24, 300, 3), (100, 330, 33, 110)]


@pytest.mark.parametrize("shape", FOOTPRINT_SHAPES, ids=["%dx%d-%dx%d" % s for s in FOOTPRINT_SHAPES])
def test_footprint_contains_taps_and_loads(L, shape):
    _check_footprints(L, *shape, "%dx%d to %dx%d" % shape)


def test_the_footprint_shapes_cover_every_skip_range():
    skips = [_taps(*s)[0] for s in FOOTPRINT_SHAPES]
    for lo, hi in ((1.0, 2.0), (2.0, 4.0), (4.0, 7.0), (7.0, 1e9)):
        assert any(lo < s < hi or (lo >= 2.0 and s == lo) for s in skips), (lo, hi, skips)
    assert any(s[0] < 8 for s in FOOTPRINT_SHAPES)


def test_footprint_refusals(L):
    out = (C.c_size_t * 4)(7, 7, 7, 7)
    fp = lambda *a: L.ipk_scaled_window_footprint(131, 97, 41, 31, *a)
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (40, 0, 2, 1), (0, 30, 1, 2), (41, 0, 1, 1), (0, 31, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        assert fp(*win, out) == INVALID, win
    assert fp(0, 0, 1, 1, None) == INVALID
    assert tuple(out) == (7, 7, 7, 7)
    assert fp(40, 30, 1, 1, out) == 0 and tuple(out) != (7, 7, 7, 7)


# ---------------------------------------------------------------------------------------------
# the route report
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(TAKEN))
def test_previews_are_windowed_with_the_bit_only(L, orc, name):
    build, w, h, crops, cfaw = TAKEN[name]
    x0, y0, cw, ch = orc.size_image(*crops, w, h)
    d1 = build()
    d1.allow_fused = ON | PREVIEWS
    dw, dh, fw, fh = _sizes(L, d1)
    # the branch named: OpDemosaic scales in one pass (demosaic.rs:44-50)
    scale = orc.calculate_scaling_total(cw, ch, dw, dh)[0]
    assert scale >= MINSCALE[cfaw] if cfaw else scale > 1.0, (name, scale)
    assert (fw, fh) == (dw, dh)
    for out_type in (0, 1, 2):
        assert L.ipk_pipeline_windows_preview(C.byref(d1), out_type) == 1, name
        for mask in (ON, ON | REGIONS, ON | FOUR | REGIONS, 0, PREVIEWS):
            d0 = build()
            d0.allow_fused = mask
            assert L.ipk_pipeline_windows_preview(C.byref(d0), out_type) == 0, (name, mask)
            for fuses in (L.ipk_pipeline_fuses_rotatecrop, L.ipk_pipeline_fuses_scaledown, L.ipk_pipeline_fuses_four_colour):
                assert fuses(C.byref(d0), out_type) == fuses(C.byref(d1), out_type) == 0      # no other report sees the bit
            for win in _windows_of(dw, dh)[:5]:
                assert _region(L, d0, *win, out_type) == (0, (x0, y0, cw, ch)), "%s mask %d %r: route 0 and the crop window" % (name, mask, win)
        for win in _windows_of(dw, dh):
            gx, gy, gw, gh = _footprint(L, cw, ch, dw, dh, win)
            assert _region(L, d1, *win, out_type) == (1, (x0 + gx, y0 + gy, gw, gh)), "%s %r" % (name, win)
        # with the other bits beside it, too; and the hashes do not see the bit
        d7 = build()
        d7.allow_fused = ON | FOUR | REGIONS | PREVIEWS
        assert _region(L, d7, 0, 0, 2, 2, out_type)[0] == 1
        d0 = build()
        ha, hb = C.create_string_buffer(256), C.create_string_buffer(256)
        assert L.ipk_pipeline_hashes(C.byref(d0), out_type, 5, ha) == 0 and L.ipk_pipeline_hashes(C.byref(d1), out_type, 5, hb) == 0
        assert ha.raw == hb.raw


def test_a_mask_without_bit_0(L):
    """allow_fused = 8.  Any non-zero mask means "on" for the whole-frame drivers (the header), and 8 is no exception; but bit 3 itself acts only
    beside IPK_FUSED_ON, so a region of a preview is cut from the whole result: route 0, the crop window"""
    d = sr._desc(131, 97, "RGGB", maxwidth=40)
    d.allow_fused = PREVIEWS
    assert L.ipk_pipeline_windows_preview(C.byref(d), 0) == 0
    assert _region(L, d, 3, 5, 17, 9) == (0, (0, 0, 131, 97))
    full = sr._desc(96, 120, "RGGB")                      # "on": a full-size frame is windowed as with allow_fused = 1
    full.allow_fused = PREVIEWS
    assert _region(L, full, 3, 5, 17, 9)[0] == 1


def test_other_descriptors_stay_whole_frame_with_the_bit(L, orc):
    cases = [("mono", sr._desc(131, 97, "", is_cfa=0, maxwidth=40)),
             ("cpp3", sr._desc(131, 97, "", cpp=3, is_cfa=0, maxwidth=40)),
             ("rotatecrop under a size limit", sr._desc(131, 97, "RGGB", maxwidth=40, rotatecrop=RC)),
             ("rotatecrop, fused flag", sr._desc(131, 97, "RGGB", maxwidth=40, rotatecrop=RC, fuse_rotatecrop=1)),
             ("raster with a rotatecrop", _raster(128, 64, maxwidth=64, rotatecrop=RC)),
             ("1 < scale < minscale, bayer", sr._desc(131, 97, "RGGB", maxwidth=87)),
             ("1 < scale < minscale, bayer, unfused", sr._desc(131, 97, "RGGB", maxwidth=87, fuse=0)),
             ("1 < scale < minscale, xtrans", sr._desc(150, 100, XT, maxwidth=60)),
             ("1 < scale < minscale, rgbe", sr._desc(131, 97, "RGBE", maxwidth=87))]
    for tag, d in cases:
        d.allow_fused = ON | PREVIEWS
        assert L.ipk_pipeline_windows_preview(C.byref(d), 0) == 0, tag
        route, fp = _region(L, d, 0, 0, 2, 2)
        assert route == 0 and fp == (0, 0, d.width, d.height), (tag, route, fp)
    # ... where bit 2 has its ground, bit 3 changes nothing
    d = sr._desc(131, 97, "RGGB", maxwidth=87)
    d.allow_fused = ON | REGIONS | PREVIEWS
    d2 = sr._desc(131, 97, "RGGB", maxwidth=87)
    d2.allow_fused = ON | REGIONS
    assert _region(L, d, 3, 5, 17, 9) == _region(L, d2, 3, 5, 17, 9) and _region(L, d, 3, 5, 17, 9)[0] == 1
    # the raster fast path
    from imagepipe_amd._lib import PipelineDesc
    fast = PipelineDesc()
    fast.src_type, fast.width, fast.height, fast.cpp, fast.use_fastpath, fast.maxwidth = 2, 128, 64, 3, 1, 64
    m = (C.c_float * 12)()
    L.ipk_const_matrix(2, m)
    fast.cam_to_xyz_normalized[:] = m[:]
    fast.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    fast.allow_fused = ON | PREVIEWS
    assert L.ipk_pipeline_takes_fastpath(C.byref(fast), 1) == 1
    assert L.ipk_pipeline_windows_preview(C.byref(fast), 1) == 0 and _region(L, fast, 0, 0, 2, 2, 1) == (0, (0, 0, 128, 64))
    assert L.ipk_pipeline_windows_preview(C.byref(fast), 0) == 1          # an f32 result never takes the fast path: the staged raster preview
    # full-size frames: windowed whatever the bits, the report is about previews
    full = sr._desc(96, 120, "RGGB")
    full.allow_fused = ON | PREVIEWS
    assert L.ipk_pipeline_windows_preview(C.byref(full), 0) == 0 and _region(L, full, 3, 5, 17, 9)[0] == 1


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (0, 1)])
def test_every_orientation_is_windowed(L, orc, rot, fh):
    """the region is mapped back through OpTransform: still route 1, and a one-pixel region at a corner of the result comes from a corner of the
    preview -- its footprint is one of the four corner footprints"""
    w, h, crops = 96, 120, SENSOR_CROPS
    d = sr._desc(w, h, "GRBG", crops, maxheight=30, rotation=rot, fliph=fh)
    d.allow_fused = ON | PREVIEWS
    dw, dh, fw, fhh = _sizes(L, d)
    x0, y0, cw, ch = orc.size_image(*crops, w, h)
    assert (fw, fhh) == ((dh, dw) if rot % 2 else (dw, dh)) and dw != dh
    corner_fps = [(x0 + f[0], y0 + f[1], f[2], f[3]) for f in (_footprint(L, cw, ch, dw, dh, win) for win in _windows_of(dw, dh)[:4])]
    assert len(set(corner_fps)) == 4
    seen = set()
    for x, y in ((0, 0), (fw - 1, 0), (0, fhh - 1), (fw - 1, fhh - 1)):
        route, fp = _region(L, d, x, y, 1, 1)
        assert route == 1 and fp in corner_fps, (x, y, fp)
        seen.add(fp)
    assert len(seen) == 4
    whole = _footprint(L, cw, ch, dw, dh, (0, 0, dw, dh))
    assert _region(L, d, 0, 0, fw, fhh) == (1, (x0 + whole[0], y0 + whole[1], whole[2], whole[3]))


def test_invalid_regions(L):
    for d in (sr._desc(131, 97, "RGGB", maxwidth=40), _raster(128, 64, maxwidth=64)):
        d.allow_fused = ON | PREVIEWS
        _, _, fw, fh = _sizes(L, d)
        assert _region(L, d, 0, 0, fw, fh)[0] == 1
        for win in ((0, 0, 0, 1), (0, 0, 1, 0), (fw - 1, 0, 2, 1), (0, fh - 1, 1, 2), (fw, 0, 1, 1), (0, fh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
            rc, fp = _region(L, d, *win)
            assert rc == INVALID and fp == (12345,) * 4, (win, rc, fp)
        assert _region(L, d, 0, 0, 1, 1, out_type=3)[0] == INVALID
        assert L.ipk_pipeline_windows_preview(C.byref(d), 3) == INVALID and L.ipk_pipeline_windows_preview(None, 0) == INVALID


def test_bindings_carry_the_bit():
    import inspect
    import imagepipe_amd
    from imagepipe_amd import _lib
    assert _lib.FUSED_WINDOW_PREVIEWS == PREVIEWS
    src = inspect.getsource(imagepipe_amd.Pipeline)
    assert "self.window_previews = False" in src and "d.allow_fused |= _lib.FUSED_WINDOW_PREVIEWS" in src
    assert callable(imagepipe_amd.Pipeline.windows_preview)
    for name in ("raw_scaled_demosaic_window", "raster_scale_down_window", "scaled_window_footprint"):
        assert callable(getattr(imagepipe_amd, name)) and name in imagepipe_amd.__all__
    for name in ("ipk_raw_scaled_demosaic_window", "ipk_raster_scale_down_window", "ipk_scaled_window_footprint", "ipk_pipeline_windows_preview"):
        assert name in _lib.SIGNATURES
    # 150 -> 50 columns (skip 149 / 49): column 10 reads samples 30..33 and loads 30..37; row 10 of 100 -> 40 reads rows 25..27
    assert imagepipe_amd.scaled_window_footprint(150, 100, 50, 40, (10, 10, 1, 1)) == (30, 25, 8, 3)
