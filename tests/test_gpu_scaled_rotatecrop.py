"""IPK_FUSED_SCALED_ROTATECROP on the GPU: an active OpRotateCrop behind an OpDemosaic that scales runs as two launches -- the scaling gofloat + demosaic
pass into the RGBE buffer (for 1 < scale < minscale k_fused_resample's RGBE output mode, ipk_raw_demosaic_scaled), then k_fused_resample's 4-channel source
mode over it -- bit for bit the CPU oracle's pipeline_run / output_8bit / output_16bit and the same pipeline with the bit clear; whole frames, regions,
special samples, what is launched, and that nothing outside a destination is written."""
import ctypes as C
import re

import numpy as np
import pytest

import util
from util import assert_bits_equal
from test_gpu_cached_region import _build, _raw_pipe, _apply, _want, _host, _same, XT
from test_gpu_cached_resample import _regions

pytestmark = pytest.mark.gpu

F32, U8, U16 = 0, 1, 2
NOCROP = (0, 0, 0, 0)
SENSOR_CROPS = (1, 3, 2, 5)
CROPS_RC = (0.1, 0.05, 0.2, 0.0)
UNSUPPORTED = -5                                                          # IPK_ERR_UNSUPPORTED
PASS2 = r"^ipk::k_fused_resample<float, [012]>\[.*rgbe=1.*\]$"
PASS1 = {"mode": r"^ipk::k_fused_resample<(unsigned short|float), 0>\[fast_ok=[01],axis=1,rgbe_out=1(,win=1)?\]$",
         "scaled": r"^ipk::k_raw_scaled_demosaic", "raster": r"^ipk::k_raster_scale_down"}


@pytest.fixture(scope="module")
def ipa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _mosaic(ipa, orc, cfa, is_float, sw, sh, seed=0, crops=NOCROP, rc=(0, 0, 0, 0, 0.02), maxwidth=0, maxheight=0, linear=False, curve=True,
            rotation=0, fliph=False, data=None, bit=True):
    """(pipeline, oracle descriptor) of a u16 / f32 mosaic"""
    if data is None:
        data = util.noise_u16(util.SEED + 17100 + seed, sh, sw)
        data = data.astype(np.float32) if is_float else data
    pipe = _raw_pipe(ipa, data, cfa, is_float, crops)
    _apply(pipe, dict(rotatecrop=rc, rotation=rotation, fliph=fliph))
    st = pipe.globals.settings
    st.maxwidth, st.maxheight, st.linear = maxwidth, maxheight, linear
    okw = {}
    if not curve:
        pipe.ops.basecurve.points = []
        okw["points"] = []
    pipe.fuse_scaled_rotatecrop = bit
    desc = orc.make_pipeline(data, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), crops=crops, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                             wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), rotatecrop=rc, maxwidth=maxwidth, maxheight=maxheight,
                             linear=linear, rotation=rotation, fliph=fliph, **okw)
    return pipe, desc


def _raster(ipa, orc, seed=0, **ops):
    pipe, desc = _build(ipa, orc, "rgb8", sw=200, sh=120, seed=2100 + seed, crops=NOCROP, **ops)
    pipe.fuse_scaled_rotatecrop = True
    return pipe, desc


def _whole(ipa, pipe, out_type, out=None):
    import torch
    with ipa.launch_log() as ran:
        got, fw, fh = pipe._run(out_type, out)
        torch.cuda.synchronize()
    return _host(got, out_type, fh, fw) if out is None else None, sorted(ran)


def _two_launches(ran, pass1, normal=True):
    """exactly one pass-1 kernel, one resampling launch over the RGBE buffer, and OpTransform's permutation behind every orientation but Normal"""
    p2 = [e for e in ran if re.match(PASS2, e)]
    p1 = [e for e in ran if re.match(PASS1[pass1], e)]
    rot = [e for e in ran if e.startswith("ipk::k_rotate")]
    assert len(p2) == 1 and len(p1) == 1 and len(rot) == (0 if normal else 1), ran
    assert sorted(p1 + p2 + rot) == sorted(ran), ran
    assert not any("k_transform_buffer" in e or "k_gofloat_cfa" in e for e in ran), ran


def _frame(ipa, orc, pipe, desc, pass1, out_types=(F32, U8, U16), normal=True):
    """-> {out_type: the oracle's result}, computed once (the oracle's 8- and 16-bit outputs set the descriptor's `linear`, as the reference does: F32 first)"""
    wants = {}
    for out_type in out_types:
        assert pipe.fuses_scaled_rotatecrop(out_type), "the case is meant to take the route"
        want = wants[out_type] = _want(orc, desc, out_type)
        got, ran = _whole(ipa, pipe, out_type)
        assert pipe.last_used_fused
        _two_launches(ran, pass1, normal)
        _same(got, want, out_type, "whole frame, out %d" % out_type)
        pipe.fuse_scaled_rotatecrop = False
        staged, ran0 = _whole(ipa, pipe, out_type)
        pipe.fuse_scaled_rotatecrop = True
        assert not any("rgbe" in e for e in ran0), ran0
        _same(got, staged, out_type, "against the bit clear, out %d" % out_type)
    return wants


def _check_regions(ipa, pipe, want, out_type, regions):
    import torch
    for x, y, w, h in regions:
        got = pipe.run_region(x, y, w, h, out_type)
        torch.cuda.synchronize()
        assert pipe.last_region_windowed, (x, y, w, h)
        assert pipe.region(x, y, w, h, out_type)[0] == 1
        _same(_host(got, out_type, h, w), want[y:y + h, x:x + w], out_type, "region %r out %d" % ((x, y, w, h), out_type))


# ---- whole frames ----
@pytest.mark.parametrize("cfa,is_float", [("RGGB", False), ("GRBG", True), (XT, False), (XT, True)])
def test_one_pixel_short(ipa, orc, cfa, is_float):
    """108x62 at rotation 0.02 negotiates 107x61: scale 1.009, pass 1 is the RGBE output mode"""
    pipe, desc = _mosaic(ipa, orc, cfa, is_float, 108, 62, seed=1)
    assert pipe.sizes()[0] == (107, 61)
    _frame(ipa, orc, pipe, desc, "mode")


@pytest.mark.parametrize("linear,curve", [(True, True), (False, False), (True, False)])
def test_crops_and_a_large_angle(ipa, orc, linear, curve):
    pipe, desc = _mosaic(ipa, orc, "RGGB", False, 262, 140, seed=2, rc=CROPS_RC + (1.0,), linear=linear, curve=curve)
    assert pipe.sizes() == ((261, 139), (132, 183))
    _frame(ipa, orc, pipe, desc, "mode", out_types=(F32, U8) if linear else (F32, U8, U16))


@pytest.mark.parametrize("angle", [0.0, 0.03, 0.3])
@pytest.mark.parametrize("cfa,is_float,maxwidth,pass1", [("RGGB", False, 180, "mode"), (XT, True, 180, "mode"), ("RGGB", True, 150, "scaled"),
                                                         (XT, False, 150, "mode"), ("GRBG", False, 100, "scaled"), (XT, True, 100, "scaled")])
def test_straightened_previews(ipa, orc, cfa, is_float, maxwidth, pass1, angle):
    pipe, desc = _mosaic(ipa, orc, cfa, is_float, 342, 150, seed=3, rc=CROPS_RC + (angle,), maxwidth=maxwidth)
    _frame(ipa, orc, pipe, desc, pass1, out_types=(F32, U8) if angle else (F32, U8, U16))


@pytest.mark.parametrize("angle", [0.0, 0.03, 0.3])
def test_raster_preview(ipa, orc, angle):
    pipe, desc = _raster(ipa, orc, seed=4, rotatecrop=CROPS_RC + (angle,), maxwidth=120)
    _frame(ipa, orc, pipe, desc, "raster")


# Normal, Rotate180, Rotate90, and Rotate90 / Rotate270 with a horizontal flip (Transpose and Transverse between them)
@pytest.mark.parametrize("rot,fliph", [(0, False), (2, False), (1, False), (1, True), (3, True)])
def test_orientations(ipa, orc, rot, fliph):
    lim = dict(maxheight=180) if rot & 1 else dict(maxwidth=180)
    pipe, desc = _mosaic(ipa, orc, "RGGB", False, 342, 150, seed=5, crops=SENSOR_CROPS, rc=CROPS_RC + (0.03,), rotation=rot, fliph=fliph, **lim)
    wants = _frame(ipa, orc, pipe, desc, "mode", normal=(rot, fliph) == (0, False))
    _, (fw, fh) = pipe.sizes()
    regions = [(0, 0, fw, fh), (3, 5, 37, 31), (fw - 33, fh - 21, 33, 21), (fw - 1, 0, 1, fh), (0, fh - 1, 5, 1), (0, 0, 1, 1)]
    for out_type in (F32, U8, U16):
        _check_regions(ipa, pipe, wants[out_type], out_type, regions)


def test_stage_names(ipa, orc):
    pipe, desc = _mosaic(ipa, orc, "RGGB", False, 342, 150, seed=6, rc=CROPS_RC + (0.03,), maxwidth=180, rotation=2)
    assert pipe.fuses_scaled_rotatecrop(U8)
    _, stages = pipe.run_timed(U8)
    assert [s for s, _ in stages] == ["gofloat+demosaic", "rotatecrop+to_lab+basecurve+from_lab+gamma", "transform"], stages
    pipe.ops.transform.rotation = 0
    _, stages = pipe.run_timed(F32)
    assert [s for s, _ in stages] == ["gofloat+demosaic", "rotatecrop+to_lab+basecurve+from_lab+gamma"], stages


# ---- regions ----
@pytest.mark.parametrize("case", ["rggb-mode", "xtrans-f32-mode", "rggb-scaled", "rggb-short", "rgb8"])
def test_regions(ipa, orc, case):
    import torch
    if case == "rgb8":
        pipe, desc = _raster(ipa, orc, seed=7, rotatecrop=CROPS_RC + (0.03,), maxwidth=120)
        pass1 = "raster"
    else:
        cfa, is_float, sw, sh, crops, rc, mw, pass1 = {
            "rggb-mode": ("RGGB", False, 342, 150, SENSOR_CROPS, CROPS_RC + (0.03,), 180, "mode"),
            "xtrans-f32-mode": (XT, True, 342, 150, NOCROP, CROPS_RC + (0.3,), 150, "mode"),
            "rggb-scaled": ("RGGB", False, 342, 150, NOCROP, CROPS_RC + (0.03,), 100, "scaled"),
            "rggb-short": ("RGGB", True, 262, 140, NOCROP, CROPS_RC + (1.0,), 0, "mode")}[case]
        pipe, desc = _mosaic(ipa, orc, cfa, is_float, sw, sh, seed=7, crops=crops, rc=rc, maxwidth=mw)
    assert pipe.fuses_scaled_rotatecrop()
    _, (fw, fh) = pipe.sizes()
    regions = _regions(fw, fh)
    assert (0, 0, fw, fh) in regions and len(regions) >= 8
    for out_type in (F32, U8, U16):
        _check_regions(ipa, pipe, _want(orc, desc, out_type), out_type, regions)
    # what a region launches: both passes as window launches, nothing whole-frame
    with ipa.launch_log() as ran:
        pipe.run_region(3, 5, 37, 9, F32)
        torch.cuda.synchronize()
    ran = sorted(ran)
    _two_launches(ran, pass1)
    assert all("win=1" in e for e in ran), ran
    # overlapping regions give equal bits
    a, b = (2, 1, min(90, fw - 2), min(30, fh - 1)), (41, 13, min(75, fw - 41), min(25, fh - 13))
    for out_type in (F32, U8):
        ga = _host(pipe.run_region(*a, out_type), out_type, a[3], a[2])
        gb = _host(pipe.run_region(*b, out_type), out_type, b[3], b[2])
        ox0, oy0, ox1, oy1 = max(a[0], b[0]), max(a[1], b[1]), min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
        assert ox1 > ox0 and oy1 > oy0
        _same(ga[oy0 - a[1]:oy1 - a[1], ox0 - a[0]:ox1 - a[0]], gb[oy0 - b[1]:oy1 - b[1], ox0 - b[0]:ox1 - b[0]], out_type, "the overlap")


def test_host_region_uploads_the_window_alone(ipa, orc):
    """ipk_host_pipeline_run_region: only the reported sensor window is uploaded, so a window that were too small would show"""
    sw, sh = 342, 150
    data = util.noise_u16(util.SEED + 17108, sh, sw)
    pipe, desc = _mosaic(ipa, orc, "RGGB", False, sw, sh, crops=SENSOR_CROPS, rc=CROPS_RC + (0.03,), maxwidth=180, data=data)
    assert pipe.fuses_scaled_rotatecrop(U8)
    _, (fw, fh) = pipe.sizes()
    want = _want(orc, desc, U8)
    d = pipe.desc()
    for x, y, w, h in ((fw // 3, fh // 3, fw // 4, fh // 4), (0, 0, fw, fh), (fw - 9, 2, 9, 13)):
        out = np.full(w * h * 3, 0xA5, np.uint8)
        win = C.c_int(0)
        rc = ipa.lib().ipk_host_pipeline_run_region(C.byref(d), data.ctypes.data_as(C.c_void_p), x, y, w, h, out.ctypes.data_as(C.c_void_p), U8, C.byref(win))
        assert rc == 0 and win.value == 1
        assert np.array_equal(out.reshape(h, w, 3), want[y:y + h, x:x + w]), (x, y, w, h)


# ---- special samples ----
@pytest.mark.parametrize("cfa,sw,sh,rc,maxwidth,pass1", [("RGGB", 108, 62, (0, 0, 0, 0, 0.02), 0, "mode"), (XT, 342, 150, CROPS_RC + (0.03,), 150, "mode"),
                                                         ("RGGB", 342, 150, CROPS_RC + (0.03,), 150, "scaled")])
def test_special_samples_in_an_f32_mosaic(ipa, orc, cfa, sw, sh, rc, maxwidth, pass1):
    """+-inf, NaN, -0.0 and values below black, each alone in an ordinary neighbourhood and at the frame's edges and corners: a zero-weight tap over inf
    stays NaN (0 * inf), in both passes"""
    raw = util.noise_u16(util.SEED + 17109, sh, sw).astype(np.float32)
    vals = [np.inf, -np.inf, np.nan, -0.0, util.BLACK, util.BLACK - 1.0, -300.0, 0.0]
    spots = [(0, 0), (0, sw - 1), (sh - 1, 0), (sh - 1, sw - 1), (0, sw // 2), (sh - 1, sw // 3), (sh // 2, 0), (sh // 3, sw - 1)]
    k = 0
    for i, v in enumerate(vals):
        r, c = spots[i]
        raw[r, c] = np.float32(v)
        for _ in range(3):                                                 # and alone among ordinary samples, 11 or more apart
            raw[7 + (11 * k) % (sh - 14), 9 + (37 * k) % (sw - 18)] = np.float32(v)
            k += 1
    pipe, desc = _mosaic(ipa, orc, cfa, True, sw, sh, rc=rc, maxwidth=maxwidth, data=raw)
    want = _frame(ipa, orc, pipe, desc, pass1)[F32]
    _, (fw, fh) = pipe.sizes()
    assert np.isfinite(want).any()
    _check_regions(ipa, pipe, want, F32, [(0, 0, 9, 7), (fw - 11, fh - 9, 11, 9), (fw // 4, fh // 4, fw // 2, fh // 3), (0, fh // 2, fw, 1)])


# ---- the tile loop ----
def test_more_tiles_than_compute_units(ipa, orc):
    """both kernels' tile loops and prefetches: a block takes several tiles in pass 1 and in pass 2"""
    pipe, desc = _mosaic(ipa, orc, "RGGB", False, 1210, 620, seed=10, rc=(0, 0, 0, 0, 0.03))
    (dw, dh), (fw, fh) = pipe.sizes()
    assert (dw, dh) == (1209, 619)
    cus = ipa.lib().ipk_device_cus()
    assert dw * dh > 2048 * cus and fw * fh > 2048 * cus
    _frame(ipa, orc, pipe, desc, "mode", out_types=(F32, U8))


# ---- ipk_raw_demosaic_scaled and its window form on their own ----
def _oracle_rgbe(orc, data, rect, cfa, nw, nh):
    x, y, w, h = rect
    branch, want = orc.demosaic_run(orc.cfa_shift(cfa, x, y), orc.gofloat_cfa(data, x, y, w, h, util.BLACK, util.WHITE), nw, nh)
    assert branch == 4 and want.shape == (nh, nw, 4), "OpDemosaic's full + scale_down_opbuf branch"
    return want


@pytest.mark.parametrize("cfa,is_float,rect,size", [("RGGB", False, (0, 0, 108, 62), (107, 61)), ("GRBG", True, (5, 1, 131, 97), (87, 64)),
                                                    (XT, False, (5, 1, 150, 100), (60, 40)), (XT, True, (0, 0, 101, 77), (51, 38)),
                                                    ("RGGB", False, (3, 2, 1210, 620), (1209, 619))])
def test_raw_demosaic_scaled(ipa, orc, cfa, is_float, rect, size):
    import torch
    x, y, w, h = rect
    nw, nh = size
    sw, sh = x + w + 3, y + h + 2
    data = util.noise_u16(util.SEED + 17111, sh, sw)
    data = data.astype(np.float32) if is_float else data
    want = _oracle_rgbe(orc, data, rect, cfa, nw, nh)
    src = util.Embedded(data, off=1)
    shifted = orc.cfa_shift(cfa, x, y)
    g = util.Guarded(nw * nh * 4, torch.float32, off=1)                     # element alignment only: 4 bytes past a 256-byte boundary
    with ipa.launch_log() as ran:
        ipa.raw_demosaic_scaled(src.view(), sw, x, y, w, h, util.BLACK, util.WHITE, shifted, nw, nh, out=g.view())
        torch.cuda.synchronize()
    assert len(ran) == 1 and re.match(PASS1["mode"], sorted(ran)[0]) and "win=1" not in sorted(ran)[0], ran
    got = g.result("whole frame").reshape(nh, nw, 4)
    assert_bits_equal(got, want, "ipk_raw_demosaic_scaled")
    assert not got[..., 3].view(np.uint32).any(), "E is +0.0"
    src.assert_untouched()
    for off, win in ((3, (0, 0, nw, nh)), (1, (nw - 1, nh - 1, 1, 1)), (2, (0, 0, 1, 1)), (1, (3, 5, 37, 9)), (3, (nw // 3, 1, 1, nh - 2)), (1, (1, nh // 2, nw - 1, 1)),
                     (2, (nw - 35, nh - 34, 35, 34))):
        wx, wy, ww, wh = win
        gw = util.Guarded(ww * wh * 4, torch.float32, off=off)
        with ipa.launch_log() as ran:
            ipa.raw_demosaic_scaled(src.view(), sw, x, y, w, h, util.BLACK, util.WHITE, shifted, nw, nh, window=win, out=gw.view())
            torch.cuda.synchronize()
        assert len(ran) == 1 and re.match(PASS1["mode"], sorted(ran)[0]) and sorted(ran)[0].endswith(",win=1]"), ran
        assert_bits_equal(gw.result("window %r" % (win,)).reshape(wh, ww, 4), want[wy:wy + wh, wx:wx + ww], "window %r" % (win,))


def test_raw_demosaic_scaled_refuses(ipa):
    import torch
    data = util.noise_u16(util.SEED + 17112, 100, 150)
    src = ipa.upload_u16(data)
    L = ipa.lib()
    for cfa, nw, nh, why in (("RGBE", 100, 66, "a fourth colour"), ("RGGB", 50, 34, "a skip of 3 or more"), (XT, 52, 34, "a row skip of exactly 3")):
        for win in (None, (1, 1, 5, 5)):
            n = nw * nh * 4 if win is None else win[2] * win[3] * 4
            g = util.Guarded(n, torch.float32, off=1)
            with ipa.launch_log() as ran:
                if win is None:
                    rc = L.ipk_raw_demosaic_scaled(src.data_ptr(), 0, 150, 0, 0, 150, 100, util.BLACK, util.WHITE, cfa.encode(), nw, nh, g.ptr, None)
                else:
                    rc = L.ipk_raw_demosaic_scaled_window(src.data_ptr(), 0, 150, 0, 0, 150, 100, util.BLACK, util.WHITE, cfa.encode(), nw, nh, *win, g.ptr, None)
                torch.cuda.synchronize()
            assert rc == UNSUPPORTED, (why, rc)
            assert not ran, (why, ran)
            assert (g.result(why) == np.float32(util.SENTINELS["float32"])).all(), why


# ---- no stray writes ----
@pytest.mark.parametrize("out_type,off", [(F32, 1), (U8, 3), (U16, 1)])
def test_nothing_outside_the_destination_is_written(ipa, orc, out_type, off):
    import torch
    dt = {U8: torch.uint8, F32: torch.float32, U16: torch.int16}[out_type]
    pipe, desc = _mosaic(ipa, orc, "RGGB", False, 342, 150, seed=13, crops=SENSOR_CROPS, rc=CROPS_RC + (0.03,), maxwidth=180)
    assert pipe.fuses_scaled_rotatecrop(out_type)
    _, (fw, fh) = pipe.sizes()
    want = _want(orc, desc, out_type)
    g = util.Guarded(fw * fh * 3, dt, off=off)
    _, ran = _whole(ipa, pipe, out_type, out=g.view())
    _two_launches(ran, "mode")
    got = g.result("whole frame")
    _same((got.view(np.uint16) if out_type == U16 else got).reshape(fh, fw, 3), want, out_type, "guarded whole frame")
    for reg in ((7, 3, 51, 7), (1, 2, 63, 11), (fw - 65, fh - 33, 65, 33)):
        x, y, w, h = reg
        g = util.Guarded(w * h * 3, dt, off=off)
        pipe.run_region(x, y, w, h, out_type, out=g.view())
        torch.cuda.synchronize()
        assert pipe.last_region_windowed
        got = g.result("region %r" % (reg,))
        _same((got.view(np.uint16) if out_type == U16 else got).reshape(h, w, 3), want[y:y + h, x:x + w], out_type, "guarded region %r" % (reg,))
