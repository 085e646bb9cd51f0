"""GPU parity of the window launches of k_fused_resample: ipk_raw_to_srgb_resampled_window / ipk_raw_to_srgb_scaled_window at op level, and regions
of the one-launch rotatecrop and scaledown routes under IPK_FUSED_WINDOW_REGIONS (Pipeline.window_regions) at pipeline level, from device and from
host memory.  Bar: bit-exact f32 (any NaN == any NaN), equal u8 / u16, against the same rectangle of the CPU oracle's result and of the whole-frame
run.  No case is skipped or filtered; every pipeline case asserts by last_region_windowed, by the launch log and by the stage names that the window
route ran.  Frames are about 100 x 130 pixels: several tiles in both directions with a partial last tile (the plans' tiles are 64x32 .. 16x16)."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_gpu_rotatecrop_fused as rcf
import test_gpu_scaledown_fused as sdf
from test_gpu_rotatecrop_fused import XT, W12, F32, U8, U16, SENSOR_CROPS, R9, R9_IDS, _mosaic, _upload, _np, _same, _oracle_ops, _oracle_desc, _want
from test_gpu_scaledown_fused import SMALL, FRAME_CFA, FRAME_CFA_IDS, CODES

pytestmark = pytest.mark.gpu

NOCROP = (0, 0, 0, 0)
INVALID = -2
NP_OUT = {F32: np.dtype(np.float32), U8: np.dtype(np.uint8), U16: np.dtype(np.uint16)}
WHOLE_FRAME_KERNELS = ("k_transform_buffer", "k_demosaic_full", "k_pointwise_chain")
DEGENERATE = {"outside": ((-4, -3), (58, 5), (-9, 49), 57, 44), "mirror": ((50, 3), (4, 3), (50, 40), 47, 38), "flat": ((3, 7), (3, 7), (3, 7), 9, 6)}


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _windows(nw, nh):
    """one pixel at each corner; a window with an odd origin off every plan's tile grid that crosses tile boundaries in both directions and ends in a
    partial tile ((37, 21, 45, 40) where it fits); one full row; one full column; the whole image"""
    assert nw >= 6 and nh >= 4
    odd = (37, 21, 45, 40) if nw >= 82 and nh >= 61 else (3, 1, nw - 4, nh - 2)
    return [(0, 0, 1, 1), (nw - 1, 0, 1, 1), (0, nh - 1, 1, 1), (nw - 1, nh - 1, 1, 1), odd, (0, nh // 2, nw, 1), (nw // 3, 0, 1, nh), (0, 0, nw, nh)]


def _plan_kw(ipa, orc, data, crops, cfa, out_type, **prm):
    oh, ow = data.shape
    x, y, cw, ch = orc.size_image(*crops, ow, oh)
    kw = dict(width=cw, height=ch, owidth=ow, x=x, y=y, is_float=data.dtype == np.float32, black0=util.BLACK, white0=util.WHITE,
              cfa=orc.cfa_shift(cfa, crops[3], crops[0]), wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), out_type=CODES[out_type])
    kw.update(prm)
    return kw


def _assert_window_launch(ran, tag, axis):
    pat = r"k_fused_resample<.*\[fast_ok=\d,axis=1,win=1\]" if axis else r"k_fused_resample<.*\[fast_ok=\d,win=1\]"
    assert any(re.search(pat, e) for e in ran), "%s: no window launch of k_fused_resample: %r" % (tag, sorted(ran))
    assert not [e for e in ran if "k_fused_resample" in e and "win=1" not in e], "%s: a whole-frame launch ran: %r" % (tag, sorted(ran))
    assert not [e for e in ran if any(k in e for k in WHOLE_FRAME_KERNELS)], "%s: staged kernels ran: %r" % (tag, sorted(ran))


# ---------------------------------------------------------------------------------------------
# op level: the two window entry points against the same rectangle of the oracle's op-by-op composition
# ---------------------------------------------------------------------------------------------
OP_CFAS = ["RGGB", XT, W12]


def _op_case(ipa, orc, data, crops, cfa, corners, out_type, scaled, tag, prm=None):
    prm = {**dict(exposure=0.0, points=[(0.5, 0.6)], linear=False), **(prm or {})}
    tl, tr, bl, nw, nh = corners
    want = _oracle_ops(orc, data, crops, cfa, util.BLACK, util.WHITE, corners, util.WB, util.cam_matrix(), prm["exposure"], prm["points"], prm["linear"], out_type)
    src = _upload(ipa, data)
    kw = _plan_kw(ipa, orc, data, crops, cfa, out_type, **prm)
    for win in _windows(nw, nh):
        wx, wy, ww, wh = win
        with ipa.launch_log() as ran:
            if scaled:
                got = ipa.raw_to_srgb_scaled_window(src, nw, nh, win, **kw)
            else:
                got = ipa.raw_to_srgb_resampled_window(src, (tl[0], tl[1], tr[0], tr[1], bl[0], bl[1]), nw, nh, win, **kw)
        _same(_np(got, out_type, wh, ww), want[wy:wy + wh, wx:wx + ww], "%s window %r" % (tag, win))
        _assert_window_launch(ran, "%s window %r" % (tag, win), scaled)


@pytest.mark.parametrize("k", range(len(R9)), ids=R9_IDS)
@pytest.mark.parametrize("ci", range(len(OP_CFAS)), ids=["RGGB", "xtrans", "12x12"])
def test_resampled_window_vs_oracle(ipa, orc, ci, k):
    """every filter meets every R9 transform (rot1.0 / rot1.3: most windows empty); sensor crops, source type, output type and curve rotate"""
    i = ci + k
    h, w = (131, 113) if i % 2 else (127, 118)
    crops = SENSOR_CROPS if (i // 2) % 2 else NOCROP
    is_float = bool((ci + k // 2) % 2)
    out_type = [F32, U8, U16][(ci + 2 * k) % 3]
    prm = rcf.OP_PARAMS[(2 * ci + k) % len(rcf.OP_PARAMS)]
    data = _mosaic(util.SEED + 12100 + 16 * ci + k, h, w, is_float)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    corners = orc.rotatecrop_corners(R9[k], cw, ch)
    assert corners is not None
    _op_case(ipa, orc, data, crops, OP_CFAS[ci], corners, out_type, False, "resampled %s %s %s %s" % (OP_CFAS[ci][:6], R9_IDS[k], "f32" if is_float else "u16", out_type), prm)


@pytest.mark.parametrize("out_type", [F32, U8, U16])
@pytest.mark.parametrize("name", list(DEGENERATE))
def test_resampled_window_clamped_and_degenerate(ipa, orc, name, out_type):
    is_float = out_type != U8
    data = _mosaic(util.SEED + 12300 + len(name), 47, 61, is_float)
    _op_case(ipa, orc, data, NOCROP, "GRBG", DEGENERATE[name], out_type, False, "resampled %s %s" % (name, out_type))


@pytest.mark.parametrize("frame,cfa", FRAME_CFA, ids=FRAME_CFA_IDS)
def test_scaled_window_vs_oracle(ipa, orc, frame, cfa):
    w, h, crops, lim, _ = SMALL[frame]
    nw, nh = sdf._negotiated(orc, w, h, crops, lim)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    corners = ((0, 0), (cw - 1, 0), (0, ch - 1), nw, nh)
    i = FRAME_CFA.index((frame, cfa))
    for j, is_float in enumerate((False, True)):
        out_type = [F32, U8, U16][(i + j) % 3]
        data = _mosaic(util.SEED + 12400 + i + is_float, h, w, is_float)
        _op_case(ipa, orc, data, crops, cfa, corners, out_type, True, "scaled %s %s %s %s" % (frame, cfa[:6], "f32" if is_float else "u16", out_type))


def test_every_source_and_output_type_meets_both_forms(ipa, orc):
    """the rotating choices above leave no kernel out: u16 / f32 source x f32 / u8 / u16 output, general and axis-aligned mode, one odd window each"""
    h, w = 97, 131
    for is_float in (False, True):
        data = _mosaic(util.SEED + 12500 + is_float, h, w, is_float)
        for out_type in (F32, U8, U16):
            for scaled, corners in ((False, orc.rotatecrop_corners(R9[3], w, h)), (True, ((0, 0), (w - 1, 0), (0, h - 1), 87, 64))):
                tl, tr, bl, nw, nh = corners
                want = _oracle_ops(orc, data, NOCROP, "GBRG", util.BLACK, util.WHITE, corners, util.WB, util.cam_matrix(), 0.0, [(0.5, 0.6)], False, out_type)
                kw = _plan_kw(ipa, orc, data, NOCROP, "GBRG", out_type)
                win = (21, 13, 45, 40)
                got = ipa.raw_to_srgb_scaled_window(_upload(ipa, data), nw, nh, win, **kw) if scaled else \
                    ipa.raw_to_srgb_resampled_window(_upload(ipa, data), (tl[0], tl[1], tr[0], tr[1], bl[0], bl[1]), nw, nh, win, **kw)
                _same(_np(got, out_type, 40, 45), want[13:53, 21:66], "%s %s %s" % ("scaled" if scaled else "resampled", "f32" if is_float else "u16", out_type))


def test_window_refusals_write_nothing(ipa, orc):
    import torch
    h, w = 97, 131
    data = _mosaic(util.SEED + 12600, h, w, True)
    src = _upload(ipa, data)
    L = ipa.lib()
    out = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    plan = ipa.FusedPlan(**_plan_kw(ipa, orc, data, NOCROP, "RGGB", F32))
    four = ipa.FusedPlan(**_plan_kw(ipa, orc, data, NOCROP, "RGBE", F32))
    corners = (3, 4, 120, 9, 1, 90)
    nw, nh = 118, 87
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (nw - 1, 0, 2, 1), (0, nh - 1, 1, 2), (nw, 0, 1, 1), (0, nh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        assert L.ipk_raw_to_srgb_resampled_window(plan._ref, src.data_ptr(), *corners, nw, nh, *win, out.data_ptr(), ipa._stream()) == INVALID, win
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (86, 0, 2, 1), (0, 63, 1, 2), (87, 0, 1, 1), (0, 64, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        assert L.ipk_raw_to_srgb_scaled_window(plan._ref, src.data_ptr(), 87, 64, *win, out.data_ptr(), ipa._stream()) == INVALID, win
    # admission is that of the whole-frame forms
    assert L.ipk_raw_to_srgb_resampled_window(plan._ref, src.data_ptr(), 0, 0, 130, 0, 0, 96, 60, 48, 0, 0, 2, 2, out.data_ptr(), ipa._stream()) == rcf.UNSUPPORTED
    assert L.ipk_raw_to_srgb_scaled_window(plan._ref, src.data_ptr(), 40, 30, 0, 0, 2, 2, out.data_ptr(), ipa._stream()) == rcf.UNSUPPORTED
    assert L.ipk_raw_to_srgb_resampled_window(four._ref, src.data_ptr(), *corners, nw, nh, 0, 0, 2, 2, out.data_ptr(), ipa._stream()) == rcf.UNSUPPORTED
    assert L.ipk_raw_to_srgb_scaled_window(four._ref, src.data_ptr(), 87, 64, 0, 0, 2, 2, out.data_ptr(), ipa._stream()) == rcf.UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to dst"


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("out_type", [F32, U8, U16])
def test_window_writes_only_its_samples(ipa, orc, out_type, off):
    """guard bands around a destination that starts 0 / 1 element past a 256-byte boundary (the source too): ww * wh * 3 samples, nothing else"""
    import torch
    h, w = 97, 131
    L = ipa.lib()
    for is_float in (False, True):
        data = _mosaic(util.SEED + 12700 + is_float, h, w, is_float)
        src = util.Embedded(data, off)
        plan = ipa.FusedPlan(**_plan_kw(ipa, orc, data, NOCROP, XT, out_type))
        for scaled, corners in ((False, orc.rotatecrop_corners(R9[8], w, h)), (True, ((0, 0), (w - 1, 0), (0, h - 1), 87, 64))):
            tl, tr, bl, nw, nh = corners
            want = _oracle_ops(orc, data, NOCROP, XT, util.BLACK, util.WHITE, corners, util.WB, util.cam_matrix(), 0.0, [(0.5, 0.6)], False, out_type)
            for wx, wy, ww, wh in ((nw - 1, nh - 1, 1, 1), (21, 13, 45, 40), (nw // 3, 0, 1, nh), (0, nh // 2, nw, 1)):
                g = util.Guarded(ww * wh * 3, NP_OUT[out_type], off)
                if scaled:
                    rc = L.ipk_raw_to_srgb_scaled_window(plan._ref, src.ptr, nw, nh, wx, wy, ww, wh, g.ptr, ipa._stream())
                else:
                    rc = L.ipk_raw_to_srgb_resampled_window(plan._ref, src.ptr, tl[0], tl[1], tr[0], tr[1], bl[0], bl[1], nw, nh, wx, wy, ww, wh, g.ptr, ipa._stream())
                assert rc == 0, L.ipk_last_error()
                torch.cuda.synchronize()
                tag = "%s %s %s off %d window %r" % ("scaled" if scaled else "resampled", "f32" if is_float else "u16", out_type, off, (wx, wy, ww, wh))
                _same(g.result(tag).reshape(wh, ww, 3), want[wy:wy + wh, wx:wx + ww], tag)
        src.assert_untouched("window launches")


# ---------------------------------------------------------------------------------------------
# pipeline level
# ---------------------------------------------------------------------------------------------
def _timed_region(ipa, pipe, x, y, w, h, code):
    from imagepipe_amd import _lib
    L = ipa.lib()
    _lib.check(L.ipk_timing_begin(), "ipk_timing_begin")
    with ipa.launch_log() as ran:
        got = pipe.run_region(x, y, w, h, code)
    arr = (_lib.StageTime * 16)()
    n = C.c_int(0)
    _lib.check(L.ipk_timing_end(arr, 16, C.byref(n)), "ipk_timing_end")
    return got, ran, [arr[i].name.decode() for i in range(min(n.value, 16))]


def _check_pipeline_regions(ipa, orc, data, cfa, crops, ops, out_types, tag, route, shortcut=False):
    """route: "rotatecrop" / "scaled".  With the bit: windowed, the window launch alone; without: the whole result and a copy; the same bits, the
    oracle's and the whole run's"""
    build = sdf._pipeline if route == "scaled" else rcf._pipeline
    pipe = build(ipa, data, cfa, crops, ops)
    pipe.fuse_rotatecrop, pipe.fuse_scaledown = route == "rotatecrop", route == "scaled"
    _, (fw, fh) = pipe.sizes()
    for out_type in out_types:
        code = CODES[out_type]
        want = _want(orc, _oracle_desc(orc, data, cfa, crops, ops), out_type)
        assert want.shape[:2] == (fh, fw), tag
        pipe.window_regions = False
        whole = rcf._out(pipe, out_type)
        assert pipe.last_used_fused is True, tag
        _same(whole, want, "%s %s whole run" % (tag, out_type))
        for reg in _windows(fw, fh):
            x, y, w, h = reg
            t = "%s %s region %r" % (tag, out_type, reg)
            pipe.window_regions = True
            assert pipe.region(x, y, w, h, code)[0] == 1, t
            got, ran, stages = _timed_region(ipa, pipe, x, y, w, h, code)
            assert pipe.last_region_windowed is True, t
            _same(_np(got, out_type, h, w), want[y:y + h, x:x + w], t)
            if shortcut:
                assert any("k_fused_bayer_window" in e for e in ran) and not [e for e in ran if "k_fused_resample" in e], "%s: %r" % (t, sorted(ran))
                assert not [e for e in ran if any(k in e for k in WHOLE_FRAME_KERNELS)], "%s: %r" % (t, sorted(ran))
            else:
                _assert_window_launch(ran, t, route == "scaled")
            assert stages and all(s.startswith("fused region") for s in stages[:1]) and not [s for s in stages if "region copy" in s], (t, stages)
            assert ("rotatecrop" if route == "rotatecrop" else "demosaic(scaled)") in stages[0], (t, stages)
            pipe.window_regions = False
            assert pipe.region(x, y, w, h, code)[0] == 0, t
            got, ran, stages = _timed_region(ipa, pipe, x, y, w, h, code)
            assert pipe.last_region_windowed is False, t
            assert "region copy" in stages and not [e for e in ran if "win=1" in e], (t, stages, sorted(ran))
            _same(_np(got, out_type, h, w), want[y:y + h, x:x + w], t + " without the bit")
    return pipe


ORIENTATIONS = [(r, f) for r in range(4) for f in (False, True)]


@pytest.mark.parametrize("rot,fh", ORIENTATIONS)
def test_rotatecrop_regions_all_orientations(ipa, orc, rot, fh):
    w, h, crops = 96, 120, SENSOR_CROPS
    is_float = bool(rot % 2)
    data = _mosaic(util.SEED + 12800 + 2 * rot + fh, h, w, is_float)
    _check_pipeline_regions(ipa, orc, data, "GRBG", crops, dict(rotatecrop=R9[3], rotation=rot, fliph=fh), (F32, U8, U16), "rot.2 orientation %d/%s" % (rot, fh), "rotatecrop")


@pytest.mark.parametrize("k", [2, 5, 6, 8], ids=["rot.04", "rot.77", "rot1.0", "crop+rot.04"])
@pytest.mark.parametrize("cfa", ["RGGB", XT], ids=["RGGB", "xtrans"])
def test_rotatecrop_regions_transforms(ipa, orc, cfa, k):
    w, h, crops = 96, 120, SENSOR_CROPS
    data = _mosaic(util.SEED + 12900 + k, h, w, k % 2 == 0)
    _check_pipeline_regions(ipa, orc, data, cfa, crops, dict(rotatecrop=R9[k]), (F32, U8), "%s %s" % (cfa[:6], R9_IDS[k]), "rotatecrop")


@pytest.mark.parametrize("rot,fh", ORIENTATIONS)
@pytest.mark.parametrize("is_float", [False, True], ids=["u16-shortcut", "f32-general"])
def test_crop_only_regions_all_orientations(ipa, orc, is_float, rot, fh):
    """a crop without an angle: u16 frames take the crop-only shortcut (the fused Bayer kernel's window form over the intersection of the two
    rectangles), f32 frames the general kernel"""
    w, h, crops = 96, 120, SENSOR_CROPS
    data = _mosaic(util.SEED + 13000 + 2 * rot + fh, h, w, is_float)
    _check_pipeline_regions(ipa, orc, data, "RGGB", crops, dict(rotatecrop=R9[1], rotation=rot, fliph=fh), (F32, U8, U16),
                            "crop-uneven %s orientation %d/%s" % ("f32" if is_float else "u16", rot, fh), "rotatecrop", shortcut=not is_float)


@pytest.mark.parametrize("rot,fh", ORIENTATIONS)
def test_scaledown_regions_all_orientations(ipa, orc, rot, fh):
    w, h, crops, lim, _ = SMALL["131x97@87"]
    data = _mosaic(util.SEED + 13100 + 2 * rot + fh, h, w, bool(rot % 2))
    _check_pipeline_regions(ipa, orc, data, "RGGB" if fh else XT, crops, dict(rotation=rot, fliph=fh, **lim), (F32, U8, U16), "131x97@87 orientation %d/%s" % (rot, fh), "scaled")


@pytest.mark.parametrize("frame,cfa", [("96x120c@h80", XT), ("101x103@51", "GRBG"), ("150x100xt@60", XT)], ids=["96x120c@h80", "101x103@51", "150x100xt@60"])
def test_scaledown_regions_frames(ipa, orc, frame, cfa):
    w, h, crops, lim, _ = SMALL[frame]
    data = _mosaic(util.SEED + 13200 + len(frame), h, w, frame.startswith("101"))
    _check_pipeline_regions(ipa, orc, data, cfa, crops, dict(lim), (F32, U16), frame, "scaled")


# ---------------------------------------------------------------------------------------------
# the launch reads only the window it reports
# ---------------------------------------------------------------------------------------------
READ_CASES = {
    "rot.2-f32": ("rotatecrop", "GRBG", True, dict(rotatecrop=R9[3]), (96, 120, SENSOR_CROPS)),
    "rot.2-u16-rot90": ("rotatecrop", XT, False, dict(rotatecrop=R9[3], rotation=1, fliph=True), (96, 120, SENSOR_CROPS)),
    "rot1.0-f32": ("rotatecrop", "RGGB", True, dict(rotatecrop=R9[6]), (96, 120, SENSOR_CROPS)),
    "crop-u16-shortcut": ("rotatecrop", "RGGB", False, dict(rotatecrop=R9[1], rotation=2), (96, 120, SENSOR_CROPS)),
    "crop-f32": ("rotatecrop", "BGGR", True, dict(rotatecrop=R9[0]), (96, 120, SENSOR_CROPS)),
    "scaled-u16": ("scaled", "RGGB", False, dict(maxwidth=87, rotation=3), (131, 97, NOCROP)),
    "scaled-f32-crops": ("scaled", XT, True, dict(maxheight=80), (96, 120, SENSOR_CROPS)),
    "scaled-2.53-f32": ("scaled", XT, True, dict(maxwidth=60), (150, 100, NOCROP)),
}


def _poisoned(data, sx, sy, sw, sh):
    out = np.full_like(data, np.nan if data.dtype == np.float32 else 0xFFFF)
    out[sy:sy + sh, sx:sx + sw] = data[sy:sy + sh, sx:sx + sw]
    return out


@pytest.mark.parametrize("case", list(READ_CASES))
def test_region_reads_only_the_reported_window(ipa, orc, case):
    """everything outside the window ipk_pipeline_region reports is NaN (f32) / 0xFFFF (u16): the inputs are noise, so any stray read -- even one
    with weight zero -- changes the result.  From device memory and through ipk_host_pipeline_run_region"""
    import torch
    from imagepipe_amd import _lib
    route, cfa, is_float, ops, (w, h, crops) = READ_CASES[case]
    build = sdf._pipeline if route == "scaled" else rcf._pipeline
    data = _mosaic(util.SEED + 13300 + len(case), h, w, is_float)
    clean = build(ipa, data, cfa, crops, ops)
    clean.fuse_rotatecrop, clean.fuse_scaledown, clean.window_regions = route == "rotatecrop", route == "scaled", True
    _, (fw, fh) = clean.sizes()
    L = ipa.lib()
    wholes = {t: rcf._out(clean, t) for t in (F32, U8, U16)}
    for i, reg in enumerate(_windows(fw, fh)[:7]):
        x, y, rw, rh = reg
        out_type = [F32, U8, U16][i % 3]
        code = CODES[out_type]
        whole = wholes[out_type]
        win, (sx, sy, sw, sh) = clean.region(x, y, rw, rh, code)
        assert win == 1, (case, reg)
        assert sx + sw <= w and sy + sh <= h
        bad = _poisoned(data, sx, sy, sw, sh)
        if sw * sh < data.size:
            assert not np.array_equal(bad.view(np.uint8), data.view(np.uint8)), "nothing is poisoned: the case tests nothing"
        pipe = build(ipa, bad, cfa, crops, ops)
        pipe.fuse_rotatecrop, pipe.fuse_scaledown, pipe.window_regions = clean.fuse_rotatecrop, clean.fuse_scaledown, True
        got = pipe.run_region(x, y, rw, rh, code)
        torch.cuda.synchronize()
        assert pipe.last_region_windowed is True
        _same(_np(got, out_type, rh, rw), whole[y:y + rh, x:x + rw], "%s region %r %s from a poisoned device frame (window %r)" % (case, reg, out_type, (sx, sy, sw, sh)))
        host = np.zeros((rh, rw, 3), NP_OUT[out_type])
        wflag = C.c_int(-1)
        d = pipe.desc()
        _lib.check(L.ipk_host_pipeline_run_region(C.byref(d), bad.ctypes.data, x, y, rw, rh, host.ctypes.data, code, C.byref(wflag)), "ipk_host_pipeline_run_region")
        assert wflag.value == 1
        _same(host, whole[y:y + rh, x:x + rw], "%s region %r %s through the host form" % (case, reg, out_type))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("out_type", [F32, U8, U16])
def test_pipeline_region_writes_only_the_region(ipa, orc, out_type, off):
    import torch
    code = CODES[out_type]
    for route, cfa, ops, (w, h, crops) in (("rotatecrop", "RGGB", dict(rotatecrop=R9[3]), (96, 120, SENSOR_CROPS)),
                                           ("rotatecrop", "RGGB", dict(rotatecrop=R9[3], rotation=1), (96, 120, SENSOR_CROPS)),
                                           ("scaled", XT, dict(maxwidth=87), (131, 97, NOCROP))):
        data = _mosaic(util.SEED + 13400, h, w, route == "scaled")
        pipe = (sdf._pipeline if route == "scaled" else rcf._pipeline)(ipa, data, cfa, crops, ops)
        pipe.fuse_rotatecrop, pipe.fuse_scaledown, pipe.window_regions = route == "rotatecrop", route == "scaled", True
        whole = rcf._out(pipe, out_type)
        _, (fw, fh) = pipe.sizes()
        for x, y, rw, rh in (_windows(fw, fh)[i] for i in (3, 4, 6)):
            g = util.Guarded(rw * rh * 3, NP_OUT[out_type], off)
            pipe.run_region(x, y, rw, rh, code, out=g.view())
            torch.cuda.synchronize()
            assert pipe.last_region_windowed is True
            tag = "%s %s off %d region %r" % (route, out_type, off, (x, y, rw, rh))
            _same(g.result(tag).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw], tag)
