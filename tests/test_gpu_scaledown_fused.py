"""GPU parity of the one-launch route through OpDemosaic's `full` + scale_down_opbuf branch (k_fused_resample's axis-aligned mode: gofloat +
demosaic::full + scale_down_opbuf + tolab .. gamma + quantisation in one launch) against the CPU oracle, op level and pipeline level, and against
the staged route on the same descriptors.  Bar: bit-exact (0 ULP, any NaN == any NaN).  Every pipeline case asserts which route ran -- by the
report, by used_fused and by the launch log -- so an input that silently stayed staged fails.
Frames are about 100 x 130 pixels: the smallest that span several tiles in both directions with a partial last tile (the plan's tiles hold at
most 2048 outputs: 64 x 22 at skip 1.5, 16 x 16 near skip 3)."""
import ctypes as C
import re

import numpy as np
import pytest

import util
from util import assert_bits_equal
import test_gpu_rotatecrop_fused as rcf
from test_gpu_rotatecrop_fused import XT, W12, F32, U8, U16, UNSUPPORTED, SENSOR_CROPS, CURVE5, _mosaic, _upload, _np, _same, _oracle_ops, _oracle_desc, _out, _want

pytestmark = pytest.mark.gpu

NOCROP = (0, 0, 0, 0)
STAGE = "fused gofloat+demosaic(scaled)+to_lab+basecurve+from_lab+gamma"
STAGED_KERNELS = ("k_transform_buffer", "k_demosaic_full", "k_fused_bayer", "k_gofloat_cfa", "k_pointwise_chain", "k_raster_chain")
# (width, height, sensor crops, size limit, filters): the taken small frames of tests/test_scaledown_route.py
SMALL = {
    "131x97@87": (131, 97, NOCROP, dict(maxwidth=87), ("RGGB", "GRBG", XT, W12)),
    "96x120c@h80": (96, 120, SENSOR_CROPS, dict(maxheight=80), ("RGGB", XT)),
    "101x77@51": (101, 77, NOCROP, dict(maxwidth=51), (XT, W12)),             # skip_x exactly 2.0: 4-wide windows; scale 2.03 by its height, so no Bayer filter
    "101x103@51": (101, 103, NOCROP, dict(maxwidth=51), ("RGGB", "GRBG")),    # both skips exactly 2.0 at scale 1.98: 4x4 windows under a Bayer filter
    "131x97@130": (131, 97, NOCROP, dict(maxwidth=130), ("RGGB", XT)),        # skips just above 1
    "150x100xt@60": (150, 100, NOCROP, dict(maxwidth=60), (XT,)),             # skips about 2.53: 4x4 windows
}
FRAME_CFA = [(f, c) for f in SMALL for c in SMALL[f][4]]
FRAME_CFA_IDS = ["%s-%s" % (f, {4: c, 36: "xtrans", 144: "12x12"}[len(c)]) for f, c in FRAME_CFA]
CODES = {F32: 0, U8: 1, U16: 2}


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _pipeline(ipa, data, cfa, crops, ops, **lv):
    pipe = rcf._pipeline(ipa, data, cfa, crops, {k: v for k, v in ops.items() if k != "maxheight"}, **lv)
    if "maxheight" in ops:
        pipe.globals.settings.maxheight = ops["maxheight"]
    return pipe


def _logged(ipa, pipe, out_type, cache=None):
    with ipa.launch_log() as ran:
        got = _out(pipe, out_type, cache)
    return got, ran


def _assert_one_launch(ran, tag):
    assert any(re.search(r"k_fused_resample<.*\[.*axis=1", e) for e in ran), "%s: no k_fused_resample launch in its axis-aligned mode: %r" % (tag, sorted(ran))
    assert not [e for e in ran if any(k in e for k in STAGED_KERNELS)], "%s: staged kernels ran beside the one launch: %r" % (tag, sorted(ran))


def _assert_staged(ran, tag):
    # (ipk_demosaic_full is k_demosaic_full, or the fused kernel's demosaic-only variant for a Bayer filter)
    for ks in (("k_gofloat_cfa",), ("k_demosaic_full", "k_fused_bayer"), ("k_transform_buffer",), ("k_pointwise_chain", "k_raster_chain")):
        assert any(k in e for k in ks for e in ran), "%s: the staged route did not launch %s: %r" % (tag, " / ".join(ks), sorted(ran))
    assert not [e for e in ran if "k_fused_resample" in e], tag


def _check_both_routes(ipa, orc, data, cfa, crops, ops, out_types, tag, **lv):
    """with the flag: the one launch; without it: the staged route; both equal to the oracle (hence to each other)"""
    pipe = _pipeline(ipa, data, cfa, crops, ops, **lv)
    assert pipe.sizes() == orc.pipeline_sizes(_oracle_desc(orc, data, cfa, crops, ops, **lv)), tag
    for out_type in out_types:
        want = _want(orc, _oracle_desc(orc, data, cfa, crops, ops, **lv), out_type)   # a fresh descriptor: output_Nbit sets `linear` on the one it is given
        pipe.fuse_scaledown = True
        assert pipe.fuses_scaledown(CODES[out_type]) is True, tag
        got, ran = _logged(ipa, pipe, out_type)
        _same(got, want, "%s %s flag 1" % (tag, out_type))
        assert pipe.last_used_fused is True, "%s %s: the flagged run took the staged route" % (tag, out_type)
        _assert_one_launch(ran, "%s %s" % (tag, out_type))
        pipe.fuse_scaledown = False
        assert pipe.fuses_scaledown(CODES[out_type]) is False
        staged, ran = _logged(ipa, pipe, out_type)
        _same(staged, want, "%s %s flag 0" % (tag, out_type))
        _same(got, staged, "%s %s flag 1 against flag 0" % (tag, out_type))
        assert pipe.last_used_fused is False, "%s %s: flag 0 must stay staged" % (tag, out_type)
        _assert_staged(ran, "%s %s" % (tag, out_type))
    return pipe


# ---------------------------------------------------------------------------------------------
# op level: ipk_raw_to_srgb_scaled against the oracle's op-by-op composition
# ---------------------------------------------------------------------------------------------
def _negotiated(orc, w, h, crops, lim):
    (dw, dh), _ = orc.pipeline_sizes(orc.make_pipeline(np.zeros((h, w), np.uint16), cfa="RGGB", crops=crops, **lim))
    return dw, dh


def _gpu_op(ipa, orc, data, crops, cfa, black, white, nw, nh, wb, cam, exposure, points, linear, out_type):
    oh, ow = data.shape
    x, y, cw, ch = orc.size_image(*crops, ow, oh)
    out = ipa.raw_to_srgb_scaled(_upload(ipa, data), nw, nh, width=cw, height=ch, owidth=ow, x=x, y=y, is_float=data.dtype == np.float32, black0=black,
                                 white0=white, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), wb_coeffs=wb, cam_to_xyz_normalized=cam, exposure=exposure,
                                 points=points, linear=linear, out_type={F32: ipa.OUT_F32, U8: ipa.OUT_U8, U16: ipa.OUT_U16}[out_type])
    return _np(out, out_type, nh, nw)


@pytest.mark.parametrize("frame,cfa", FRAME_CFA, ids=FRAME_CFA_IDS)
def test_op_vs_oracle_composition(ipa, orc, frame, cfa):
    w, h, crops, lim, _ = SMALL[frame]
    nw, nh = _negotiated(orc, w, h, crops, lim)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    corners = ((0, 0), (cw - 1, 0), (0, ch - 1), nw, nh)                      # scale_down_opbuf's (src/scaling.rs:46)
    for is_float in (False, True):
        data = _mosaic(util.SEED + 9600 + len(frame) + len(cfa) + is_float, h, w, is_float)
        for out_type in (F32, U8, U16):
            tail = (util.WB, util.cam_matrix(), 0.0, [(0.5, 0.6)], False, out_type)
            want = _oracle_ops(orc, data, crops, cfa, util.BLACK, util.WHITE, corners, *tail)
            got = _gpu_op(ipa, orc, data, crops, cfa, util.BLACK, util.WHITE, nw, nh, *tail)
            _same(got, want, "op %s %s %s %s" % (frame, cfa[:6], "f32" if is_float else "u16", out_type))


def test_op_refuses_and_writes_nothing(ipa):
    import torch
    h, w = 100, 150
    src = _upload(ipa, _mosaic(util.SEED + 9700, h, w, True))

    def refused(cfa, nw, nh):
        out = torch.full((max(nw * nh, 1) * 3,), 7.0, dtype=torch.float32, device="cuda")
        plan = ipa.FusedPlan(width=w, height=h, is_float=True, black0=util.BLACK, white0=util.WHITE, cfa=cfa, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix())
        rc = ipa.lib().ipk_raw_to_srgb_scaled(plan._ref, src.data_ptr(), nw, nh, out.data_ptr(), ipa._stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (cfa[:6], nw, nh, rc)
        assert bool((out == 7.0).all()), "a refused call wrote to dst"

    refused(XT, 1, 60)                                                        # nwidth 1
    refused(XT, 60, 1)
    refused(XT, 52, 34)                                                       # skip_y = 99 / 33 = 3.0
    refused(XT, 40, 40)                                                       # skip_x = 149 / 39 > 3
    refused(XT, 151, 100)                                                     # a skip below 1: not a scale-down
    refused("RGBE", 100, 67)                                                  # a four-colour filter at an admitted size
    out = ipa.raw_to_srgb_scaled(src, 100, 67, width=w, height=h, is_float=True, black0=util.BLACK, white0=util.WHITE, cfa=XT, wb_coeffs=util.WB,
                                 cam_to_xyz_normalized=util.cam_matrix())   # the control: the same size with three colours is taken
    assert bool(torch.isfinite(out).all())


# ---------------------------------------------------------------------------------------------
# pipeline level
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("is_float", [False, True], ids=["u16", "f32"])
@pytest.mark.parametrize("frame,cfa", FRAME_CFA, ids=FRAME_CFA_IDS)
def test_pipeline_vs_oracle(ipa, orc, frame, cfa, is_float):
    w, h, crops, lim, _ = SMALL[frame]
    data = _mosaic(util.SEED + 9800 + len(frame) + len(cfa), h, w, is_float)
    _check_both_routes(ipa, orc, data, cfa, crops, dict(lim), (F32, U8, U16), "pipeline %s %s %s" % (frame, cfa[:6], "f32" if is_float else "u16"))


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (False, True)])
def test_pipeline_orientations_behind_the_launch(ipa, orc, rot, fh):
    w, h, crops, lim, _ = SMALL["96x120c@h80"]
    data = _mosaic(util.SEED + 9900 + 2 * rot + fh, h, w, bool(rot % 2))
    _check_both_routes(ipa, orc, data, "GRBG", crops, dict(lim, rotation=rot, fliph=fh), (F32, U8, U16), "orientation %d/%s" % (rot, fh))


CURVES = {"nocurve": dict(points=[]), "2knots": dict(points=[(0.3, 0.22), (0.7, 0.81)]), "3knots": dict(points=[(0.25, 0.2), (0.5, 0.6), (0.75, 0.85)]),
          "6knots": dict(points=CURVE5 + [(0.95, 0.97)]), "exposure": dict(exposure=0.7), "linear": dict(linear=True)}


@pytest.mark.parametrize("prm", list(CURVES))
def test_pipeline_curve_parameters(ipa, orc, prm):
    w, h, crops, lim, _ = SMALL["131x97@87"]
    data = _mosaic(util.SEED + 10000, h, w, True)
    _check_both_routes(ipa, orc, data, XT, crops, dict(lim, **CURVES[prm]), (F32, U8, U16), "parameters %s" % prm)


def test_run_timed_shows_the_single_stage(ipa, orc):
    w, h, crops, lim, _ = SMALL["131x97@87"]
    data = _mosaic(util.SEED + 10100, h, w, False)
    pipe = _pipeline(ipa, data, "RGGB", crops, dict(lim))
    pipe.fuse_scaledown = True
    out, stages = pipe.run_timed()
    assert [s[0] for s in stages] == [STAGE] and STAGE.startswith("fused") and stages[0][1] > 0.0, stages
    _, (fw, fh) = pipe.sizes()
    assert_bits_equal(out.cpu().numpy().reshape(fh, fw, 3), orc.pipeline_run(_oracle_desc(orc, data, "RGGB", crops, dict(lim))), "timed run")
    pipe.fuse_scaledown = False
    _, stages = pipe.run_timed()
    assert len(stages) > 1 and "demosaic" in [s[0] for s in stages], stages
    oriented = _pipeline(ipa, data, "RGGB", crops, dict(lim, rotation=1))
    oriented.fuse_scaledown = True
    _, stages = oriented.run_timed()
    assert [s[0] for s in stages] == [STAGE, "transform"], stages


# ---------------------------------------------------------------------------------------------
# hostile data
# ---------------------------------------------------------------------------------------------
def _planted(orc, w, h, crops, lim):
    """sensor positions of special samples: the first and the last tap of an interior window (its corners: zero weight, and 0 * inf is NaN), and the
    cropped frame's four edges"""
    nw, nh = _negotiated(orc, w, h, crops, lim)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    f = np.float32
    sx, sy = f(cw - 1) / f(nw - 1), f(ch - 1) / f(nh - 1)
    r, c = nh // 2, nw // 3
    win = [(int(np.floor(sy * f(r))), int(np.floor(sx * f(c)))), (int(np.floor(sy * f(r + 5))), int(np.floor(sx * f(c + 7)))),
           (min(ch - 1, int(np.floor(sy * f(r + 11)))), min(cw - 1, int(np.floor(sx * f(c + 16)))))]
    edges = [(0, cw // 2), (ch - 1, cw // 4), (ch // 3, 0), (ch // 2, cw - 1), (0, 0), (ch - 1, cw - 1)]
    return [(crops[0] + y, crops[3] + x) for y, x in win + edges]


# (scale 2.5 is scaled_demosaic's branch for a Bayer filter: X-Trans and the 12x12 pattern stay in this one)
HOSTILE = [("96x120c@h80", "BGGR"), ("96x120c@h80", XT), ("101x103@51", "BGGR"), ("101x77@51", XT), ("150x100xt@60", XT), ("150x100xt@60", W12)]


@pytest.mark.parametrize("levels", [(0.0, 1.0), (util.BLACK, util.WHITE), (0.0, 1e-37)], ids=["unit", "14bit", "tiny-range"])
@pytest.mark.parametrize("frame,cfa", HOSTILE, ids=["%s-%s" % (f, {4: c, 36: "xtrans", 144: "12x12"}[len(c)]) for f, c in HOSTILE])
def test_hostile_f32_mosaics(ipa, orc, frame, cfa, levels):
    w, h, crops, lim, _ = SMALL[frame]
    black, white = levels
    data = rcf._hostile_mosaic(10200 + len(frame) + len(cfa), h, w, max(white, 1.0))
    tame = data.copy()
    vals = [-np.inf, np.inf, -np.inf, np.nan, -0.0, -np.inf, np.inf, -3e38, 3e38]
    for (y, x), v in zip(_planted(orc, w, h, crops, lim), vals):
        data[y, x] = v
        tame[y, x] = 0.5 * white
    _check_both_routes(ipa, orc, data, cfa, crops, dict(lim), (F32, U8, U16), "hostile %s %s levels %r" % (frame, cfa[:6], levels), black=black, white=white)
    # (OpToLab's min(1.0) turns a NaN channel into 1.0, so what the planted values do shows as changed pixels, not as NaN)
    want, without = (orc.pipeline_run(_oracle_desc(orc, d, cfa, crops, dict(lim), black=black, white=white)) for d in (data, tame))
    changed = (want.view(np.uint32) != without.view(np.uint32)).any(axis=2)
    assert changed.sum() > len(vals), "the planted values do not reach neighbouring outputs: the case tests nothing"


@pytest.mark.parametrize("levels", [(util.BLACK, util.WHITE), (700.0, 700.0), (0.0, 1e-37), (util.WHITE, util.BLACK)], ids=["14bit", "empty-range", "tiny-range", "black>white"])
@pytest.mark.parametrize("frame", ["131x97@87", "101x103@51"])
@pytest.mark.parametrize("cfa", ["BGGR", XT], ids=["BGGR", "xtrans"])
def test_extreme_u16_mosaics(ipa, orc, cfa, frame, levels):
    """0 and 65535 among ordinary samples; with an empty, tiny or negative range (v - black) / range is inf, -inf, NaN or negative and the
    normalisation takes the literal division -- either way the bytes are the oracle's"""
    w, h, crops, lim, _ = SMALL[frame]
    black, white = levels
    rng = np.random.default_rng(10300 + len(frame))
    data = rng.integers(0, 1400, size=(h, w)).astype(np.uint16)
    flat = data.reshape(-1)
    flat[rng.choice(flat.size, 64, replace=False)] = np.array([0, 65535, 511, 512, 513, 699, 700, 701, 16383, 16384, 65535, 40000, 0, 3, 1023, 1024] * 4, np.uint16)
    data[0, 0], data[h - 1, w - 1], data[0, w - 1], data[h - 1, 0] = 65535, 0, 0, 65535
    _check_both_routes(ipa, orc, data, cfa, crops, dict(lim), (F32, U8, U16), "extreme u16 %s %s levels %r" % (frame, cfa[:6], levels), black=black, white=white)


# ---------------------------------------------------------------------------------------------
# the drivers
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_type", [F32, U8, U16])
def test_drivers_agree(ipa, orc, out_type):
    """the plain run, the cold cached run, a warm hit, a batch of three, the host-pointer run and two regions: one route, one result"""
    import torch
    w, h, crops, lim, _ = SMALL["96x120c@h80"]
    frames = [_mosaic(util.SEED + 10400 + i, h, w, True) for i in range(3)]
    ops = dict(lim)
    wants = [_want(orc, _oracle_desc(orc, f, XT, crops, ops), out_type) for f in frames]
    code = CODES[out_type]
    pipes = [_pipeline(ipa, f, XT, crops, ops) for f in frames]
    for flag in (True, False):
        for p in pipes:
            p.fuse_scaledown = flag
        pipe = pipes[0]
        tag = "%s flag %d" % (out_type, flag)
        _same(_out(pipe, out_type), wants[0], tag + " run")
        assert pipe.last_used_fused is flag
        cache = ipa.PipelineCache(1 << 28)
        try:
            got, ran = _logged(ipa, pipe, out_type, cache)
            _same(got, wants[0], tag + " cold cached run")
            assert pipe.last_used_fused is flag and pipe.last_ops_run == 0xFF        # every op reported as run
            if flag:                                                                 # one launch, only the final buffer is stored
                assert cache.stats()["entries"] == 1 and cache.contains(pipe.hashes(code)[7]) and not cache.contains(pipe.hashes(code)[1])
                assert any(re.search(r"k_fused_resample<.*axis=1", e) for e in ran) and not [e for e in ran if any(k in e for k in STAGED_KERNELS)], sorted(ran)
            else:
                assert cache.stats()["entries"] > 1 and cache.contains(pipe.hashes(code)[1])
            _same(_out(pipe, out_type, cache), wants[0], tag + " warm hit")
            assert pipe.last_ops_run == 0
        finally:
            cache.close()
        _, (fw, fh) = pipe.sizes()
        dt = {F32: torch.float32, U8: torch.uint8, U16: torch.int16}[out_type]
        outs = [torch.empty(fw * fh * 3, dtype=dt, device="cuda") for _ in range(3)]
        srcs = (C.c_void_p * 3)(*[p.globals.image.data.data_ptr() for p in pipes]); dsts = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
        used = C.c_int(-1)
        assert ipa.lib().ipk_pipeline_run_batch(C.byref(pipe.desc()), srcs, dsts, 3, code, C.byref(used), ipa._stream()) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
        assert bool(used.value) is flag, tag + ": batch of three"
        for i in range(3):
            _same(_np(outs[i], out_type, fh, fw), wants[i], tag + " batch frame %d" % i)
        host = np.empty(fw * fh * 3, {F32: np.float32, U8: np.uint8, U16: np.uint16}[out_type])
        src = np.ascontiguousarray(frames[0])
        used = C.c_int(-1)
        assert ipa.lib().ipk_host_pipeline_run(C.byref(pipe.desc()), src.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), code, C.byref(used)) == 0, ipa.lib().ipk_last_error()
        assert bool(used.value) is flag, tag + ": host run"
        _same(host.reshape(fh, fw, 3), wants[0], tag + " host run")
        for x, y, rw, rh in ((fw // 4, fh // 3, 23, 17), (fw - 19, 0, 19, fh)):      # an interior rectangle, and one on three edges
            reg = _np(pipe.run_region(x, y, rw, rh, code), out_type, rh, rw)
            assert pipe.last_region_windowed is False                                # whole frame, copy out
            _same(reg, np.ascontiguousarray(wants[0][y:y + rh, x:x + rw]), tag + " region %r" % ((x, y, rw, rh),))


# ---------------------------------------------------------------------------------------------
# one full-size frame: every output sample is compared (the oracle takes a few seconds)
# ---------------------------------------------------------------------------------------------
def test_full_frame_vs_oracle(ipa, orc):
    h, w = 4000, 6000
    data = rcf._big(util.SEED + 10500, h, w, False)
    ops = dict(maxwidth=3840)
    want = _want(orc, _oracle_desc(orc, data, "RGGB", NOCROP, ops), U8)
    assert want.shape == (2560, 3840, 3)
    pipe = _pipeline(ipa, data, "RGGB", NOCROP, ops)
    for flag in (True, False):
        pipe.fuse_scaledown = flag
        got = _out(pipe, U8)
        assert pipe.last_used_fused is flag
        _same(got, want, "full frame 6000x4000 u16 -> u8 at maxwidth 3840, flag %d" % flag)
        del got
