"""GPU parity of the one-launch route through an active OpRotateCrop (k_fused_resample: gofloat + demosaic::full + transform_buffer + tolab ..
gamma + quantisation in one launch) against the CPU oracle, op level and pipeline level, and against the staged route on the same descriptors.
Bar: bit-exact (0 ULP, any NaN == any NaN).  No case is skipped or filtered: every pipeline case asserts which route ran, so an input that
silently stayed staged fails."""
import ctypes as C

import numpy as np
import pytest

import util
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
W12 = (XT[0:6] + XT[18:24] + XT[6:12] + XT[24:30] + XT[12:18] + XT[30:36]) * 2 + (XT[18:24] + XT[0:6] + XT[24:30] + XT[6:12] + XT[30:36] + XT[12:18]) * 2
W12 = (W12 * 2)[:144]
F32, U8, U16 = "f32", "u8", "u16"
UNSUPPORTED = -5                                                          # IPK_ERR_UNSUPPORTED
SENSOR_CROPS = (3, 1, 2, 5)                                               # top, right, bottom, left: odd offsets
STAGE = "fused gofloat+demosaic+rotatecrop+to_lab+basecurve+from_lab+gamma(+transform)"


def f32s(*v):
    return tuple(float(np.float32(x)) for x in v)


# (crop_top, crop_right, crop_bottom, crop_left, rotation); at 0.77 about half of the windows are empty, at 1.0 and 1.3 nearly all
R9 = [f32s(0.05, 0.05, 0.05, 0.05, 0), f32s(0.1, 0.05, 0.2, 0, 0), f32s(0, 0, 0, 0, 0.04), f32s(0.1, 0, 0, 0, 0.2), f32s(0, 0, 0, 0, 0.5),
      f32s(0.02, 0.03, 0.01, 0.02, 0.77), f32s(0, 0, 0, 0, 1.0), f32s(0, 0, 0, 0, 1.3), f32s(0.07, 0.11, 0.05, 0.02, 0.04)]
R9_IDS = ["crop5", "crop-uneven", "rot.04", "rot.2", "rot.5", "rot.77", "rot1.0", "rot1.3", "crop+rot.04"]
# (width, height, sensor crops): every R9 setting negotiates a demosaic size >= the cropped frame here (tests/test_rotatecrop_route.py)
FRAMES = {"47x61": (47, 61, (0, 0, 0, 0)), "96x120c": (96, 120, SENSOR_CROPS)}
CURVE5 = [(0.1, 0.07), (0.3, 0.33), (0.5, 0.6), (0.7, 0.78), (0.9, 0.93)]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _mosaic(seed, h, w, is_float):
    data = util.noise_u16(seed, h, w)
    if is_float:
        data = data.astype(np.float32) + util.uniform_f32(seed + 1, data.size, -0.5, 0.5).reshape(data.shape)
    return data


def _upload(ipa, data):
    import torch
    return torch.from_numpy(np.ascontiguousarray(data, np.float32).ravel()).cuda() if data.dtype == np.float32 else ipa.upload_u16(data)


def _np(t, out_type, nh, nw):
    a = t.cpu().numpy()
    return (a.view(np.uint16) if out_type == U16 else a).reshape(nh, nw, 3)


def _same(got, want, what):
    if want.dtype == np.float32:
        assert_bits_equal(got, want, what)
    else:
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d samples differ" % (what, int((got != want).sum()) if got.shape == want.shape else -1)


# ---------------------------------------------------------------------------------------------
# op level: ipk_raw_to_srgb_resampled against the oracle's op-by-op composition
# ---------------------------------------------------------------------------------------------
def _oracle_ops(orc, data, crops, cfa, black, white, corners, wb, cam, exposure, points, linear, out_type):
    oh, ow = data.shape
    x, y, cw, ch = orc.size_image(*crops, ow, oh)
    tl, tr, bl, nw, nh = corners
    buf = orc.demosaic_full(orc.cfa_shift(cfa, crops[3], crops[0]), orc.gofloat_cfa(data, x, y, cw, ch, black, white))
    buf = orc.transform_buffer(buf, cw, ch, tl, tr, bl, nw, nh, 4)
    buf = orc.gamma(orc.fromlab(orc.basecurve(orc.tolab(buf, wb, cam), exposure, points)), linear)
    return buf if out_type == F32 else (orc.output8bit(buf) if out_type == U8 else orc.output16bit(buf))


def _gpu_op(ipa, orc, data, crops, cfa, black, white, corners, wb, cam, exposure, points, linear, out_type):
    oh, ow = data.shape
    x, y, cw, ch = orc.size_image(*crops, ow, oh)
    tl, tr, bl, nw, nh = corners
    out = ipa.raw_to_srgb_resampled(_upload(ipa, data), (tl[0], tl[1], tr[0], tr[1], bl[0], bl[1]), nw, nh, width=cw, height=ch, owidth=ow, x=x, y=y,
                                    is_float=data.dtype == np.float32, black0=black, white0=white, cfa=orc.cfa_shift(cfa, crops[3], crops[0]),
                                    wb_coeffs=wb, cam_to_xyz_normalized=cam, exposure=exposure, points=points, linear=linear,
                                    out_type={F32: ipa.OUT_F32, U8: ipa.OUT_U8, U16: ipa.OUT_U16}[out_type])
    return _np(out, out_type, nh, nw)


OP_CFAS = ["RGGB", "BGGR", "GRBG", "GBRG", XT, W12]
OP_SHAPES = [(23, 19), (61, 47), (97, 131), (40, 52), (77, 90), (64, 64)]      # (height, width)
OP_PARAMS = [dict(), dict(points=[]), dict(points=CURVE5), dict(exposure=0.7), dict(linear=True), dict(points=CURVE5, exposure=0.7, linear=True)]


@pytest.mark.parametrize("k", range(len(R9)), ids=R9_IDS)
@pytest.mark.parametrize("ci", range(len(OP_CFAS)), ids=["RGGB", "BGGR", "GRBG", "GBRG", "xtrans", "12x12"])
def test_op_vs_oracle_composition(ipa, orc, ci, k):
    """every filter meets every R9 transform; frame size, sensor crops, source type, output type and curve parameters rotate with the case"""
    i = ci + k
    h, w = OP_SHAPES[i % len(OP_SHAPES)]
    crops = SENSOR_CROPS if i % 2 else (0, 0, 0, 0)
    is_float = bool((ci + k // 2) % 2)
    out_type = [F32, U8, U16][(ci + 2 * k) % 3]
    prm = dict(exposure=0.0, points=[(0.5, 0.6)], linear=False)
    prm.update(OP_PARAMS[(2 * ci + k) % len(OP_PARAMS)])
    data = _mosaic(util.SEED + 8100 + 16 * ci + k, h, w, is_float)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    corners = orc.rotatecrop_corners(R9[k], cw, ch)
    assert corners is not None
    args = (data, crops, OP_CFAS[ci], util.BLACK, util.WHITE, corners, util.WB, util.cam_matrix(), prm["exposure"], prm["points"], prm["linear"], out_type)
    _same(_gpu_op(ipa, orc, *args), _oracle_ops(orc, *args), "op %s %s %dx%d crops %r %s %r" % (OP_CFAS[ci][:6], R9_IDS[k], w, h, crops, out_type, prm))


@pytest.mark.parametrize("out_type", [F32, U8, U16])
@pytest.mark.parametrize("is_float", [False, True], ids=["u16", "f32"])
@pytest.mark.parametrize("name,corners", [
    ("outside", ((-4, -3), (58, 5), (-9, 49), 57, 44)),                       # corners outside the frame on every side: the windows clamp
    ("narrow", ((5, 40), (6, 39), (30, 44), 2, 31)),                          # nwidth = 2: both skip_x are whole pixels, one of them negative
    ("mirror", ((50, 3), (4, 3), (50, 40), 47, 38)),                          # a negative skip_x_x
    ("flat", ((3, 7), (3, 7), (3, 7), 9, 6)),                                 # every skip zero: each division is by zero
], ids=["outside", "narrow", "mirror", "flat"])
def test_op_clamped_and_degenerate_transforms(ipa, orc, name, corners, is_float, out_type):
    h, w = 47, 61
    data = _mosaic(util.SEED + 8300 + len(name), h, w, is_float)
    args = (data, (0, 0, 0, 0), "GRBG", util.BLACK, util.WHITE, corners, util.WB, util.cam_matrix(), 0.0, [(0.5, 0.6)], False, out_type)
    _same(_gpu_op(ipa, orc, *args), _oracle_ops(orc, *args), "op %s %s" % (name, out_type))


def test_op_refuses_large_windows_and_writes_nothing(ipa):
    import torch
    h, w = 47, 61
    src = _upload(ipa, _mosaic(util.SEED + 8400, h, w, True))
    for corners, nw, nh in (((0, 0, 60, 0, 0, 46), 30, 23),                   # skip_x_x = 60 / 29 > 2: scaling down
                            ((0, 0, 40, 40, 0, 46), 41, 47),                  # |skip_x_x| + |skip_y_x| fine, |skip_x_y| + |skip_y_y| = 1 + 1 = 2
                            ((0, 0, 60, 0, 0, 46), 61, 1)):                   # one output row
        out = torch.full((nw * nh * 3,), 7.0, dtype=torch.float32, device="cuda")
        plan = ipa.FusedPlan(width=w, height=h, is_float=True, black0=util.BLACK, white0=util.WHITE, cfa="RGGB", wb_coeffs=util.WB,
                             cam_to_xyz_normalized=util.cam_matrix())
        rc = ipa.lib().ipk_raw_to_srgb_resampled(plan._ref, src.data_ptr(), *corners, nw, nh, out.data_ptr(), ipa._stream())
        torch.cuda.synchronize()
        assert rc == UNSUPPORTED, (corners, nw, nh, rc)
        assert bool((out == 7.0).all()), "a refused call wrote to dst"
    plan = ipa.FusedPlan(width=w, height=h, is_float=True, black0=util.BLACK, white0=util.WHITE, cfa="RGBE", wb_coeffs=util.WB,
                         cam_to_xyz_normalized=util.cam_matrix())
    out = torch.full((40 * 30 * 3,), 7.0, dtype=torch.float32, device="cuda")
    assert ipa.lib().ipk_raw_to_srgb_resampled(plan._ref, src.data_ptr(), 2, 2, 41, 2, 2, 31, 40, 30, out.data_ptr(), ipa._stream()) == UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())


# ---------------------------------------------------------------------------------------------
# pipeline level
# ---------------------------------------------------------------------------------------------
def _pipeline(ipa, data, cfa, crops, ops, black=util.BLACK, white=util.WHITE, wb=util.WB, cam=None):
    h, w = data.shape
    is_float = data.dtype == np.float32
    img = ipa.RawImage(width=w, height=h, data=_upload(ipa, data), cpp=1, cfa=cfa, crops=crops, blacklevels=[black] * 4, whitelevels=[white] * 4,
                       wb_coeffs=wb, cam_to_xyz_normalized=util.cam_matrix() if cam is None else cam, is_float=is_float)
    pipe = ipa.Pipeline.new_from_source(img)
    r = pipe.ops.rotatecrop
    r.crop_top, r.crop_right, r.crop_bottom, r.crop_left, r.rotation = ops.get("rotatecrop", (0.0,) * 5)
    for k in ("rotation", "fliph", "flipv"):
        if k in ops:
            setattr(pipe.ops.transform, k, ops[k])
    for k in ("maxwidth", "linear"):
        if k in ops:
            setattr(pipe.globals.settings, k, ops[k])
    if "points" in ops:
        pipe.ops.basecurve.points = ops["points"]
    if "exposure" in ops:
        pipe.ops.basecurve.exposure = ops["exposure"]
    return pipe


def _oracle_desc(orc, data, cfa, crops, ops, black=util.BLACK, white=util.WHITE, wb=util.WB, cam=None):
    return orc.make_pipeline(data, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), crops=crops, blacklevels=[black] * 4, whitelevels=[white] * 4,
                             wb_coeffs=wb, cam_to_xyz_normalized=util.cam_matrix() if cam is None else cam, **ops)


def _out(pipe, out_type, cache=None):
    if out_type == F32:
        return pipe.run(cache).numpy()
    ww, hh, o = pipe.output_8bit(cache) if out_type == U8 else pipe.output_16bit(cache)
    return _np(o, out_type, hh, ww)


def _want(orc, desc, out_type):
    return {F32: orc.pipeline_run, U8: orc.pipeline_output_8bit, U16: orc.pipeline_output_16bit}[out_type](desc)


def _check_both_routes(ipa, orc, data, cfa, crops, ops, out_types, tag, fused=True, **lv):
    """with the flag: the one launch (or, fused=False, a descriptor that must stay staged); without it: the staged route; both equal to the oracle"""
    pipe = _pipeline(ipa, data, cfa, crops, ops, **lv)
    assert pipe.sizes() == orc.pipeline_sizes(_oracle_desc(orc, data, cfa, crops, ops, **lv)), tag
    for out_type in out_types:
        want = _want(orc, _oracle_desc(orc, data, cfa, crops, ops, **lv), out_type)   # a fresh descriptor: output_Nbit sets `linear` on the one it is given
        code = {F32: ipa.OUT_F32, U8: ipa.OUT_U8, U16: ipa.OUT_U16}[out_type]
        pipe.fuse_rotatecrop = True
        assert pipe.fuses_rotatecrop(code) is fused, tag
        _same(_out(pipe, out_type), want, "%s %s flag 1" % (tag, out_type))
        assert pipe.last_used_fused is fused, "%s %s: the flagged run took the %s route" % (tag, out_type, "staged" if fused else "fused")
        pipe.fuse_rotatecrop = False
        assert pipe.fuses_rotatecrop(code) is False
        _same(_out(pipe, out_type), want, "%s %s flag 0" % (tag, out_type))
        assert pipe.last_used_fused is False, "%s %s: flag 0 must stay staged" % (tag, out_type)
    return pipe


@pytest.mark.parametrize("k", range(len(R9)), ids=R9_IDS)
@pytest.mark.parametrize("is_float", [False, True], ids=["u16", "f32"])
@pytest.mark.parametrize("cfa", ["RGGB", XT], ids=["RGGB", "xtrans"])
@pytest.mark.parametrize("frame", list(FRAMES))
def test_pipeline_vs_oracle(ipa, orc, frame, cfa, is_float, k):
    w, h, crops = FRAMES[frame]
    data = _mosaic(util.SEED + 8500 + 32 * k + len(cfa), h, w, is_float)
    _check_both_routes(ipa, orc, data, cfa, crops, dict(rotatecrop=R9[k]), (F32, U8, U16), "pipeline %s %s %s %s" % (frame, cfa[:6], "f32" if is_float else "u16", R9_IDS[k]))


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (False, True)])
@pytest.mark.parametrize("k", [1, 3], ids=["crop-uneven", "rot.2"])
def test_pipeline_orientations_behind_the_launch(ipa, orc, k, rot, fh):
    w, h, crops = FRAMES["96x120c"]
    data = _mosaic(util.SEED + 8700 + 8 * k + 2 * rot + fh, h, w, bool(rot % 2))
    _check_both_routes(ipa, orc, data, "GRBG", crops, dict(rotatecrop=R9[k], rotation=rot, fliph=fh), (F32, U8, U16), "orientation %d/%s %s" % (rot, fh, R9_IDS[k]))


@pytest.mark.parametrize("prm", [dict(points=[]), dict(points=CURVE5), dict(exposure=0.7), dict(linear=True)], ids=["nocurve", "curve5", "exposure", "linear"])
def test_pipeline_curve_parameters(ipa, orc, prm):
    w, h, crops = FRAMES["47x61"]
    data = _mosaic(util.SEED + 8800, h, w, True)
    _check_both_routes(ipa, orc, data, XT, crops, dict(rotatecrop=R9[3], **prm), (F32, U8, U16), "parameters %r" % prm)


def test_pipeline_stays_staged_when_demosaic_scales(ipa, orc):
    """150x100 at (0.04, 0.01, 0.03, 0.02 | 0.02) negotiates a 149x99 demosaic size: OpDemosaic scales, and the flag changes nothing"""
    rc = f32s(0.04, 0.01, 0.03, 0.02, 0.02)
    data = _mosaic(util.SEED + 8900, 100, 150, False)
    (dw, dh), _ = orc.pipeline_sizes(_oracle_desc(orc, data, "RGGB", (0, 0, 0, 0), dict(rotatecrop=rc)))
    assert (dw, dh) == (149, 99)
    _check_both_routes(ipa, orc, data, "RGGB", (0, 0, 0, 0), dict(rotatecrop=rc), (F32, U8, U16), "one pixel short", fused=False)


@pytest.mark.parametrize("out_type", [F32, U8, U16])
@pytest.mark.parametrize("k", [0, 3, 5], ids=["crop5", "rot.2", "rot.77"])
def test_drivers_agree(ipa, orc, k, out_type):
    """the plain run, the cold cached run, a warm hit, a batch of two and the host-pointer run: one route, one result"""
    import torch
    w, h, crops = FRAMES["96x120c"]
    frames = [_mosaic(util.SEED + 9000 + 4 * k + i, h, w, True) for i in range(2)]
    ops = dict(rotatecrop=R9[k])
    wants = [_want(orc, _oracle_desc(orc, f, XT, crops, ops), out_type) for f in frames]
    code = {F32: ipa.OUT_F32, U8: ipa.OUT_U8, U16: ipa.OUT_U16}[out_type]
    pipes = [_pipeline(ipa, f, XT, crops, ops) for f in frames]
    for flag in (True, False):
        for p in pipes:
            p.fuse_rotatecrop = flag
        pipe = pipes[0]
        tag = "%s %s flag %d" % (R9_IDS[k], out_type, flag)
        _same(_out(pipe, out_type), wants[0], tag + " run")
        assert pipe.last_used_fused is flag
        cache = ipa.PipelineCache(1 << 28)
        try:
            _same(_out(pipe, out_type, cache), wants[0], tag + " cold cached run")
            assert pipe.last_used_fused is flag and pipe.last_ops_run == 0xFF
            assert cache.contains(pipe.hashes(code)[7]) and cache.contains(pipe.hashes(code)[1]) is (not flag)   # one launch: only the final buffer is stored
            _same(_out(pipe, out_type, cache), wants[0], tag + " warm hit")
            assert pipe.last_ops_run == 0
        finally:
            cache.close()
        _, (fw, fh) = pipe.sizes()
        dt = {F32: torch.float32, U8: torch.uint8, U16: torch.int16}[out_type]
        outs = [torch.empty(fw * fh * 3, dtype=dt, device="cuda") for _ in range(2)]
        srcs = (C.c_void_p * 2)(*[p.globals.image.data.data_ptr() for p in pipes]); dsts = (C.c_void_p * 2)(*[o.data_ptr() for o in outs])
        used = C.c_int(-1)
        assert ipa.lib().ipk_pipeline_run_batch(C.byref(pipe.desc()), srcs, dsts, 2, code, C.byref(used), ipa._stream()) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
        assert bool(used.value) is flag, tag + ": batch of two"
        for i in range(2):
            _same(_np(outs[i], out_type, fh, fw), wants[i], tag + " batch frame %d" % i)
        host = np.empty(fw * fh * 3, {F32: np.float32, U8: np.uint8, U16: np.uint16}[out_type])
        src = np.ascontiguousarray(frames[0])
        used = C.c_int(-1)
        assert ipa.lib().ipk_host_pipeline_run(C.byref(pipe.desc()), src.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), code, C.byref(used)) == 0, ipa.lib().ipk_last_error()
        assert bool(used.value) is flag, tag + ": host run"
        _same(host.reshape(fh, fw, 3), wants[0], tag + " host run")


def test_run_timed_shows_the_single_stage(ipa, orc):
    w, h, crops = FRAMES["47x61"]
    data = _mosaic(util.SEED + 9100, h, w, False)
    pipe = _pipeline(ipa, data, "RGGB", crops, dict(rotatecrop=R9[3]))
    pipe.fuse_rotatecrop = True
    out, stages = pipe.run_timed()
    assert [s[0] for s in stages] == [STAGE] and stages[0][1] > 0.0, stages
    _, (fw, fh) = pipe.sizes()
    assert_bits_equal(out.cpu().numpy().reshape(fh, fw, 3), orc.pipeline_run(_oracle_desc(orc, data, "RGGB", crops, dict(rotatecrop=R9[3]))), "timed run")
    pipe.fuse_rotatecrop = False
    _, stages = pipe.run_timed()
    assert len(stages) > 1 and "rotatecrop" in [s[0] for s in stages], stages


# ---------------------------------------------------------------------------------------------
# hostile f32 mosaics: NaN, +-inf, denormals, -0.0, samples below black, huge values -- crop-only and rotated, both kinds of levels
# ---------------------------------------------------------------------------------------------
def _hostile_mosaic(seed, h, w, top):
    rng = np.random.default_rng(seed)
    data = rng.uniform(-0.1 * top - 0.02, 1.2 * top, size=(h, w)).astype(np.float32)
    flat = data.reshape(-1)
    pos = rng.choice(flat.size, util.SPECIALS.size + 12, replace=False)
    with np.errstate(over="ignore", invalid="ignore"):
        flat[pos[:util.SPECIALS.size]] = util.SPECIALS * np.float32(top)
    flat[pos[util.SPECIALS.size:]] = np.array([np.nan, np.inf, -np.inf, -0.0, 1e-42, -1e-42, 3e38, -3e38, 1e-39, -0.0, np.inf, np.nan], np.float32)
    return data


@pytest.mark.parametrize("levels", [(0.0, 1.0), (util.BLACK, util.WHITE)], ids=["unit", "14bit"])
@pytest.mark.parametrize("k", [0, 1, 3, 5, 8], ids=["crop5", "crop-uneven", "rot.2", "rot.77", "crop+rot.04"])
@pytest.mark.parametrize("cfa", ["BGGR", XT], ids=["BGGR", "xtrans"])
def test_hostile_f32_mosaics(ipa, orc, cfa, k, levels):
    w, h, crops = FRAMES["96x120c"]
    black, white = levels
    data = _hostile_mosaic(9200 + 16 * k + len(cfa), h, w, white)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    (tl, tr, bl, nw, nh) = orc.rotatecrop_corners(R9[k], cw, ch)
    # -inf (OpGoFloat's min(1.0) turns NaN and +inf into 1.0; -inf passes) and +inf a single pixel outside the output rectangle's first corner and last
    # row (sensor coordinates): demosaic::full spreads them into the rectangle's rim, where a zero-weight tap turns 0 * -inf into NaN -- taps the
    # resampler may not skip
    oy, ox = crops[0], crops[3]
    spots = [(oy + max(tl[1] - 1, 0), ox + max(tl[0] - 1, 0)), (oy + min(bl[1] + 1, ch - 1), ox + min(bl[0] + 1, cw - 1))]
    tame = data.copy()
    for (r, c), v in zip(spots, (-np.inf, np.inf)):
        data[r, c] = v
        tame[r, c] = 0.5 * white
    _check_both_routes(ipa, orc, data, cfa, crops, dict(rotatecrop=R9[k]), (F32, U8, U16), "hostile %s %s levels %r" % (cfa[:6], R9_IDS[k], levels),
                       black=black, white=white)
    # (OpToLab's min(1.0) turns a NaN channel into 1.0, so what the planted values do shows as changed pixels, not as NaN)
    want, without = (orc.pipeline_run(_oracle_desc(orc, d, cfa, crops, dict(rotatecrop=R9[k]), black=black, white=white)) for d in (data, tame))
    assert (want.view(np.uint32) != without.view(np.uint32)).any(), "the planted values do not reach the result: the case tests nothing"


@pytest.mark.parametrize("levels", [(0.0, 1.0), (util.BLACK, util.WHITE), (700.0, 700.0), (0.0, 1e-37)], ids=["unit", "14bit", "empty-range", "tiny-range"])
@pytest.mark.parametrize("k", [0, 1, 3], ids=["crop5", "crop-uneven", "rot.2"])
@pytest.mark.parametrize("cfa", ["BGGR", XT], ids=["BGGR", "xtrans"])
def test_extreme_u16_mosaics(ipa, orc, cfa, k, levels):
    """u16 frames are finite by type: with ordinary levels a crop-only run is the fused kernel's window launch over the rectangle (the pick
    is exact), with an empty or tiny range ((v - black) / range is inf, -inf or NaN) it is not -- either way the bytes are the oracle's"""
    w, h, crops = FRAMES["96x120c"]
    black, white = levels
    rng = np.random.default_rng(9500 + k)
    data = rng.integers(0, 1400, size=(h, w)).astype(np.uint16)
    flat = data.reshape(-1)
    flat[rng.choice(flat.size, 64, replace=False)] = np.array([0, 1, 511, 512, 513, 699, 700, 701, 16383, 16384, 65535, 40000, 2, 3, 1023, 1024] * 4, np.uint16)
    _check_both_routes(ipa, orc, data, cfa, crops, dict(rotatecrop=R9[k]), (F32, U8, U16), "extreme u16 %s %s levels %r" % (cfa[:6], R9_IDS[k], levels),
                       black=black, white=white)


def test_inf_outside_a_crop_rectangle_reaches_its_neighbours(ipa, orc):
    """crop-only: every window is 2x2 with the weights {1, 0, 0, 0}, and 0 * -inf is NaN: a -inf sample (the one special value OpGoFloat's min(1.0)
    lets through) that demosaic::full spreads to the column right of the rectangle changes the rectangle's last column exactly where the oracle says"""
    w, h, crops = FRAMES["47x61"]
    rc = R9[0]
    data = _mosaic(util.SEED + 9300, h, w, True)
    tl, tr, bl, nw, nh = orc.rotatecrop_corners(rc, w, h)
    clean = orc.pipeline_run(_oracle_desc(orc, data, "RGGB", crops, dict(rotatecrop=rc)))
    assert np.isfinite(clean).all()
    data[tl[1] + nh // 2, tr[0] + 2] = -np.inf                             # two columns right of the rectangle: demosaic brings it to tr[0] + 1
    want = orc.pipeline_run(_oracle_desc(orc, data, "RGGB", crops, dict(rotatecrop=rc)))
    hit = (want.view(np.uint32) != clean.view(np.uint32)).any(axis=2)      # (OpToLab's min(1.0) turns a NaN channel into 1.0: changed pixels, not NaN)
    assert hit.any() and not hit[:, :-1].any(), "the sample should show in the last output column only"
    _check_both_routes(ipa, orc, data, "RGGB", crops, dict(rotatecrop=rc), (F32,), "-inf outside the crop rectangle")


# ---------------------------------------------------------------------------------------------
# full-size frames: every output sample is compared (the oracle takes a few seconds each)
# ---------------------------------------------------------------------------------------------
def _big(seed, h, w, is_float):
    """an odd-sized noise block tiled (prime periods, so no kernel stride lines up with them)"""
    blk = _mosaic(seed, min(h, 1009), min(w, 997), is_float)
    return np.ascontiguousarray(np.tile(blk, (-(-h // blk.shape[0]), -(-w // blk.shape[1])))[:h, :w])


FULL = {
    "24mp_crop5": ("RGGB", (4000, 6000), True, f32s(0.05, 0.05, 0.05, 0.05, 0), F32),
    "24mp_rot1/30": ("RGGB", (4000, 6000), True, f32s(0, 0, 0, 0, 1.0 / 30.0), F32),
    "6024x4016_u8": ("RGGB", (4016, 6024), False, f32s(0.013, 0.021, 0.017, 0.009, 0.011), U8),
    "100mp_xtrans": (XT, (10000, 10000), True, f32s(0.02, 0.03, 0.01, 0.02, 0.1), F32),
}


@pytest.mark.parametrize("case", list(FULL))
def test_full_frames_vs_oracle(ipa, orc, case):
    import torch
    cfa, (h, w), is_float, rc, out_type = FULL[case]
    data = _big(util.SEED + 9400 + len(case), h, w, is_float)
    ops = dict(rotatecrop=rc)
    want = _want(orc, _oracle_desc(orc, data, cfa, (0, 0, 0, 0), ops), out_type)
    pipe = _pipeline(ipa, data, cfa, (0, 0, 0, 0), ops)
    for flag in (True, False):
        pipe.fuse_rotatecrop = flag
        got = _out(pipe, out_type)
        assert pipe.last_used_fused is flag, case
        if out_type == F32:
            if not torch.equal(torch.from_numpy(got).view(torch.int32), torch.from_numpy(want).view(torch.int32)):   # NaN payloads aside, report where
                assert_bits_equal(got, want, "full frame %s flag %d" % (case, flag))
        else:
            _same(got, want, "full frame %s flag %d" % (case, flag))
        del got
