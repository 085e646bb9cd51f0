"""GPU parity of the STAGED pipeline driver (gofloat, demosaic, rotatecrop, then the point-wise chain as separate kernels) against the CPU
oracle: the sources the fused launch never takes (mono raws, three-sample raws, four-colour filters), every demosaic branch, rotatecrop with
and without rotation, orientations, sensor crops, the three output types, the cache, special values and full-size frames.
Bar: bit-exact (0 ULP, any NaN == any NaN)."""
import ctypes as C
import itertools
import math
import os

import numpy as np
import pytest

import util
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
L16 = "8x2:RGBGRBGGGBGRGRBG"                   # sixteen letters, shape stated by the caller
F32, U8, U16 = "f32", "u8", "u16"


def _cam4():
    """the synthetic camera with a nonzero fourth column: the E channel of an RGBE filter counts"""
    cm = util.cam_matrix().copy()
    cm[:, 3] = [0.05, -0.03, 0.08]
    return cm


# ---------------------------------------------------------------------------------------------
# sources: (data, RawImage fields) -- everything here is plain numpy, so the cases can be built without a GPU
# ---------------------------------------------------------------------------------------------
SOURCES = ["mono_u16", "mono_f32", "rgb3_u16", "rgb3_f32", "bayer", "xtrans", "rgbe", "l16"]


def _source(name, h, w, seed):
    src = dict(cfa="", cpp=1, is_float=False, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4)
    if name.startswith("mono"):
        data = util.noise_u16(seed, h, w, 4600)
        src.update(blacklevels=[96.0, 10.0, 20.0, 0.0], whitelevels=[4095.0, 5000.0, 6000.0, 0.0])
    elif name.startswith("rgb3"):
        data = util.noise_u16(seed, h, w * 3, 4600).reshape(h, w, 3)
        src.update(cpp=3, blacklevels=[64.0, 70.0, 80.0, 0.0], whitelevels=[4000.0, 3900.0, 4095.0, 0.0])
    else:
        src["cfa"] = {"bayer": "GRBG", "xtrans": XT, "rgbe": "RGBE", "l16": L16}[name]
        data = util.noise_u16(seed, h, w)
    if name.endswith("f32") or name == "xtrans":
        data = data.astype(np.float32) + (util.uniform_f32(seed + 1, data.size, -0.5, 0.5).reshape(data.shape))
        src["is_float"] = True
    return data, src


def _minscale(cfa):
    """OpDemosaic's minscale (demosaic.rs:33-39) by CFA width; sources without a CFA use the Bayer arm"""
    if not cfa:
        return 2.0
    wide = int(cfa.split(":")[0].split("x")[0]) if ":" in cfa else {4: 2, 36: 6, 144: 12}[len(cfa)]
    return {2: 2.0, 6: 3.0, 8: 2.0, 12: 12.0}.get(wide, 2.0)


def _oracle_desc(orc, data, src, crops, ops):
    cfa = orc.cfa_shift(src["cfa"], crops[3], crops[0]) if src["cfa"] else ""
    kw = {k: v for k, v in src.items() if k not in ("cfa", "is_float")}
    return orc.make_pipeline(data, cfa=cfa, crops=crops, **kw, **ops)


def _place_scale(orc, data, src, crops, ops, branch):
    """sets ops["maxwidth"] so that OpDemosaic sees a scale in the wanted band ("le1": no limit; "mid": 1 < scale < minscale, demosaic::full
    then scale_down_opbuf for a CFA; "ge": scale >= minscale, scaled_demosaic) and returns that scale"""
    ops.pop("maxwidth", None)
    desc = _oracle_desc(orc, data, src, crops, ops)
    _, (fw, fh) = orc.pipeline_sizes(desc)
    cw, ch = data.shape[1] - crops[1] - crops[3], data.shape[0] - crops[0] - crops[2]
    if branch == "le1":
        return 1.0
    ms = _minscale(src["cfa"])
    lo, hi = (1.0, ms) if branch == "mid" else (ms, ms * 4)
    target = (lo + hi) / 2 if branch == "mid" else ms + 0.6
    for mw in sorted(range(2, fw), key=lambda m: abs(fw / m - target)):
        ops["maxwidth"] = mw
        (dw, dh), _ = orc.pipeline_sizes(_oracle_desc(orc, data, src, crops, ops))
        s = orc.calculate_scaling_total(cw, ch, dw, dh)[0]
        if lo < s < hi or (branch == "ge" and s == lo):
            return s
    raise AssertionError("no maxwidth reaches the %s branch" % branch)


ROTATECROPS = {"none": None, "crop": (0.1, 0.05, 0.08, 0.12, 0.0), "rot": (0.04, 0.07, 0.05, 0.03, 0.3)}
ORIENTS = {"normal": {}, "rotflip": dict(rotation=1, fliph=True)}           # Rotate90 + horizontal flip = Transpose
CROPS = {"zero": (0, 0, 0, 0), "crop": (3, 2, 1, 5)}


def _case_ops(rc, orient):
    ops = {}
    if ROTATECROPS[rc] is not None:
        ops["rotatecrop"] = tuple(float(np.float32(v)) for v in ROTATECROPS[rc])
    ops.update(ORIENTS[orient])
    return ops


# ---------------------------------------------------------------------------------------------
# GPU side
# ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _upload(ipa, data, is_float):
    import torch
    return torch.from_numpy(np.ascontiguousarray(data, np.float32).ravel()).cuda() if is_float else ipa.upload_u16(data)


def _pipeline(ipa, data, src, crops, ops, wb=util.WB, cam=None):
    h, w = data.shape[:2]
    img = ipa.RawImage(width=w, height=h, data=_upload(ipa, data, src["is_float"]), cpp=src["cpp"], cfa=src["cfa"],
                       crops=crops, blacklevels=src["blacklevels"], whitelevels=src["whitelevels"], wb_coeffs=wb,
                       cam_to_xyz_normalized=_cam4() if cam is None else cam, is_float=src["is_float"])
    pipe = ipa.Pipeline.new_from_source(img)
    _apply(pipe, ops)
    return pipe


def _apply(pipe, ops):
    rc = ops.get("rotatecrop", (0.0, 0.0, 0.0, 0.0, 0.0))
    pipe.ops.rotatecrop.crop_top, pipe.ops.rotatecrop.crop_right, pipe.ops.rotatecrop.crop_bottom, pipe.ops.rotatecrop.crop_left, pipe.ops.rotatecrop.rotation = rc
    for k in ("rotation", "fliph", "flipv"):
        if k in ops:
            setattr(pipe.ops.transform, k, ops[k])
    for k in ("maxwidth", "maxheight", "linear"):
        if k in ops:
            setattr(pipe.globals.settings, k, ops[k])
    if "points" in ops:
        pipe.ops.basecurve.points = ops["points"]
    if "exposure" in ops:
        pipe.ops.basecurve.exposure = ops["exposure"]


def _out(pipe, out_type):
    if out_type == F32:
        return pipe.run().numpy()
    if out_type == U8:
        ww, hh, o = pipe.output_8bit()
        return o.cpu().numpy().reshape(hh, ww, 3)
    ww, hh, o = pipe.output_16bit()
    return o.cpu().numpy().view(np.uint16).reshape(hh, ww, 3)


def _want(orc, desc, out_type):
    return {F32: orc.pipeline_run, U8: orc.pipeline_output_8bit, U16: orc.pipeline_output_16bit}[out_type](desc)


def _same(got, want, what):
    if want.dtype == np.float32:
        assert_bits_equal(got, want, what)
    else:
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d samples differ" % (what, int((got != want).sum()) if got.shape == want.shape else -1)


def _check_driver(ipa, orc, data, src, crops, ops, out_type, must_stage, tag, **pkw):
    """pipe.run() / output_Nbit (fused launches allowed), the staged driver (allow_fused = False) and the op-by-op loop, all against the oracle"""
    def desc():       # a fresh one per oracle run: output_8bit / output_16bit force `linear` on the descriptor they are given (pipeline.rs:405, :452)
        return _oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=pkw.get("wb", util.WB), cam_to_xyz_normalized=pkw.get("cam", _cam4())))
    pipe = _pipeline(ipa, data, src, crops, ops, **pkw)
    assert pipe.sizes() == orc.pipeline_sizes(desc()), tag
    want = _want(orc, desc(), out_type)
    _same(_out(pipe, out_type), want, tag + " driver")
    if must_stage:
        assert pipe.last_used_fused is False, tag
    pipe.allow_fused = False
    _same(_out(pipe, out_type), want, tag + " staged driver")
    assert pipe.last_used_fused is False, tag
    assert_bits_equal(pipe.run_ops().numpy(), want if out_type == F32 else orc.pipeline_run(desc()), tag + " op loop")


def _must_stage(name, ops, scale):
    return name in ("mono_u16", "mono_f32", "rgb3_u16", "rgb3_f32", "rgbe") or "rotatecrop" in ops or scale > 1.0


# ---------------------------------------------------------------------------------------------
# source x branch matrix: each source meets every demosaic branch, rotatecrop kind and output type once, both orientations and both crop
# settings at least once (case i of source j: branch i, rotatecrop (i + j) % 3, orientation (i + j) % 2, crops (i + j + 1) % 2, output (i + 2j) % 3)
# ---------------------------------------------------------------------------------------------
MATRIX = [(name, i) for name in SOURCES for i in range(3)]


def _matrix_case(orc, name, i):
    j = SOURCES.index(name)
    branch = ["le1", "mid", "ge"][i]
    rc = ["none", "crop", "rot"][(i + j) % 3]
    orient = ["normal", "rotflip"][(i + j) % 2]
    crops = CROPS[["zero", "crop"][(i + j + 1) % 2]]
    out_type = [F32, U8, U16][(i + 2 * j) % 3]
    h, w = 60 + 9 * i + 3 * j, 84 + 13 * j + 7 * i
    data, src = _source(name, h, w, util.SEED + 7000 + 10 * j + i)
    ops = _case_ops(rc, orient)
    scale = _place_scale(orc, data, src, crops, ops, branch)
    return data, src, crops, ops, out_type, scale, "%s case %d (%s, rotatecrop %s, %s, crops %r, %s, scale %.3f)" % (name, i, branch, rc, orient, crops, out_type, scale)


@pytest.mark.parametrize("name,i", MATRIX, ids=["%s-%d" % c for c in MATRIX])
def test_staged_source_branch_matrix(ipa, orc, name, i):
    data, src, crops, ops, out_type, scale, tag = _matrix_case(orc, name, i)
    _check_driver(ipa, orc, data, src, crops, ops, out_type, _must_stage(name, ops, scale), tag)


# ---------------------------------------------------------------------------------------------
# one routing decision: ipk_pipeline_run, a cold ipk_pipeline_run_cached and ipk_pipeline_run_batch (two frames, OpTransform a no-op) report
# the same used_fused for every raw descriptor
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", SOURCES)
def test_drivers_agree_on_the_fused_route(ipa, name):
    import torch
    j = SOURCES.index(name)
    data, src = _source(name, 40 + 2 * j, 72 + 6 * j, util.SEED + 9100 + j)
    w = data.shape[1]
    dtypes = {F32: torch.float32, U8: torch.uint8, U16: torch.int16}
    codes = {F32: ipa.OUT_F32, U8: ipa.OUT_U8, U16: ipa.OUT_U16}
    seen = set()
    for crops, rc, orient, mw, fused, out_type in itertools.product(CROPS.values(), ("none", "crop"), ORIENTS, (0, w // 2, w // 5), (True, False),
                                                                    (F32, U8, U16)):
        ops = _case_ops(rc, orient)
        if mw:
            ops["maxwidth"] = mw
        pipe = _pipeline(ipa, data, src, crops, ops)
        pipe.allow_fused = fused
        tag = "%s crops %r rotatecrop %s %s maxwidth %d allow_fused %s %s" % (name, crops, rc, orient, mw, fused, out_type)
        pipe._run(codes[out_type])
        run = pipe.last_used_fused
        cache = ipa.PipelineCache(1 << 28)
        pipe._run(codes[out_type], cache=cache)
        cache.close()
        assert pipe.last_used_fused == run, tag + ": cold cached run"
        seen.add(run)
        if orient != "normal":
            continue
        _, (fw, fh) = pipe.sizes()
        outs = [torch.empty(fw * fh * 3, dtype=dtypes[out_type], device="cuda") for _ in range(2)]
        p = pipe.globals.image.data.data_ptr()
        srcs, dsts = (C.c_void_p * 2)(p, p), (C.c_void_p * 2)(*[o.data_ptr() for o in outs])
        used = C.c_int(-1)
        assert ipa.lib().ipk_pipeline_run_batch(C.byref(pipe.desc()), srcs, dsts, 2, codes[out_type], C.byref(used), ipa._stream()) == 0, tag
        assert bool(used.value) == run, tag + ": batch of two"
    torch.cuda.synchronize()
    if src["cfa"] in ("GRBG", XT):
        assert seen == {False, True}, name + ": the matrix reaches both routes"


@pytest.mark.parametrize("out_type", [F32, U8, U16])
@pytest.mark.parametrize("name", ["mono_f32", "rgb3_u16", "rgbe"])
@pytest.mark.parametrize("shape", [(17, 15), (16, 16), (15, 18)])      # 255, 256 and 270 output pixels
def test_staged_output_switch_at_256_pixels(ipa, orc, name, shape, out_type):
    """below 256 output pixels the staged driver quantises in a pass of its own and ipk_tolab takes its literal kernel; from 256 on
    ipk_pointwise_chain_out writes the 8- / 16-bit image in the chain's pass (ipk_api.cpp, the staged driver's point-wise tail)"""
    h, w = shape
    data, src = _source(name, h, w, util.SEED + 7300 + h)
    _check_driver(ipa, orc, data, src, (0, 0, 0, 0), {}, out_type, True, "%s %dx%d %s" % (name, w, h, out_type))


# ---------------------------------------------------------------------------------------------
# a mono source through the cache: cold run, hit, white-balance edit, rotatecrop edit
# ---------------------------------------------------------------------------------------------
def _cache_get_mono(ipa, cache, key):
    p, w, h, c, m = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    rc = ipa.lib().ipk_cache_get(cache.handle, key, C.byref(p), C.byref(w), C.byref(h), C.byref(c), C.byref(m))
    assert rc == 0, "the buffer is not memoised"
    return m.value


def _expected_mask(cache, hashes):
    """the hash chain's answer: every op after the last memoised output runs (pipeline.rs:352-372)"""
    start = 0
    for i, hh in enumerate(hashes):
        if cache.contains(hh):
            start = i + 1
    return (0xFF << start) & 0xFF


@pytest.mark.parametrize("name", ["mono_u16", "mono_f32"])
def test_mono_through_the_cache(ipa, orc, name):
    h, w = 90, 130
    crops = (2, 1, 3, 4)
    data, src = _source(name, h, w, util.SEED + 7400)
    ops = {}
    scale = _place_scale(orc, data, src, crops, ops, "mid")             # OpDemosaic runs scale_down_opbuf: its output is a new, memoised buffer
    assert scale > 1.0
    pipe = _pipeline(ipa, data, src, crops, ops)
    def desc(wb=util.WB, **more):
        return _oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=wb, cam_to_xyz_normalized=_cam4(), **more))

    cache = ipa.PipelineCache(1 << 28)
    try:
        hs = pipe.hashes()
        assert _expected_mask(cache, hs) == 0xFF
        assert_bits_equal(pipe.run(cache).numpy(), orc.pipeline_run(desc()), "cold")
        assert pipe.last_ops_run == 0xFF and not pipe.last_used_fused
        # the memoised demosaic output: the oracle's gofloat + demosaic, and it still says monochrome
        (dw, dh), _ = orc.pipeline_sizes(desc())
        x, y, cw, ch = orc.size_image(*crops, w, h)
        _, dem = orc.demosaic_run("", orc.gofloat_mono(data, x, y, cw, ch, src["blacklevels"][0], src["whitelevels"][0]), dw, dh)
        assert_bits_equal(cache.get(hs[1]), dem, "memoised demosaic buffer")
        assert _cache_get_mono(ipa, cache, hs[1]) == 1
        assert _cache_get_mono(ipa, cache, hs[7]) == 1
        assert _expected_mask(cache, pipe.hashes()) == 0
        assert_bits_equal(pipe.run(cache).numpy(), orc.pipeline_run(desc()), "hit")
        assert pipe.last_ops_run == 0
        # white balance: to_lab and everything after it rerun from the memoised rotatecrop / demosaic output
        wb2 = (1.7, 1.0, 2.2, 1.0)
        pipe.ops.tolab.wb_coeffs = list(wb2)
        exp = _expected_mask(cache, pipe.hashes())
        assert exp == 0xF8
        assert_bits_equal(pipe.run(cache).numpy(), orc.pipeline_run(desc(wb=wb2)), "white balance edit")
        assert pipe.last_ops_run == exp
        # rotatecrop: under a size limit the crop changes the negotiated demosaic size, so the hash chain reruns every op
        rc = tuple(float(np.float32(v)) for v in (0.05, 0.1, 0.0, 0.07, 0.2))
        _apply(pipe, dict(rotatecrop=rc))
        exp = _expected_mask(cache, pipe.hashes())
        assert exp == 0xFF
        assert_bits_equal(pipe.run(cache).numpy(), orc.pipeline_run(desc(wb=wb2, rotatecrop=rc)), "rotatecrop edit")
        assert pipe.last_ops_run == exp
        assert _cache_get_mono(ipa, cache, pipe.hashes()[2]) == 1
    finally:
        cache.close()


# ---------------------------------------------------------------------------------------------
# hostile inputs on the staged path
# ---------------------------------------------------------------------------------------------
def _hostile_case(orc, seed):
    rng = np.random.default_rng(9000 + seed)
    name = ["mono", "rgb3", "bayer", "xtrans", "rgbe", "l16"][int(rng.integers(0, 6))]
    is_float = rng.random() < 0.75
    h, w = int(rng.integers(24, 110)), int(rng.integers(24, 180))
    src = dict(cfa="", cpp=1, is_float=is_float)
    if name == "rgb3":
        src["cpp"] = 3
    elif name != "mono":
        src["cfa"] = {"bayer": ["RGGB", "BGGR", "GRBG", "GBRG"][int(rng.integers(0, 4))], "xtrans": XT, "rgbe": "RGBE", "l16": L16}[name]
    shape = (h, w, 3) if name == "rgb3" else (h, w)
    # levels: ordinary (different per channel), a range so tiny that (v - black) / range overflows to -inf, zero, or inverted
    lv = int(rng.integers(0, 6))
    if lv <= 2:
        black = [float(rng.choice([0.0, 64.0, 256.5, 512.0, 1024.0])) + float(rng.integers(0, 40)) for _ in range(4)]
        white = [float(rng.choice([1023.0, 4095.0, 16383.0, 65535.0])) - float(rng.integers(0, 40)) for _ in range(4)]
    elif lv == 3:
        black = [0.0] * 4; white = [1e-37] * 4
    elif lv == 4:
        black = [700.0] * 4; white = [700.0] * 4
    else:
        black = [4000.0, 3000.0, 3500.0, 0.0]; white = [100.0, 200.0, 50.0, 0.0]
    top = max(white[:3]) if lv <= 2 else 4000.0
    if is_float:
        data = rng.uniform(-0.1 * top - 50.0, 1.2 * top, size=shape).astype(np.float32)
        if lv == 3:
            data = rng.uniform(-200.0, 50.0, size=shape).astype(np.float32)
        flat = data.reshape(-1)
        pos = rng.choice(flat.size, util.SPECIALS.size, replace=False)
        with np.errstate(over="ignore", invalid="ignore"):
            flat[pos] = util.SPECIALS * np.float32(top)
        n_lone = int(rng.integers(3, 9))
        flat[rng.choice(flat.size, n_lone, replace=False)] = np.where(rng.random(n_lone) < 0.5, -np.inf, -3e38).astype(np.float32)
    else:
        data = rng.integers(0, int(min(top, 65000)) + 200, size=shape).astype(np.uint16)
    src.update(blacklevels=black, whitelevels=white)
    wb = (float(rng.uniform(0.5, 3.0)), float(rng.uniform(0.8, 1.2)), float(rng.uniform(0.5, 3.0)),
          float(rng.choice([0.0, np.nan, np.inf, -np.inf, 1.0, 2.5])))
    cm = (util.cam_matrix() * rng.uniform(0.7, 1.3, size=(3, 1)).astype(np.float32) + rng.normal(0, 0.05, size=(3, 4)).astype(np.float32)).astype(np.float32)
    cm[:, 3] = rng.normal(0, 0.2, 3).astype(np.float32)
    cm = cm.astype(np.float32)
    crops = tuple(int(v) for v in rng.integers(1, 5, 4)) if rng.integers(0, 3) else (0, 0, 0, 0)
    rc = ["none", "crop", "rot"][int(rng.integers(0, 3))]
    branch = ["le1", "mid", "ge"][int(rng.integers(0, 3))]
    if name in ("bayer", "xtrans", "l16") and rc == "none" and branch == "le1":
        rc = "rot"                                                          # a three-colour filter at full scale would take the fused launch
    ops = {}
    if rc != "none":
        r = [float(np.float32(v)) for v in rng.uniform(0.0, 0.15, 4)] + [0.0 if rc == "crop" else float(np.float32(rng.uniform(-0.5, 0.5)))]
        ops["rotatecrop"] = tuple(r)
    if rng.integers(0, 2):
        ops.update(rotation=int(rng.integers(0, 4)), fliph=bool(rng.integers(0, 2)), flipv=bool(rng.integers(0, 2)))
    npts = int(rng.integers(0, 5))
    xs = np.sort(rng.uniform(0.05, 0.95, npts)); ys = np.sort(rng.uniform(0.05, 0.95, npts))
    ops["points"] = [(float(np.float32(a)), float(np.float32(b))) for a, b in zip(xs, ys)]
    ops["exposure"] = float(rng.choice([0.0, 0.0, 0.3, -0.7]))
    ops["linear"] = bool(rng.integers(0, 2))
    scale = _place_scale(orc, data, src, crops, ops, branch)
    out_type = [F32, U8, U16][int(rng.integers(0, 3))]
    tag = "hostile seed %d: %s %s %dx%d levels %d crops %r %s rotatecrop %s scale %.3f wb %r %s" % (
        seed, name, "f32" if is_float else "u16", w, h, lv, crops, branch, rc, scale, wb, out_type)
    return data, src, crops, ops, out_type, wb, cm, tag


@pytest.mark.parametrize("seed", range(int(os.environ.get("IPK_RANDOM_SEEDS_STAGED", "60"))))   # IPK_RANDOM_SEEDS_STAGED=500 for a soak run
def test_staged_hostile_inputs(ipa, orc, seed):
    data, src, crops, ops, out_type, wb, cm, tag = _hostile_case(orc, seed)
    _check_driver(ipa, orc, data, src, crops, ops, out_type, True, tag, wb=wb, cam=cm)


# ---------------------------------------------------------------------------------------------
# op level: OpRotateCrop on 1-, 3- and 4-component buffers and OpDemosaic's scale_down_opbuf branch, buffers holding specials
# ---------------------------------------------------------------------------------------------
def _specials_buffer(seed, h, w, comps):
    rng = np.random.default_rng(seed)
    buf = util.uniform_f32(util.SEED + seed, h * w * comps, -0.1, 1.1)
    pos = rng.choice(buf.size, util.SPECIALS.size + 8, replace=False)
    buf[pos[:util.SPECIALS.size]] = util.SPECIALS
    buf[pos[util.SPECIALS.size:]] = np.array([-np.inf] * 4 + [-3e38] * 4, np.float32)
    buf = buf.reshape(h, w, comps)
    buf[h // 2, w // 2, 0] = -np.inf                                 # inside every window the tests use
    buf[h // 2 + 3, w // 3, comps - 1] = -3e38
    return buf


def _plain_axis(tl, tr, bl, nw, nh):
    """k_transform_buffer's multiply-fma path: scale_down_buffer's corner (0, 0), no cross terms, both skips >= 1"""
    return tl == (0, 0) and tr[1] == 0 and bl[0] == 0 and tr[0] / (nw - 1) >= 1.0 and bl[1] / (nh - 1) >= 1.0


@pytest.mark.parametrize("comps", [1, 3, 4])
@pytest.mark.parametrize("params,plain", [((0.0, 0.1, 0.15, 0.0, 0.0), True), ((0.1, 0.05, 0.08, 0.12, 0.0), False),
                                          ((0.05, 0.1, 0.0, 0.07, 0.35), False), ((0.03, 0.02, 0.05, 0.04, 0.9), False)],
                         ids=["axis", "crop", "rotated", "rotated-steep"])
def test_op_rotatecrop_with_specials(ipa, orc, comps, params, plain):
    h, w = 70, 90
    buf = _specials_buffer(7500 + comps, h, w, comps)
    p5 = [float(np.float32(v)) for v in params]
    tl, tr, bl, nw, nh = orc.rotatecrop_corners(p5, w, h)
    assert _plain_axis(tl, tr, bl, nw, nh) == plain, (tl, tr, bl, nw, nh)
    if not plain and params[4] != 0.0:
        assert tr[0] < tl[0] or tr[1] < tl[1] or bl[0] < tl[0], "rotated corners should give a negative skip"
    op = ipa.OpRotateCrop()
    op.crop_top, op.crop_right, op.crop_bottom, op.crop_left, op.rotation = p5
    out = op.run(ipa.PipelineGlobals(None), ipa.OpBuffer.from_numpy(buf if comps > 1 else buf[:, :, 0], monochrome=True))
    assert (out.width, out.height, out.colors, out.monochrome) == (nw, nh, comps, True)
    want = orc.transform_buffer(buf, w, h, tl, tr, bl, nw, nh, comps)
    assert_bits_equal(out.data.cpu().numpy().reshape(nh, nw, comps), want, "OpRotateCrop %d components %r" % (comps, params))
    assert not np.isfinite(want).all()


@pytest.mark.parametrize("shape,dsize", [((61, 83), (29, 21)), ((64, 96), (60, 40)), ((50, 50), (7, 7))])
def test_op_demosaic_scale_down_opbuf_with_specials(ipa, orc, shape, dsize):
    h, w = shape
    buf = _specials_buffer(7600 + h, h, w, 4)
    g = ipa.PipelineGlobals(None)
    g.settings.demosaic_width, g.settings.demosaic_height = dsize
    op = ipa.OpDemosaic(ipa.OtherImage(w, h, None))
    out = op.run(g, ipa.OpBuffer.from_numpy(buf, monochrome=True))
    branch, want = orc.demosaic_run("", buf, *dsize)
    assert branch == 1 and want.shape == (dsize[1], dsize[0], 4)
    assert (out.width, out.height, out.colors, out.monochrome) == (dsize[0], dsize[1], 4, True)
    assert_bits_equal(out.numpy(), want, "OpDemosaic scale_down_opbuf %r -> %r" % (shape, dsize))
    assert np.isnan(want).any()


# ---------------------------------------------------------------------------------------------
# full-size frames (the oracle takes a few seconds each)
# ---------------------------------------------------------------------------------------------
def _big(name, h, w, seed):
    """a full-size source: an odd-sized noise block tiled (prime periods, so no kernel stride lines up with them)"""
    bh, bw = min(h, 1009), min(w, 997)
    data, src = _source(name, bh, bw, seed)
    reps = (-(-h // bh), -(-w // bw)) + ((1,) if data.ndim == 3 else ())
    return np.ascontiguousarray(np.tile(data, reps)[:h, :w]), src


def _full_frame(ipa, orc, data, src, crops, ops, must_stage, tag, out_type=F32):
    import torch
    desc = _oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=util.WB, cam_to_xyz_normalized=_cam4()))
    want = _want(orc, desc, out_type)
    pipe = _pipeline(ipa, data, src, crops, ops)
    for allow in (True, False):
        pipe.allow_fused = allow
        got = _out(pipe, out_type)
        assert pipe.last_used_fused is False or not must_stage, tag
        if out_type == F32:
            same = torch.equal(torch.from_numpy(got).view(torch.int32), torch.from_numpy(want).view(torch.int32))
            if not same:                                                 # NaN payloads aside, report where
                assert_bits_equal(got, want, tag + (" driver" if allow else " staged driver"))
        else:
            _same(got, want, tag + (" driver" if allow else " staged driver"))
        del got


RAD3 = float(np.float32(3.0 * math.pi / 180.0))
FULL = {
    "crop5": ("bayer", (4000, 6000), (0, 0, 0, 0), dict(rotatecrop=(0.05, 0.05, 0.05, 0.05, 0.0)), F32),
    "rot3": ("bayer", (4000, 6000), (0, 0, 0, 0), dict(rotatecrop=(0.0, 0.0, 0.0, 0.0, RAD3)), F32),
    "scale1.5": ("bayer", (4000, 6000), (0, 0, 0, 0), dict(maxwidth=4000), F32),
    "rgbe": ("rgbe", (4000, 6000), (0, 0, 0, 0), {}, U8),
    "mono_u16": ("mono_u16", (4000, 6000), (0, 0, 0, 0), {}, F32),
    "rgb3_f32": ("rgb3_f32", (4000, 6000), (7, 5, 3, 9), {}, U16),
    "100mp_rot": ("xtrans", (10000, 10000), (0, 0, 0, 0), dict(rotatecrop=(0.02, 0.03, 0.01, 0.02, float(np.float32(0.1)))), F32),
    "tall_crop": ("bayer", (70000, 200), (0, 0, 0, 0), dict(rotatecrop=(0.01, 0.02, 0.015, 0.03, 0.0)), F32),
    "tall_rgbe": ("rgbe", (70000, 200), (2, 1, 0, 3), {}, F32),
}


@pytest.mark.parametrize("case", list(FULL))
def test_staged_full_frames_vs_oracle(ipa, orc, case):
    """every staged branch at a real frame size: frames taller than the 65 535-row grid cap make the staged kernels loop over rows"""
    name, (h, w), crops, ops, out_type = FULL[case]
    data, src = _big(name, h, w, util.SEED + 7700 + len(case))
    if case == "scale1.5":
        cw = w - crops[1] - crops[3]
        s = orc.calculate_scaling_total(cw, h, ops["maxwidth"], 0)[0]
        assert 1.0 < s < 2.0, s                                          # demosaic::full, then scale_down_opbuf
    _full_frame(ipa, orc, data, src, crops, ops, True, "full frame %s" % case, out_type)
