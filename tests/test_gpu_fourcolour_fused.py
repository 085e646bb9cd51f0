"""GPU parity of the one-launch raw->sRGB route for filters with a fourth colour (ipk_fused_params.four_colour, ipk_pipeline_desc.allow_fused bit 1):
every result bit-identical (f32) or equal (u8 / u16) to the CPU oracle and to the staged run of the same descriptor; the launch log holds the one
generic-CFA runtime-flag kernel with its [four=1] tag and none of the staged kernels; the plain, cached, batch, host, region, oriented, banded and
queue-less runs agree; nothing outside the destination is written; and without the opt-in everything refuses or stages as before."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_staged_paths as sp
import util
from util import Embedded, Guarded

pytestmark = pytest.mark.gpu

F32, U8, U16 = sp.F32, sp.U8, sp.U16
E8 = "RGRGRGBEBEBERGBE"
# 2 wide x 8 high: rows RG RG RG BE BE BE RG BE -- the windows centred on rows 1 and 4 of the tile see two colours only
FILTERS = {"RGBE": "RGBE", "ERBG": "ERBG", "8x2": "8x2:" + E8, "2x8": "2x8:" + E8}
STAGED_KERNELS = ("k_gofloat_cfa", "k_demosaic_full", "k_pointwise_chain", "k_raster_chain")
UNSUPPORTED, INVALID = -5, -2
CURVES = {"default": {}, "nocurve": dict(points=[]), "6knots": dict(points=[(0.1, 0.07), (0.25, 0.2), (0.4, 0.45), (0.6, 0.7), (0.8, 0.88), (0.95, 0.97)]),
          "linear": dict(linear=True), "exposure": dict(exposure=0.7)}
# (sensor height, sensor width, sensor crops): the cropped frames are 36x11 and 13x40 (narrow variant), 257x12 and 300x23 (full strips, shifted
# last strip); the odd crops shift the filter and put a u16 frame 2 bytes off a dword on an odd pitch
SHAPES = {"36x11": (11, 36, (0, 0, 0, 0)), "13x40c": (46, 19, (3, 1, 3, 5)), "257x12c": (16, 263, (1, 3, 3, 3)), "300x23": (23, 300, (0, 0, 0, 0))}
WB4 = (2.0, 1.0, 1.5, 1.3)


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _src(cfa, is_float, black=util.BLACK):
    return dict(cfa=cfa, cpp=1, is_float=is_float, blacklevels=[black] * 4, whitelevels=[util.WHITE if black else 1.0] * 4)


def _mosaic(kind, h, w, seed):
    """u16 noise; "f32": the same plus a fraction; "specials": f32 samples in [0, 1.2) for black level 0 with util.SPECIALS, lone infinities, NaN
    and -0.0 among them"""
    data = util.noise_u16(seed, h, w)
    if kind == "u16":
        return data
    if kind == "f32":
        return data.astype(np.float32) + util.uniform_f32(seed + 1, h * w, -0.5, 0.5).reshape(h, w)
    v = util.uniform_f32(seed + 2, h * w, 0.0, 1.2).reshape(h, w)
    pos = (util.splitmix64(seed + 3, 4 * util.SPECIALS.size) % np.uint64(h * w)).astype(np.int64)
    v.ravel()[pos] = np.tile(util.SPECIALS, 4)
    for k, s in enumerate((np.inf, -np.inf, np.nan, -0.0)):            # lone ones, away from each other where the frame allows it
        v[(2 + 3 * k) % h, (5 + 7 * k) % w] = np.float32(s)
    return v


def _pipe(ipa, data, src, crops, ops, wb=WB4, four=True):
    pipe = sp._pipeline(ipa, data, src, crops, ops, wb=wb)
    pipe.fuse_four_colour = four
    return pipe


def _desc(orc, data, src, crops, ops, wb=WB4):
    return sp._oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=wb, cam_to_xyz_normalized=sp._cam4()))


def _np(t, out_type, h, w):
    a = t.cpu().numpy()
    return (a.view(np.uint16) if out_type == U16 else a).reshape(h, w, 3)


CODES = {F32: 0, U8: 1, U16: 2}


def _logged(ipa, pipe, out_type):
    with ipa.launch_log() as ran:
        got = sp._out(pipe, out_type)
    return got, ran


def _one_four_kernel(ran, is_float, out_type, full, window=False):
    S = "float, true" if is_float else "unsigned short, false"
    if window:
        name = "ipk::k_fused_bayer_window<%s, %d, %s, true, true, 0>[four=1]" % (S, CODES[out_type], "true" if full else "false")
    else:
        name = "ipk::k_fused_bayer<%s, %d, %s, true, true, 0, false>[four=1]" % (S, CODES[out_type], "true" if full else "false")
    assert sorted(ran) == [name], sorted(ran)


# ---------------------------------------------------------------------------------------------
# the plain run against the oracle and the staged run: shapes x filters, sources, outputs and curves in rotation
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fname", list(FILTERS))
@pytest.mark.parametrize("shape", list(SHAPES))
def test_plain_run_vs_oracle_and_staged(ipa, orc, shape, fname):
    h, w, crops = SHAPES[shape]
    cw = w - crops[1] - crops[3]
    k = list(SHAPES).index(shape) * 4 + list(FILTERS).index(fname)
    curves = list(CURVES)
    runs = [("u16", F32), ("u16", U8), ("f32", U16), ("specials", F32), ("specials", U8), ("f32", F32), ("u16", U16)]
    for i, (kind, out_type) in enumerate(runs):
        curve = curves[(k + i) % len(curves)]
        wb = WB4 if (k + i) % 2 == 0 else util.WB                          # util.WB: wb_coeffs[3] is NaN
        data = _mosaic(kind, h, w, util.SEED + 14000 + 16 * k + i)
        src = _src(FILTERS[fname], kind != "u16", 0.0 if kind == "specials" else util.BLACK)
        ops = dict(CURVES[curve])
        tag = "%s %s %s %s %s wb3=%r" % (shape, fname, kind, out_type, curve, wb[3])
        want = sp._want(orc, _desc(orc, data, src, crops, ops, wb), out_type)
        pipe = _pipe(ipa, data, src, crops, ops, wb)
        assert pipe.fuses_four_colour(CODES[out_type]), tag
        got, ran = _logged(ipa, pipe, out_type)
        assert pipe.last_used_fused is True, tag
        sp._same(got, want, tag + " one launch vs oracle")
        _one_four_kernel(ran, kind != "u16", out_type, cw >= 256)
        assert not [e for e in ran if any(s in e for s in STAGED_KERNELS)], sorted(ran)
        pipe.fuse_four_colour = False
        staged, ran = _logged(ipa, pipe, out_type)
        assert pipe.last_used_fused is False and not [e for e in ran if "four=1" in e], tag
        sp._same(got, staged, tag + " one launch vs staged")


def test_a_window_without_a_colour_gives_an_exact_zero(ipa, orc):
    """the 2x8 tile has cells whose 3x3 window holds two colours: the demosaiced B and E there are exactly 0.0 (demosaic.rs:110-114), and the run with
    such pixels is the oracle's"""
    h, w = 23, 40
    data = _mosaic("f32", h, w, util.SEED + 14500)
    rgbe = orc.demosaic_full(FILTERS["2x8"], orc.gofloat_cfa(data, 0, 0, w, h, util.BLACK, util.WHITE))
    assert (rgbe[1:-1, 1:-1, 2] == 0.0).any() and (rgbe[1:-1, 1:-1, 3] == 0.0).any() and (rgbe[..., 3] != 0.0).any()
    src = _src(FILTERS["2x8"], True)
    pipe = _pipe(ipa, data, src, (0, 0, 0, 0), {})
    sp._same(sp._out(pipe, F32), orc.pipeline_run(_desc(orc, data, src, (0, 0, 0, 0), {})), "2x8 tile")
    assert pipe.last_used_fused is True


# ---------------------------------------------------------------------------------------------
# one route, one result
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_type", [F32, U8])
@pytest.mark.parametrize("fname", ["RGBE", "2x8"])
def test_drivers_share_the_route(ipa, orc, fname, out_type):
    import torch
    h, w, crops = 29, 306, (3, 1, 3, 5)                                       # a 300x23 cropped frame
    is_float = out_type == F32
    frames = [_mosaic("f32" if is_float else "u16", h, w, util.SEED + 14600 + i) for i in range(3)]
    src = _src(FILTERS[fname], is_float)
    wants = [sp._want(orc, _desc(orc, f, src, crops, {}), out_type) for f in frames]
    code = CODES[out_type]
    pipes = [_pipe(ipa, f, src, crops, {}) for f in frames]
    pipe = pipes[0]
    plain = sp._out(pipe, out_type)
    sp._same(plain, wants[0], "plain run")
    cache = ipa.PipelineCache(1 << 28)
    try:
        with ipa.launch_log() as ran:
            data, fw, fh = pipe._run(code, None, cache)
        sp._same(_np(data, out_type, fh, fw), plain, "cold cached run")
        assert pipe.last_used_fused is True and pipe.last_ops_run == 0xFF
        if out_type == F32:
            assert cache.stats()["entries"] == 1 and cache.contains(pipe.hashes(code)[7])
            _one_four_kernel(ran, is_float, F32, True)
        data, fw, fh = pipe._run(code, None, cache)
        sp._same(_np(data, out_type, fh, fw), plain, "warm hit")
        assert pipe.last_ops_run == 0
    finally:
        cache.close()
    dt = {F32: torch.float32, U8: torch.uint8}[out_type]
    outs = [torch.empty(fw * fh * 3, dtype=dt, device="cuda") for _ in range(3)]
    srcs = (C.c_void_p * 3)(*[p.globals.image.data.data_ptr() for p in pipes]); dsts = (C.c_void_p * 3)(*[o.data_ptr() for o in outs])
    used = C.c_int(-1)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_pipeline_run_batch(C.byref(pipe.desc()), srcs, dsts, 3, code, C.byref(used), ipa._stream()) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    assert used.value == 1
    _one_four_kernel(ran, is_float, out_type, True)
    for i in range(3):
        sp._same(_np(outs[i], out_type, fh, fw), wants[i], "batch frame %d" % i)
    host = np.empty(fw * fh * 3, {F32: np.float32, U8: np.uint8}[out_type])
    hsrc = np.ascontiguousarray(frames[0])
    used = C.c_int(-1)
    assert ipa.lib().ipk_host_pipeline_run(C.byref(pipe.desc()), hsrc.ctypes.data_as(C.c_void_p), host.ctypes.data_as(C.c_void_p), code, C.byref(used)) == 0, ipa.lib().ipk_last_error()
    assert used.value == 1
    sp._same(host.reshape(fh, fw, 3), plain, "host run")
    # one region inside a 256-wide strip, one across the last strip's edge (the last strip starts at column 300 - 256 = 44)
    for (x, y, rw, rh), full in (((60, 4, 31, 9), False), ((17, 0, 283, fh), True)):
        with ipa.launch_log() as ran:
            reg = _np(pipe.run_region(x, y, rw, rh, code), out_type, rh, rw)
        assert pipe.last_region_windowed is True
        _one_four_kernel(ran, is_float, out_type, full, window=True)
        sp._same(reg, np.ascontiguousarray(plain[y:y + rh, x:x + rw]), "region %r" % ((x, y, rw, rh),))


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (0, 1)])
def test_all_orientations(ipa, orc, rot, fh):
    """a non-Normal orientation: ipk_raw_to_srgb_oriented refuses the fourth colour, the driver runs the launch plus the permutation"""
    h, w = 23, 300
    data = _mosaic("u16", h, w, util.SEED + 14700)
    src = _src("ERBG", False)
    ops = dict(rotation=rot, fliph=bool(fh))
    for out_type in (F32, U16):
        want = sp._want(orc, _desc(orc, data, src, (0, 0, 0, 0), ops), out_type)
        pipe = _pipe(ipa, data, src, (0, 0, 0, 0), ops)
        got, ran = _logged(ipa, pipe, out_type)
        assert pipe.last_used_fused is True
        sp._same(got, want, "rotation %d fliph %d %s" % (rot, fh, out_type))
        # the one four-colour launch by its exact name, and besides it nothing but OpTransform's permutation of the result
        _one_four_kernel({e for e in ran if not e.startswith("ipk::k_rotate")}, False, out_type, True)
        assert len(ran) == (1 if (rot, fh) == (0, 0) else 2), sorted(ran)
        x, y, rw, rh = 3, 2, min(17, want.shape[1] - 3), min(9, want.shape[0] - 2)
        reg = _np(pipe.run_region(x, y, rw, rh, CODES[out_type]), out_type, rh, rw)
        assert pipe.last_region_windowed is True
        sp._same(reg, np.ascontiguousarray(want[y:y + rh, x:x + rw]), "region, rotation %d fliph %d" % (rot, fh))


def _fused_kw(cfa, w, h, is_float, out_type, **more):
    return dict(width=w, height=h, is_float=is_float, black0=util.BLACK, white0=util.WHITE, cfa=cfa, wb_coeffs=WB4, cam_to_xyz_normalized=sp._cam4(),
                out_type=CODES[out_type], four_colour=True, **more)


@pytest.mark.parametrize("is_float", [True, False])
def test_two_bands_concatenate_to_the_frame(ipa, orc, is_float):
    import torch
    h, w = 41, 300
    data = _mosaic("f32" if is_float else "u16", h, w, util.SEED + 14800)
    t = sp._upload(ipa, data, is_float)
    for out_type in (F32, U8):
        kw = _fused_kw(FILTERS["8x2"], w, h, is_float, out_type)
        whole = ipa.raw_to_srgb(t, **kw)
        pipe = _pipe(ipa, data, _src(FILTERS["8x2"], is_float), (0, 0, 0, 0), dict(points=[(0.5, 0.6)]))
        assert torch.equal(whole.view(torch.uint8), pipe._run(CODES[out_type])[0].view(torch.uint8)), "ipk_raw_to_srgb against the driver"
        parts = []
        for r0, r1 in ((0, 17), (17, h)):                                     # odd split: the second band starts on an odd tile row
            s0, s1 = max(r0 - 1, 0), min(r1 + 1, h)
            parts.append(ipa.raw_to_srgb(t[s0 * w:], band=(s0, s1 - s0, r0, r1 - r0), **kw))
        assert torch.equal(torch.cat(parts).view(torch.uint8), whole.view(torch.uint8)), "bands, %s" % out_type
    torch.cuda.synchronize()


def test_queue_less_schedule(ipa):
    """ipk_selftest_task_queue(0): no queue slot for the stream, so the 300x700 frame's 2 strips x 175 four-row tasks are walked statically (groups of four
    tasks per block, takeovers inside a block); the result must be the queued launch's"""
    import torch
    h, w = 700, 300
    t = sp._upload(ipa, _mosaic("u16", h, w, util.SEED + 14900), False)
    kw = _fused_kw("RGBE", w, h, False, F32)
    want = ipa.raw_to_srgb(t, **kw)
    torch.cuda.synchronize()
    L = ipa.lib()
    assert L.ipk_selftest_task_queue(0) == 0
    try:
        got = ipa.raw_to_srgb(t, **kw)
        torch.cuda.synchronize()
    finally:
        assert L.ipk_selftest_task_queue(1) == 0
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


# ---------------------------------------------------------------------------------------------
# guards: nothing outside width*rows*3 elements is written, nothing outside the frame is read into the result
# ---------------------------------------------------------------------------------------------
_GUARD_RUNS = [(shape, kind, out) for shape in ("36x11", "300x23") for kind, out in (("f32", F32), ("u16", U8), ("u16", U16))]


@pytest.mark.parametrize("shape,kind,out_type", _GUARD_RUNS, ids=["%s-%s-%s" % c for c in _GUARD_RUNS])
def test_guard_bands(ipa, orc, shape, kind, out_type):
    import torch
    h, w, crops = SHAPES[shape]
    data = _mosaic(kind, h, w, util.SEED + 15000 + w)
    src = _src("RGBE", kind != "u16")
    want = sp._want(orc, _desc(orc, data, src, crops, {}), out_type)
    tdt = {F32: torch.float32, U8: torch.uint8, U16: torch.int16}[out_type]
    for so, do in ((0, 0), (1, 1), (3, 5)):                                   # u16 source 2 bytes off a dword; destinations off their 16-byte groups
        emb, g = Embedded(data, so), Guarded(h * w * 3, tdt, do)
        img = ipa.RawImage(width=w, height=h, data=emb.view(), cfa="RGBE", blacklevels=src["blacklevels"], whitelevels=src["whitelevels"], wb_coeffs=WB4,
                           cam_to_xyz_normalized=sp._cam4(), is_float=src["is_float"])
        pipe = ipa.Pipeline.new_from_source(img)
        pipe.fuse_four_colour = True
        pipe._run(CODES[out_type], g.view(), None)
        torch.cuda.synchronize()
        assert pipe.last_used_fused is True
        got = g.result("run src+%d dst+%d" % (so, do))
        sp._same(got.reshape(h, w, 3), want, "run src+%d dst+%d" % (so, do))
        emb.assert_untouched(shape)
        x, y, rw, rh = 5, 2, w - 9, h - 4
        gr = Guarded(rw * rh * 3, tdt, do)
        pipe.run_region(x, y, rw, rh, CODES[out_type], gr.view())
        torch.cuda.synchronize()
        assert pipe.last_region_windowed is True
        sp._same(gr.result("region dst+%d" % do).reshape(rh, rw, 3), np.ascontiguousarray(want[y:y + rh, x:x + rw]), "region src+%d dst+%d" % (so, do))
        emb.assert_untouched(shape)


# ---------------------------------------------------------------------------------------------
# opt-in only
# ---------------------------------------------------------------------------------------------
def test_opt_in_only(ipa):
    import torch
    L = ipa.lib()
    h, w = 40, 300
    t = sp._upload(ipa, _mosaic("f32", h, w, util.SEED + 15100), True)
    with pytest.raises(ipa.IpkError) as e:
        ipa.raw_to_srgb(t, width=w, height=h, cfa="RGBE")
    assert e.value.code == UNSUPPORTED
    with pytest.raises(ipa.IpkError) as e:
        ipa.raw_to_srgb(t, width=w, height=h, cfa="RGXB", four_colour=True)     # an unknown letter stays refused either way
    assert e.value.code < 0
    g = Guarded(h * w * 3, torch.float32, 0)
    plan = ipa.FusedPlan(**_fused_kw("RGBE", w, h, True, F32))
    st = ipa._stream()
    plan.params.four_colour = 2
    assert L.ipk_raw_to_srgb(plan._ref, t.data_ptr(), g.ptr, st) == INVALID
    plan.params.four_colour = 1
    ow, oh = C.c_size_t(), C.c_size_t()
    for ori in (ipa._lib.OR_NORMAL, ipa._lib.OR_ROT90, ipa._lib.OR_HFLIP):
        assert L.ipk_raw_to_srgb_oriented(plan._ref, t.data_ptr(), ori, g.ptr, C.byref(ow), C.byref(oh), st) == UNSUPPORTED, ori
    assert L.ipk_raw_to_srgb_resampled(plan._ref, t.data_ptr(), 2, 2, w - 3, 2, 2, h - 3, w - 4, h - 4, g.ptr, st) == UNSUPPORTED
    assert L.ipk_raw_to_srgb_scaled(plan._ref, t.data_ptr(), w * 2 // 3, h * 2 // 3, g.ptr, st) == UNSUPPORTED
    assert L.ipk_stream_probe(plan._ref, t.data_ptr(), g.ptr, st) == UNSUPPORTED
    torch.cuda.synchronize()
    assert (g.whole() == g.sentinel).all(), "a refused call wrote to its destination"
    # three-colour filters do not look at the flag
    a = ipa.raw_to_srgb(t, width=w, height=h, cfa="GRBG", four_colour=True)
    b = ipa.raw_to_srgb(t, width=w, height=h, cfa="GRBG")
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    # the descriptor: without bit 1 the frame stages, used_fused = 0
    pipe = _pipe(ipa, _mosaic("u16", h, w, 7), _src("RGBE", False), (0, 0, 0, 0), {}, four=False)
    with ipa.launch_log() as ran:
        pipe.run()
    assert pipe.last_used_fused is False and any("k_demosaic_full" in e for e in ran) and not [e for e in ran if "four=1" in e]
