"""GPU parity of batches whose frames carry their own colour settings: ipk_pointwise_chain_out_batch (the frame-table mode of k_pointwise_chain_small and
k_raster_chain<Rgbe32, 1 | 2>: a grid plane per frame, the frame's arguments from a device table, the launch log's batch=1) and ipk_pipeline_run_batch_each
on top of it.  Bar: bit-exact (f32 bit patterns, any NaN == any NaN; equal u8 / u16) -- the primitive against ipk_pointwise_chain_out per frame, the
driver against the CPU oracle's pipeline with THAT FRAME'S OWN settings and against ipk_pipeline_run(descs[i]).  Every frame has its own seed and its own
parameters, so a mixed-up frame or table index cannot pass; every destination lies between sentinels at an odd element offset."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_batch_previews_route as br
import test_gpu_batch_previews as bp
from test_batch_previews_route import XT, ON, PLAIN_PREVIEWS, BATCH, OUT_F32, OUT_U8, OUT_U16
from test_gpu_batch_previews import NP_OUT, Spec, Frames, same

pytestmark = pytest.mark.gpu

S1 = "batch gofloat+demosaic"
S2E = {OUT_F32: "batch-each to_lab+basecurve+from_lab+gamma", OUT_U8: "batch-each to_lab+basecurve+from_lab+gamma+quantise",
       OUT_U16: "batch-each to_lab+basecurve+from_lab+gamma+quantise"}
CARRIER = {OUT_F32: r"^ipk::k_pointwise_chain_small\[fast_ok=[01],batch=1\]$", OUT_U8: r"^ipk::k_raster_chain<ipk::Rgbe32, 1>\[fast_ok=[01],batch=1\]$",
           OUT_U16: r"^ipk::k_raster_chain<ipk::Rgbe32, 2>\[fast_ok=[01],batch=1\]$"}
LINEAR = {OUT_F32: 0, OUT_U8: 0, OUT_U16: 1}                               # output_8bit forces the gamma on, output_16bit off
CURVE_GRID = [(0.2, 0.1), (0.4, 0.5), (0.6, 0.55), (0.8, 0.9)]             # six knots with the end points, one per grid cell at most: the grid form
CURVE_DENSE = [(0.2, 0.15), (0.4, 0.42), (0.401, 0.4215), (0.7, 0.75), (0.9, 0.93)]   # 0.4 and 0.401 share one of the grid's 256 cells: the knot search


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def param_set(i):
    """frame i's own parameters: seven kinds in turn, and a white balance no other frame of the batch has"""
    big = util.cam_matrix()
    big[1, 2] = np.float32(3.0e6)                                           # above 2^20: fast_ok = 0 for this frame alone
    other = (util.cam_matrix() * np.array([[0.9], [1.0], [1.1]], np.float32)).astype(np.float32)
    kinds = [dict(),                                                        # the synthetic camera's defaults
             dict(wb=(float("nan"), 1.0, 0.0, 2.0)),
             dict(points=[], exposure=0.0),                                 # no curve: has_curve = 0
             dict(points=CURVE_GRID, exposure=0.5),
             dict(points=CURVE_DENSE),
             dict(cam=big),
             dict(cam=other, exposure=-0.25)]
    p = dict(wb=util.WB, cam=util.cam_matrix(), exposure=0.0, points=[(0.5, 0.6)])
    p.update(kinds[i % 7])
    wb = list(p["wb"])
    wb[1] = wb[1] * (1.0 + (i // 7 + 1) / 32.0 + (i % 7) / 512.0)
    p["wb"] = tuple(wb)
    return p


def test_the_parameter_sets_are_what_they_claim():
    assert len({repr(sorted(param_set(i).items(), key=lambda kv: kv[0])) for i in range(65)}) == 65
    f = np.float32
    cells = [int((f(x) - f(0.0)) * f(256.0)) for x, _ in CURVE_DENSE]
    assert cells[1] == cells[2] and len(CURVE_GRID) + 2 == 6
    assert abs(param_set(5)["cam"][1, 2]) > 2.0 ** 20 and np.abs(param_set(6)["cam"]).max() < 2.0


def _stage_names(L, run):
    return bp._stage_names(L, run)


def carriers(ran):
    return sorted(e for e in ran if "batch=1" in e and ("k_pointwise_chain_small" in e or "k_raster_chain<" in e))


class Slots:
    """n destinations of `sizes` elements inside ONE sentinel-filled allocation, frame i in slot order[i]; `gap` elements between two slots (0: the
    destinations follow each other).  The first slot starts one element past a 256-byte boundary"""

    def __init__(self, sizes, out, order=None, gap=0):
        n = len(sizes)
        order = list(range(n)) if order is None else order
        by_slot = sorted(range(n), key=lambda i: order[i])
        self.start, pos = [0] * n, 0
        for i in by_slot:
            self.start[i] = pos
            pos += sizes[i] + gap
        self.sizes, self.total = sizes, max(pos, 1)
        self.g = util.Guarded(self.total, NP_OUT[out], off=1)
        esz = NP_OUT[out].itemsize
        self.ptrs = [self.g.ptr + s * esz for s in self.start]

    def results(self, what):
        a = self.g.result(what)
        sentinel = np.array(util.SENTINELS[a.dtype.name]).astype(a.dtype)
        mask = np.ones(self.total, bool)
        for s, z in zip(self.start, self.sizes):
            mask[s: s + z] = False
        assert (a[mask] == sentinel).all(), "%s: the gaps between the destinations were written" % what
        return [a[s: s + z] for s, z in zip(self.start, self.sizes)]


# ---------------------------------------------------------------------------------------------
# 1. the primitive
# ---------------------------------------------------------------------------------------------
def rgbe_frames(n, npix, seed):
    """n random RGBE buffers, each from its own seed: E = +0.0 but in the last frame, where every seventh pixel has one; the suite's special values in
    frame 0 (and in frame 1 where there is one)"""
    a = np.zeros((n, npix, 4), np.float32)
    for i in range(n):
        a[i, :, :3] = util.uniform_f32(seed + 7919 * i, npix * 3, -0.25, 1.5).reshape(npix, 3)
    for i in (0, 1)[:n]:
        flat = a[i, :, :3].reshape(-1)
        k = min(flat.size, util.SPECIALS.size)
        flat[(i * 5) % max(1, flat.size - k + 1):][:k] = util.SPECIALS[:k]
    a[n - 1, ::7, 3] = util.uniform_f32(seed + 3, a[n - 1, ::7, 3].size, 0.125, 0.5)
    return a


def chain_params(ipa, p):
    return ipa.chain_params(p["wb"], p["cam"], p["exposure"], p["points"])


def single_chain(ipa, src_ptr, w, h, p, linear, out):
    """ipk_pointwise_chain_out for one frame -> its w * h * 3 samples"""
    import torch
    L = ipa.lib()
    g = util.Guarded(w * h * 3, NP_OUT[out], off=3)
    cp = chain_params(ipa, p)
    rc = L.ipk_pointwise_chain_out(src_ptr, w, h, 0, cp.wb_coeffs, cp.cam_to_xyz_normalized, cp.exposure, cp.points, cp.npoints, linear, out, g.ptr, None)
    assert rc == 0, L.ipk_last_error()
    torch.cuda.synchronize()
    return g.result("single")


def blocks_per_frame(L, npix, out, n):
    """the launcher's rule (ipk_launch.hpp, chain_batch_blocks): sixteen wave-chunks of 128 (f32) / 256 pixels per block, capped at ceil(CUs / n)"""
    chunks = -(-npix // (128 if out == OUT_F32 else 256))
    return max(1, min(-(-chunks // 16), -(-L.ipk_device_cus() // n)))


def check_primitive(ipa, w, h, n, out, linear, seed):
    import torch
    L = ipa.lib()
    npix = w * h
    host = rgbe_frames(n, npix, seed)
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * npix * 16 for i in range(n)])
    ps = [param_set(i) for i in range(n)]
    from imagepipe_amd._lib import ChainParams
    arr = (ChainParams * n)(*[chain_params(ipa, p) for p in ps])
    slots = Slots([npix * 3] * n, out, order=list(range(n))[::-1], gap=37)
    dp = (C.c_void_p * n)(*slots.ptrs)
    tag = "%dx%d, n = %d, out %d, linear %d" % (w, h, n, out, linear)

    def call():
        assert L.ipk_pointwise_chain_out_batch(sp, w, h, 0, arr, n, linear, out, dp, ipa._stream()) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    with ipa.launch_log() as ran:
        names = _stage_names(L, call)
    got = slots.results(tag)
    assert names == ["pointwise_chain_out_batch"] * -(-n // 64), (tag, names)
    hits = carriers(ran)
    assert len(hits) >= 1 and all(re.match(CARRIER[out], e) for e in hits) and sorted(ran) == hits, (tag, sorted(ran))
    if n >= 6:
        assert any("fast_ok=0" in e for e in hits), (tag, hits)             # frame 5's matrix
    for i in range(n):
        want = single_chain(ipa, sp[i], w, h, ps[i], linear, out)
        same(got[i], want, "%s: frame %d against ipk_pointwise_chain_out" % (tag, i))
    assert np.array_equal(src.cpu().numpy().view(np.uint32), host.view(np.uint32)), tag + ": the sources were written"
    return got


SIZES = [(16, 16), (257, 1), (23, 17), (100, 66)]


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
@pytest.mark.parametrize("w,h", SIZES)
def test_primitive_sizes(ipa, w, h, out):
    """the 256-pixel floor, one pixel past it, the thumbnail, several blocks per frame"""
    L = ipa.lib()
    if (w, h) == (100, 66):
        assert blocks_per_frame(L, w * h, out, 5) > 1
    assert 16 * 16 == 256
    check_primitive(ipa, w, h, 5, out, LINEAR[out], util.SEED + 30000 + w)


@pytest.mark.parametrize("npix", [1, 127, 129])
def test_primitive_f32_takes_any_size(ipa, npix):
    for linear in (0, 1):
        check_primitive(ipa, npix, 1, 3, OUT_F32, linear, util.SEED + 30500 + npix)


@pytest.mark.parametrize("n", [1, 2, 65])
@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_primitive_frame_counts(ipa, n, out):
    """65 frames cross the 64-frame launch"""
    check_primitive(ipa, 23, 17, n, out, LINEAR[out], util.SEED + 31000 + n)


def test_primitive_monochrome(ipa):
    """monochrome = 1: the sRGB matrix and unit multipliers for every frame, the curves still per frame"""
    import torch
    L = ipa.lib()
    w, h, n, out = 23, 17, 3, OUT_U8
    host = rgbe_frames(n, w * h, util.SEED + 31500)
    host[:, :, 3] = 0.0
    src = torch.from_numpy(host).cuda()
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * w * h * 16 for i in range(n)])
    from imagepipe_amd._lib import ChainParams
    ps = [param_set(i + 2) for i in range(n)]
    arr = (ChainParams * n)(*[chain_params(ipa, p) for p in ps])
    slots = Slots([w * h * 3] * n, out, gap=5)
    assert L.ipk_pointwise_chain_out_batch(sp, w, h, 1, arr, n, 0, out, (C.c_void_p * n)(*slots.ptrs), None) == 0, L.ipk_last_error()
    torch.cuda.synchronize()
    got = slots.results("monochrome")
    for i in range(n):
        g = util.Guarded(w * h * 3, NP_OUT[out], off=3)
        cp = arr[i]
        assert L.ipk_pointwise_chain_out(sp[i], w, h, 1, cp.wb_coeffs, cp.cam_to_xyz_normalized, cp.exposure, cp.points, cp.npoints, 0, out, g.ptr, None) == 0
        torch.cuda.synchronize()
        same(got[i], g.result("single"), "monochrome frame %d" % i)


def test_primitive_refusals(ipa):
    """u8 / u16 under 256 pixels per frame, a curve the single form refuses, null and misaligned pointers, a wrong struct_size: nothing is written
    and nothing is launched; n = 0 is IPK_OK"""
    import torch
    L = ipa.lib()
    from imagepipe_amd._lib import ChainParams
    n, w, h = 3, 15, 17
    assert w * h == 255
    src = torch.from_numpy(rgbe_frames(n, 400, util.SEED + 32000)).cuda()
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * 400 * 16 for i in range(n)])
    arr = (ChainParams * n)(*[chain_params(ipa, param_set(i)) for i in range(n)])
    err = lambda: L.ipk_last_error().decode()
    for out in (OUT_U8, OUT_U16, OUT_F32):
        slots = Slots([400 * 3] * n, out, gap=4)
        dp = (C.c_void_p * n)(*slots.ptrs)
        with ipa.launch_log() as ran:
            if out != OUT_F32:
                assert L.ipk_pointwise_chain_out_batch(sp, w, h, 0, arr, n, 0, out, dp, None) == -5, out
                assert "256" in err()
            assert L.ipk_pointwise_chain_out_batch(sp, 20, 20, 0, arr, 0, 0, out, dp, None) == 0
            assert L.ipk_pointwise_chain_out_batch(None, 20, 20, 0, None, 0, 0, out, None, None) == 0
            bad = (ChainParams * n)(*[chain_params(ipa, param_set(i)) for i in range(n)])
            bad[2].npoints = 1
            bad[2].points[0], bad[2].points[1] = 0.0, 2.0                   # takes neither end point: a single knot, which the spline refuses
            assert L.ipk_pointwise_chain_out_batch(sp, 20, 20, 0, bad, n, 0, out, dp, None) == -2 and "params[2]" in err(), err()
            bad[2].npoints = 65
            assert L.ipk_pointwise_chain_out_batch(sp, 20, 20, 0, bad, n, 0, out, dp, None) == -2 and "params[2]" in err(), err()
            bad = (ChainParams * n)(*[chain_params(ipa, param_set(i)) for i in range(n)])
            bad[1].struct_size = 584
            assert L.ipk_pointwise_chain_out_batch(sp, 20, 20, 0, bad, n, 0, out, dp, None) == -2 and "params[1]" in err(), err()
            holed = (C.c_void_p * n)(sp[0], None, sp[2])
            assert L.ipk_pointwise_chain_out_batch(holed, 20, 20, 0, arr, n, 0, out, dp, None) == -2 and "index 1" in err(), err()
            holed = (C.c_void_p * n)(dp[0], dp[1], None)
            assert L.ipk_pointwise_chain_out_batch(sp, 20, 20, 0, arr, n, 0, out, holed, None) == -2 and "index 2" in err(), err()
            off = (C.c_void_p * n)(sp[0] + 4, sp[1], sp[2])
            assert L.ipk_pointwise_chain_out_batch(off, 20, 20, 0, arr, n, 0, out, dp, None) == -2 and "frame 0" in err(), err()
            assert L.ipk_pointwise_chain_out_batch(sp, 20, 20, 0, arr, n, 0, 3, dp, None) == -2
            torch.cuda.synchronize()
        assert not ran, sorted(ran)
        for r in slots.results("refusals"):
            assert (r == np.array(util.SENTINELS[r.dtype.name]).astype(r.dtype)).all(), "a refused call wrote to a destination"


def test_the_python_wrapper_of_the_primitive(ipa):
    import torch
    w, h, n = 23, 17, 4
    host = rgbe_frames(n, w * h, util.SEED + 32500)
    src = torch.from_numpy(host).cuda()
    ps = [param_set(i) for i in range(n)]
    outs = ipa.pointwise_chain_out_batch([src[i] for i in range(n)], w, h, [chain_params(ipa, p) for p in ps], out_type=OUT_U16, linear=True)
    torch.cuda.synchronize()
    assert len(outs) == n and tuple(outs[0].shape) == (h, w, 3) and outs[0].dtype == torch.int16
    for i in (0, 3):
        want = single_chain(ipa, src[i].data_ptr(), w, h, ps[i], 1, OUT_U16)
        same(outs[i].cpu().numpy().view(np.uint16).ravel(), want, "wrapper frame %d" % i)


# ---------------------------------------------------------------------------------------------
# 2. the driver
# ---------------------------------------------------------------------------------------------
KINDS = {
    "rggb-u16": dict(src="u16", **bp.MOSAICS["rggb"]),
    "rggb-f32": dict(src="f32", **bp.MOSAICS["rggb"]),                      # frame 1 holds the special values
    "xtrans-u16": dict(src="u16", **bp.MOSAICS["xtrans"]),                  # 300x240 under maxwidth 30: scale 10 >= minscale 3
    "mono-u16": dict(kind="mono", src="u16", w=131, h=113, maxwidth=30, crops=(3, 1, 2, 5), mask=ON | BATCH | PLAIN_PREVIEWS),
    "rgbe-u16": dict(kind="RGBE", src="u16", w=211, h=157, maxwidth=23, crops=(2, 3, 4, 5)),
}
_FR = {}


def kind_frames(name, n=3):
    if name not in _FR or len(_FR[name][1].host) < n:
        spec = Spec(**KINDS[name])
        _FR[name] = (spec, Frames(spec, n, util.SEED + 33000 + 100 * sorted(KINDS).index(name)))
    return _FR[name]


def desc_of(spec, L, out, p, mask=None):
    d = spec.desc(L, out, mask=mask)
    d.wb_coeffs[:] = [float(v) for v in p["wb"]]
    d.cam_to_xyz_normalized[:] = [float(v) for v in np.asarray(p["cam"], np.float32).ravel()]
    d.exposure = p["exposure"]
    pts = np.asarray(p["points"], np.float32).ravel()
    d.npoints = pts.size // 2
    for k in range(128):
        d.points[k] = float(pts[k]) if k < pts.size else 0.0
    return d


def oracle_of(orc, L, spec, data, out, p):
    desc = orc.make_pipeline(data, cfa=spec.shifted(L), is_cfa=bool(spec.cfa), cpp=spec.cpp, crops=spec.crops, blacklevels=spec.levels[0],
                             whitelevels=spec.levels[1], cam_to_xyz_normalized=p["cam"], wb_coeffs=p["wb"], exposure=p["exposure"], points=list(p["points"]),
                             maxwidth=spec.maxwidth, linear=False, **spec.ops)
    threads = orc.max_threads()
    orc.set_num_threads(1)                                                  # a thumbnail's source: a team of threads costs more than the frame
    try:
        with np.errstate(all="ignore"):
            return {OUT_F32: orc.pipeline_run, OUT_U8: orc.pipeline_output_8bit, OUT_U16: orc.pipeline_output_16bit}[out](desc)
    finally:
        orc.set_num_threads(threads)


def run_each(ipa, descs, ptrs, out, sizes, layout):
    """ipk_pipeline_run_batch_each into one sentinel-filled allocation -> ([frame i's samples], the launch log, the stage names, used_fused)"""
    import torch
    from imagepipe_amd._lib import PipelineDesc
    L = ipa.lib()
    n = len(descs)
    slots = Slots(sizes, out) if layout == "packed" else Slots(sizes, out, order=list(range(n))[::-1], gap=41)
    dp = (C.POINTER(PipelineDesc) * n)(*[C.pointer(d) for d in descs])
    sp, op = (C.c_void_p * n)(*ptrs), (C.c_void_p * n)(*slots.ptrs)
    used = C.c_int(-1)

    def call():
        assert L.ipk_pipeline_run_batch_each(dp, sp, op, n, out, C.byref(used), ipa._stream()) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    with ipa.launch_log() as ran:
        names = _stage_names(L, call)
    return slots.results("batch-each of %d" % n), ran, names, used.value


def run_single(ipa, d, ptr, out, size):
    import torch
    L = ipa.lib()
    g = util.Guarded(size, NP_OUT[out], off=3)
    used = C.c_int(-1)

    def call():
        assert L.ipk_pipeline_run(C.byref(d), ptr, g.ptr, out, C.byref(used), ipa._stream()) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    with ipa.launch_log() as ran:
        names = _stage_names(L, call)
    return g.result("single"), ran, names, used.value


def plan_of(L, descs, out):
    from imagepipe_amd._lib import PipelineDesc
    n = len(descs)
    dp = (C.POINTER(PipelineDesc) * n)(*[C.pointer(d) for d in descs])
    route, first = (C.c_int * n)(), (C.c_size_t * n)()
    assert L.ipk_pipeline_batch_each_plan(dp, n, out, route, first) == 0, L.ipk_last_error()
    return list(route), list(first)


def check_varied(ipa, orc, name, n, out, layout, oracle_frames=None):
    L = ipa.lib()
    spec, frames = kind_frames(name, n)
    ps = [param_set(i) for i in range(n)]
    descs = [desc_of(spec, L, out, p) for p in ps]
    dw, dh, fw, fh = br.sizes(L, descs[0])
    assert (dw, dh) == (fw, fh) and dw * dh >= 256
    px3 = fw * fh * 3
    tag = "%s %dx%d, n = %d, out %d, %s" % (name, dw, dh, n, out, layout)
    taken, chunk, _ = br.report(L, descs[0], n, out)
    assert taken == 1 and chunk == 64 and plan_of(L, descs, out) == ([2] * n, [0] * n), tag
    got, ran, names, used = run_each(ipa, descs, frames.ptrs[:n], out, [px3] * n, layout)
    singles = [run_single(ipa, descs[i], frames.ptrs[i], out, px3) for i in range(n)]
    for i in range(n):
        same(got[i], singles[i][0], "%s: frame %d against ipk_pipeline_run" % (tag, i))
    for i in (range(n) if oracle_frames is None else oracle_frames):
        want = oracle_of(orc, L, spec, frames.host[i], out, ps[i])
        assert want.shape == (fh, fw, 3), tag
        same(got[i], want, "%s: frame %d against the oracle with its own settings" % (tag, i))
    # one scaling launch group and exactly ONE pass-2 launch per chunk, wherever the destinations lie; a final chunk of one frame is ipk_pipeline_run
    full, rest = divmod(n, chunk)
    multi = full + (1 if rest > 1 else 0)
    assert names[: 2 * multi] == [S1, S2E[out]] * multi, (tag, names)
    assert names[2 * multi:] == (singles[n - 1][2] if rest == 1 else []), (tag, names)
    hits = carriers(ran)
    assert len(hits) == 1 and re.match(CARRIER[out], hits[0]), (tag, sorted(ran))
    assert used == singles[n - 1][3] == 0, tag
    assert not any("batch" in e for s in singles for e in s[1]) and not any(x.startswith("batch") for s in singles for x in s[2]), tag
    return descs, frames, got


@pytest.mark.parametrize("layout", ["packed", "reverse"])
@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
@pytest.mark.parametrize("n", [2, 3])
def test_driver_small_batches(ipa, orc, n, out, layout):
    check_varied(ipa, orc, "rggb-u16", n, out, layout)


@pytest.mark.parametrize("out,layout", [(OUT_U8, "reverse"), (OUT_F32, "packed")])
def test_driver_crosses_the_launch(ipa, orc, out, layout):
    """65 frames: a chunk of 64 and a chunk of one frame, which takes the single path"""
    check_varied(ipa, orc, "rggb-u16", 65, out, layout, oracle_frames=(0, 5, 63, 64))


@pytest.mark.parametrize("name,out", [("rggb-f32", OUT_F32), ("rggb-f32", OUT_U8), ("xtrans-u16", OUT_U16), ("xtrans-u16", OUT_F32), ("mono-u16", OUT_U8),
                                      ("mono-u16", OUT_F32)])
def test_driver_frame_kinds(ipa, orc, name, out):
    check_varied(ipa, orc, name, 3, out, "reverse")


def test_driver_four_colour_filter(ipa, orc):
    """a filter with a fourth colour keeps E through the scaling pass, so every pixel of the chain takes the literal form: on the route exactly where the
    uniform route's report admits it"""
    L = ipa.lib()
    spec, _ = kind_frames("rgbe-u16")
    d = desc_of(spec, L, OUT_U8, param_set(0))
    admitted = br.report(L, d, 3, OUT_U8)[0] == 1
    descs = [desc_of(spec, L, OUT_U8, param_set(i)) for i in range(3)]
    assert plan_of(L, descs, OUT_U8)[0] == ([2] * 3 if admitted else [0] * 3)
    if admitted:
        check_varied(ipa, orc, "rgbe-u16", 3, OUT_U8, "reverse")
    else:
        _, frames = kind_frames("rgbe-u16")
        px3 = br.sizes(L, d)[2] * br.sizes(L, d)[3] * 3
        got, ran, _, _ = run_each(ipa, descs, frames.ptrs[:3], OUT_U8, [px3] * 3, "reverse")
        assert not carriers(ran)
        for i in range(3):
            same(got[i], run_single(ipa, descs[i], frames.ptrs[i], OUT_U8, px3)[0], "rgbe frame %d" % i)


def test_mixed_batch(ipa, orc):
    """two shapes interleaved, a portrait frame, a run of identical descriptors, a varied run: every frame is its own ipk_pipeline_run"""
    L = ipa.lib()
    out = OUT_U8
    a, fa = kind_frames("rggb-u16", 8)
    x, fx = kind_frames("xtrans-u16", 3)
    portrait = Spec(src="u16", rotation=1, maxheight=23, **bp.MOSAICS["rggb"])
    items = [(a, fa, 0, 0), (x, fx, 0, 1), (a, fa, 1, 2), (x, fx, 1, 3),          # interleaved: runs of one
             (portrait, fa, 2, 4),                                              # Rotate90: a run of one
             (a, fa, 3, 5), (a, fa, 4, 5), (a, fa, 5, 5),                       # identical descriptors: the uniform batch
             (x, fx, 2, 6),
             (a, fa, 6, 7), (a, fa, 7, 8)]                                      # a varied run of two
    descs = [desc_of(s, L, out, param_set(k)) for s, _, _, k in items]
    ptrs = [f.ptrs[i] for _, f, i, _ in items]
    sizes = [br.sizes(L, d)[2] * br.sizes(L, d)[3] * 3 for d in descs]
    assert br.sizes(L, descs[4])[2:] == (17, 23)
    route, first = plan_of(L, descs, out)
    assert route == [0, 0, 0, 0, 0, 1, 1, 1, 0, 2, 2] and first == [0, 1, 2, 3, 4, 5, 5, 5, 8, 9, 9]
    got, ran, names, used = run_each(ipa, descs, ptrs, out, sizes, "reverse")
    for i, (s, f, j, k) in enumerate(items):
        one, _, _, _ = run_single(ipa, descs[i], ptrs[i], out, sizes[i])
        same(got[i], one, "mixed frame %d against ipk_pipeline_run" % i)
        if i in (0, 4, 6, 10):
            want = oracle_of(orc, L, s, f.host[j], out, param_set(k))
            same(got[i], want, "mixed frame %d against the oracle" % i)
    # the varied run: one pass-2 launch; the uniform run keeps ipk_pipeline_run_batch's rule, a chain launch per frame for these scattered destinations
    assert names.count(S2E[out]) == 1 and names.count(bp.S2[out]) == 3 and names.count(S1) == 2, names
    assert len(carriers(ran)) == 1, sorted(ran)


def test_without_the_bit(ipa, orc):
    """the same results from the loop, and no frame-table launch"""
    L = ipa.lib()
    out, n = OUT_U8, 3
    spec, frames = kind_frames("rggb-u16", n)
    ps = [param_set(i) for i in range(n)]
    on = [desc_of(spec, L, out, p) for p in ps]
    off = [desc_of(spec, L, out, p, mask=ON) for p in ps]
    assert plan_of(L, off, out) == ([0] * n, [0] * n)
    px3 = 23 * 17 * 3
    got1, _, _, _ = run_each(ipa, on, frames.ptrs[:n], out, [px3] * n, "packed")
    got0, ran0, names0, used0 = run_each(ipa, off, frames.ptrs[:n], out, [px3] * n, "packed")
    assert not [e for e in ran0 if "batch=1" in e] and not [s for s in names0 if s.startswith("batch")] and used0 == 0, (sorted(ran0), names0)
    _, _, names1, _ = run_single(ipa, off[0], frames.ptrs[0], out, px3)
    assert names0 == names1 * n
    for i in range(n):
        same(got0[i], got1[i], "frame %d without the bit" % i)


def test_the_uniform_batch_keeps_its_launches(ipa, orc):
    """ipk_pipeline_run_batch on one of these descriptors: its old stages, and the chain's flat launch without the new tag"""
    L = ipa.lib()
    out, n = OUT_U8, 3
    spec, frames = kind_frames("rggb-u16", n)
    d = desc_of(spec, L, out, param_set(3))
    got, ran, names, used = bp.run_batch(ipa, d, frames.ptrs[:n], out, 23 * 17 * 3)
    assert names == [S1, bp.S2[out]] and used == 0, names
    assert "ipk::k_raster_chain<ipk::Rgbe32, 1>[fast_ok=1]" in ran and not carriers(ran), sorted(ran)
    assert len(bp.batch_entries(ran)) == 1 and re.match(bp.mosaic_tag("u16"), bp.batch_entries(ran)[0]), sorted(ran)
    for i in range(n):
        same(got[i], oracle_of(orc, L, spec, frames.host[i], out, param_set(3)), "uniform frame %d" % i)
    # and through the new entry point, where identical descriptors are route 1
    descs = [desc_of(spec, L, out, param_set(3)) for _ in range(n)]
    assert plan_of(L, descs, out) == ([1] * n, [0] * n)
    got_e, ran_e, names_e, _ = run_each(ipa, descs, frames.ptrs[:n], out, [23 * 17 * 3] * n, "packed")
    assert names_e == names and not carriers(ran_e)
    for i in range(n):
        same(got_e[i], got[i], "route 1 frame %d" % i)


def test_driver_refusals(ipa):
    """an invalid descriptor, a degenerate curve, a null frame pointer: IPK_ERR_INVALID with the index, nothing launched, nothing written; n = 0 is IPK_OK"""
    import torch
    from imagepipe_amd._lib import PipelineDesc
    L = ipa.lib()
    out, n = OUT_U8, 3
    spec, frames = kind_frames("rggb-u16", n)
    px3 = 23 * 17 * 3
    err = lambda: L.ipk_last_error().decode()

    def attempt(descs, ptrs, dsts=None):
        slots = Slots([px3] * n, out, gap=3)
        dp = (C.POINTER(PipelineDesc) * n)(*[C.pointer(d) if d is not None else None for d in descs])
        op = (C.c_void_p * n)(*(slots.ptrs if dsts is None else dsts(slots.ptrs)))
        with ipa.launch_log() as ran:
            rc = L.ipk_pipeline_run_batch_each(dp, (C.c_void_p * n)(*ptrs), op, n, out, None, None)
            torch.cuda.synchronize()
        assert rc == -2 and not ran, (rc, sorted(ran))
        for r in slots.results("refused"):
            assert (r == np.uint8(util.SENTINELS["uint8"])).all()
        return err()
    good = lambda: [desc_of(spec, L, out, param_set(i)) for i in range(n)]
    ds = good(); ds[2].fuse_rotatecrop = 7
    assert "descriptor 2" in attempt(ds, frames.ptrs[:n])
    ds = good(); ds[1].npoints = 1
    ds[1].points[0], ds[1].points[1] = 0.0, 2.0                             # a single knot: a curve the launches refuse
    assert "descriptor 1" in attempt(ds, frames.ptrs[:n])
    ds = good(); ds[0] = None
    assert "index 0" in attempt(ds, frames.ptrs[:n])
    assert "index 1" in attempt(good(), [frames.ptrs[0], None, frames.ptrs[2]])
    assert "index 2" in attempt(good(), frames.ptrs[:n], dsts=lambda p: [p[0], p[1], None])
    assert L.ipk_pipeline_run_batch_each(None, None, None, 0, out, None, None) == 0


def test_the_python_wrapper_of_the_driver(ipa, orc):
    import torch
    L = ipa.lib()
    spec, frames = kind_frames("rggb-u16", 3)
    pipes = []
    sets = [param_set(3 * i) for i in range(3)]                             # the defaults, the grid curve, the second matrix (RawImage wants a normal wb)
    for i in range(3):
        p = sets[i]
        img = ipa.RawImage(width=spec.w, height=spec.h, data=frames.views[i], cfa="RGGB", crops=spec.crops, blacklevels=[util.BLACK] * 4,
                           whitelevels=[util.WHITE] * 4, wb_coeffs=p["wb"], cam_to_xyz_normalized=p["cam"])
        pipe = ipa.Pipeline.new_from_source(img)
        pipe.globals.settings.maxwidth = spec.maxwidth
        pipe.ops.basecurve.points = list(p["points"])
        pipe.ops.basecurve.exposure = p["exposure"]
        pipe.batch_previews = True
        pipes.append(pipe)
    assert ipa.batch_each_plan(pipes, OUT_U8) == [(2, 0)] * 3
    with ipa.launch_log() as ran:
        outs = ipa.run_batch_each(pipes, frames.views[:3], OUT_U8)
        torch.cuda.synchronize()
    assert len(carriers(ran)) == 1 and tuple(outs[0].shape) == (17, 23, 3) and pipes[0].last_used_fused is False
    for i in range(3):
        same(outs[i].cpu().numpy().ravel(), oracle_of(orc, L, spec, frames.host[i], OUT_U8, sets[i]), "run_batch_each frame %d" % i)


# ---------------------------------------------------------------------------------------------
# 3. rasters: a frame with the default ops takes the integer fast path, inside a batch as alone
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out,exposures,want_route", [(OUT_U8, (0.25, 0.5, 0.0, 0.0, 0.25, 0.5), [2, 2, 1, 1, 2, 2]), (OUT_U8, (0.25, 0.0, 0.5), [0, 0, 0]),
                                                      (OUT_U16, (0.0, 0.25, 0.5), [0, 2, 2]), (OUT_F32, (0.25, 0.0, 0.5), [2, 2, 2])])
def test_rasters_with_and_without_the_fast_path(ipa, orc, out, exposures, want_route):
    import test_batch_each_route as ber
    L = ipa.lib()
    n = len(exposures)
    spec = Spec("rgb8", "rgb8", 131, 113, 40)
    frames = Frames(spec, n, util.SEED + 34000 + out)
    descs = [ber.raster(L, e) for e in exposures]
    assert [L.ipk_pipeline_takes_fastpath(C.byref(d), out) for d in descs] == [int(e == 0.0 and out != OUT_F32) for e in exposures]
    assert plan_of(L, descs, out)[0] == want_route
    fw, fh = br.sizes(L, descs[0])[2:]
    px3 = fw * fh * 3
    got, ran, names, _ = run_each(ipa, descs, frames.ptrs, out, [px3] * n, "reverse")
    for i in range(n):
        one, _, names1, _ = run_single(ipa, descs[i], frames.ptrs[i], out, px3)
        same(got[i], one, "raster frame %d (exposure %s) against ipk_pipeline_run" % (i, exposures[i]))
        assert (names1 == ["fastpath"]) == (exposures[i] == 0.0 and out != OUT_F32), names1
        desc = orc.make_pipeline(frames.host[i], exposure=exposures[i], maxwidth=40, use_fastpath=True)
        with np.errstate(all="ignore"):
            want = {OUT_F32: orc.pipeline_run, OUT_U8: orc.pipeline_output_8bit, OUT_U16: orc.pipeline_output_16bit}[out](desc)
        same(got[i], want, "raster frame %d against the oracle" % i)
    assert names.count(S2E[out]) == want_route.count(2) // 2 and len(carriers(ran)) == (1 if 2 in want_route else 0), (names, sorted(ran))
    assert names.count("fastpath") == sum(e == 0.0 and out != OUT_F32 for e in exposures), names
