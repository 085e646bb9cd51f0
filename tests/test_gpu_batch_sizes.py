"""GPU parity of batches whose frames have their own preview size: ipk_scaled_demosaic_batch_sized (the sized frame-table mode of k_raw_scaled_demosaic<T>:
the record also brings the frame's result size and its slice's offset; the launch log's batch=1,frames=1,sized=1), ipk_pointwise_chain_out_batch_sized (a
record brings its frame's pixel count; batch=1,sized=1) and ipk_pipeline_run_batch_each under IPK_FUSED_BATCH_SIZES on top of both.  Bar: bit-exact (f32
bit patterns, any NaN == any NaN; equal u8 / u16) -- the primitives against the single-frame calls on that frame's own arguments and size and against the
CPU oracle, the driver against ipk_pipeline_run(descs[i]) and against the oracle's pipeline with THAT FRAME'S OWN settings.  Destinations lie between
sentinels; sources are compared with their host copies afterwards.  Launches are COUNTED by ipk_timing's marks and NAMED by the launch log."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_batch_previews_route as br
import test_gpu_batch_previews as bp
import test_gpu_batch_each as eb
import test_gpu_batch_oriented as ob
import test_gpu_batch_sensor as sb
from test_batch_previews_route import XT, ON, PLAIN_PREVIEWS, BATCH, OUT_F32, OUT_U8, OUT_U16
from test_gpu_batch_previews import NP_OUT, Spec, Frames, same, B3, W3
from test_gpu_batch_each import param_set, desc_of, oracle_of, run_each, run_single, plan_of, S2E, LINEAR, Slots, rgbe_frames, chain_params
from test_gpu_batch_sensor import Case, LEVELS, CT, SRC, S1E, PLAIN_RGB, PLAIN_MONO

pytestmark = pytest.mark.gpu

ORIENTED, SENSOR, SIZES = 512, 1024, 2048
PRIM1, PRIM2 = "scaled_demosaic_batch_sized", "pointwise_chain_out_batch_sized"
S2T = {k: v.replace("+gamma", "+gamma+transform") for k, v in S2E.items()}
# (filter, pitch, x, y, width, height) -> (nwidth, nheight): RGGB at an odd x, GRBG, X-Trans, a larger sensor, and a wide strip whose 130 columns need a
# second block column beside the narrow ones; every skip is above 7, and 19x14 is both narrower and shorter than 25x19
MOSAICS = [(("RGGB", 216, 5, 2, 203, 151), (19, 14)), (("GRBG", 211, 4, 1, 203, 151), (25, 19)), ((XT, 221, 3, 1, 216, 162), (19, 15)),
           (("RGGB", 230, 0, 0, 230, 170), (23, 19)), (("RGGB", 1003, 2, 1, 1000, 100), (130, 10)), (("GRBG", 203, 0, 0, 203, 151), (17, 12))]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def sized_tag(T, plain=""):
    return r"^ipk::k_raw_scaled_demosaic<%s>\[norm_fast=0,norm_light=0,fast_x=0,fast_y=0,xcd=0%s,batch=1,frames=1,sized=1\]$" % (T, plain)


class SizedCase:
    """n frames, frame i a one-frame Case of its own size: its device copy, its record and the two references, computed once"""

    def __init__(self, ipa, orc, src, kind, geoms, levels, seed):
        self.ipa, self.src, self.kind = ipa, src, kind
        self.one = [Case(ipa, orc, src, kind, [g], [lv], nw, nh, seed + 7919 * i) for i, ((g, (nw, nh)), lv) in enumerate(zip(geoms, levels))]
        self.sizes = [s for _, s in geoms]

    def call(self, n, dst_ptr, sizes=None, recs=None):
        from imagepipe_amd._lib import ScaledFrame
        L = self.ipa.lib()
        arr = (ScaledFrame * max(n, 1))(*(recs if recs is not None else [c.rec[0] for c in self.one[:n]]))
        sp = (C.c_void_p * max(n, 1))(*[c.dev[0].data_ptr() for c in self.one[:n]])
        sz = (C.c_size_t * max(2 * n, 1))(*[v for wh in (self.sizes[:n] if sizes is None else sizes) for v in wh])
        return L.ipk_scaled_demosaic_batch_sized(sp, arr, sz, n, SRC[self.src], self.kind, dst_ptr, None)

    def check(self, n, off, tag_re, what):
        import torch
        L = self.ipa.lib()
        lens = [w * h * 4 for w, h in self.sizes[:n]]
        starts = np.concatenate([[0], np.cumsum(lens)]).astype(int)
        g = util.Guarded(int(starts[-1]), np.dtype(np.float32), off=off)

        def run():
            assert self.call(n, g.ptr) == 0, L.ipk_last_error()
            torch.cuda.synchronize()
        with self.ipa.launch_log() as ran:
            names = bp._stage_names(L, run)
        got = g.result(what)                                                # (the guard bands on both sides are checked there)
        for i in range(n):
            part = got[starts[i]: starts[i + 1]]
            same(part, self.one[i].single[0], "%s: slice %d against the single-frame call" % (what, i))
            same(part, self.one[i].oracle[0], "%s: slice %d against the oracle" % (what, i))
        assert names == [PRIM1] * -(-n // 64), (what, names)
        assert len(ran) == 1 and re.match(tag_re, sorted(ran)[0]), (what, sorted(ran))
        for c in self.one[:n]:
            now, host = c.dev[0].cpu().numpy(), c.host[0]
            assert np.array_equal(now.view(np.uint16) if host.dtype == np.uint16 else now.view(np.uint32),
                                  host if host.dtype == np.uint16 else host.view(np.uint32)), "%s: a source changed" % what


_CASES = {}


def mosaic_case(ipa, orc, src):
    if src not in _CASES:
        n = 65
        _CASES[src] = SizedCase(ipa, orc, src, -1, [MOSAICS[i % 6] for i in range(n)], [LEVELS[i % 5] for i in range(n)],
                                util.SEED + 51000 + (500 if src == "f32" else 0))
    return _CASES[src]


def test_the_frames_are_what_they_claim():
    f = np.float32
    for (cfa, pitch, x, y, w, h), (nw, nh) in MOSAICS:
        assert br.general_kernel(w, h, nw, nh) and x + w <= pitch
        assert (f(w - 1) - f(0)) / f(nw - 1) > 7.0 and (f(h - 1) - f(0)) / f(nh - 1) > 7.0
    sizes = [s for _, s in MOSAICS]
    assert MOSAICS[0][0][2] % 2 == 1 and len(set(sizes)) == 6 and max(w for w, _ in sizes) > 128 and min(w for w, _ in sizes) < 20
    assert any(w < 25 and h < 19 for w, h in sizes) and {i % 6 for i in range(6)} == set(range(6))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [2, 6, 65])
@pytest.mark.parametrize("src", ["u16", "f32"])
def test_sized_scaling_mosaics(ipa, orc, src, n, off):
    mosaic_case(ipa, orc, src).check(n, off, sized_tag(CT[src]), "sized mosaics %s n = %d, dst %d off" % (src, n, off))


@pytest.mark.parametrize("kind", [PLAIN_MONO, PLAIN_RGB])
@pytest.mark.parametrize("src", ["u16", "f32"])
def test_sized_scaling_plain_kinds(ipa, orc, src, kind):
    """monochrome and three-sample raws, every frame with its own source size, pitch, level pairs and result size"""
    geoms = [(("", 137, 5, 3, 131, 113), (30, 26)), (("", 100, 0, 0, 100, 90), (19, 17)), (("", 64, 1, 2, 61, 47), (7, 5)), (("", 211, 4, 1, 203, 151), (25, 19))]
    levels = [(B3, W3), ((10.0, 20.0, 30.0, 0.0), (4000.0, 8000.0, 16000.0, 0.0)), ((64.0, 300.0, 256.0, 0.0), (1023.0, 300.0, 16383.0, 0.0)),
              ((0.0, 1.0, 2.0, 0.0), (16383.0, 100.0, 2.0 ** -70, 0.0))]
    c = SizedCase(ipa, orc, src, kind, geoms, levels, util.SEED + 53000 + kind)
    tag = sized_tag(CT[src], ",plain=%d" % (1 if kind == PLAIN_MONO else 3))
    c.check(4, 0, tag, "sized plain kind %d %s" % (kind, src))
    c.check(3, 1, tag, "sized plain kind %d %s, one off" % (kind, src))


def test_sized_scaling_equal_sizes_and_refusals(ipa, orc):
    import torch
    L = ipa.lib()
    err = lambda: L.ipk_last_error().decode()
    c = mosaic_case(ipa, orc, "u16")
    sentinel = np.array(util.SENTINELS["float32"], np.float32)
    # frames 0 and 6 share 19x14: equal sizes are the call without sizes -- the frame-table launch without sized=1
    two = SizedCase.__new__(SizedCase)
    two.ipa, two.src, two.kind, two.one, two.sizes = ipa, "u16", -1, [c.one[0], c.one[6]], [(19, 14), (19, 14)]
    two.check(2, 0, sb.frames_tag(CT["u16"]), "equal sizes")
    g = util.Guarded(sum(w * h * 4 for w, h in c.sizes[:3]), np.dtype(np.float32))

    def refused(code, text, **kw):
        with ipa.launch_log() as ran:
            rc = c.call(3, g.ptr, **kw)
            torch.cuda.synchronize()
        assert rc == code and text in err() and not ran, (rc, err(), sorted(ran))
        assert (g.result(text) == sentinel).all(), "%s: the destination was written" % text
    refused(-2, "sizes[1]", sizes=[(19, 14), (0, 19), (19, 15)])
    refused(-2, "sizes[2]", sizes=[(19, 14), (25, 19), (19, 1 << 31)])
    assert not br.general_kernel(203, 151, 60, 44)
    refused(-5, "frames[1]", sizes=[(19, 14), (60, 44), (19, 15)])          # a window-8 geometry at its own size
    r = [k.rec[0] for k in c.one[:3]]
    bad = ipa.scaled_frame(216, 14, 2, 203, 151, [util.BLACK] * 4, [util.WHITE] * 4, "RGGB")
    refused(-2, "frames[0]", recs=[bad] + r[1:])
    with ipa.launch_log() as ran:
        assert c.call(0, g.ptr) == 0 and L.ipk_scaled_demosaic_batch_sized(None, None, None, 0, 0, -1, None, None) == 0
        torch.cuda.synchronize()
    assert not ran
    sz = (C.c_size_t * 6)(19, 14, 25, 19, 19, 15)
    assert L.ipk_scaled_demosaic_batch_sized(None, None, sz, 3, 0, -1, g.ptr, None) == -2
    assert L.ipk_scaled_demosaic_batch_sized(None, None, None, 3, 0, -1, g.ptr, None) == -2


# ---------------------------------------------------------------------------------------------
# the sized chain
# ---------------------------------------------------------------------------------------------
def chain_tag(out, oriented):
    return "^" + ob.KERNEL[out] + (r"\[fast_ok=[01],batch=1,orient=1,sized=1\]$" if oriented else r"\[fast_ok=[01],batch=1,sized=1\]$")


def check_chain(ipa, sizes, oris, out, seed, pass_null=False):
    """frame i of sizes[i] pixels with param_set(i) and orientation oris[i], into reversed slots with gaps, against the single form and the rotate entry
    point at its own size"""
    import torch
    from imagepipe_amd._lib import ChainParams
    L = ipa.lib()
    n, linear = len(sizes), LINEAR[out]
    npix = [w * h for w, h in sizes]
    starts = np.concatenate([[0], np.cumsum(npix)]).astype(int)
    host = np.concatenate([rgbe_frames(1, npix[i], seed + 104729 * i)[0] for i in range(n)])
    host[:, 3] = 0.0                                                        # E = +0.0 (the fast form) everywhere but in frame 1
    if n > 2:
        host[starts[1]: starts[2]: 5, 3] = util.uniform_f32(seed + 5, host[starts[1]: starts[2]: 5, 3].size, 0.125, 0.5)   # E samples: the literal form there
    src = torch.from_numpy(host).cuda()
    assert src.data_ptr() % 16 == 0
    sp = (C.c_void_p * n)(*[src.data_ptr() + int(starts[i]) * 16 for i in range(n)])
    ps = [param_set(i) for i in range(n)]
    arr = (ChainParams * n)(*[chain_params(ipa, p) for p in ps])
    ori = None if pass_null else (C.c_int * n)(*oris)
    sz = (C.c_size_t * (2 * n))(*[v for wh in sizes for v in wh])
    slots = Slots([p * 3 for p in npix], out, order=list(range(n))[::-1], gap=37)
    dp = (C.c_void_p * n)(*slots.ptrs)
    tag = "sizes %s, orientations %s, out %d" % (sizes[:8], "NULL" if pass_null else list(oris)[:8], out)

    def call():
        assert L.ipk_pointwise_chain_out_batch_sized(sp, sz, 0, arr, ori, n, linear, out, dp, ipa._stream()) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    with ipa.launch_log() as ran:
        names = eb._stage_names(L, call)
    got = slots.results(tag)
    assert names == [PRIM2] * -(-n // 64), (tag, names)
    hits = eb.carriers(ran)
    assert hits and sorted(ran) == hits and all("sized=1" in e for e in hits), (tag, sorted(ran))
    want_tags = {chain_tag(out, not pass_null and any(o not in (0, 8) for o in oris[k: k + 64])) for k in range(0, n, 64)}
    assert all(any(re.match(t, e) for t in want_tags) for e in hits) and all(any(re.match(t, e) for e in hits) for t in want_tags), (tag, hits)
    for i in range(n):
        w, h = sizes[i]
        want = ob.wanted(ipa, ("sized", tag, seed, i), sp[i], w, h, ps[i], linear, out, 0 if pass_null else oris[i])
        same(got[i], want, "%s: frame %d (%dx%d) against the single form and the rotate entry point" % (tag, i, w, h))
    assert np.array_equal(src.cpu().numpy().view(np.uint32), host.view(np.uint32)), tag + ": the sources were written"
    return hits


# 256 pixels: the floor, one chunk; 257: the last chunk overlaps the first by 255; 511: by one; 100 x 66 beside them: the grid has several blocks per
# frame, so the small frames see blocks with no work
FLOOR = [(16, 16), (257, 1), (7, 73), (100, 66), (1, 257), (19, 14)]


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_sized_chain_floor_and_overlap(ipa, out):
    assert [w * h for w, h in FLOOR[:3]] == [256, 257, 511]
    check_chain(ipa, FLOOR, [0] * 6, out, util.SEED + 54000, pass_null=True)
    check_chain(ipa, FLOOR, [0, 8, 0, 0, 8, 0], out, util.SEED + 54000)
    check_chain(ipa, FLOOR, [5, 1, 7, 2, 6, 4], out, util.SEED + 54100)


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_sized_chain_eight_orientations_on_non_square_frames(ipa, out):
    shapes = [(23, 17), (9, 33), (25, 19), (100, 66)]
    sizes = [shapes[(i + i // 8) % 4] for i in range(32)]
    oris = [i % 8 for i in range(32)]
    assert {(s, o) for s, o in zip(sizes, oris)} >= {(s, o) for s in shapes for o in range(8)}
    hits = check_chain(ipa, sizes, oris, out, util.SEED + 55000)
    assert any("fast_ok=0" in e for e in hits), hits                        # frame 5's matrix


def test_sized_chain_f32_takes_small_frames_and_crosses_the_launch(ipa):
    sizes = [[(1, 1), (3, 5), (16, 16), (129, 1), (23, 17)][i % 5] for i in range(66)]
    check_chain(ipa, sizes, [(3 * i) % 8 for i in range(66)], OUT_F32, util.SEED + 56000)


def test_sized_chain_equal_sizes_and_refusals(ipa):
    import torch
    from imagepipe_amd._lib import ChainParams
    L = ipa.lib()
    err = lambda: L.ipk_last_error().decode()
    n = 3
    host = rgbe_frames(n, 600, util.SEED + 57000)
    src = torch.from_numpy(host).cuda()
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * 600 * 16 for i in range(n)])
    arr = (ChainParams * n)(*[chain_params(ipa, param_set(i)) for i in range(n)])
    for out in (OUT_F32, OUT_U8):
        slots = Slots([600 * 3] * n, out, gap=5)
        dp = (C.c_void_p * n)(*slots.ptrs)
        sz = (C.c_size_t * 6)(30, 20, 30, 20, 30, 20)
        ori = (C.c_int * 3)(0, 5, 2)

        def call():
            assert L.ipk_pointwise_chain_out_batch_sized(sp, sz, 0, arr, ori, n, LINEAR[out], out, dp, None) == 0, err()
            torch.cuda.synchronize()
        with ipa.launch_log() as ran:
            names = eb._stage_names(L, call)
        hits = eb.carriers(ran)
        assert names == [PRIM2] and len(hits) == 1 and re.match(ob.ORIENT1[out], hits[0]), (names, hits)   # exactly the oriented call's launch and tag
        got = slots.results("equal sizes")
        for i in range(n):
            same(got[i], ob.wanted(ipa, ("sized-equal", out, i), sp[i], 30, 20, param_set(i), LINEAR[out], out, ori[i]), "equal sizes: frame %d" % i)
    slots = Slots([600 * 3] * n, OUT_U8, gap=5)
    dp = (C.c_void_p * n)(*slots.ptrs)

    def refused(code, text, sizes, out=OUT_U8, oris=(0, 0, 0)):
        sz = (C.c_size_t * 6)(*[v for wh in sizes for v in wh])
        with ipa.launch_log() as ran:
            rc = L.ipk_pointwise_chain_out_batch_sized(sp, sz, 0, arr, (C.c_int * 3)(*oris), n, 0, out, dp, None)
            torch.cuda.synchronize()
        assert rc == code and text in err() and not ran, (rc, err(), sorted(ran))
        slots.results(text)
    refused(-5, "sizes[1]", [(30, 20), (15, 17), (20, 30)])                 # 255 pixels to 8 bits
    refused(-2, "sizes[2]", [(30, 20), (20, 30), (0, 30)])
    refused(-2, "orientations[1]", [(30, 20), (20, 30), (10, 60)], oris=(0, 9, 0))
    assert L.ipk_pointwise_chain_out_batch_sized(sp, None, 0, arr, None, n, 0, OUT_U8, dp, None) == -2
    assert L.ipk_pointwise_chain_out_batch_sized(None, None, 0, None, None, 0, 0, OUT_U8, None, None) == 0


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
ROT = ON | BATCH | ORIENTED | SIZES
SEN = ON | BATCH | SENSOR | SIZES
BOTH = ROT | SENSOR
TRIPLES = [(0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 0, 0), (0, 0, 1), (1, 1, 0)]


def thumb(k, mask, src="u16", **ops):
    return Spec(kind="RGGB", src=src, w=211, h=157, maxwidth=19, crops=(2, 3, 4, 5), mask=mask, **ops)


def body(k, mask, src="u16", **ops):
    return Spec(kind="GRBG", src=src, w=200, h=160, maxwidth=19, mask=mask, levels=([util.BLACK + 2.0 + k] * 4, [util.WHITE - 30.0] * 4), **ops)


def turn(k):
    r, h, v = TRIPLES[k % 6]
    return dict(rotation=r, fliph=h, flipv=v)


RUNS = {
    "rotations": (lambda k, mask=ROT, src="u16": thumb(k, mask, src, **turn(k)), True, False),
    "bodies": (lambda k, mask=SEN, src="u16": (thumb if k % 2 == 0 else body)(k, mask, src), False, True),
    "both": (lambda k, mask=BOTH, src="u16": (thumb if k % 3 else body)(k, mask, src, **turn(k)), True, True),
}
_DRV = {}


def driver_frames(key, n, src="u16"):
    have = _DRV.setdefault((key, src), [])
    for k in range(len(have), n):
        spec = RUNS[key][0](k, src=src)
        have.append((spec, Frames(spec, 1, util.SEED + 58000 + 7919 * k, specials_in=0 if k % 3 == 1 else 1)))
    return have[:n]


def sized_entries(ran):
    return sorted(e for e in ran if "frames=1" in e)


def check_driver(ipa, orc, key, n, out, layout, oracle_frames=None, src="u16", T="unsigned short"):
    L = ipa.lib()
    make, turned, _ = RUNS[key]
    fr = driver_frames(key, n, src)
    specs = [make(k, src=src) for k in range(n)]
    ps = [param_set(i) for i in range(n)]
    descs = [desc_of(specs[i], L, out, ps[i]) for i in range(n)]
    sizes = [br.sizes(L, d) for d in descs]
    assert len({s[:2] for s in sizes}) > 1, sizes                           # the run's frames do differ in demosaic size
    px3 = [s[2] * s[3] * 3 for s in sizes]
    ptrs = [f.ptrs[0] for _, f in fr]
    tag = "%s n = %d, out %d, %s" % (key, n, out, layout)
    assert plan_of(L, descs, out) == ([2] * n, [0] * n), tag
    got, ran, names, used = run_each(ipa, descs, ptrs, out, px3, layout)
    singles = [run_single(ipa, descs[i], ptrs[i], out, px3[i]) for i in range(n)]
    for i in range(n):
        same(got[i], singles[i][0], "%s: frame %d against ipk_pipeline_run" % (tag, i))
    for i in (range(n) if oracle_frames is None else oracle_frames):
        want = oracle_of(orc, L, specs[i], fr[i][1].host[0], out, ps[i])
        assert want.shape == (sizes[i][3], sizes[i][2], 3), tag
        same(got[i], want, "%s: frame %d against the oracle with its own settings" % (tag, i))
    # per chunk of several frames: ONE sized scaling launch and ONE sized chain launch; a final chunk of one frame is ipk_pipeline_run
    full, rest = divmod(n, 64)
    multi = full + (1 if rest > 1 else 0)
    s2 = (S2T if turned else S2E)[out]
    assert names[: 2 * multi] == [S1E, s2] * multi and names[2 * multi:] == (singles[n - 1][2] if rest == 1 else []), (tag, names)
    hits = sized_entries(ran)
    assert len(hits) == 1 and re.match(sized_tag(T), hits[0]), (tag, sorted(ran))
    chain = eb.carriers(ran)
    assert 1 <= len(chain) <= multi and all(re.match(chain_tag(out, turned), e) for e in chain), (tag, sorted(ran))
    assert used == singles[n - 1][3] == 0, tag
    assert not any("batch" in e for s in singles for e in s[1]), tag
    for spec, f in fr:
        now, size = f.t.cpu().numpy(), f.host[0].size
        assert np.array_equal(now.view(np.uint16)[1: 1 + size] if f.host[0].dtype == np.uint16 else now.view(np.uint32)[1: 1 + size],
                              f.host[0].ravel() if f.host[0].dtype == np.uint16 else f.host[0].ravel().view(np.uint32)), "%s: a source changed" % tag
    return descs, names, ran, got


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
@pytest.mark.parametrize("key", list(RUNS))
def test_driver_run_kinds(ipa, orc, key, out):
    check_driver(ipa, orc, key, 2, out, "packed")
    check_driver(ipa, orc, key, 5, out, "reverse")


def test_driver_f32_sources(ipa, orc):
    check_driver(ipa, orc, "both", 4, OUT_U16, "reverse", src="f32", T="float")


@pytest.mark.parametrize("key", ["rotations", "both"])
def test_driver_67_frames(ipa, orc, key):
    """a chunk of 64 and a chunk of 3, both of mixed sizes"""
    L = ipa.lib()
    descs, names, _, _ = check_driver(ipa, orc, key, 67, OUT_U8, "reverse", oracle_frames=(0, 1, 63, 64, 66))
    assert len(names) == 4
    from imagepipe_amd._lib import PipelineDesc
    dp = (C.POINTER(PipelineDesc) * 67)(*[C.pointer(d) for d in descs])
    first = (C.c_size_t * 67)()
    assert L.ipk_pipeline_batch_each_chunks(dp, 67, OUT_U8, first) == 0 and list(first) == [0] * 64 + [64] * 3


@pytest.mark.parametrize("key", list(RUNS))
def test_without_the_bit_the_stage_list_is_the_loops(ipa, orc, key):
    """the same descriptors without bit 11: every frame a run of its own, the stages of n calls of ipk_pipeline_run, the same results"""
    L = ipa.lib()
    out, n = OUT_U8, 5
    make = RUNS[key][0]
    fr = driver_frames(key, n)
    ptrs = [f.ptrs[0] for _, f in fr]
    on = [desc_of(make(k), L, out, param_set(k)) for k in range(n)]
    off = [desc_of(make(k), L, out, param_set(k)) for k in range(n)]
    for d in off:
        d.allow_fused &= ~SIZES
    px3 = [br.sizes(L, d)[2] * br.sizes(L, d)[3] * 3 for d in on]
    assert plan_of(L, on, out) == ([2] * n, [0] * n)
    route, first = plan_of(L, off, out)
    assert first == list(range(n)) and route == [0] * n, (route, first)
    got1, ran1, _, _ = run_each(ipa, on, ptrs, out, px3, "packed")
    got0, ran0, names0, _ = run_each(ipa, off, ptrs, out, px3, "packed")
    singles = [run_single(ipa, off[i], ptrs[i], out, px3[i]) for i in range(n)]
    assert names0 == [s for one in singles for s in one[2]], names0
    assert sized_entries(ran1) and not [e for e in ran0 if "batch=1" in e], sorted(ran0)
    for i in range(n):
        same(got0[i], got1[i], "frame %d without bit 11" % i)


def test_a_chunk_of_equal_sizes_takes_the_old_launches(ipa, orc):
    """bit 11 set, Normal and Rotate180 only: one demosaic size, so the chunk is the uniform scaling launch and the oriented chain launch of bit 9"""
    L = ipa.lib()
    out, n = OUT_U8, 4
    specs = [thumb(k, ROT, rotation=2 * (k % 2)) for k in range(n)]
    frames = Frames(specs[0], n, util.SEED + 59000)
    descs = [desc_of(specs[k], L, out, param_set(k)) for k in range(n)]
    assert plan_of(L, descs, out) == ([2] * n, [0] * n) and {br.sizes(L, d)[:2] for d in descs} == {(19, 14)}
    px3 = 19 * 14 * 3
    got, ran, names, _ = run_each(ipa, descs, frames.ptrs, out, [px3] * n, "packed")
    assert names == [eb.S1, S2T[out]] and not [e for e in ran if "sized=1" in e], (names, sorted(ran))
    for i in range(n):
        same(got[i], run_single(ipa, descs[i], frames.ptrs[i], out, px3)[0], "frame %d" % i)


def test_the_python_wrappers(ipa, orc):
    import torch
    L = ipa.lib()
    c = mosaic_case(ipa, orc, "u16")
    out = ipa.scaled_demosaic_batch_sized([k.dev[0] for k in c.one[:5]], [k.rec[0] for k in c.one[:5]], c.sizes[:5])
    torch.cuda.synchronize()
    got, pos = out.cpu().numpy(), 0
    for i in range(5):
        w, h = c.sizes[i]
        same(got[pos: pos + w * h * 4], c.one[i].oracle[0], "scaled_demosaic_batch_sized slice %d" % i)
        pos += w * h * 4
    assert pos == got.size
    sizes = [(16, 16), (9, 33), (25, 19)]
    host = [rgbe_frames(1, w * h, util.SEED + 60000 + i)[0] for i, (w, h) in enumerate(sizes)]
    for a in host:
        a[:, 3] = 0.0
    dev = [torch.from_numpy(a).cuda() for a in host]
    ps = [param_set(i) for i in range(3)]
    outs = ipa.pointwise_chain_out_batch_sized(dev, sizes, [chain_params(ipa, p) for p in ps], out_type=OUT_U8, orientations=[0, 5, 3])
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == [(16, 16, 3), (9, 33, 3), (19, 25, 3)]
    for i, (w, h) in enumerate(sizes):
        want = ob.wanted(ipa, ("sized-wrapper", i), dev[i].data_ptr(), w, h, ps[i], 0, OUT_U8, [0, 5, 3][i])
        same(outs[i].cpu().numpy().ravel(), want, "pointwise_chain_out_batch_sized frame %d" % i)
    fr = driver_frames("rotations", 3)
    pipes = []
    for i, (spec, f) in enumerate(fr):
        p = param_set(3 * i)
        img = ipa.RawImage(width=spec.w, height=spec.h, data=f.views[0], cfa=spec.cfa, crops=spec.crops, blacklevels=list(spec.levels[0]),
                           whitelevels=list(spec.levels[1]), wb_coeffs=p["wb"], cam_to_xyz_normalized=p["cam"])
        pipe = ipa.Pipeline.new_from_source(img)
        pipe.globals.settings.maxwidth = 19
        pipe.ops.basecurve.points = list(p["points"])
        pipe.ops.basecurve.exposure = p["exposure"]
        pipe.ops.transform.rotation, pipe.ops.transform.fliph, pipe.ops.transform.flipv = spec.ops["rotation"], bool(spec.ops["fliph"]), bool(spec.ops["flipv"])
        pipe.batch_sizes = pipe.batch_oriented = True                       # nothing without batch_previews
        assert pipe.desc().allow_fused & (SIZES | ORIENTED) == 0
        pipe.batch_previews = True
        assert pipe.desc().allow_fused & (BATCH | ORIENTED | SIZES) == BATCH | ORIENTED | SIZES
        pipes.append(pipe)
    assert ipa.batch_each_plan(pipes, OUT_U8) == [(2, 0)] * 3 and ipa.batch_each_chunks(pipes, OUT_U8) == [0, 0, 0]
    with ipa.launch_log() as ran:
        outs = ipa.run_batch_each(pipes, [f.views[0] for _, f in fr], OUT_U8)
        torch.cuda.synchronize()
    assert len(sized_entries(ran)) == 1, sorted(ran)
    for i, (spec, f) in enumerate(fr):
        same(outs[i].cpu().numpy().ravel(), oracle_of(orc, L, spec, f.host[0], OUT_U8, param_set(3 * i)), "run_batch_each frame %d" % i)
