"""GPU parity of batches whose frames carry their own sensor settings: ipk_scaled_demosaic_batch_each (the frame-table mode of k_raw_scaled_demosaic<T>:
a grid plane per frame, the frame's source, pitch, window, skips, levels and filter from a device table, the launch log's batch=1,frames=1) and
ipk_pipeline_run_batch_each under IPK_FUSED_BATCH_SENSOR on top of it.  Bar: bit-exact (f32 bit patterns, any NaN == any NaN; equal u8 / u16) -- the
primitive against ipk_raw_scaled_demosaic / ipk_plain_scale_down on that frame's own arguments and against the CPU oracle, the driver against
ipk_pipeline_run(descs[i]) and against the oracle's pipeline with THAT FRAME'S OWN settings.  Every frame has its own seed; destinations lie between
sentinels; sources are compared with their host copies afterwards.
The launch log keeps each distinct entry once, so launches are COUNTED by ipk_timing's marks (one per launch) and NAMED by the log."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_batch_previews_route as br
import test_gpu_batch_previews as bp
import test_gpu_batch_each as eb
from test_batch_previews_route import XT, ON, PLAIN_PREVIEWS, BATCH, OUT_F32, OUT_U8, OUT_U16
from test_gpu_batch_previews import NP_OUT, Spec, Frames, same, B3, W3
from test_gpu_batch_each import param_set, desc_of, oracle_of, run_each, run_single, plan_of, S2E, S1, CARRIER

pytestmark = pytest.mark.gpu

ORIENTED, SENSOR = 512, 1024
S1E = "batch-each gofloat+demosaic"
PRIM = "scaled_demosaic_batch_each"
CT = {"u16": "unsigned short", "f32": "float"}
SRC = {"u16": br.U16, "f32": br.F32}
PLAIN_RGB, PLAIN_MONO = 1, 2
# the five level sets of tests/test_gpu_kernel_coverage.py (_RSD_LEVELS): ordinary, zero black, tiny, empty and inverted range
LEVELS = [(util.BLACK, util.WHITE), (0.0, util.WHITE), (0.0, 2.0 ** -70), (512.0, 512.0), (512.0, 100.0)]
# (filter, pitch, x, y, width, height): RGGB at an odd x, GRBG, X-Trans, a larger sensor -- all scaled to 23 x 17 with both skips above 7
MOSAICS = [("RGGB", 216, 5, 2, 203, 151), ("GRBG", 211, 4, 1, 203, 151), (XT, 221, 3, 1, 216, 162), ("RGGB", 230, 0, 0, 230, 170)]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def frames_tag(T, plain=""):
    return r"^ipk::k_raw_scaled_demosaic<%s>\[norm_fast=0,norm_light=0,fast_x=0,fast_y=0,xcd=0%s,batch=1,frames=1\]$" % (T, plain)


def sensor(seed, src, rows, pitch, spp=1, window=None):
    """a rows x pitch frame of noise from its own seed; f32 frames carry the suite's special values, +-inf and a NaN inside `window` (x, y, w, h)"""
    data = util.noise_u16(seed, rows, pitch * spp, 18000)
    if src == "f32":
        data = data.astype(np.float32) + util.uniform_f32(seed + 1, data.size, -0.5, 0.5).reshape(data.shape)
        x, y, w, h = window
        with np.errstate(over="ignore"):
            spc = util.SPECIALS * np.float32(16383.0)
        row = w * spp
        for k in range(0, spc.size, row):
            part = spc[k: k + row]
            data[y + min(h - 1, 1 + 2 * (k // row)), x * spp: x * spp + part.size] = part
        data[y + h // 2, (x + w // 3) * spp] = -np.inf
        data[y + h - 1, (x + min(3, w - 1)) * spp + spp - 1] = np.nan
        data[y + min(5, h - 1), (x + w - 1) * spp] = np.inf
    return data


class Case:
    """n frames of one primitive call: host data, device copies, the ipk_scaled_frame records, and the two references per frame -- computed once"""

    def __init__(self, ipa, orc, src, kind, geoms, levels, nw, nh, seed):
        import torch
        self.ipa, self.src, self.kind, self.nw, self.nh, self.n = ipa, src, kind, nw, nh, len(geoms)
        L = ipa.lib()
        spp = 3 if kind == PLAIN_RGB else 1
        self.host, self.dev, self.rec, self.single, self.oracle = [], [], [], [], []
        for i, ((cfa, pitch, x, y, w, h), (black, white)) in enumerate(zip(geoms, levels)):
            rows = y + h + 2
            data = sensor(seed + 7919 * i, src, rows, pitch, spp, (x, y, w, h))
            self.host.append(data)
            t = torch.from_numpy(data.view(np.int16) if data.dtype == np.uint16 else data).cuda()
            self.dev.append(t)
            b4 = list(black) if isinstance(black, (tuple, list)) else [black] * 4
            w4 = list(white) if isinstance(white, (tuple, list)) else [white] * 4
            self.rec.append(ipa.scaled_frame(pitch, x, y, w, h, b4, w4, cfa))
            g = util.Guarded(nw * nh * 4, np.dtype(np.float32), off=1)               # one element off: the general kernel whatever the geometry
            fb, fw = (C.c_float * 4)(*b4), (C.c_float * 4)(*w4)
            if kind == -1:
                rc = L.ipk_raw_scaled_demosaic(t.data_ptr(), SRC[src], pitch, x, y, w, h, b4[0], w4[0], cfa.encode(), nw, nh, g.ptr, None)
            else:
                rc = L.ipk_plain_scale_down(t.data_ptr(), SRC[src], kind, pitch, x, y, w, h, fb, fw, nw, nh, g.ptr, None)
            assert rc == 0, L.ipk_last_error()
            torch.cuda.synchronize()
            self.single.append(g.result("single frame %d" % i))
            with np.errstate(all="ignore"):
                if kind == -1:
                    want = orc.scaled_demosaic(cfa, orc.gofloat_cfa(data, x, y, w, h, b4[0], w4[0]), nw, nh)
                elif kind == PLAIN_MONO:
                    want = orc.scale_down_opbuf(orc.gofloat_mono(data, x, y, w, h, b4[0], w4[0]), nw, nh)
                else:
                    want = orc.scale_down_opbuf(orc.gofloat_rgb(data.reshape(rows, pitch, 3), x, y, w, h, b4, w4), nw, nh)
            self.oracle.append(want)

    def call(self, n, dst_ptr, recs=None, ptrs=None, kind=None):
        from imagepipe_amd._lib import ScaledFrame
        L = self.ipa.lib()
        recs = self.rec[:n] if recs is None else recs
        ptrs = [t.data_ptr() for t in self.dev[:n]] if ptrs is None else ptrs
        arr = (ScaledFrame * max(n, 1))(*recs)
        sp = (C.c_void_p * max(n, 1))(*ptrs)
        return L.ipk_scaled_demosaic_batch_each(sp, arr, n, SRC[self.src], self.kind if kind is None else kind, self.nw, self.nh, dst_ptr, None)

    def check(self, n, off, tag_re, what):
        import torch
        L = self.ipa.lib()
        slice_ = self.nw * self.nh * 4
        g = util.Guarded(n * slice_, np.dtype(np.float32), off=off)

        def run():
            assert self.call(n, g.ptr) == 0, L.ipk_last_error()
            torch.cuda.synchronize()
        with self.ipa.launch_log() as ran:
            names = bp._stage_names(L, run)
        got = g.result(what)
        for i in range(n):
            same(got[i * slice_: (i + 1) * slice_], self.single[i], "%s: slice %d against the single-frame call" % (what, i))
            same(got[i * slice_: (i + 1) * slice_], self.oracle[i], "%s: slice %d against the oracle" % (what, i))
        assert names == [PRIM] * -(-n // 64), (what, names)
        assert len(ran) == 1 and re.match(tag_re, sorted(ran)[0]), (what, sorted(ran))
        for i in range(n):
            now = self.dev[i].cpu().numpy()
            assert np.array_equal(now.view(np.uint16) if self.host[i].dtype == np.uint16 else now.view(np.uint32),
                                  self.host[i] if self.host[i].dtype == np.uint16 else self.host[i].view(np.uint32)), "%s: source %d changed" % (what, i)


_CASES = {}


def mosaic_case(ipa, orc, src):
    if src not in _CASES:
        n = 65
        _CASES[src] = Case(ipa, orc, src, -1, [MOSAICS[i % 4] for i in range(n)], [LEVELS[i % 5] for i in range(n)], 23, 17,
                           util.SEED + 41000 + (500 if src == "f32" else 0))
    return _CASES[src]


def test_the_frames_are_what_they_claim():
    for cfa, pitch, x, y, w, h in MOSAICS:
        assert br.general_kernel(w, h, 23, 17) and x + w <= pitch
        f = np.float32
        assert (f(w - 1) - f(0)) / f(22) > 7.0 and (f(h - 1) - f(0)) / f(16) > 7.0
    assert MOSAICS[0][2] % 2 == 1 and len({m[0] for m in MOSAICS}) == 3 and len({m[1] for m in MOSAICS}) == 4
    # five frames meet the four geometries and the five level sets
    assert {i % 4 for i in range(5)} == set(range(4)) and {i % 5 for i in range(5)} == set(range(5))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("n", [1, 2, 5, 65])
@pytest.mark.parametrize("src", ["u16", "f32"])
def test_primitive_mosaics(ipa, orc, src, n, off):
    mosaic_case(ipa, orc, src).check(n, off, frames_tag(CT[src]), "mosaics %s n = %d, dst %d off" % (src, n, off))


@pytest.mark.parametrize("src", ["u16", "f32"])
def test_primitive_geometry_extremes(ipa, orc, src):
    """a frame under 8 samples wide, a skip of 74 and no scaling at all, in one launch to 3 x 10"""
    geoms = [("RGGB", 12, 3, 1, 7, 30), ("GRBG", 153, 2, 1, 150, 100), ("RGGB", 3, 0, 0, 3, 10)]
    for _, _, _, _, w, h in geoms:
        assert br.general_kernel(w, h, 3, 10)
    c = Case(ipa, orc, src, -1, geoms, [LEVELS[0], LEVELS[1], LEVELS[0]], 3, 10, util.SEED + 42000)
    c.check(3, 0, frames_tag(CT[src]), "extremes %s" % src)
    c.check(3, 1, frames_tag(CT[src]), "extremes %s, one off" % src)


@pytest.mark.parametrize("kind", [PLAIN_MONO, PLAIN_RGB])
@pytest.mark.parametrize("src", ["u16", "f32"])
def test_primitive_plain_kinds(ipa, orc, src, kind):
    """monochrome and three-sample raws, every frame with its own size, pitch and level pairs (distinct per channel)"""
    geoms = [("", 137, 5, 3, 131, 113), ("", 100, 0, 0, 100, 90), ("", 64, 1, 2, 61, 47), ("", 211, 4, 1, 203, 151)]
    levels = [(B3, W3), ((10.0, 20.0, 30.0, 0.0), (4000.0, 8000.0, 16000.0, 0.0)), ((64.0, 300.0, 256.0, 0.0), (1023.0, 300.0, 16383.0, 0.0)),
              ((0.0, 1.0, 2.0, 0.0), (16383.0, 100.0, 2.0 ** -70, 0.0))]
    c = Case(ipa, orc, src, kind, geoms, levels, 30, 26, util.SEED + 43000 + kind)
    tag = frames_tag(CT[src], ",plain=%d" % (1 if kind == PLAIN_MONO else 3))
    c.check(4, 0, tag, "plain kind %d %s" % (kind, src))
    c.check(3, 1, tag, "plain kind %d %s, one off" % (kind, src))


def test_primitive_refusals(ipa, orc):
    import torch
    L = ipa.lib()
    err = lambda: L.ipk_last_error().decode()
    c = mosaic_case(ipa, orc, "u16")
    g = util.Guarded(3 * 23 * 17 * 4, np.dtype(np.float32))
    sentinel = np.array(util.SENTINELS["float32"], np.float32)

    def untouched(what):
        assert (g.result(what) == sentinel).all(), "%s: the destination was written" % what

    def refused(code, text, **kw):
        with ipa.launch_log() as ran:
            rc = c.call(3, g.ptr, **kw)
            torch.cuda.synchronize()
        assert rc == code and text in err() and not ran, (rc, err(), sorted(ran))
        untouched(text)

    def recs():
        return [ipa.scaled_frame(*MOSAICS[i][1:], [LEVELS[i][0]] * 4, [LEVELS[i][1]] * 4, MOSAICS[i][0]) for i in range(3)]
    # a window-8 geometry between admissible frames: 150x100 -> 50x40 in the issue's words; here every frame shares 23x17, where 150x100 has skips 6.77 and 6.19
    assert not br.general_kernel(150, 100, 23, 17) and not br.general_kernel(150, 100, 50, 40)
    r = recs(); r[1] = ipa.scaled_frame(153, 2, 1, 150, 100, [util.BLACK] * 4, [util.WHITE] * 4, "RGGB")
    refused(-5, "frames[1]", recs=r)
    # and at 50x40 itself, where the first frame is the first offender
    saved = (c.nw, c.nh)
    r = recs(); r[0] = ipa.scaled_frame(216, 5, 2, 150, 100, [util.BLACK] * 4, [util.WHITE] * 4, "RGGB")
    c.nw, c.nh = 50, 40
    try:
        g50 = util.Guarded(3 * 50 * 40 * 4, np.dtype(np.float32))
        with ipa.launch_log() as ran:
            rc = c.call(3, g50.ptr, recs=r)
            torch.cuda.synchronize()
        assert rc == -5 and "frames[0]" in err() and not ran and (g50.result("50x40") == sentinel).all(), (rc, err(), sorted(ran))
    finally:
        c.nw, c.nh = saved
    ptrs = [t.data_ptr() for t in c.dev[:3]]
    refused(-2, "index 2", ptrs=ptrs[:2] + [None])
    r = recs(); r[2].struct_size = 236
    refused(-2, "frames[2].struct_size", recs=r)
    r = recs(); r[1].cfa = b"RGXB"
    refused(-2, "frames[1]", recs=r)
    r = recs(); r[0].x = 14                                                 # 14 + 203 > 216
    refused(-2, "frames[0]", recs=r)
    r = recs(); r[2].height = 0
    refused(-2, "frames[2]", recs=r)
    refused(-5, "raster", kind=0)
    with ipa.launch_log() as ran:
        assert c.call(0, g.ptr) == 0 and L.ipk_scaled_demosaic_batch_each(None, None, 0, 0, -1, 23, 17, None, None) == 0
        torch.cuda.synchronize()
    assert not ran
    untouched("n = 0")


# ---------------------------------------------------------------------------------------------
# the driver
# ---------------------------------------------------------------------------------------------
MASK = ON | BATCH | SENSOR


def variant(k, mask=MASK, src="u16", **ops):
    """frame k's own sensor settings: the thumbnail, its levels moved, another crop origin (the filter's phase moves with it), an X-Trans body, a larger
    sensor with a zero black level -- all negotiating 23 x 17 under maxwidth 23"""
    lv = lambda b, w: ([b] * 4, [w] * 4)
    kinds = [dict(kind="RGGB", w=211, h=157, crops=(2, 3, 4, 5)),
             dict(kind="RGGB", w=211, h=157, crops=(2, 3, 4, 5), levels=lv(util.BLACK + 3.0 + k, util.WHITE - 50.0)),
             dict(kind="RGGB", w=211, h=157, crops=(2, 4, 4, 4), levels=lv(util.BLACK - 1.0, util.WHITE + float(k))),
             dict(kind=XT, w=216, h=162),
             dict(kind="RGGB", w=230, h=170, levels=lv(0.0, util.WHITE))]
    kw = dict(kinds[k % 5])
    kw.update(ops)
    return Spec(src=src, maxwidth=23, mask=mask, **kw)


_DRV = {}


def driver_frames(n, src="u16", make=variant, key="mosaic"):
    have = _DRV.setdefault((key, src), [])
    for k in range(len(have), n):
        spec = make(k, src=src)
        have.append((spec, Frames(spec, 1, util.SEED + 45000 + 7919 * k, specials_in=0 if k % 3 == 1 else 1)))
    return have[:n]


def chunk_entries(ran):
    return sorted(e for e in ran if "frames=1" in e)


def check_driver(ipa, orc, n, out, layout, oracle_frames=None, make=variant, key="mosaic", src="u16", T="unsigned short", plain=""):
    L = ipa.lib()
    fr = driver_frames(n, src, make, key)
    specs = [make(k, src=src) for k in range(n)]
    ps = [param_set(i) for i in range(n)]
    descs = [desc_of(specs[i], L, out, ps[i]) for i in range(n)]
    sizes = [br.sizes(L, d) for d in descs]
    assert all(s[:2] == sizes[0][:2] for s in sizes), sizes
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
    full, rest = divmod(n, 64)
    multi = full + (1 if rest > 1 else 0)
    assert names[0: 2 * multi: 2] == [S1E] * multi and all(x.startswith("batch-each to_lab") for x in names[1: 2 * multi: 2]), (tag, names)
    assert names[2 * multi:] == (singles[n - 1][2] if rest == 1 else []), (tag, names)
    hits = chunk_entries(ran)
    assert len(hits) == 1 and re.match(frames_tag(T, plain), hits[0]), (tag, sorted(ran))
    # one chain launch per chunk of several frames; the log keeps distinct entries, and fast_ok is the AND over ONE launch's frames: two chunks may differ in it
    assert 1 <= len(eb.carriers(ran)) <= multi, (tag, sorted(ran))
    assert used == singles[n - 1][3] == 0, tag
    assert not any("batch" in e for s in singles for e in s[1]), tag
    for spec, f in fr:
        now = f.t.cpu().numpy()
        size = f.host[0].size
        assert np.array_equal(now.view(np.uint16)[1: 1 + size] if f.host[0].dtype == np.uint16 else now.view(np.uint32)[1: 1 + size],
                              f.host[0].ravel() if f.host[0].dtype == np.uint16 else f.host[0].ravel().view(np.uint32)), "%s: a source changed" % tag
    return descs, names, ran


@pytest.mark.parametrize("layout", ["packed", "reverse"])
@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
@pytest.mark.parametrize("n", [2, 3])
def test_driver_small_batches(ipa, orc, n, out, layout):
    _, names, _ = check_driver(ipa, orc, n, out, layout)
    assert names == [S1E, S2E[out]], names


@pytest.mark.parametrize("out,layout", [(OUT_U8, "reverse"), (OUT_F32, "packed")])
def test_driver_crosses_the_launch(ipa, orc, out, layout):
    """65 frames: a chunk of 64 and a chunk of one frame, which takes the single path"""
    _, names, _ = check_driver(ipa, orc, 65, out, layout, oracle_frames=(0, 5, 63, 64))
    assert names[:2] == [S1E, S2E[out]], names


def test_driver_f32_sources(ipa, orc):
    check_driver(ipa, orc, 5, OUT_U16, "reverse", src="f32", T="float")


TRIPLES = [(0, 0, 0), (1, 0, 0), (2, 1, 0), (3, 0, 0), (0, 0, 1)]


def oriented_variant(k, src="u16"):
    """bits 9 and 10: frame k's own sensor settings and its own orientation, under the 23 x 23 box"""
    r, h, v = TRIPLES[k % 5]
    return variant(k, mask=MASK | ORIENTED, src=src, maxheight=23, rotation=r, fliph=h, flipv=v)


def test_driver_with_orientations_too(ipa, orc):
    """bits 9 and 10: sensor settings and orientation both vary inside one run under the 23 x 23 box"""
    _, names, ran = check_driver(ipa, orc, 5, OUT_U8, "reverse", make=oriented_variant, key="oriented")
    assert names == [S1E, "batch-each to_lab+basecurve+from_lab+gamma+transform+quantise"], names
    assert any("orient=1" in e for e in eb.carriers(ran)), sorted(ran)


@pytest.mark.parametrize("make,key,stage2", [(variant, "mosaic", S2E[OUT_U8]),
                                             (oriented_variant, "oriented", "batch-each to_lab+basecurve+from_lab+gamma+transform+quantise")],
                         ids=["bits_0_8_10", "bits_0_8_9_10"])
def test_driver_second_chunk_of_several_frames(ipa, orc, make, key, stage2):
    """67 frames: a chunk of 64 and a chunk of 3, whose shared settings are those of ITS first frame (frame 64), not of the run's"""
    _, names, ran = check_driver(ipa, orc, 67, OUT_U8, "reverse", oracle_frames=(0, 63, 64, 66), make=make, key=key)
    assert names == [S1E, stage2, S1E, stage2], names
    assert any("fast_ok=0" in e for e in eb.carriers(ran)), sorted(ran)    # frame 5's matrix, in the first chunk


@pytest.mark.parametrize("kind,plain", [("mono", ",plain=1"), ("cpp3", ",plain=3")])
def test_driver_plain_frames_with_their_own_levels(ipa, orc, kind, plain):
    """monochrome / three-sample raws under bit 7, every frame with its own level pairs, two sensor sizes"""
    def make(k, src="u16"):
        lv = ([64.0 + k, 128.0, 256.0 - k, 0.0], [1023.0 + 100 * k, 4095.0, 16383.0, 0.0]) if kind == "cpp3" else ([util.BLACK + k] * 4, [util.WHITE - 7.0 * k] * 4)
        w, h, crops = ((131, 113, (3, 1, 2, 5)), (140, 121, (0, 0, 0, 0)))[k % 2]
        return Spec(kind=kind, src=src, w=w, h=h, maxwidth=30, crops=crops, levels=lv, mask=MASK | PLAIN_PREVIEWS)
    check_driver(ipa, orc, 4, OUT_U8, "reverse", make=make, key=kind, plain=plain)


def test_sensor_fields_equal_and_colours_varied_is_the_old_launch(ipa, orc):
    L = ipa.lib()
    out, n = OUT_U8, 3
    spec = variant(0)
    frames = Frames(spec, n, util.SEED + 46000)
    descs = [desc_of(spec, L, out, param_set(i)) for i in range(n)]
    assert plan_of(L, descs, out) == ([2] * n, [0] * n)
    px3 = 23 * 17 * 3
    got, ran, names, _ = run_each(ipa, descs, frames.ptrs, out, [px3] * n, "packed")
    assert names == [S1, S2E[out]] and not chunk_entries(ran), (names, sorted(ran))
    assert [e for e in ran if re.match(r"^ipk::k_raw_scaled_demosaic<unsigned short>\[.*xcd=0,batch=1\]$", e)], sorted(ran)
    for i in range(n):
        same(got[i], run_single(ipa, descs[i], frames.ptrs[i], out, px3)[0], "frame %d" % i)


def test_without_the_bit(ipa, orc):
    """the same results from the loop, and no frame-table scaling launch"""
    L = ipa.lib()
    out, n = OUT_U8, 5
    fr = driver_frames(n)
    ptrs = [f.ptrs[0] for _, f in fr]
    on = [desc_of(variant(k), L, out, param_set(k)) for k in range(n)]
    off = [desc_of(variant(k, mask=ON | BATCH), L, out, param_set(k)) for k in range(n)]
    assert plan_of(L, on, out) == ([2] * n, [0] * n) and plan_of(L, off, out) == ([0] * n, list(range(n)))
    px3 = [23 * 17 * 3] * n
    got1, ran1, _, _ = run_each(ipa, on, ptrs, out, px3, "packed")
    got0, ran0, names0, _ = run_each(ipa, off, ptrs, out, px3, "packed")
    assert chunk_entries(ran1) and not [e for e in ran0 if "batch=1" in e] and not [s for s in names0 if s.startswith("batch")], (sorted(ran0), names0)
    for i in range(n):
        same(got0[i], got1[i], "frame %d without bit 10" % i)


def test_mixed_batch(ipa, orc):
    """joinable frames interleaved with cutting ones: a 23 x 16 frame, a window-8 geometry, a frame without the bit"""
    L = ipa.lib()
    out = OUT_U8
    cut16 = Spec(kind="RGGB", src="u16", w=204, h=150, maxwidth=23, mask=MASK)
    w8 = Spec(kind="RGGB", src="u16", w=211, h=157, crops=(2, 3, 4, 5), maxwidth=60, mask=MASK)
    nobit = variant(1, mask=ON | BATCH)
    fr = driver_frames(5)
    extra = [(s, Frames(s, 1, util.SEED + 47000 + 31 * i)) for i, s in enumerate((cut16, w8, nobit))]
    items = [fr[0], fr[1], extra[0], fr[2], fr[3], fr[4], extra[1], extra[1], fr[0], extra[2], fr[1], fr[2]]
    specs = [variant(0), variant(1), cut16, variant(2), variant(3), variant(4), w8, w8, variant(0), nobit, variant(1), variant(2)]
    descs = [desc_of(s, L, out, param_set(k)) for k, s in enumerate(specs)]
    ptrs = [f.ptrs[0] for _, f in items]
    sizes = [br.sizes(L, d)[2] * br.sizes(L, d)[3] * 3 for d in descs]
    assert br.sizes(L, descs[2])[:2] == (23, 16) and br.report(L, descs[6], 2, out) == (1, 64, 0)
    route, first = plan_of(L, descs, out)
    assert first == [0, 0, 2, 3, 3, 3, 6, 6, 8, 9, 10, 10] and route == [2, 2, 0, 2, 2, 2, 2, 2, 0, 0, 2, 2], (route, first)
    got, ran, names, _ = run_each(ipa, descs, ptrs, out, sizes, "reverse")
    for i in range(len(items)):
        same(got[i], run_single(ipa, descs[i], ptrs[i], out, sizes[i])[0], "mixed frame %d against ipk_pipeline_run" % i)
    for i in (1, 4, 11):
        same(got[i], oracle_of(orc, L, specs[i], items[i][1].host[0], out, param_set(i)), "mixed frame %d against the oracle" % i)
    # three runs with frame-table scaling launches; the window-8 run keeps the per-frame scaling launches under the old name
    assert names.count(S1E) == 3 and names.count(S1) == 1 and names.count(S2E[out]) == 4, names
    assert len(chunk_entries(ran)) == 1, sorted(ran)


def test_the_python_wrappers(ipa, orc):
    import torch
    L = ipa.lib()
    c = mosaic_case(ipa, orc, "u16")
    out = ipa.scaled_demosaic_batch_each(c.dev[:5], c.rec[:5], 23, 17)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    for i in range(5):
        same(got[i * 23 * 17 * 4: (i + 1) * 23 * 17 * 4], c.oracle[i], "scaled_demosaic_batch_each slice %d" % i)
    assert ipa.scaled_demosaic_batch_each([], [], 23, 17).numel() == 0
    fr = driver_frames(3)
    sets = [param_set(3 * i) for i in range(3)]
    pipes = []
    for i, (spec, f) in enumerate(fr):
        p = sets[i]
        img = ipa.RawImage(width=spec.w, height=spec.h, data=f.views[0], cfa=spec.cfa, crops=spec.crops, blacklevels=list(spec.levels[0]),
                           whitelevels=list(spec.levels[1]), wb_coeffs=p["wb"], cam_to_xyz_normalized=p["cam"])
        pipe = ipa.Pipeline.new_from_source(img)
        pipe.globals.settings.maxwidth = 23
        pipe.ops.basecurve.points = list(p["points"])
        pipe.ops.basecurve.exposure = p["exposure"]
        pipe.batch_sensor = True                                            # nothing without batch_previews
        assert pipe.desc().allow_fused & SENSOR == 0
        pipe.batch_previews = True
        assert pipe.desc().allow_fused & (BATCH | SENSOR) == BATCH | SENSOR
        pipes.append(pipe)
    assert ipa.batch_each_plan(pipes, OUT_U8) == [(2, 0)] * 3
    with ipa.launch_log() as ran:
        outs = ipa.run_batch_each(pipes, [f.views[0] for _, f in fr], OUT_U8)
        torch.cuda.synchronize()
    assert len(chunk_entries(ran)) == 1, sorted(ran)
    for i, (spec, f) in enumerate(fr):
        same(outs[i].cpu().numpy().ravel(), oracle_of(orc, L, spec, f.host[0], OUT_U8, sets[i]), "run_batch_each frame %d" % i)
