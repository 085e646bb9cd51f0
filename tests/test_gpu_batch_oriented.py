"""GPU parity of batches whose frames carry their own orientation (IPK_FUSED_BATCH_ORIENTED, allow_fused bit 9): ipk_pointwise_chain_out_batch_oriented --
the frame-table launch of k_pointwise_chain_small / k_raster_chain<Rgbe32, 1 | 2> in which a frame's record gathers through its own orientation (the launch
log's orient=1) -- and the two batch drivers on top of it.  Bar: bit-exact (f32 bit patterns, any NaN == any NaN; equal u8 / u16) -- the primitive against
ipk_pointwise_chain_out per frame followed by ipk_rotate_image_u8 / _u16 / ipk_rotate_buffer, the drivers against ipk_pipeline_run(descs[i]) and against
the CPU oracle's pipeline with THAT FRAME'S OWN settings and rotation / fliph / flipv.  Every frame has its own seed, parameters and orientation, so a
mixed-up frame, record or walk cannot pass; every destination lies between sentinels at an odd element offset.

The host predicate "tile or gather" of the header is constantly gather (the transposed tile walk was measured and deleted), so every oriented launch is
tagged orient=1 whatever the frame size; the sizes below are those at which a walk over rows and columns can go wrong, the tile sizes of the deleted walk
(32 x 8 output pixels) among them as ordinary sizes."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_batch_previews_route as br
import test_gpu_batch_previews as bp
import test_gpu_batch_each as eb
from test_batch_previews_route import ON, PLAIN_PREVIEWS, BATCH, OUT_F32, OUT_U8, OUT_U16
from test_gpu_batch_previews import NP_OUT, Spec, Frames, same
from test_gpu_batch_each import Slots, rgbe_frames, param_set, chain_params, single_chain, LINEAR, oracle_of, desc_of, run_each, run_single, plan_of
from test_batch_oriented_route import ORIENTED, ALL, ONE_OF_EACH, TRANSPOSING

pytestmark = pytest.mark.gpu

S1 = "batch gofloat+demosaic"
S2O = {OUT_F32: "batch-each to_lab+basecurve+from_lab+gamma+transform", OUT_U8: "batch-each to_lab+basecurve+from_lab+gamma+transform+quantise",
       OUT_U16: "batch-each to_lab+basecurve+from_lab+gamma+transform+quantise"}
S2U = {k: v.replace("batch-each ", "batch ") for k, v in S2O.items()}
KERNEL = {OUT_F32: r"ipk::k_pointwise_chain_small", OUT_U8: r"ipk::k_raster_chain<ipk::Rgbe32, 1>", OUT_U16: r"ipk::k_raster_chain<ipk::Rgbe32, 2>"}
ORIENT1 = {o: "^" + k + r"\[fast_ok=[01],batch=1,orient=1\]$" for o, k in KERNEL.items()}
PLAIN = {o: "^" + k + r"\[fast_ok=[01],batch=1\]$" for o, k in KERNEL.items()}


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def launch_tag(oris, out):
    """the tag of ONE launch over frames with these orientations: orient=1 exactly when one of its records gathers"""
    return (ORIENT1 if any(o not in (0, 8) for o in oris) else PLAIN)[out]


def rotated(ipa, flat, w, h, ori, out):
    """ipk_rotate_buffer / ipk_rotate_image_u8 / _u16 of a w x h x 3 host image -> (its samples, the rotated width, the rotated height)"""
    import torch
    L = ipa.lib()
    a = np.ascontiguousarray(flat)
    t = torch.from_numpy(a.view(np.int16) if a.dtype == np.uint16 else a).cuda()
    g = util.Guarded(w * h * 3, NP_OUT[out], off=3)
    ow, oh = C.c_size_t(0), C.c_size_t(0)
    fn = {OUT_F32: L.ipk_rotate_buffer, OUT_U8: L.ipk_rotate_image_u8, OUT_U16: L.ipk_rotate_image_u16}[out]
    assert fn(t.data_ptr(), w, h, ori, g.ptr, C.byref(ow), C.byref(oh), None) == 0, L.ipk_last_error()
    torch.cuda.synchronize()
    return g.result("rotated"), ow.value, oh.value


_WANT = {}


def wanted(ipa, key, src_ptr, w, h, p, linear, out, ori, mono=0):
    """the single form followed by the rotate entry point, computed once per (case, frame)"""
    if key not in _WANT:
        if mono:
            import torch
            L = ipa.lib()
            g = util.Guarded(w * h * 3, NP_OUT[out], off=3)
            cp = chain_params(ipa, p)
            assert L.ipk_pointwise_chain_out(src_ptr, w, h, 1, cp.wb_coeffs, cp.cam_to_xyz_normalized, cp.exposure, cp.points, cp.npoints, linear, out, g.ptr, None) == 0
            torch.cuda.synchronize()
            flat = g.result("single")
        else:
            flat = single_chain(ipa, src_ptr, w, h, p, linear, out)
        got, ow, oh = rotated(ipa, flat, w, h, ori, out)
        assert (ow, oh) == ((h, w) if ori in TRANSPOSING else (w, h))
        _WANT[key] = got
    return _WANT[key]


def check_oriented(ipa, w, h, oris, out, seed, mono=0, sets=None, pass_null=False, want_tag=None, e_frame=None):
    """n = len(oris) frames, frame i with param_set(sets[i]) and orientation oris[i], into reversed slots with gaps"""
    import torch
    from imagepipe_amd._lib import ChainParams
    L = ipa.lib()
    n, npix, linear = len(oris), w * h, LINEAR[out]
    host = rgbe_frames(n, npix, seed)
    if mono:
        host[:, :, 3] = 0.0
    if e_frame is not None:                                                 # non-zero E samples inside an oriented record: the literal form there
        assert oris[e_frame] not in (0, 8)
        host[n - 1, :, 3] = 0.0
        host[e_frame, ::5, 3] = util.uniform_f32(seed + 5, host[e_frame, ::5, 3].size, 0.125, 0.5)
    src = torch.from_numpy(host).cuda()
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * npix * 16 for i in range(n)])
    sets = list(range(n)) if sets is None else sets
    ps = [param_set(k) for k in sets]
    arr = (ChainParams * n)(*[chain_params(ipa, p) for p in ps])
    ori = None if pass_null else (C.c_int * n)(*oris)
    slots = Slots([npix * 3] * n, out, order=list(range(n))[::-1], gap=37)
    dp = (C.c_void_p * n)(*slots.ptrs)
    tag = "%dx%d, orientations %s, out %d, mono %d" % (w, h, "NULL" if pass_null else list(oris), out, mono)

    def call():
        assert L.ipk_pointwise_chain_out_batch_oriented(sp, w, h, mono, arr, ori, n, linear, out, dp, ipa._stream()) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    with ipa.launch_log() as ran:
        names = eb._stage_names(L, call)
    got = slots.results(tag)
    assert names == ["pointwise_chain_out_batch_oriented"] * -(-n // 64), (tag, names)
    hits = eb.carriers(ran)
    assert hits and sorted(ran) == hits, (tag, sorted(ran))
    # a launch is tagged by the strongest mode among ITS frames (64 per launch)
    want_tags = {launch_tag(oris[k: k + 64], out) for k in range(0, n, 64)} if want_tag is None else {want_tag}
    assert all(any(re.match(t, e) for t in want_tags) for e in hits) and all(any(re.match(t, e) for e in hits) for t in want_tags), (tag, hits)
    for i in range(n):
        want = wanted(ipa, (tag, seed, i), sp[i], w, h, ps[i], linear, out, 0 if pass_null else oris[i], mono)
        same(got[i], want, "%s: frame %d against the single form and the rotate entry point" % (tag, i))
    assert np.array_equal(src.cpu().numpy().view(np.uint32), host.view(np.uint32)), tag + ": the sources were written"
    return got, hits


# 16 x 16: the 256-pixel floor; 257 x 1 and 1 x 257: a transposed output one pixel wide, and a source one pixel wide; 23 x 17: the thumbnail; 8 x 32 and
# 9 x 33: one 256-pixel chunk whose transposed image is eight rows of 32, and a pixel more each way; 100 x 66: several blocks per frame, with tails on both axes
SIZES = [(16, 16), (257, 1), (1, 257), (23, 17), (8, 32), (9, 33), (100, 66)]


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
@pytest.mark.parametrize("w,h", SIZES)
def test_primitive_one_frame_per_orientation(ipa, w, h, out):
    """nine frames, orientation values 0 .. 8 (Unknown is Normal), each with its own seed and parameters; frame 5 has fast_ok = 0"""
    if (w, h) == (100, 66):
        assert eb.blocks_per_frame(ipa.lib(), w * h, out, 9) > 1
    _, hits = check_oriented(ipa, w, h, list(range(9)), out, util.SEED + 40000 + 13 * w + h)
    assert any("fast_ok=0" in e for e in hits) and all("orient=1" in e for e in hits), hits


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_primitive_without_orientations_is_the_plain_batch(ipa, out):
    """orientations == NULL and all-Normal (with an Unknown): exactly [fast_ok=,batch=1], and ipk_pointwise_chain_out_batch's results"""
    import torch
    from imagepipe_amd._lib import ChainParams
    L = ipa.lib()
    w, h, n, seed = 23, 17, 5, util.SEED + 41000
    a, _ = check_oriented(ipa, w, h, [0] * n, out, seed, pass_null=True, want_tag=PLAIN[out])
    b, _ = check_oriented(ipa, w, h, [0, 8, 0, 0, 8], out, seed, want_tag=PLAIN[out])
    src = torch.from_numpy(rgbe_frames(n, w * h, seed)).cuda()
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * w * h * 16 for i in range(n)])
    arr = (ChainParams * n)(*[chain_params(ipa, param_set(i)) for i in range(n)])
    slots = Slots([w * h * 3] * n, out, gap=3)
    assert L.ipk_pointwise_chain_out_batch(sp, w, h, 0, arr, n, LINEAR[out], out, (C.c_void_p * n)(*slots.ptrs), None) == 0, L.ipk_last_error()
    torch.cuda.synchronize()
    for i, want in enumerate(slots.results("plain batch")):
        same(a[i], want, "NULL orientations, frame %d" % i)
        same(b[i], want, "Normal orientations, frame %d" % i)


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8])
def test_primitive_crosses_the_launch(ipa, out):
    """65 frames: the second launch holds one frame, Rotate90"""
    oris = [(3 * i + 1) % 8 for i in range(65)]
    assert oris[64] == 1
    check_oriented(ipa, 23, 17, oris, out, util.SEED + 41500)
    # and one whose second launch is Normal: that launch keeps the plain tag
    check_oriented(ipa, 23, 17, [5] * 64 + [0], OUT_U8, util.SEED + 41600, sets=[i % 7 for i in range(65)])


def test_primitive_monochrome(ipa):
    check_oriented(ipa, 23, 17, [5, 0, 6, 1], OUT_U8, util.SEED + 42000, mono=1, sets=[2, 3, 4, 6])


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_primitive_e_samples_in_an_oriented_record(ipa, out):
    """frame 1 (Rotate270) holds non-zero E samples, frame 2 (Transpose) has fast_ok = 0"""
    for w, h in ((33, 9), (9, 33)):
        check_oriented(ipa, w, h, [0, 7, 4, 2], out, util.SEED + 42500 + w, sets=[0, 3, 5, 6], e_frame=1)


def test_primitive_refusals(ipa):
    """an orientation outside 0 .. 8 names its index; u8 under 256 pixels, null and misaligned pointers with an orientation array present: nothing is
    launched and nothing is written"""
    import torch
    from imagepipe_amd._lib import ChainParams
    L = ipa.lib()
    n = 3
    src = torch.from_numpy(rgbe_frames(n, 400, util.SEED + 43000)).cuda()
    sp = (C.c_void_p * n)(*[src.data_ptr() + i * 400 * 16 for i in range(n)])
    arr = (ChainParams * n)(*[chain_params(ipa, param_set(i)) for i in range(n)])
    err = lambda: L.ipk_last_error().decode()
    ok = (C.c_int * n)(5, 0, 7)
    f = L.ipk_pointwise_chain_out_batch_oriented
    for out in (OUT_U8, OUT_U16, OUT_F32):
        slots = Slots([400 * 3] * n, out, gap=4)
        dp = (C.c_void_p * n)(*slots.ptrs)
        with ipa.launch_log() as ran:
            assert f(sp, 20, 20, 0, arr, (C.c_int * n)(5, 0, 9), n, 0, out, dp, None) == -2 and "orientations[2]" in err(), err()
            assert f(sp, 20, 20, 0, arr, (C.c_int * n)(5, -1, 7), n, 0, out, dp, None) == -2 and "orientations[1]" in err(), err()
            if out != OUT_F32:
                assert f(sp, 15, 17, 0, arr, ok, n, 0, out, dp, None) == -5 and "256" in err(), err()
            assert f(sp, 20, 20, 0, arr, ok, 0, 0, out, dp, None) == 0
            assert f((C.c_void_p * n)(sp[0], None, sp[2]), 20, 20, 0, arr, ok, n, 0, out, dp, None) == -2 and "index 1" in err(), err()
            assert f(sp, 20, 20, 0, arr, ok, n, 0, out, (C.c_void_p * n)(dp[0], dp[1], None), None) == -2 and "index 2" in err(), err()
            assert f((C.c_void_p * n)(sp[0] + 4, sp[1], sp[2]), 20, 20, 0, arr, ok, n, 0, out, dp, None) == -2 and "frame 0" in err(), err()
            assert f(sp, 20, 20, 0, None, ok, n, 0, out, dp, None) == -2
            torch.cuda.synchronize()
        assert not ran, sorted(ran)
        for r in slots.results("refusals"):
            assert (r == np.array(util.SENTINELS[r.dtype.name]).astype(r.dtype)).all(), "a refused call wrote to a destination"


def test_the_python_wrapper_of_the_primitive(ipa):
    import torch
    w, h, oris = 23, 17, [5, 0, 2, 4]
    n = len(oris)
    host = rgbe_frames(n, w * h, util.SEED + 43500)
    src = torch.from_numpy(host).cuda()
    ps = [param_set(i) for i in range(n)]
    outs = ipa.pointwise_chain_out_batch([src[i] for i in range(n)], w, h, [chain_params(ipa, p) for p in ps], out_type=OUT_U16, linear=True, orientations=oris)
    torch.cuda.synchronize()
    assert [tuple(o.shape) for o in outs] == [(w, h, 3), (h, w, 3), (h, w, 3), (w, h, 3)] and outs[0].dtype == torch.int16
    for i in range(n):
        want = wanted(ipa, ("wrapper", i), src[i].data_ptr(), w, h, ps[i], 1, OUT_U16, oris[i])
        same(outs[i].cpu().numpy().view(np.uint16).ravel(), want, "wrapper frame %d" % i)


# ---------------------------------------------------------------------------------------------
# 2. the drivers
# ---------------------------------------------------------------------------------------------
def oriented_spec(name, triple, box, mask=None):
    """the frame kind `name` of tests/test_gpu_batch_each.py under a box x box size limit with this (rotation, fliph, flipv), bit 9 beside its own bits"""
    kw = dict(eb.KINDS[name])
    kw["maxwidth"] = box
    kw["mask"] = (kw.get("mask", ON | BATCH) | ORIENTED) if mask is None else mask
    return Spec(maxheight=box, rotation=triple[0], fliph=triple[1], flipv=triple[2], **kw)


def check_driver(ipa, orc, name, box, triples, out, layout, demosaic, oracle_frames=None):
    L = ipa.lib()
    n = len(triples)
    _, frames = eb.kind_frames(name, n)
    specs = [oriented_spec(name, t, box) for t in triples]
    ps = [param_set(i) for i in range(n)]
    descs = [desc_of(specs[i], L, out, ps[i]) for i in range(n)]
    oris = [L.ipk_transform_orientation(*t) for t in triples]
    sizes = [br.sizes(L, d) for d in descs]
    dw, dh = demosaic
    for o, s in zip(oris, sizes):
        assert s == ((dw, dh, dh, dw) if o in TRANSPOSING else (dw, dh, dw, dh)), (o, s)
    px3 = dw * dh * 3
    tag = "%s under %dx%d, orientations %s, out %d, %s" % (name, box, box, oris, out, layout)
    assert plan_of(L, descs, out) == ([2] * n, [0] * n), tag
    got, ran, names, used = run_each(ipa, descs, frames.ptrs[:n], out, [px3] * n, layout)
    singles = [run_single(ipa, descs[i], frames.ptrs[i], out, px3) for i in range(n)]
    for i in range(n):
        same(got[i], singles[i][0], "%s: frame %d against ipk_pipeline_run" % (tag, i))
    for i in (range(n) if oracle_frames is None else oracle_frames):
        want = oracle_of(orc, L, specs[i], frames.host[i], out, ps[i])
        assert want.shape == (sizes[i][3], sizes[i][2], 3), tag
        same(got[i], want, "%s: frame %d against the oracle with its own settings and orientation" % (tag, i))
    full, rest = divmod(n, 64)
    multi = full + (1 if rest > 1 else 0)
    chunk_oriented = [any(o != 0 for o in oris[k: k + 64]) for k in range(0, 64 * multi, 64)]
    chunk_tags = [launch_tag(oris[k: k + 64], out) for k in range(0, 64 * multi, 64)]
    want_names = []
    for x in chunk_oriented:
        want_names += [S1, S2O[out] if x else eb.S2E[out]]
    assert names[: 2 * multi] == want_names and names[2 * multi:] == (singles[n - 1][2] if rest == 1 else []), (tag, names)
    hits = eb.carriers(ran)
    # exactly one carrier launch per chunk (the log keeps each distinct entry once: one chunk, one entry)
    assert multi != 1 or len(hits) == 1, (tag, sorted(ran))
    assert all(any(re.match(t, e) for e in hits) for t in chunk_tags) and all(any(re.match(t, e) for t in chunk_tags) for e in hits), (tag, sorted(ran))
    assert used == singles[n - 1][3] == 0, tag
    assert not any("batch" in e for s in singles for e in s[1]), tag
    return descs, frames, got


@pytest.mark.parametrize("layout", ["packed", "reverse"])
@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_driver_eight_orientations(ipa, orc, out, layout):
    """RGGB u16 thumbnails under the 23 x 23 box: one scaling launch group, ONE oriented pass-2 launch"""
    check_driver(ipa, orc, "rggb-u16", 23, ONE_OF_EACH, out, layout, (23, 17))


@pytest.mark.parametrize("out", [OUT_F32, OUT_U8, OUT_U16])
def test_driver_a_larger_preview(ipa, orc, out):
    """the same source under a 48 x 48 box: 48 x 35, several chunks per frame and rows that do not divide them"""
    check_driver(ipa, orc, "rggb-u16", 48, ONE_OF_EACH, out, "reverse", (48, 35))


@pytest.mark.parametrize("name,out,demosaic", [("xtrans-u16", OUT_U16, (30, 24)), ("mono-u16", OUT_U8, None)])
def test_driver_frame_kinds(ipa, orc, name, out, demosaic):
    if demosaic is None:
        demosaic = br.sizes(ipa.lib(), oriented_spec(name, (0, 0, 0), 30).desc(ipa.lib(), out))[:2]
        assert oriented_spec(name, (0, 0, 0), 30).mask == ON | BATCH | PLAIN_PREVIEWS | ORIENTED
    check_driver(ipa, orc, name, 30, [ONE_OF_EACH[i] for i in (5, 0, 6, 1)], out, "reverse", demosaic)


def test_driver_crosses_the_launch(ipa, orc):
    """65 frames: a chunk of 64 and a chunk of one frame, which takes the single path"""
    triples = [ONE_OF_EACH[(3 * i + 5) % 8] for i in range(65)]
    check_driver(ipa, orc, "rggb-u16", 23, triples, OUT_U8, "reverse", (23, 17), oracle_frames=(0, 5, 63, 64))


@pytest.mark.parametrize("triple", [(1, 0, 0), (2, 0, 0)])
@pytest.mark.parametrize("out", [OUT_F32, OUT_U8])
def test_the_uniform_route(ipa, orc, triple, out):
    """ipk_pipeline_run_batch of three frames on ONE oriented descriptor: the chunk walk's pass 1, one oriented frame-table launch"""
    L = ipa.lib()
    n = 3
    _, frames = eb.kind_frames("rggb-u16", n)
    spec = oriented_spec("rggb-u16", triple, 23)
    p = param_set(3)
    d = desc_of(spec, L, out, p)
    assert br.report(L, d, n, out) == (1, 64, 1)
    px3 = 23 * 17 * 3
    got, ran, names, used = bp.run_batch(ipa, d, frames.ptrs[:n], out, px3, slots=[2, 0, 1])
    assert names == [S1, S2U[out]] and used == 0, names
    hits = eb.carriers(ran)
    assert len(hits) == 1 and re.match(ORIENT1[out], hits[0]), sorted(ran)
    for i, s in enumerate([2, 0, 1]):
        same(got[s], run_single(ipa, d, frames.ptrs[i], out, px3)[0], "uniform frame %d against ipk_pipeline_run" % i)
        same(got[s], oracle_of(orc, L, spec, frames.host[i], out, p), "uniform frame %d against the oracle" % i)
    # identical descriptors through the per-frame entry point are route 1: the same launches
    descs = [desc_of(spec, L, out, p) for _ in range(n)]
    assert plan_of(L, descs, out) == ([1] * n, [0] * n)
    got_e, ran_e, names_e, _ = run_each(ipa, descs, frames.ptrs[:n], out, [px3] * n, "packed")
    assert names_e == names and eb.carriers(ran_e) == hits
    for i, s in enumerate([2, 0, 1]):
        same(got_e[i], got[s], "route 1 frame %d" % i)
    # without bit 9 the descriptor is the parent's loop
    off = desc_of(oriented_spec("rggb-u16", triple, 23, mask=ON | BATCH), L, out, p)
    assert br.report(L, off, n, out) == (0, 0, 0)
    got0, ran0, names0, _ = bp.run_batch(ipa, off, frames.ptrs[:n], out, px3)
    assert not [e for e in ran0 if "batch=1" in e] and not [s for s in names0 if s.startswith("batch")], (sorted(ran0), names0)
    for i, s in enumerate([2, 0, 1]):
        same(got0[i], got[s], "frame %d without bit 9" % i)


def mixed_items(mask_bits):
    a = oriented_spec("rggb-u16", (0, 0, 0), 23, mask=ON | BATCH | mask_bits)
    portrait = oriented_spec("rggb-u16", (1, 0, 0), 23, mask=ON | BATCH | mask_bits)
    x = Spec(src="u16", mask=ON | BATCH | mask_bits, **bp.MOSAICS["xtrans"])
    _, fa = eb.kind_frames("rggb-u16", 8)
    _, fx = eb.kind_frames("xtrans-u16", 3)
    return [(a, fa, 0, 0), (x, fx, 0, 1), (a, fa, 1, 2), (portrait, fa, 2, 4), (a, fa, 3, 5), (x, fx, 1, 6), (portrait, fa, 4, 7), (portrait, fa, 5, 7)]


def test_a_mixed_shoot(ipa, orc):
    """two shapes interleaved and a portrait frame: with bit 9 on every descriptor the portrait frame sits inside its neighbours' run; without it the
    parent's plan, launches and names -- and the same bits"""
    L = ipa.lib()
    out = OUT_U8
    items = mixed_items(ORIENTED)
    descs = [desc_of(s, L, out, param_set(k)) for s, _, _, k in items]
    ptrs = [f.ptrs[i] for _, f, i, _ in items]
    sizes = [br.sizes(L, d)[2] * br.sizes(L, d)[3] * 3 for d in descs]
    assert br.sizes(L, descs[3]) == (23, 17, 17, 23)
    assert plan_of(L, descs, out) == ([0, 0, 2, 2, 2, 0, 1, 1], [0, 1, 2, 2, 2, 5, 6, 6])
    got, ran, names, _ = run_each(ipa, descs, ptrs, out, sizes, "reverse")
    for i, (s, f, j, k) in enumerate(items):
        same(got[i], run_single(ipa, descs[i], ptrs[i], out, sizes[i])[0], "mixed frame %d against ipk_pipeline_run" % i)
        if i in (2, 3, 4, 7):
            same(got[i], oracle_of(orc, L, s, f.host[j], out, param_set(k)), "mixed frame %d against the oracle" % i)
    # the varied run of three and the uniform run of two portraits: one oriented launch each, under their own names
    assert names.count(S2O[out]) == 1 and names.count(S2U[out]) == 1 and names.count(S1) == 2, names
    hits = eb.carriers(ran)                                                 # (frame 4's matrix makes the varied launch fast_ok=0, the portraits' is fast_ok=1)
    assert len(hits) == 2 and all(re.match(ORIENT1[out], e) for e in hits), sorted(ran)
    # without bit 9
    items0 = mixed_items(0)
    descs0 = [desc_of(s, L, out, param_set(k)) for s, _, _, k in items0]
    assert plan_of(L, descs0, out) == ([0, 0, 0, 0, 0, 0, 1, 1], [0, 1, 2, 3, 4, 5, 6, 6])
    got0, ran0, names0, _ = run_each(ipa, descs0, ptrs, out, sizes, "reverse")
    assert not [e for e in ran0 if "batch=1" in e] and not [s for s in names0 if s.startswith("batch")], (sorted(ran0), names0)
    assert names0 == [x for i in range(len(items0)) for x in run_single(ipa, descs0[i], ptrs[i], out, sizes[i])[2]]
    for i in range(len(items)):
        same(got0[i], got[i], "mixed frame %d without bit 9" % i)


def test_the_python_wrapper_of_the_driver(ipa, orc):
    import torch
    L = ipa.lib()
    spec, frames = eb.kind_frames("rggb-u16", 3)
    triples = [(0, 0, 0), (1, 0, 0), (2, 1, 0)]
    sets = [param_set(3 * i) for i in range(3)]                             # the defaults, the grid curve, the second matrix (RawImage wants a normal wb)
    pipes = []
    for i in range(3):
        p = sets[i]
        img = ipa.RawImage(width=spec.w, height=spec.h, data=frames.views[i], cfa="RGGB", crops=spec.crops, blacklevels=[util.BLACK] * 4,
                           whitelevels=[util.WHITE] * 4, wb_coeffs=p["wb"], cam_to_xyz_normalized=p["cam"])
        pipe = ipa.Pipeline.new_from_source(img)
        pipe.globals.settings.maxwidth = pipe.globals.settings.maxheight = 23
        pipe.ops.basecurve.points = list(p["points"])
        pipe.ops.basecurve.exposure = p["exposure"]
        pipe.ops.transform.rotation, pipe.ops.transform.fliph, pipe.ops.transform.flipv = triples[i][0], bool(triples[i][1]), bool(triples[i][2])
        pipe.batch_oriented = True                                          # nothing without batch_previews
        assert pipe.desc().allow_fused & ORIENTED == 0
        pipe.batch_previews = True
        assert pipe.desc().allow_fused & (BATCH | ORIENTED) == BATCH | ORIENTED
        pipes.append(pipe)
    assert ipa.batch_each_plan(pipes, OUT_U8) == [(2, 0)] * 3
    with ipa.launch_log() as ran:
        outs = ipa.run_batch_each(pipes, frames.views[:3], OUT_U8)
        torch.cuda.synchronize()
    hits = eb.carriers(ran)
    assert len(hits) == 1 and re.match(ORIENT1[OUT_U8], hits[0]), sorted(ran)
    assert [tuple(o.shape) for o in outs] == [(17, 23, 3), (23, 17, 3), (17, 23, 3)]
    for i in range(3):
        s = oriented_spec("rggb-u16", triples[i], 23)
        same(outs[i].cpu().numpy().ravel(), oracle_of(orc, L, s, frames.host[i], OUT_U8, sets[i]), "run_batch_each frame %d" % i)
