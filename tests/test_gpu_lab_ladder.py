"""The out-of-table step of the XYZ -> Lab lookup as pointwise4_fast runs it (imagepipe_amd/csrc/ipk_lab_slots.inc): a wave-row whose ratios all
lie in [+0, 2) -- one unsigned maximum of their bit patterns below 0x40000000 -- takes a lean body (compare, masked short cube root); every other
row takes the general ladder (ratios >= 2, negative ratios, -0, non-finite ones).

Two proofs on the device:
  * one slot on EVERY f32 bit pattern against the literal lab_lookup, with consecutive patterns side by side in a wave (the classes then meet only at
    1.0, 2.0, +inf and the sign bit) and again with one value of [+0, 2) and one from outside in neighbouring lanes, so that in every wave the lanes
    that alone would have gone lean sit beside one that pulls the row off the lean body;
  * frames built so that the class boundary falls INSIDE waves -- strips whose lanes are all above the table and below 2, with single lanes at a ratio
    of 2 or more and single negative ones -- each bit-identical to the CPU oracle.  The RGGB whole-frame, rotated, batch and window cases assert by the
    launch log that the kernel WITHOUT per-pixel guards ran: those are the instantiations that carry the lean body.  The X-Trans, staged-chain and
    ipk_tolab cases run guarded instantiations, which keep the general ladder alone: they pin that ladder on the same inputs.  The lone NaN / +inf / -inf
    samples of the f32 frames flag their rows, which the fused kernels then recompute literally: they test that hand-over, not the ladder; non-finite
    RATIOS are the selftest's and the chain cases' business.
"""
import ctypes as C

import numpy as np
import pytest

import util
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
CURVE3 = [(0.5, 0.6)]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


# =============================================================================================
# One slot on every f32 bit pattern
# =============================================================================================
CHUNK = 1 << 26                       # bit patterns per launch (three f32 buffers of 256 MiB)


def _slot(L, x, variant):
    """ipk_selftest_cbrtf variants 3 / 4 (the kernels' slot, without / with per-pixel guards) and 5 (lab_lookup) on a device tensor of f32"""
    import torch
    o = torch.empty_like(x)
    assert L.ipk_selftest_cbrtf(C.c_void_p(x.data_ptr()), C.c_void_p(o.data_ptr()), x.numel(), variant, None) == 0, L.ipk_last_error()
    return o


def _mismatches(got, want, x):
    """-> (count, first input's bits): bit equality, any NaN equal to any NaN (util.assert_bits_equal's rule)"""
    import torch
    bad = (got.view(torch.int32) != want.view(torch.int32)) & ~(torch.isnan(got) & torch.isnan(want))
    n = int(bad.sum().item())
    first = int(x.view(torch.int32)[bad][0].item()) & 0xFFFFFFFF if n else 0
    return n, first


def _patterns(start, n):
    import torch
    b = torch.arange(start, start + n, dtype=torch.int64, device="cuda")
    return torch.where(b >= (1 << 31), b - (1 << 32), b).to(torch.int32)


@pytest.mark.parametrize("variant", [3, 4], ids=["lean-or-ladder", "ladder-with-guards"])
def test_one_lab_slot_equals_lab_lookup_on_every_f32(ipa, orc, variant):
    """consecutive bit patterns in consecutive lanes: all 2^32"""
    import torch
    L = ipa.lib()
    total, first = 0, None
    for start in range(0, 1 << 32, CHUNK):
        x = _patterns(start, CHUNK).view(torch.float32)
        n, f = _mismatches(_slot(L, x, variant), _slot(L, x, 5), x)
        if n and first is None:
            first = f
        total += n
    print("variant %d, consecutive patterns: %d mismatches of 2^32" % (variant, total))
    assert total == 0, "%d mismatches, first v bits 0x%08x" % (total, first)
    # the literal form itself against the CPU oracle, on the special values and on a stride through every exponent
    xs = np.concatenate([util.SPECIALS, np.arange(0, 1 << 32, 65521, dtype=np.uint64).astype(np.uint32).view(np.float32)])
    xs = np.resize(xs, (xs.size + 255) // 256 * 256).astype(np.float32)
    with np.errstate(all="ignore"):
        want = orc.lookup(orc.LUT_XYZ_LAB, xs)
    for v in (variant, 5):
        assert_bits_equal(_slot(L, torch.from_numpy(xs).cuda(), v).cpu().numpy(), want, "slot variant %d vs the oracle's lookup" % v)


@pytest.mark.parametrize("variant", [3, 4], ids=["lean-or-ladder", "ladder-with-guards"])
def test_one_lab_slot_with_the_classes_interleaved_in_every_wave(ipa, variant):
    """even lanes: a value of [+0, 2) (bits below 0x40000000); odd lanes: one from outside (bits from 0x40000000 up: >= 2, non-finite, -0, negative).
    Every outside pattern appears once, the inside ones three times each: 3 * 2^31 lanes"""
    import torch
    L = ipa.lib()
    total, first = 0, None
    half = CHUNK // 2
    for j in range(0, 3 << 30, half):
        x = torch.empty(CHUNK, dtype=torch.int32, device="cuda")
        x[0::2] = _patterns(j % (1 << 30), half)
        x[1::2] = _patterns((1 << 30) + j, half)
        x = x.view(torch.float32)
        n, f = _mismatches(_slot(L, x, variant), _slot(L, x, 5), x)
        if n and first is None:
            first = f
        total += n
    print("variant %d, interleaved classes: %d mismatches of 3 * 2^31" % (variant, total))
    assert total == 0, "%d mismatches, first v bits 0x%08x" % (total, first)


# =============================================================================================
# Frames with the class boundary inside waves
# =============================================================================================
H, W = 240, 518                       # two full 256-pixel strips and a few columns over
KINDS = ["boundary", "ordinary", "out-of-class"]


def cam25():
    """SRGB_D65_43 with every row scaled by 2.5: a pixel at half the white level has its three ratios between 1.5 and 1.95, a saturated one at 2.5"""
    m = np.array([[0.4124564, 0.3575761, 0.1804375, 0.0],
                  [0.2126729, 0.7151522, 0.0721750, 0.0],
                  [0.0193339, 0.1191920, 0.9503041, 0.0]], dtype=np.float32)
    return (m * np.float32(2.5)).astype(np.float32)


def _levels(kind, seed, h, w):
    """normalised sample levels (0 = black, 1 = white) of a frame of the given kind, before the lone samples"""
    n = util.uniform_f32(seed, h * w, -0.01, 0.01).reshape(h, w)
    if kind == "out-of-class":
        return np.float32(1.2) + n                           # saturated everywhere: every ratio is 2.5
    lv = np.float32(0.5) + n                                 # r clips to 1, g = 0.5, b = 0.75: ratios 1.91, 1.56, 1.82 -- above the table, below 2
    lv[:, 300:420] = util.uniform_f32(seed + 1, h * 120, 0.0, 0.3).reshape(h, 120)   # and a band inside the table
    return lv


def mosaic(kind, src, seed, h=H, w=W):
    """sensor data for a frame of `kind`; `boundary` adds, to the ordinary frame, lone samples that leave [+0, 2): every third row one saturated sample
    (its bilinear footprint covers at most two lanes of three rows), one sample far below black (u16: a 3x3 patch of zeros), and for f32 sources one
    sample each at -0.0, NaN, +inf and -inf (the last three flag their rows for the literal form: see the module docstring)"""
    lv = _levels(kind, seed, h, w)
    data = np.float32(util.BLACK) + lv * np.float32(util.WHITE - util.BLACK)
    if kind == "boundary":
        for r in range(1, h - 1, 3):
            data[r, (37 * r + 11) % 290 + 2] = np.float32(util.WHITE) * np.float32(1.5)
        data[h // 2 + 1, 200] = np.float32(util.BLACK - 40.0 * (util.WHITE - util.BLACK)) if src == "f32" else 0.0
        if src != "f32":
            data[h // 2: h // 2 + 3, 199: 202] = 0.0
    if src != "f32":
        return np.clip(np.rint(data), 0, 65535).astype(np.uint16)
    if kind == "boundary":
        data[5, 70] = -0.0; data[11, 130] = np.nan; data[17, 190] = np.inf; data[23, 250] = -np.inf
    if kind == "out-of-class":
        data[:, 64:128] = np.float32(util.BLACK - 40.0 * (util.WHITE - util.BLACK))      # a coherent negative region
    return data.astype(np.float32)


def _upload(ipa, a):
    import torch
    a = np.ascontiguousarray(a)
    return ipa.upload_u16(a) if a.dtype == np.uint16 else torch.from_numpy(a.ravel()).cuda()


def _same(got, want, what):
    if want.dtype == np.float32:
        assert_bits_equal(got, want, what)
    else:
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d samples differ" % (what, int((got != want).sum()) if got.shape == want.shape else -1)


F32, U16 = "float", "unsigned short"


def _ran(ran, kernel):
    """the launch log holds `kernel`, with or without a [tag]"""
    import re
    assert [n for n in ran if re.search("^" + re.escape(kernel) + r"(\[|$)", n)], "%s did not run; launched: %s" % (kernel, sorted(ran))


def _pipeline(ipa, orc, data, cfa, linear, rotation=0):
    img = ipa.RawImage(width=data.shape[1], height=data.shape[0], data=_upload(ipa, data), cfa=cfa, is_float=data.dtype == np.float32,
                       blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=cam25())
    pipe = ipa.Pipeline.new_from_source(img)
    pipe.ops.basecurve.points = list(CURVE3)
    pipe.globals.settings.linear = bool(linear)
    pipe.ops.transform.rotation = rotation
    desc = orc.make_pipeline(data, cfa=cfa, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                             cam_to_xyz_normalized=cam25(), points=list(CURVE3), linear=bool(linear), rotation=rotation)
    return pipe, desc


def _oracle_out(orc, desc, out):
    with np.errstate(all="ignore"):
        return [orc.pipeline_run, orc.pipeline_output_8bit, orc.pipeline_output_16bit][out](desc)


def _run(ipa, pipe, out):
    import torch
    if out == 0:
        got = pipe.run().numpy()
    elif out == 1:
        w, h, t = pipe.output_8bit(); got = t.cpu().numpy().reshape(h, w, 3)
    else:
        w, h, t = pipe.output_16bit(); got = t.cpu().numpy().view(np.uint16).reshape(h, w, 3)
    torch.cuda.synchronize()
    return got


# (name, source, output, filter, rotation)
ROUTES = [("f32-to-f32", "f32", 0, "RGGB", 0), ("u16-to-u8", "u16", 1, "RGGB", 0), ("u16-to-u16", "u16", 2, "RGGB", 0),
          ("f32-rot180", "f32", 0, "RGGB", 2), ("xtrans-f32", "f32", 0, XT, 0), ("xtrans-u16-to-u8", "u16", 1, XT, 0)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("route", ROUTES, ids=[r[0] for r in ROUTES])
def test_whole_frame(ipa, orc, route, kind):
    name, src, out, cfa, rotation = route
    data = mosaic(kind, src, util.SEED + 12000 + 17 * KINDS.index(kind) + out)
    pipe, desc = _pipeline(ipa, orc, data, cfa, linear=out == 2, rotation=rotation)
    with ipa.launch_log() as ran:
        got = _run(ipa, pipe, out)
    assert pipe.last_used_fused
    _same(got, _oracle_out(orc, desc, out), "%s, %s frame" % (name, kind))
    if cfa == "RGGB":                                        # the common-parameter kernel without guards: <SrcT, VEC, OUT, FULL, GEN = false, PXG = false, CM = 1, ROT>
        _ran(ran, "ipk::k_fused_bayer<%s, %s, %d, true, false, false, 1, %s>" % (F32 if src == "f32" else U16, "true" if src == "f32" else "false", out,
                                                                                 "true" if rotation else "false"))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,out", [("f32", 0), ("u16", 1), ("u16", 2)], ids=["f32-to-f32", "u16-to-u8", "u16-to-u16"])
def test_batch_launch(ipa, orc, src, out, kind):
    import torch
    frames = [mosaic(kind, src, util.SEED + 12100 + 5 * k + out) for k in range(3)]
    plan = ipa.FusedPlan(width=W, height=H, owidth=W, x=0, y=0, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa="RGGB",
                         wb_coeffs=util.WB, cam_to_xyz_normalized=cam25(), points=CURVE3, linear=out == 2, out_type=out)
    srcs = [_upload(ipa, d) for d in frames]
    outs = [plan.new_output() for _ in frames]
    with ipa.launch_log() as ran:
        ipa.FusedBatchPlan(plan, srcs, outs).run()
        torch.cuda.synchronize()
    _ran(ran, "ipk::k_fused_bayer_batch<%s, %s, %d, false>" % (F32 if src == "f32" else U16, "true" if src == "f32" else "false", out))
    for k, (d, o) in enumerate(zip(frames, outs)):
        desc = orc.make_pipeline(d, cfa="RGGB", blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                                 cam_to_xyz_normalized=cam25(), points=CURVE3, linear=out == 2)
        got = o.cpu().numpy()
        _same((got.view(np.uint16) if out == 2 else got).reshape(H, W, 3), _oracle_out(orc, desc, out), "batch frame %d, %s" % (k, kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("src,out,cfa", [("f32", 0, "RGGB"), ("u16", 1, "RGGB"), ("u16", 2, "RGGB"), ("f32", 0, XT)],
                         ids=["f32-to-f32", "u16-to-u8", "u16-to-u16", "xtrans-f32"])
def test_window(ipa, orc, src, out, cfa, kind):
    """ipk_pipeline_run_region on a window that starts off a strip boundary"""
    import torch
    data = mosaic(kind, src, util.SEED + 12200 + 3 * KINDS.index(kind) + out)
    pipe, desc = _pipeline(ipa, orc, data, cfa, linear=out == 2)
    x, y, rw, rh = 9, 3, 500, 201
    with ipa.launch_log() as ran:
        t = pipe.run_region(x, y, rw, rh, out_type=out)
        torch.cuda.synchronize()
    assert pipe.last_region_windowed
    if cfa == "RGGB":
        _ran(ran, "ipk::k_fused_bayer_window<%s, %s, %d, true, false, false, 1>" % (F32 if src == "f32" else U16, "true" if src == "f32" else "false", out))
    got = t.cpu().numpy()
    got = (got.view(np.uint16) if out == 2 else got).reshape(rh, rw, 3)
    _same(got, _oracle_out(orc, desc, out)[y: y + rh, x: x + rw], "window, %s frame" % kind)


def _fa(v):
    v = [float(x) for x in np.asarray(v, np.float32).ravel()]
    return (C.c_float * len(v))(*v)


def chain_pixels(kind, seed, npix):
    """RGBE pixels for the staged chain, where a pixel IS a lane's input: `boundary` puts, into strips whose ratios all lie in (1, 2), single pixels
    at a ratio of 2.5, single negative ones and one each at -0.0 (all three ratios -0), NaN, +inf and -inf"""
    lv = _levels(kind, seed, 1, npix).ravel()
    px = np.zeros((npix, 4), np.float32)
    px[:, 0] = np.minimum(lv * np.float32(2.0), np.float32(1.2)) / np.float32(2.0); px[:, 1] = lv; px[:, 2] = lv    # times WB (2, 1, 1.5): r = 1, g = 0.5, b = 0.75
    if kind == "out-of-class":
        px[64:128, :3] = -3.0
    if kind == "boundary":
        for i in range(100, npix - 8, 769):                  # 769 = 3 * 256 + 1: one lane of every third wave-row, at a lane that moves
            px[i, :3] = 1.5
        for i in range(300, npix - 8, 2311):
            px[i, :3] = -3.0
        for i, s in zip(range(1000, npix - 8, 1283), [-0.0, np.nan, np.inf, -np.inf, 0.0, 1.0, 2.0]):
            px[i, :3] = s
    return np.ascontiguousarray(px).reshape(1, npix, 4)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("out", [0, 1, 2], ids=["f32", "u8", "u16"])
def test_staged_chain(ipa, orc, out, kind):
    """ipk_pointwise_chain_out: k_pointwise_chain_small / k_raster_chain<Rgbe32, OUT>"""
    import torch
    npix = 256 * 96 + 5
    buf = chain_pixels(kind, util.SEED + 12300 + out, npix)
    dst = torch.full((npix * 3,), 0, dtype=[torch.float32, torch.uint8, torch.int16][out], device="cuda")
    src = _upload(ipa, buf)
    pts = [c for p in CURVE3 for c in p]
    rc = ipa.lib().ipk_pointwise_chain_out(src.data_ptr(), npix, 1, 0, _fa(util.WB), _fa(cam25()), 0.0, _fa(pts), len(CURVE3), 0, out, dst.data_ptr(), None)
    assert rc == 0, ipa.lib().ipk_last_error()
    torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = orc.gamma(orc.fromlab(orc.basecurve(orc.tolab(buf, util.WB, cam25()), 0.0, CURVE3)), False)
    want = want if out == 0 else (orc.output8bit(want) if out == 1 else orc.output16bit(want))
    got = dst.cpu().numpy()
    _same((got.view(np.uint16) if out == 2 else got).reshape(1, npix, 3), want, "staged chain, %s pixels" % kind)


def test_tolab_stage(ipa, orc):
    """ipk_tolab -> k_pointwise_chain<true>: the step alone, handing back Lab"""
    import torch
    npix = 256 * 64
    for kind in KINDS:
        buf = chain_pixels(kind, util.SEED + 12400, npix)
        dst = torch.zeros(npix * 3, dtype=torch.float32, device="cuda")
        src = _upload(ipa, buf)
        assert ipa.lib().ipk_tolab(src.data_ptr(), npix, 1, 0, _fa(util.WB), _fa(cam25()), dst.data_ptr(), None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
        with np.errstate(all="ignore"):
            want = orc.tolab(buf, util.WB, cam25())
        assert_bits_equal(dst.cpu().numpy().reshape(1, npix, 3), want, "ipk_tolab, %s pixels" % kind)
