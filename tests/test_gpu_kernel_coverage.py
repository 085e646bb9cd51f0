"""One table keyed by KERNEL: every kernel variant the library compiles is run by a case that was built for it, and the case says so.

Each case derives its inputs from the host predicate that selects the variant (quoted beside the case), runs through the public surface, and asserts
two things: parity with the CPU oracle (bit-exact f32, equal u8 / u16) and that the kernel it names -- a regex over the launch log's
`ipk::<kernel><template arguments>[tag]` entries (imagepipe_amd.launch_log, ipk_selftest_launch_log) -- was launched by that call.  The closing test
lists the kernels of the built library (the extraction of tests/test_kernel_resources.py) and fails when one of them was named by no case.

The predicates live in imagepipe_amd/csrc/ipk_kernels.hip (launch_fused_t, launch_fused_window_t, launch_fused_bayer, launch_raw_scaled_demosaic,
launch_gofloat_cfa, launch_rotate*, launch_pointwise_chain) and ipk_api.cpp (fused_impl: px_guard / fast_ok / exact_norm; ipk_tolab)."""
import ctypes as C
import re

import numpy as np
import pytest

import util
from util import Guarded, assert_bits_equal

pytestmark = pytest.mark.gpu

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
F32, U16 = "float", "unsigned short"
OUTS = [0, 1, 2]                                   # IPK_OUT_F32, IPK_OUT_U8, IPK_OUT_U16
SOURCES = ["f32", "u16a", "u16odd"]                # f32; u16 on a dword boundary with an even pitch; u16 starting one sample off it (odd x, odd pitch)

ALL_CASES = []                                     # ids of every case of the table (filled at collection)
RAN_CASES = set()                                  # ids that ran to the end of their log check
NAMED = set()                                      # launch-log entries some case asked for by name and found


def _cases(prefix, params, ids):
    ids = ["%s-%s" % (prefix, i) for i in ids]
    ALL_CASES.extend(ids)
    return pytest.mark.parametrize("case", [pytest.param((i, p), id=i) for i, p in zip(ids, params)])


def _named(ran, pattern, case_id=None):
    """the case's second assertion: a launched kernel matches `pattern`"""
    hits = [n for n in ran if re.search(pattern, n)]
    assert hits, "no launched kernel matches %r; launched: %s" % (pattern, sorted(ran))
    NAMED.update(hits)
    if case_id is not None:
        RAN_CASES.add(case_id)


def _exact(name):
    return "^" + re.escape(name) + r"(\[|$)"


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _b(v):
    return "true" if v else "false"


def _upload(ipa, a):
    import torch
    a = np.ascontiguousarray(a)
    return ipa.upload_u16(a) if a.dtype == np.uint16 else torch.from_numpy(a.ravel()).cuda()


def _fa(v):
    v = [float(x) for x in np.asarray(v, np.float32).ravel()]
    return (C.c_float * len(v))(*v)


def _same(got, want, what):
    if want.dtype == np.float32:
        assert_bits_equal(got, want, what)
    else:
        assert got.shape == want.shape and np.array_equal(got, want), "%s: %d samples differ" % (what, int((got != want).sum()) if got.shape == want.shape else -1)


# =============================================================================================
# The fused raw -> sRGB families: a product of axes
# =============================================================================================
CURVE3 = [(0.5, 0.6)]                                                      # three knots with the end points: the compiled-in 3-knot form (CM = 1)
CURVE_GRID = [(0.2, 0.1), (0.4, 0.5), (0.6, 0.55), (0.8, 0.9)]             # six knots, one per grid cell at most: spline_grid_ok (CM = 2)


def _cam(guard):
    cm = util.cam_matrix()
    if guard:
        # fused_impl: `plain = plain && (c == 0.0f || (c >= 0x1p-12f && c <= 0x1p20f))` over the matrix -> px_guard = 1, while
        # `sane(v) = fabs(v) <= 0x1p20f` keeps fast_ok = 1: the common-curve variants WITH per-pixel guards
        cm[2, 0] = np.float32(2.0 ** -13)
    return cm


def _mosaic(kind, h, w, seed):
    """-> (sensor data, crops): u16odd carries one extra column on the left that the crop removes, so the frame's first sample sits 2 bytes off a dword
    boundary on an odd pitch; f32 frames hold util.SPECIALS scaled to the white level and lone non-finite samples"""
    left = 1 if kind == "u16odd" else 0
    raw = util.noise_u16(seed, h, w + left)
    if kind != "f32":
        return raw, (0, 0, 0, left)
    data = raw.astype(np.float32) + util.uniform_f32(seed + 1, raw.size, -0.5, 0.5).reshape(raw.shape)
    with np.errstate(over="ignore"):
        sp = util.SPECIALS * np.float32(16383.0)
    if w >= sp.size + 4:
        data[3, 2: 2 + sp.size] = sp
    else:
        data.ravel()[w + 1: w + 1 + sp.size] = sp
    data[h // 2, w // 2] = -np.inf; data[h - 2, 3] = np.nan; data[1, w - 2] = np.inf      # each alone in an ordinary neighbourhood
    return data, (0, 0, 0, 0)


def _pipeline(ipa, orc, data, crops, cfa, guard, points, linear, rotation=0):
    import torch
    h, w = data.shape
    dev = _upload(ipa, data)
    img = ipa.RawImage(width=w, height=h, data=dev, cfa=cfa, crops=crops, is_float=data.dtype == np.float32, blacklevels=[util.BLACK] * 4,
                       whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=_cam(guard))
    pipe = ipa.Pipeline.new_from_source(img)
    pipe.ops.basecurve.points = list(points)
    pipe.globals.settings.linear = bool(linear)
    pipe.ops.transform.rotation = rotation
    desc = lambda: orc.make_pipeline(data, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), crops=crops, blacklevels=[util.BLACK] * 4,
                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=_cam(guard), points=list(points),
                                     linear=bool(linear), rotation=rotation)
    return pipe, desc


def _pipe_out(ipa, pipe, out):
    import torch
    with ipa.launch_log() as ran:
        if out == 0:
            got = pipe.run().numpy()
        elif out == 1:
            w, h, t = pipe.output_8bit(); got = t.cpu().numpy().reshape(h, w, 3)
        else:
            w, h, t = pipe.output_16bit(); got = t.cpu().numpy().view(np.uint16).reshape(h, w, 3)
        torch.cuda.synchronize()
    return got, ran


def _oracle_out(orc, desc, out):
    return [orc.pipeline_run, orc.pipeline_output_8bit, orc.pipeline_output_16bit][out](desc())


# leaf -> (generic CFA, curve, px_guard wanted, full strips (W >= 256), rotation)
FUSED_LEAVES = {
    "common":        (False, CURVE3, False, True, 0),
    "common-guard":  (False, CURVE3, True, True, 0),
    "grid":          (False, CURVE_GRID, False, True, 0),
    "grid-guard":    (False, CURVE_GRID, True, True, 0),
    "plain":         (False, [], False, True, 0),
    "plain-guard":   (False, [], True, True, 0),
    "narrow":        (False, [], False, False, 0),
    "gen-common":    (True, CURVE3, False, True, 0),
    "gen-plain":     (True, [], False, True, 0),
    "gen-narrow":    (True, [], False, False, 0),
    "rot90":         (False, CURVE3, False, True, 1),
    "rot180-guard":  (False, CURVE3, True, True, 2),
    "gen-rot90":     (True, CURVE3, False, True, 1),
}


def fused_kernel(src, out, leaf):
    """launch_fused_t<SrcT, VEC, OUT>, restated: the k_fused_bayer<SrcT, VEC, OUT, FULL, GEN, PXG, CM, ROT> it picks for the leaf"""
    gen, curve, guard, full, rotation = FUSED_LEAVES[leaf]
    S = F32 if src == "f32" else U16
    v4 = S == F32                                       # `sizeof(SrcT) == 4`: the variants with one load flavour per source type
    vec = src != "u16odd"                               # launch_fused_bayer: `vec = f.src_is_u16 ? f.src_aligned4 : true`
    cm = 1 if curve is CURVE3 else (2 if curve is CURVE_GRID else 0)
    if rotation:                                        # `if (a.ori != 0)`: gen_cells -> <.., true, true, true, 1, true>, else PXG = px_guard
        t = (v4, out, True, True, True, 1, True) if gen else (v4, out, True, False, guard, 1, True)
    elif gen:                                           # `if (a.gen_cells)`: common / W >= 256 / narrow
        t = (v4, out, True, True, True, 1, False) if cm == 1 else (v4, out, full, True, True, 0, False)
    elif S == U16 and not guard and full:               # `if (a.px_guard == 0 && a.W >= 256u)`: common / common_grid / else, all <u16, false, ..>
        t = (False, out, True, False, False, cm, False)
    elif cm and full:                                   # `if (common_grid)` / `if (common)`: f32 without guards, or PXG = true
        t = (v4, out, True, False, guard, cm, False)
    else:                                               # `a.W >= 256u ? <SrcT, VEC, OUT, true, false> : <SrcT, VEC, OUT, false, false>` (PXG = true, CM = 0)
        t = (vec, out, full, False, True, 0, False)
    return "ipk::k_fused_bayer<%s, %s, %d, %s, %s, %s, %d, %s>" % (S, _b(t[0]), t[1], _b(t[2]), _b(t[3]), _b(t[4]), t[5], _b(t[6]))


_FUSED = [(s, o, l) for l in FUSED_LEAVES for s in SOURCES for o in OUTS]


@_cases("fused", _FUSED, ["%s-out%d-%s" % c for c in _FUSED])
def test_fused_whole_frame_variants(ipa, orc, case):
    """Pipeline.run / output_8bit / output_16bit on a frame whose parameters select exactly one leaf of launch_fused_t.
    common: fast_ok && has_curve && 3 knots && !exact_norm && (linear != 0) == (OUT == 2) && W >= 256 && 2^-70 <= |black| <= 2^70."""
    cid, (src, out, leaf) = case
    gen, curve, guard, full, rotation = FUSED_LEAVES[leaf]
    w, h = (262, 20) if full else (70, 20)
    if rotation == 1:
        w, h = 24, 262                                  # fused_impl: `(t ? p->height : p->width) < 256` has no rotated-space variant
    data, crops = _mosaic(src, h, w, util.SEED + 9000 + len(cid) * 7 + out)
    linear = bool(curve) and out == 2                   # `(a.linear != 0) == (OUT == 2)`
    pipe, desc = _pipeline(ipa, orc, data, crops, XT if gen else "RGGB", guard, curve, linear, rotation)
    got, ran = _pipe_out(ipa, pipe, out)
    assert pipe.last_used_fused
    _same(got, _oracle_out(orc, desc, out), cid)
    if rotation:
        # launch_rotate1: `(y_step == 1 || y_step == -1) && x_step != 1 && x_step != -1` (the transposing orientations) or the row form
        _named(ran, _exact("ipk::k_rotate1_%s<%s>" % ("transposed" if rotation == 1 else "rows", F32 if src == "f32" else U16)))
    _named(ran, _exact(fused_kernel(src, out, leaf)), cid)


# leaf -> (generic CFA, curve, px_guard wanted, window of 256 columns or more)
WINDOW_LEAVES = {
    "common":       (False, CURVE3, False, True),
    "common-guard": (False, CURVE3, True, True),
    "plain":        (False, [], False, True),
    "narrow":       (False, CURVE3, False, False),
    "gen-common":   (True, CURVE3, False, True),
    "gen-plain":    (True, [], False, True),
    "gen-narrow":   (True, CURVE3, False, False),
}
_WINDOW = [(s, o, l) for l in WINDOW_LEAVES for s in SOURCES for o in OUTS]


@_cases("window", _WINDOW, ["%s-out%d-%s" % c for c in _WINDOW])
def test_fused_region_variants(ipa, orc, case):
    """Pipeline.run_region: launch_fused_window_t<SrcT, OUT> -> k_fused_bayer_window<SrcT, V, OUT, FL, G, P, C>.
    `full = w.x1 - w.x0 >= 256u`; `common = full && fast_ok && has_curve && !exact_norm && (linear != 0) == (OUT == 2) && ... npoints == 3`;
    gen_cells: common / full / narrow; else common && px_guard == 0 / common / full / narrow."""
    import torch
    cid, (src, out, leaf) = case
    gen, curve, guard, full = WINDOW_LEAVES[leaf]
    w, h = 300, 24
    x, y, rw, rh = (9, 3, 277, 17) if full else (5, 2, 50, 19)
    data, crops = _mosaic(src, h, w, util.SEED + 9500 + len(cid) * 5 + out)
    linear = bool(curve) and out == 2
    pipe, desc = _pipeline(ipa, orc, data, crops, XT if gen else "RGGB", guard, curve, linear)
    with ipa.launch_log() as ran:
        t = pipe.run_region(x, y, rw, rh, out_type=out)
        torch.cuda.synchronize()
    assert pipe.last_region_windowed
    got = t.cpu().numpy()
    got = (got.view(np.uint16) if out == 2 else got).reshape(rh, rw, 3)
    _same(got, _oracle_out(orc, desc, out)[y: y + rh, x: x + rw], cid)
    common = full and bool(curve)
    if gen:
        t5 = (full, True, True, 1 if common else 0)
    elif common:
        t5 = (True, False, guard, 1)
    else:
        t5 = (full, False, True, 0)
    S = F32 if src == "f32" else U16
    _named(ran, _exact("ipk::k_fused_bayer_window<%s, %s, %d, %s, %s, %s, %d>" % (S, _b(S == F32), out, _b(t5[0]), _b(t5[1]), _b(t5[2]), t5[3])), cid)


_BATCH = [(s, o) for s in SOURCES for o in OUTS]


@_cases("batch", _BATCH, ["%s-out%d" % c for c in _BATCH])
def test_fused_batch_variants(ipa, orc, case):
    """FusedBatchPlan: `batchable = common && a.ori == 0 && !a.gen_cells && a.px_guard == 0 && f.batch_n > 1` -> k_fused_bayer_batch<T, V, O, false>"""
    import torch
    cid, (src, out) = case
    w, h = 262, 16
    frames = [_mosaic(src, h, w, util.SEED + 9800 + 3 * k + out) for k in range(3)]
    left = frames[0][1][3]
    cfa = orc.cfa_shift("RGGB", left, 0)
    plan = ipa.FusedPlan(width=w, height=h, owidth=w + left, x=left, y=0, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa=cfa,
                         wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), points=CURVE3, linear=out == 2, out_type=out)
    srcs = [_upload(ipa, d) for d, _ in frames]
    outs = [plan.new_output() for _ in frames]
    with ipa.launch_log() as ran:
        ipa.FusedBatchPlan(plan, srcs, outs).run()
        torch.cuda.synchronize()
    for (d, crops), o in zip(frames, outs):
        desc = lambda: orc.make_pipeline(d, cfa=cfa, crops=crops, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                                         cam_to_xyz_normalized=util.cam_matrix(), points=CURVE3, linear=out == 2)
        got = o.cpu().numpy()
        _same((got.view(np.uint16) if out == 2 else got).reshape(h, w, 3), _oracle_out(orc, desc, out), cid)
    S = F32 if src == "f32" else U16
    _named(ran, _exact("ipk::k_fused_bayer_batch<%s, %s, %d, false>" % (S, _b(S == F32), out)), cid)


_RESAMPLE = [(s, o, hostile) for s in ("f32", "u16a") for o in OUTS for hostile in ("", "matrix", "curve")]
STEEP = [(0.5, 0.1), (float(np.nextafter(np.float32(0.5), np.float32(1.0))), 0.9)]    # neighbouring knots: c2, c3 beyond 2^40 -> fast_ok = 0


def _hostile(kind):
    """-> (matrix, curve points): PointwisePrep / fused_impl `sane(v) = fabs(v) <= 0x1p20f` over the matrix, `fabs(c2), fabs(c3) <= 0x1p40f` over the curve"""
    cm = util.cam_matrix()
    if kind == "matrix":
        cm[1, 1] = np.float32(2.0 ** 21)
    return cm, (STEEP if kind == "curve" else CURVE3)


@_cases("resample", _RESAMPLE, ["%s-out%d-%s" % (s, o, k or "ordinary") for s, o, k in _RESAMPLE])
def test_fused_resample_variants(ipa, orc, case):
    """raw_to_srgb_resampled -> k_fused_resample<T, O>, with ordinary parameters and with fast_ok = 0 through an absurd matrix and a curve whose
    coefficients exceed 2^40 (the launcher's tag)"""
    from test_gpu_rotatecrop_fused import _gpu_op, _oracle_ops
    cid, (src, out, kind) = case
    h, w = 61, 47
    data, _ = _mosaic(src, h, w, util.SEED + 9900 + out)
    corners = orc.rotatecrop_corners((0.02, 0.03, 0.01, 0.02, 0.2), w, h)
    assert corners is not None
    cm, points = _hostile(kind)
    args = (data, (0, 0, 0, 0), "GRBG", util.BLACK, util.WHITE, corners, util.WB, cm, 0.0, points, out == 2, ["f32", "u8", "u16"][out])
    with ipa.launch_log() as ran:
        got = _gpu_op(ipa, orc, *args)
    _same(got, _oracle_ops(orc, *args), cid)
    _named(ran, _exact("ipk::k_fused_resample<%s, %d>" % (F32 if src == "f32" else U16, out)) + r"fast_ok=%d\]" % (0 if kind else 1), cid)


_GENHOSTILE = [(s, k) for s in ("f32", "u16a") for k in ("matrix", "curve")]


@_cases("fused-hostile", _GENHOSTILE, ["%s-%s" % c for c in _GENHOSTILE])
def test_fused_generic_cfa_with_absurd_parameters(ipa, orc, case):
    """fast_ok = 0 in a generic-CFA frame: every pixel takes the literal form inside k_fused_bayer<.., true, true, true, 0, false>"""
    cid, (src, kind) = case
    data, crops = _mosaic(src, 20, 262, util.SEED + 9950)
    cm, points = _hostile(kind)
    import torch
    img = ipa.RawImage(width=262, height=20, data=_upload(ipa, data), cfa=XT, is_float=src == "f32", blacklevels=[util.BLACK] * 4,
                       whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=cm)
    pipe = ipa.Pipeline.new_from_source(img)
    pipe.ops.basecurve.points = list(points)
    got, ran = _pipe_out(ipa, pipe, 0)
    assert pipe.last_used_fused
    want = orc.pipeline_run(orc.make_pipeline(data, cfa=XT, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                                              cam_to_xyz_normalized=cm, points=list(points)))
    _same(got, want, cid)
    S = F32 if src == "f32" else U16
    _named(ran, _exact("ipk::k_fused_bayer<%s, %s, 0, true, true, true, 0, false>" % (S, _b(S == F32))), cid)


# =============================================================================================
# Staged demosaic (OUT == 3 of the row-walking kernel), the four-colour kernel, and the stream probe (OUT == 4)
# =============================================================================================
_DEMOSAIC = [("RGGB", 262, "ipk::k_fused_bayer<float, true, 3, true, false, true, 0, false>"),
             ("GBRG", 70, "ipk::k_fused_bayer<float, true, 3, false, false, true, 0, false>"),
             (XT, 262, "ipk::k_fused_bayer<float, true, 3, true, true, true, 0, false>"),
             (XT, 70, "ipk::k_fused_bayer<float, true, 3, false, true, true, 0, false>"),
             ("RGBE", 70, "ipk::k_demosaic_full")]


@_cases("demosaic", _DEMOSAIC, ["%s-%d" % (c[0][:4], c[1]) for c in _DEMOSAIC])
def test_staged_demosaic_variants(ipa, orc, case):
    """ipk_demosaic_full: Bayer phase / any other three-colour filter -> launch_demosaic_bayer (`a.W >= 256u` picks FULL), a fourth colour -> k_demosaic_full"""
    import torch
    cid, (cfa, w, kernel) = case
    h = 18
    buf = util.uniform_f32(util.SEED + 9100 + w, h * w, -0.05, 1.0).reshape(h, w)
    buf.ravel()[w + 1: w + 1 + util.SPECIALS.size] = util.SPECIALS
    buf[h // 2, w // 2] = np.nan; buf[h - 2, 2] = -np.inf
    dst = Guarded(h * w * 4, torch.float32)
    src = _upload(ipa, buf)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_demosaic_full(src.data_ptr(), w, h, cfa.encode(), dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(h, w, 4), orc.demosaic_full(cfa, buf), cid)
    _named(ran, _exact(kernel), cid)


@_cases("probe", ["f32", "u16a"], ["f32", "u16a"])
def test_stream_probe_variants(ipa, orc, case):
    """FusedPlan.probe (ipk_stream_probe): `f.out_type == 4` -> k_fused_bayer<T, sizeof(T) == 4, 4, true, false, false, 1>; the demosaiced R, G, B"""
    import torch
    cid, src = case
    w, h = 262, 20
    data, _ = _mosaic("u16a", h, w, util.SEED + 9200)
    if src == "f32":
        data = data.astype(np.float32) + np.float32(0.25)
    plan = ipa.FusedPlan(width=w, height=h, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa="BGGR", wb_coeffs=util.WB,
                         cam_to_xyz_normalized=util.cam_matrix())
    out = torch.full((h * w * 3,), -7.0, dtype=torch.float32, device="cuda")
    dev = _upload(ipa, data)
    with ipa.launch_log() as ran:
        plan.probe(dev, out)
        torch.cuda.synchronize()
    want = orc.demosaic_full("BGGR", orc.gofloat_cfa(data, 0, 0, w, h, util.BLACK, util.WHITE))[:, :, :3]
    _same(out.cpu().numpy().reshape(h, w, 3), np.ascontiguousarray(want), cid)
    S = F32 if src == "f32" else U16
    _named(ran, _exact("ipk::k_fused_bayer<%s, %s, 4, true, false, false, 1, false>" % (S, _b(S == F32))), cid)


# =============================================================================================
# OpGoFloat
# =============================================================================================
# (source type, pitch, x, width, height, bytes the source pointer sits off a dword boundary, kernel[tag])
_GOFLOAT = [
    # launch_gofloat_cfa: `(w & 3) == 0 && (dst & 3) == 0 && (src & 3) == 0`, then u16: `(owidth & 1) == 0 && (x & 1) == 0` -> the 8-byte load
    ("u16", 64, 4, 52, 21, 0, r"ipk::k_gofloat_cfa_v4<unsigned short, true>\[rowwrap=0\]"),
    ("u16", 64, 5, 52, 21, 0, r"ipk::k_gofloat_cfa_v4<unsigned short, false>\[rowwrap=0\]"),      # odd x: the 2-byte-aligned load (GfU4s)
    ("u16", 63, 4, 52, 21, 0, r"ipk::k_gofloat_cfa_v4<unsigned short, false>\[rowwrap=0\]"),      # odd pitch
    ("u16", 64, 4, 53, 21, 0, r"ipk::k_gofloat_cfa<unsigned short>$"),                             # w % 4 != 0
    ("u16", 64, 4, 52, 21, 2, r"ipk::k_gofloat_cfa<unsigned short>$"),                             # source 2 bytes off a dword boundary
    ("u16", 16, 2, 8, 4101, 0, r"ipk::k_gofloat_cfa_v4<unsigned short, true>\[rowwrap=1\]"),       # h > 4096: the grid's rows wrap
    ("u16", 15, 3, 8, 4101, 0, r"ipk::k_gofloat_cfa_v4<unsigned short, false>\[rowwrap=1\]"),
    ("f32", 64, 5, 52, 21, 0, r"ipk::k_gofloat_cfa_v4<float, true>\[rowwrap=0\]"),                 # f32 has one load form: x and pitch parity do not matter
    ("f32", 64, 4, 53, 21, 0, r"ipk::k_gofloat_cfa<float>$"),
    ("f32", 13, 3, 8, 4101, 0, r"ipk::k_gofloat_cfa_v4<float, true>\[rowwrap=1\]"),
]


@_cases("gofloat", _GOFLOAT, ["%s-p%d-x%d-w%d-h%d-o%d" % c[:6] for c in _GOFLOAT])
def test_gofloat_cfa_variants(ipa, orc, case):
    import torch
    cid, (src, pitch, x, w, h, off, kernel) = case
    y, oh = 2, h + 3
    raw = util.noise_u16(util.SEED + 9300 + pitch + x + w, oh, pitch, maxval=17000)
    if src == "f32":
        raw = raw.astype(np.float32) + util.uniform_f32(util.SEED + 9301, raw.size, -0.5, 0.5).reshape(raw.shape)
        with np.errstate(over="ignore"):
            sp = util.SPECIALS * np.float32(16383.0)
        raw.ravel()[y * pitch: y * pitch + sp.size] = sp
        raw[y + h - 1, x + 1] = np.nan; raw[y + 3, x + w - 1] = -np.inf
    flat = np.ascontiguousarray(raw).ravel()
    big = torch.zeros(flat.size + 8, dtype=torch.int16 if src == "u16" else torch.float32, device="cuda")
    sh = off // 2 if src == "u16" else 0
    big[sh: sh + flat.size] = _upload(ipa, flat)
    dst = Guarded(w * h, torch.float32)
    fn = ipa.lib().ipk_gofloat_cfa_u16 if src == "u16" else ipa.lib().ipk_gofloat_cfa_f32
    with ipa.launch_log() as ran:
        assert fn(big.data_ptr() + off, pitch, x, y, w, h, util.BLACK, util.WHITE, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(h, w), orc.gofloat_cfa(raw, x, y, w, h, util.BLACK, util.WHITE), cid)
    _named(ran, kernel, cid)


@_cases("gofloat-other", ["mono-u16", "mono-f32", "rgb-u16", "rgb-f32", "raster-u8", "raster-u16"], ["mono-u16", "mono-f32", "rgb-u16", "rgb-f32", "raster-u8", "raster-u16"])
def test_gofloat_mono_rgb_raster(ipa, orc, case):
    """OpGoFloat.run on monochrome, three-sample and raster sources: k_gofloat_mono<T>, k_gofloat_rgb<T>, k_gofloat_other_u8 / _u16"""
    import torch
    cid, kind = case
    h, w = 23, 29
    g = ipa.PipelineGlobals(None)
    bl, wl = [64.0, 70.0, 80.0, 0.0], [4000.0, 3900.0, 4095.0, 0.0]
    if kind.startswith("mono"):
        raw = util.noise_u16(util.SEED + 9400, h, w, 4095)
        raw = raw if kind.endswith("u16") else raw.astype(np.float32) + np.float32(0.25)
        img = ipa.RawImage(w, h, _upload(ipa, raw), cfa="", blacklevels=[64.0] * 4, whitelevels=[4000.0] * 4, is_float=kind.endswith("f32"))
        want, kernel = orc.gofloat_mono(raw, 0, 0, w, h, 64.0, 4000.0), "ipk::k_gofloat_mono<%s>" % (U16 if kind.endswith("u16") else F32)
    elif kind.startswith("rgb"):
        raw = util.noise_u16(util.SEED + 9401, h, w * 3, 4095).reshape(h, w, 3)
        raw = raw if kind.endswith("u16") else raw.astype(np.float32) + np.float32(0.25)
        img = ipa.RawImage(w, h, _upload(ipa, raw), cpp=3, cfa="", blacklevels=bl, whitelevels=wl, is_float=kind.endswith("f32"))
        want, kernel = orc.gofloat_rgb(raw, 0, 0, w, h, bl, wl), "ipk::k_gofloat_rgb<%s>" % (U16 if kind.endswith("u16") else F32)
    else:
        bits = 8 if kind.endswith("u8") else 16
        raw = (util.splitmix64(util.SEED + 9402, h * w * 3) & np.uint64((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16).reshape(h, w, 3)
        img = ipa.OtherImage(w, h, _upload(ipa, raw), bits=bits)
        want, kernel = orc.gofloat_other(raw, 0, 0, w, h), "ipk::k_gofloat_other_u%d" % bits
    g.image = img
    with ipa.launch_log() as ran:
        got = ipa.OpGoFloat(img).run(g).numpy()
    _same(got, want, cid)
    _named(ran, _exact(kernel), cid)


# =============================================================================================
# ipk_raw_scaled_demosaic: every kernel it selects, and the switches inside them
# =============================================================================================
def _rsd(ipa, orc, cid, src, cfa, w, h, nw, nh, black, white, kernel, dst_off=0, x=3, y=1):
    import torch
    oh, ow = h + y + 2, w + x + 3
    raw = util.noise_u16(util.SEED + 9600 + w * h + nw, oh, ow)
    if src == "f32":
        raw = raw.astype(np.float32) + util.uniform_f32(util.SEED + 9601, oh * ow).reshape(oh, ow)
        with np.errstate(over="ignore"):
            sp = util.SPECIALS * np.float32(16383.0)
        raw[y + 2, x: x + min(w, sp.size)] = sp[: min(w, sp.size)]
        raw[y + h // 2, x + w // 2] = -np.inf; raw[y + h - 2, x + 1] = np.nan
    dev = _upload(ipa, raw)
    dst = Guarded(nh * nw * 4, torch.float32, off=dst_off)
    with ipa.launch_log() as ran:
        rc = ipa.lib().ipk_raw_scaled_demosaic(dev.data_ptr(), 1 if src == "f32" else 0, ow, x, y, w, h, black, white, cfa.encode(), nw, nh, dst.ptr, None)
        assert rc == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = orc.scaled_demosaic(cfa, orc.gofloat_cfa(raw, x, y, w, h, black, white), nw, nh)
    _same(dst.result().reshape(nh, nw, 4), want, cid)
    _named(ran, kernel, cid)


W16x12 = "16x12:" + "".join("RGB"[(3 * r + c * c + r * c) % 3] for r in range(12) for c in range(16))     # 192 cells > kW8MaxCells: no LDS cell table
# (cfa, w, h, nw, nh, kernel): launch_raw_scaled_demosaic -- `1 <= skip <= 7 on both axes && width >= 8 && dst 16-byte aligned` -> the window-8 kernels;
# `pw * ph <= kW8MaxCells && 48 % pw == 0 && 48 % ph == 0` -> w8m<T, 5 | 3 | 2, fourth colour> by `skip_x_x >= 4` / `>= 2`; else the general kernel
_RSD_SHAPES = [
    (XT, 150, 100, 100, 40, r"w8m<%s, 2u, false>"), (XT, 150, 100, 50, 40, r"w8m<%s, 3u, false>"), (XT, 150, 100, 30, 40, r"w8m<%s, 5u, false>"),
    ("RGBE", 150, 100, 100, 40, r"w8m<%s, 2u, true>"), ("RGBE", 150, 100, 50, 40, r"w8m<%s, 3u, true>"), ("RGBE", 150, 100, 30, 40, r"w8m<%s, 5u, true>"),
    (W16x12, 150, 100, 50, 40, r"w8<%s>"), ("RGGB", 150, 100, 15, 40, r"<%s>"), ("RGGB", 7, 30, 3, 10, r"<%s>"),
]
_RSD = [(s,) + c for s in ("f32", "u16") for c in _RSD_SHAPES]


@_cases("rsd", _RSD, ["%s-%s-%dx%d-%dx%d" % (c[0], c[1][:5], c[2], c[3], c[4], c[5]) for c in _RSD])
def test_raw_scaled_demosaic_kernels(ipa, orc, case):
    cid, (src, cfa, w, h, nw, nh, kernel) = case
    _rsd(ipa, orc, cid, src, cfa, w, h, nw, nh, util.BLACK, util.WHITE, r"^ipk::k_raw_scaled_demosaic_?" + kernel % (F32 if src == "f32" else U16) + r"\[")


# levels: validate_cdiv_for_range rejects a range outside [2^-60, 2^60] (tiny), zero (empty) and negative (inverted) -> norm_fast = 0;
# `norm_light = 2^-70 <= |black| <= 2^70`
_RSD_LEVELS = {"ordinary": (util.BLACK, util.WHITE, 1, 1), "zero-black": (0.0, util.WHITE, 1, 0), "tiny": (0.0, 2.0 ** -70, 0, 0),
               "empty": (512.0, 512.0, 0, 1), "inverted": (512.0, 100.0, 0, 1)}
# output rows: `grid2.y >= 8 * group` (32 block rows) turns the XCD row grouping of the w8m kernels on; rows past a multiple of 32 are its leftovers
_RSD_SWITCH = [(s, k, lv, nh) for s in ("f32", "u16") for k in range(8) for lv in _RSD_LEVELS for nh in (31, 32, 41)]


@_cases("rsd-switch", _RSD_SWITCH, ["%s-%s-%d-%s-rows%d" % (s, _RSD_SHAPES[k][0][:5], _RSD_SHAPES[k][3], lv, nh) for s, k, lv, nh in _RSD_SWITCH])
def test_raw_scaled_demosaic_switches(ipa, orc, case):
    """Every kernel ipk_raw_scaled_demosaic selects -- the six w8m shapes, w8 and the general kernel, per source type -- under norm_fast 0 / 1 and
    norm_light 0 / 1 (all five level sets), at 31, 32 and 41 output rows: for the w8m kernels no XCD grouping, grouping, grouping with leftover
    rows; each asserted by the launcher's tag.
    fast_x / fast_y (cdiv_host_ok of the scale) are met on one side only.  A host scan of the scales (w - 1) / (nw - 1) in [1, 7] for w <= 330
    (46 550 divisors through cdiv_mantissa_exhaustive_ok, run once while this module was written, not part of the suite) found none that the check
    rejects; none is known outside that range either.  The cases therefore assert fast_x = fast_y = 1, and the true-division side of these
    kernels' window weights has no case."""
    cid, (src, k, lv, nh) = case
    cfa, w, h, nw, _nh, kernel = _RSD_SHAPES[k]
    black, white, norm_fast, norm_light = _RSD_LEVELS[lv]
    xcd = (0 if nh < 32 else (1 if nh == 32 else 2)) if kernel.startswith("w8m") else 0
    fast_x = 1 if (w - 1) / (nw - 1) <= 7 else r"\d"      # beyond the window-8 kernels' scales the general kernel runs; its divisor was not scanned
    tag = r"\[norm_fast=%d,norm_light=%d,fast_x=%s,fast_y=1,xcd=%d\]" % (norm_fast, norm_light, fast_x, xcd)
    _rsd(ipa, orc, cid, src, cfa, w, h, nw, nh, black, white, r"^ipk::k_raw_scaled_demosaic_?" + kernel % (F32 if src == "f32" else U16) + tag)


@_cases("rsd-unaligned", ["f32", "u16"], ["f32", "u16"])
def test_raw_scaled_demosaic_unaligned_destination(ipa, orc, case):
    """`(reinterpret_cast<uintptr_t>(dst4) & 15) == 0` fails: the general kernel"""
    cid, src = case
    _rsd(ipa, orc, cid, src, XT, 150, 100, 50, 40, util.BLACK, util.WHITE, r"^ipk::k_raw_scaled_demosaic<%s>\[" % (F32 if src == "f32" else U16), dst_off=1)


# =============================================================================================
# Scaling kernels of the staged path
# =============================================================================================
@_cases("transform", ["f32", "u8", "u16"], ["f32", "u8", "u16"])
def test_transform_buffer_variants(ipa, orc, case):
    """ipk_transform_buffer_f32 / _u8 / _u16 -> k_transform_buffer<T>"""
    import torch
    cid, kind = case
    h, w, nh, nw = 40, 52, 17, 23
    if kind == "f32":
        src = util.uniform_f32(util.SEED + 9700, h * w * 3, -0.1, 1.1).reshape(h, w, 3)
        src.ravel()[: util.SPECIALS.size] = util.SPECIALS
        dt = torch.float32
    else:
        bits = 8 if kind == "u8" else 16
        src = (util.splitmix64(util.SEED + 9701, h * w * 3) & np.uint64((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16).reshape(h, w, 3)
        dt = torch.uint8 if bits == 8 else torch.int16
    tl, tr, bl = (2, 1), (w - 3, 4), (5, h - 2)
    dst = Guarded(nh * nw * 3, dt)
    dev = _upload(ipa, src)
    fn = getattr(ipa.lib(), "ipk_transform_buffer_" + kind)
    with ipa.launch_log() as ran:
        assert fn(dev.data_ptr(), w, h, tl[0], tl[1], tr[0], tr[1], bl[0], bl[1], nw, nh, 3, None, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(nh, nw, 3), orc.transform_buffer(src, w, h, tl, tr, bl, nw, nh, 3), cid)
    _named(ran, _exact("ipk::k_transform_buffer<%s>" % {"f32": F32, "u8": "unsigned char", "u16": U16}[kind]), cid)


@_cases("raster-scale", [8, 16], ["u8", "u16"])
def test_raster_scale_down_variants(ipa, orc, case):
    """ipk_raster_scale_down -> k_raster_scale_down<uint8_t / uint16_t>"""
    import torch
    cid, bits = case
    h, w, nh, nw, cx, cy = 57, 83, 19, 29, 3, 2
    oh, ow = h + cy + 1, w + cx + 2
    img = (util.splitmix64(util.SEED + 9710 + bits, oh * ow * 3) & np.uint64((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16).reshape(oh, ow, 3)
    dst = Guarded(nh * nw * 4, torch.float32)
    dev = _upload(ipa, img)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_raster_scale_down(dev.data_ptr(), 2 if bits == 8 else 3, ow, cx, cy, w, h, nw, nh, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(nh, nw, 4), orc.scale_down_opbuf(orc.gofloat_other(img, cx, cy, w, h), nw, nh), cid)
    _named(ran, _exact("ipk::k_raster_scale_down<%s>" % ("unsigned char" if bits == 8 else U16)), cid)


# =============================================================================================
# Point-wise stages
# =============================================================================================
def _rgbe(n, seed):
    v = util.uniform_f32(seed, n * 4, -0.1, 1.3).reshape(-1, 4)
    v[:, 3] = 0.0
    k = util.SPECIALS.size
    if n >= 3 * k:
        v[:k, 0] = util.SPECIALS; v[k:2 * k, 1] = util.SPECIALS; v[2 * k:3 * k, 2] = util.SPECIALS
        v[5, 3] = 0.7; v[6, 3] = np.nan
    return v


_P20 = float(2.0 ** 20)
_TOLAB = [
    # ipk_tolab: `ok = every |mul|, |cm| <= 0x1p20f; if (ok && width * height >= 256)` the fast form, else the literal k_tolab
    ("255px", 255, None, "ipk::k_tolab"), ("256px", 256, None, "ipk::k_pointwise_chain<true>"),
    ("2^20", 4096, _P20, "ipk::k_pointwise_chain<true>"), ("above-2^20", 4096, float(np.nextafter(np.float32(_P20), np.float32(np.inf))), "ipk::k_tolab"),
    ("inf", 4096, float("inf"), "ipk::k_tolab"), ("nan", 4096, float("nan"), "ipk::k_tolab"),
    # launch_tolab: `grid_1d(npix, 1024, num_cus * 2)` -- past 2048 pixels per CU the literal kernel's grid is capped and its stride loop turns
    ("large-grid-literal", None, float("inf"), "ipk::k_tolab"), ("large-grid-fast", None, None, "ipk::k_pointwise_chain<true>"),
]


@_cases("tolab", _TOLAB, [c[0] for c in _TOLAB])
def test_tolab_variants(ipa, orc, case):
    import torch
    cid, (_, npix, entry, kernel) = case
    if npix is None:
        npix = ipa.lib().ipk_device_cus() * 2 * 1024 + 1024 + 37
    buf = np.ascontiguousarray(_rgbe(npix, util.SEED + 9720)).reshape(1, npix, 4)
    cm = util.cam_matrix()
    if entry is not None:
        cm[0, 1] = np.float32(entry)
    src = _upload(ipa, buf)
    dst = Guarded(npix * 3, torch.float32)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_tolab(src.data_ptr(), npix, 1, 0, _fa(util.WB), _fa(cm), dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    with np.errstate(all="ignore"):
        want = orc.tolab(buf, util.WB, cm)
    _same(dst.result().reshape(1, npix, 3), want, cid)
    _named(ran, _exact(kernel), cid)


@_cases("curve-fromlab", ["basecurve", "fromlab"], ["basecurve", "fromlab"])
def test_basecurve_and_fromlab(ipa, orc, case):
    import torch
    cid, which = case
    n = 64 * 96 + 5
    buf = util.uniform_f32(util.SEED + 9730, n * 3, -0.2, 1.2).reshape(1, n, 3)
    buf.reshape(-1, 3)[: util.SPECIALS.size, 0] = util.SPECIALS
    src = _upload(ipa, buf)
    dst = Guarded(n * 3, torch.float32)
    L = ipa.lib()
    with ipa.launch_log() as ran:
        if which == "basecurve":
            assert L.ipk_basecurve(src.data_ptr(), n, 1, 0.3, _fa([0.2, 0.1, 0.7, 0.9]), 2, dst.ptr, None) == 0, L.ipk_last_error()
        else:
            assert L.ipk_fromlab(src.data_ptr(), n, 1, dst.ptr, None) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    want = orc.basecurve(buf, 0.3, [(0.2, 0.1), (0.7, 0.9)]) if which == "basecurve" else orc.fromlab(buf)
    _same(dst.result().reshape(1, n, 3), want, cid)
    _named(ran, _exact("ipk::k_" + which), cid)


def _samples(n, seed):
    v = util.uniform_f32(seed, n, -0.2, 1.2)
    k = min(n, util.SPECIALS.size)
    v[:k] = util.SPECIALS[:k]
    return v


# (samples, source offset in elements, destination offset in elements): both at element alignment only, inside a larger allocation
_ALIGN = [(n, so, do) for n in (3, 4096, 4097, 4098, 4099) for so, do in ((0, 0), (1, 0), (0, 1), (3, 2))]


@_cases("gamma", _ALIGN, ["n%d-s%d-d%d" % c for c in _ALIGN])
def test_gamma_alignment_forms(ipa, orc, case):
    """k_gamma: `n4 = ((src | dst) & 15) == 0 ? n / 4 : 0` -- 16-byte groups plus a tail, or sample by sample"""
    import torch
    cid, (n, so, do) = case
    v = _samples(n, util.SEED + 9740 + n)
    big = torch.zeros(n + 8, dtype=torch.float32, device="cuda"); big[so: so + n] = _upload(ipa, v)
    dst = Guarded(n, torch.float32, off=do)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_gamma(big.data_ptr() + 4 * so, n, 1, 1, 0, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(1, n, 1), orc.gamma(v.reshape(1, n, 1)), cid)
    _named(ran, r"^ipk::k_gamma\[vec4=%d,wrap=0\]" % (1 if so % 4 == 0 and do % 4 == 0 else 0), cid)


@_cases("gamma-wrap", [0, 1], ["aligned", "offset"])
def test_gamma_past_the_grid_cap(ipa, orc, case):
    """launch_gamma: `grid_1d((n / 4 + 3) / 4, 1024, num_cus * 16)` -- past 16 blocks per CU the grid is capped and every block's stride loop turns"""
    import torch
    cid, so = case
    stride = ipa.lib().ipk_device_cus() * 16 * 1024 * 16                             # samples one turn of the capped grid covers
    n = stride + 16 * 1024 * 3 + 7
    period = 1000003                                                                 # the input's period must not divide the stride: a second turn that
    assert stride % period != 0                                                      # read one stride early, or did not advance, then gives other bits
    v = np.resize(_samples(period, util.SEED + 9750), n)
    big = torch.zeros(n + 8, dtype=torch.float32, device="cuda"); big[so: so + n] = torch.from_numpy(v).cuda()
    dst = Guarded(n, torch.float32)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_gamma(big.data_ptr() + 4 * so, n, 1, 1, 0, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    want = np.resize(orc.gamma(v[:period].reshape(1, -1, 1)).ravel(), n)             # the input repeats with that period: so does the result
    got = dst.result()
    del big, dst
    _same(got, want, cid)
    _named(ran, r"^ipk::k_gamma\[vec4=%d,wrap=1\]" % (0 if so else 1), cid)


@_cases("output8", _ALIGN, ["n%d-s%d-d%d" % c for c in _ALIGN])
def test_output8_alignment_forms(ipa, orc, case):
    """k_output8: `n4 = ((src & 15) | (dst & 3)) == 0 ? n / 4 : 0`.  Its grid is flat (flat_cap = 2^31 - 1 blocks of 1024 samples): no sample count a
    test can hold reaches the cap, so the stride loop's second turn has no case"""
    import torch
    cid, (n, so, do) = case
    v = _samples(n, util.SEED + 9760 + n)
    big = torch.zeros(n + 8, dtype=torch.float32, device="cuda"); big[so: so + n] = _upload(ipa, v)
    dst = Guarded(n, torch.uint8, off=do)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_output8bit(big.data_ptr() + 4 * so, n, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result(), orc.output8bit(v), cid)
    _named(ran, r"^ipk::k_output8\[vec4=%d\]" % (1 if so % 4 == 0 and do % 4 == 0 else 0), cid)


@_cases("output16", _ALIGN, ["n%d-s%d-d%d" % c for c in _ALIGN])
def test_output16_alignment_forms(ipa, orc, case):
    """k_output16: `n4 = ((src & 15) | (dst & 7)) == 0 ? n / 4 : 0` (flat grid, as k_output8)"""
    import torch
    cid, (n, so, do) = case
    v = _samples(n, util.SEED + 9770 + n)
    big = torch.zeros(n + 8, dtype=torch.float32, device="cuda"); big[so: so + n] = _upload(ipa, v)
    dst = Guarded(n, torch.int16, off=do)
    with ipa.launch_log() as ran:
        assert ipa.lib().ipk_output16bit(big.data_ptr() + 4 * so, n, dst.ptr, None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result(), orc.output16bit(v), cid)
    _named(ran, r"^ipk::k_output16\[vec4=%d\]" % (1 if so % 4 == 0 and do % 4 == 0 else 0), cid)


def _chain_want(orc, buf, cm, points, linear, out):
    with np.errstate(all="ignore"):
        want = orc.gamma(orc.fromlab(orc.basecurve(orc.tolab(buf, util.WB, cm), 0.0, points)), linear)
    return want if out == 0 else (orc.output8bit(want) if out == 1 else orc.output16bit(want))


_CHAIN = [(o, k) for o in OUTS for k in ("", "matrix", "curve")]


@_cases("chain", _CHAIN, ["out%d-%s" % (o, k or "ordinary") for o, k in _CHAIN])
def test_pointwise_chain_variants(ipa, orc, case):
    """ipk_pointwise_chain / _out on a frame under the long-chunk threshold: k_pointwise_chain_small (f32), k_raster_chain<Rgbe32, 1 | 2>; fast_ok = 0
    through an absurd matrix and through a curve whose coefficients exceed 2^40"""
    import torch
    cid, (out, kind) = case
    npix = 64 * 96 + 3
    buf = np.ascontiguousarray(_rgbe(npix, util.SEED + 9780)).reshape(1, npix, 4)
    cm, points = _hostile(kind)
    pts = [c for p in points for c in p]
    src = _upload(ipa, buf)
    dst = Guarded(npix * 3, [torch.float32, torch.uint8, torch.int16][out])
    with ipa.launch_log() as ran:
        rc = ipa.lib().ipk_pointwise_chain_out(src.data_ptr(), npix, 1, 0, _fa(util.WB), _fa(cm), 0.0, _fa(pts), len(points), 0, out, dst.ptr, None)
        assert rc == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(1, npix, 3), _chain_want(orc, buf, cm, points, False, out), cid)
    kernel = "ipk::k_pointwise_chain_small" if out == 0 else "ipk::k_raster_chain<ipk::Rgbe32, %d>" % out
    _named(ran, _exact(kernel) + r"fast_ok=%d\]" % (0 if kind else 1), cid)


@_cases("chain-long", [""], ["ordinary"])
def test_pointwise_chain_long_chunk_form(ipa, orc, case):
    """launch_pointwise_chain: `npix < cus * 16 * 256 * 6` takes the two-pixel form; from there on k_pointwise_chain<false>"""
    import torch
    cid, _ = case
    npix = ipa.lib().ipk_device_cus() * 16 * 256 * 6 + 37
    period = 250007                                     # pixels; must not divide the 256 pixels x 16 waves x blocks one turn of the grid covers
    assert (ipa.lib().ipk_device_cus() * 16 * 256) % period != 0
    tile = _rgbe(period, util.SEED + 9790)
    buf = np.ascontiguousarray(np.resize(tile, (npix, 4))).reshape(1, npix, 4)
    src = _upload(ipa, buf)
    dst = Guarded(npix * 3, torch.float32)
    cm = util.cam_matrix()
    with ipa.launch_log() as ran:
        rc = ipa.lib().ipk_pointwise_chain(src.data_ptr(), npix, 1, 0, _fa(util.WB), _fa(cm), 0.0, _fa([0.5, 0.6]), 1, 0, dst.ptr, None)
        assert rc == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    want_tile = _chain_want(orc, tile.reshape(1, period, 4), cm, CURVE3, False, 0).reshape(period, 3)
    got = dst.result().reshape(npix, 3)
    del src, dst
    _same(got, np.resize(want_tile, (npix, 3)), cid)                                   # the input repeats with that period: so does the result
    _named(ran, r"^ipk::k_pointwise_chain<false>\[fast_ok=1\]", cid)


_RASTER = [(b, o, k) for b in (8, 16) for o in OUTS for k in ("", "matrix", "curve")]


@_cases("raster", _RASTER, ["u%d-out%d-%s" % (b, o, k or "ordinary") for b, o, k in _RASTER])
def test_raster_chain_variants(ipa, orc, case):
    """ipk_raster_to_srgb -> k_raster_chain<uint8_t | uint16_t, OUT>, ordinary and with fast_ok = 0"""
    import torch
    cid, (bits, out, kind) = case
    h, w = 7, 333
    img = (util.splitmix64(util.SEED + 9800 + bits, h * w * 3) & np.uint64((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16).reshape(h, w, 3)
    img.ravel()[:6] = [0, 1, (1 << bits) - 1, 2, (1 << bits) - 2, 128]
    cm, points = _hostile(kind)
    pts = [c for p in points for c in p]
    src = _upload(ipa, img)
    dst = Guarded(h * w * 3, [torch.float32, torch.uint8, torch.int16][out])
    with ipa.launch_log() as ran:
        rc = ipa.lib().ipk_raster_to_srgb(src.data_ptr(), 2 if bits == 8 else 3, w, h, _fa(util.WB), _fa(cm), 0.0, _fa(pts), len(points), 0, out, dst.ptr, None)
        assert rc == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    _same(dst.result().reshape(h, w, 3), _chain_want(orc, orc.gofloat_other(img, 0, 0, w, h), cm, points, False, out), cid)
    _named(ran, _exact("ipk::k_raster_chain<%s, %d>" % ("unsigned char" if bits == 8 else U16, out)) + r"fast_ok=%d\]" % (0 if kind else 1), cid)


# =============================================================================================
# Channel-depth conversions of the raster fast path, and the permutations of the 3-channel result
# =============================================================================================
_CHAN = [(16, 2000), (16, 2001), (16, 1999), (8, 16), (8, 17), (8, 15)]      # (source bits, width) of an 11-row raster: 3 * 11 * width % 16 = 0, 1, 15


@_cases("chan", _CHAN, ["u%d-w%d" % c for c in _CHAN])
def test_fast_path_channel_conversions(ipa, orc, case):
    """output_8bit of an RGB16 raster / output_16bit of an RGB8 raster on the fast path: k_chan_16_to_8 over all 65 536 values, k_chan_8_to_16 over all
    256, whole 16-sample groups (`i0 + 16u <= n`) and the sample-by-sample tail"""
    import torch
    cid, (bits, w) = case
    h = 11                                              # the pipeline takes sources of 10 x 10 pixels or more
    n = w * h * 3
    assert n % 16 in (0, 1, 15) and n >= (1 << bits)
    vals = np.arange(n, dtype=np.uint64) % np.uint64(1 << bits)
    vals[1 << bits:] = util.splitmix64(util.SEED + 9810, n - (1 << bits)) & np.uint64((1 << bits) - 1)
    img = vals.astype(np.uint8 if bits == 8 else np.uint16).reshape(h, w, 3)
    pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(w, h, _upload(ipa, img), bits=bits))
    with ipa.launch_log() as ran:
        if bits == 16:
            ow, oh, t = pipe.output_8bit(); got = t.cpu().numpy().reshape(oh, ow, 3)
        else:
            ow, oh, t = pipe.output_16bit(); got = t.cpu().numpy().view(np.uint16).reshape(oh, ow, 3)
        torch.cuda.synchronize()
    desc = orc.make_pipeline(img, use_fastpath=True)
    _same(got, orc.pipeline_output_8bit(desc) if bits == 16 else orc.pipeline_output_16bit(desc), cid)
    _named(ran, _exact("ipk::k_chan_16_to_8" if bits == 16 else "ipk::k_chan_8_to_16"), cid)


_ROTATE = [(k, o) for k in ("f32", "u8", "u16") for o in (2, 5)]       # IPK_OR_ROT180 keeps rows as rows, IPK_OR_ROT90 transposes


@_cases("rotate", _ROTATE, ["%s-or%d" % c for c in _ROTATE])
def test_rotate_buffer_variants(ipa, orc, case):
    """launch_rotate: `(y_step == 1 || y_step == -1) && x_step != 1 && x_step != -1` -> k_rotate_transposed<T>, else k_rotate<T>"""
    import torch
    cid, (kind, orientation) = case
    h, w = 33, 65
    rng = np.random.default_rng(util.SEED + 9820)
    if kind == "f32":
        img = rng.random((h, w, 3)).astype(np.float32)
        img.ravel()[: util.SPECIALS.size] = util.SPECIALS
        fn, dt = ipa.lib().ipk_rotate_buffer, torch.float32
    else:
        bits = 8 if kind == "u8" else 16
        img = rng.integers(0, 1 << bits, (h, w, 3)).astype(np.uint8 if bits == 8 else np.uint16)
        fn, dt = getattr(ipa.lib(), "ipk_rotate_image_" + kind), (torch.uint8 if bits == 8 else torch.int16)
    src = _upload(ipa, img)
    dst = Guarded(h * w * 3, dt)
    ow, oh = C.c_size_t(), C.c_size_t()
    with ipa.launch_log() as ran:
        assert fn(src.data_ptr(), w, h, orientation, dst.ptr, C.byref(ow), C.byref(oh), None) == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    # the permutation, checked on bit patterns: every sample is moved, none is computed
    want = orc.rotate_buffer(np.arange(h * w * 3, dtype=np.float32).reshape(h, w, 3), orientation).astype(np.int64)
    assert (oh.value, ow.value) == want.shape[:2]
    got = dst.result().reshape(oh.value, ow.value, 3)
    flat = img.ravel()
    expect = flat[want.ravel()].reshape(want.shape)
    assert np.array_equal(got.view(np.uint32) if kind == "f32" else got, expect.view(np.uint32) if kind == "f32" else expect), cid
    T = {"f32": F32, "u8": "unsigned char", "u16": U16}[kind]
    _named(ran, _exact("ipk::k_rotate%s<%s>" % ("_transposed" if orientation == 5 else "", T)), cid)


# =============================================================================================
# The log itself, and the closing test
# =============================================================================================
def test_oriented_refuses_mosaics_wider_than_the_transposing_permutation(ipa):
    """ipk_raw_to_srgb_oriented, transposing orientations: fused_impl `t && p->width > kRotate1MaxTransposedRows` (65535 * 64 columns, one grid row of
    k_rotate1_transposed per 64 output rows) returns IPK_ERR_UNSUPPORTED before anything is read, written or launched -- the caller then rotates the
    3-channel result, as for every other frame without a rotated-space variant.  The check sits in front of every access, so a descriptor of that width (256 rows: the rotated
    frame is then wide enough for every other condition) over a small buffer is enough to meet it."""
    import torch
    L = ipa.lib()
    buf = torch.zeros(4096, dtype=torch.float32, device="cuda")
    out = torch.full((4096,), -7.0, dtype=torch.float32, device="cuda")
    plan = ipa.FusedPlan(width=65535 * 64 + 1, height=256, is_float=True, black0=util.BLACK, white0=util.WHITE, wb_coeffs=util.WB,
                         cam_to_xyz_normalized=util.cam_matrix())
    ow, oh = C.c_size_t(), C.c_size_t()
    with ipa.launch_log() as ran:
        for orientation in (4, 5, 6, 7):                # IPK_OR_TRANSPOSE, ROT90, TRANSVERSE, ROT270
            assert L.ipk_raw_to_srgb_oriented(plan._ref, buf.data_ptr(), orientation, out.data_ptr(), C.byref(ow), C.byref(oh), None) == -5
            assert (ow.value, oh.value) == (256, 65535 * 64 + 1)
        torch.cuda.synchronize()
    assert ran == set() and bool((out == -7.0).all())


def test_launch_log_reads_sizes_and_stops(ipa):
    """the read call against a log that holds entries: the size query, a too-small buffer (terminated prefix, full size returned), a full read;
    a disabled log stays empty while kernels run"""
    import torch
    L = ipa.lib()
    v = _upload(ipa, _samples(4096, 1))
    out = torch.empty(4096, dtype=torch.uint8, device="cuda")
    assert L.ipk_selftest_launch_log(1) == 0
    assert L.ipk_output8bit(v.data_ptr(), 4096, out.data_ptr(), None) == 0
    g = torch.empty(4096, dtype=torch.float32, device="cuda")
    assert L.ipk_gamma(v.data_ptr(), 4096, 1, 1, 0, g.data_ptr(), None) == 0
    need = L.ipk_selftest_launch_log_read(None, 0)
    full = C.create_string_buffer(need)
    assert L.ipk_selftest_launch_log_read(full, need) == need
    lines = full.value.decode().split("\n")
    assert len(lines) == 2 and lines == sorted(lines) and all(l.startswith("_ZN3ipk") and l.endswith("]") for l in lines), lines
    small = C.create_string_buffer(b"\x55" * 16, 16)
    assert L.ipk_selftest_launch_log_read(small, 10) == need
    assert small.raw[:10] == full.raw[:9] + b"\x00" and small.raw[10:] == b"\x55" * 6
    assert L.ipk_selftest_launch_log(0) == 0
    assert L.ipk_output8bit(v.data_ptr(), 4096, out.data_ptr(), None) == 0
    torch.cuda.synchronize()
    assert L.ipk_selftest_launch_log_read(None, 0) == 1 and ipa.read_launch_log() == set()


# kernels no parity case can name, each with its reason
ALLOWED = {
    r"^ipk::k_selftest_": "the exhaustive on-device proofs themselves (tests/test_gpu_selftest.py runs them)",
    r"^ipk::k_(copy|mix|clock)_probe$": "measurement aids without a reference counterpart (bench.py, tests/test_gpu_bench.py)",
    r"^ipk::k_build_q8$": "runs inside ipk_init, before a log can be enabled; ipk_selftest_q8 checks its table on every f32",
}


def test_every_compiled_kernel_was_named_by_a_case():
    """The kernels in the built library (llvm-readelf --notes, as tests/test_kernel_resources.py reads them) against the launch-log entries the cases
    of this module asked for by name and found.  Skips when a -k selection ran only part of the table."""
    from test_kernel_resources import _kernels
    missing_cases = [c for c in ALL_CASES if c not in RAN_CASES]
    if missing_cases:
        pytest.skip("%d of %d cases of the table did not run (first: %s)" % (len(missing_cases), len(ALL_CASES), missing_cases[0]))
    compiled = sorted({re.sub(r"\(.*$", "", n.replace("void ", "", 1)) for n, _v, _s, _sp in _kernels() if n})
    assert len(compiled) > 100 and all(k.startswith("ipk::k_") for k in compiled), [k for k in compiled if not k.startswith("ipk::k_")]
    named = {n.split("[", 1)[0] for n in NAMED}
    product = [k for k in compiled if not any(re.search(p, k) for p in ALLOWED)]
    uncovered = [k for k in product if k not in named]
    print("kernel coverage: %d product kernels named by a case, of %d compiled (%d allow-listed)" % (len(product) - len(uncovered), len(compiled), len(compiled) - len(product)))
    assert not uncovered, "%d compiled kernels were run by no case of this table:\n%s" % (len(uncovered), "\n".join(uncovered))
    stray = sorted(named - set(compiled))
    assert not stray, "the log names kernels the library does not hold: %s" % stray
