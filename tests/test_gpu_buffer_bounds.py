"""Stray writes and odd alignments on the one-launch routes.

Every other parity test hands the library a fresh, 256-byte-aligned `torch.empty(w*h*3)` and compares exactly those samples, so a store a few pixels
past the last row (or in front of the first) lands in allocator padding nobody looks at, and no kernel ever meets a pointer that is aligned to its
element type only.  Here every destination is a util.Guarded -- the result inside a larger allocation, pre-filled with sentinels, with a band of
sentinels on both sides -- and every source a util.Embedded -- the frame among poison (f32: NaN, u16: 0xFFFF), so that a sample from outside the
frame that enters the arithmetic, even with weight 0, breaks parity.  Each case runs through the public surface and asserts
  * the whole result, bit for bit, against the CPU oracle (f32 bits, equal u8 / u16),
  * both bands untouched (and, in the batch, the gaps between frames),
  * through the launch log, that the intended kernel family ran -- a case that silently went staged fails,
for every combination of the source and destination offsets below.  The oracle is computed once per case; the offsets do not enter it.

Band: 1024 elements.  One 256-pixel strip is 768 samples of a 3-channel result and 1024 of the 4-channel demosaic result, so a write misplaced by up
to a whole strip still lands inside the band.
Offsets (elements past a 256-byte boundary): destination 0 and 1 -- u8 results at an odd byte, u16 at 2 mod 4, f32 at 4 mod 16 -- and 3 for f32
(12 mod 16); source 0 and 1 -- u16 at base % 4 == 2 with an even pitch (the half of `src_aligned4` no crop reaches), f32 at 4 mod 16 (every f32 row
load is a 16-byte `f4u`).
Frames are the smallest that reach the geometry: pipelines take 10 x 10 or more, 11 rows (odd) are enough for a first, a last and interior rows.

Families:
  whole frame  Pipeline, Bayer and X-Trans, f32 / u16, the three outputs.  Full-strip widths 256 (one strip, no shift), 257..260 (a second strip
               shifted left by 255..252 pixels: every residue of W mod 4), 511 and 513 (one pixel short of / past two strips: the last strip
               overlaps all but one / only one pixel of its neighbour).  Narrow widths 10, 12, 13, 14, 15 and 255: W & 3 takes 0..3 and W & 1
               both values, so both arms of `store_aligned` (packed u3w / dword stores, sample-by-sample stores) meet an odd destination, and the
               last lane holds 1..4 pixels.  The leaf (curve / no curve, guards / no guards) rotates with the width.
  rotated      rotation 1 on 24 x 262 and rotation 2 on 262 x 12: the rotated-space kernels behind k_rotate1_transposed / k_rotate1_rows, which
               read the offset, embedded source.
  row bands    FusedPlan(band=...): rows [3, 9) of a 12-row frame, 257 and 13 columns; the source holds the band's rows and halos only.
  regions      run_region(out=) on a 300 x 24 frame: first columns 1, 2, 3 mod 4, widths 1, 3, 255, 256, 277, regions on the right and bottom
               edges (win_store's straddling lanes, the staged stores of inner strips at a packed pitch).
  batch        three 257 x 11 frames through FusedBatchPlan into one allocation: packed back to back (8481 samples a frame: frames 1 and 2 start
               at odd bytes / odd elements) and with a sentinel gap between them, so that frame i's overrun is not hidden by frame i+1's stores.
  resample     raw_to_srgb_resampled (47 x 61: crop-uneven, rot.2, rot.77) and raw_to_srgb_scaled (131x97@87, 101x103@51): output widths 45, 64,
               70, 87, 51 -- odd and even, the odd ones drop the lane's second pixel at the row end
               (test_resample_cases_have_odd_and_even_output_widths keeps that true).
  demosaic     ipk_demosaic_full (widths 70 and 262, Bayer and X-Trans) and FusedPlan.probe, destination offsets 1 and 3.
  staged       ipk_pipeline_run on its staged route (a four-colour filter; a Bayer frame with allow_fused = 0), 13 and 257 columns: k_gofloat_cfa* in
               front of the offset source, the last stage in front of the offset destination.  ipk_pointwise_chain_out and ipk_raster_to_srgb at
               destination offset 1 (the coverage module guards them at offset 0)."""
import re

import numpy as np
import pytest

import util
from util import Embedded, Guarded
import test_gpu_kernel_coverage as cov
import test_gpu_rotatecrop_fused as rcf
import test_gpu_scaledown_fused as sdf

pytestmark = pytest.mark.gpu

XT, F32, U16, OUTS = cov.XT, cov.F32, cov.U16, cov.OUTS
SRC_OFFS = (0, 1)
DST_OFFS = {0: (0, 1, 3), 1: (0, 1), 2: (0, 1)}                        # by output type: f32 also at 12 mod 16
STAGED = ("k_gofloat", "k_demosaic_full", "k_pointwise_chain", "k_raster_chain", "k_transform_buffer", "k_tolab", "k_output")


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _tdt(out):
    import torch
    return [torch.float32, torch.uint8, torch.int16][out]


def _kind(src, so, pitch):
    """the coverage module's name for the source: a u16 frame 2 bytes off a dword boundary, or one with an odd pitch, takes the kernels of its "u16odd"
    frames (fused_impl: `src_aligned4 = base % 4 == 0 && owidth % 2 == 0`)"""
    return "f32" if src == "f32" else ("u16odd" if so % 2 or pitch % 2 else "u16a")


class Findings:
    """collects what the offset combinations of one case find, so that one failing combination does not hide the others; [band] / [parity] says which
    assertion it was"""

    def __init__(self, cid):
        self.cid, self.errs = cid, []

    def verify(self, g, want, what, gaps=()):
        """g: the Guarded destination after the run; want: the oracle's samples for its interior (gaps: (start, count) runs of the interior that must
        still hold the sentinel)"""
        a = g.whole()
        what = "%s %s" % (self.cid, what)
        try:
            util.guard_check(a, g.n, g.off, g.band, what)
        except AssertionError as e:
            self.errs.append("[band] %s" % str(e).split("\n")[0])
        inner = a[g.lo: g.lo + g.n]
        keep = np.ones(g.n, bool)
        for s, c in gaps:
            keep[s: s + c] = False
            if not np.all(inner[s: s + c] == np.array(g.sentinel).astype(inner.dtype)):
                self.errs.append("[band] %s: the gap at %d..%d between two frames was written" % (what, s, s + c))
        try:
            cov._same(inner[keep], np.ascontiguousarray(want).ravel(), what)
        except AssertionError as e:
            self.errs.append("[parity] %s" % str(e).split("\n")[0])

    def ran(self, ran, patterns, nothing_staged=True):
        for p in patterns:
            if not [n for n in ran if re.search(p, n)]:
                self.errs.append("[route] %s: no launched kernel matches %r; launched: %s" % (self.cid, p, sorted(ran)))
        if nothing_staged:
            stray = [n for n in ran if any(k in n for k in STAGED)]
            if stray:
                self.errs.append("[route] %s: staged kernels ran: %s" % (self.cid, stray))

    def close(self):
        assert not self.errs, "%d findings:\n%s" % (len(self.errs), "\n".join(self.errs))


def _pipe(ipa, dev, w, h, is_float, cfa, guard, points, linear, rotation=0):
    img = ipa.RawImage(width=w, height=h, data=dev, cfa=cfa, is_float=is_float, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                       wb_coeffs=util.WB, cam_to_xyz_normalized=cov._cam(guard))
    pipe = ipa.Pipeline.new_from_source(img)
    pipe.ops.basecurve.points = list(points)
    pipe.globals.settings.linear = bool(linear)
    pipe.ops.transform.rotation = rotation
    return pipe


def _want(orc, data, cfa, guard, points, linear, out, rotation=0):
    desc = orc.make_pipeline(data, cfa=cfa, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                             cam_to_xyz_normalized=cov._cam(guard), points=list(points), linear=bool(linear), rotation=rotation)
    return [orc.pipeline_run, orc.pipeline_output_8bit, orc.pipeline_output_16bit][out](desc)


def _offsets(out):
    return [(so, do) for so in SRC_OFFS for do in DST_OFFS[out]]


# =============================================================================================
# Whole frames (and the rotated-space variants)
# =============================================================================================
FULL_W = {256: "common", 257: "plain", 258: "common-guard", 259: "grid", 260: "plain-guard", 511: "grid-guard", 513: "common"}
GEN_FULL_W = {256: "gen-common", 257: "gen-plain", 258: "gen-common", 259: "gen-plain", 260: "gen-common", 511: "gen-plain", 513: "gen-common"}
NARROW_W = (10, 12, 13, 14, 15, 255)
_WHOLE = [(w, 11, gen, (GEN_FULL_W if gen else FULL_W)[w]) for gen in (False, True) for w in FULL_W] + \
         [(w, 11, gen, "gen-narrow" if gen else "narrow") for gen in (False, True) for w in NARROW_W] + \
         [(24, 262, False, "rot90"), (262, 12, False, "rot180-guard"), (24, 262, True, "gen-rot90")]
_WHOLE = [(w, h, gen, leaf, s, o) for w, h, gen, leaf in _WHOLE for s in ("f32", "u16") for o in OUTS]


@pytest.mark.parametrize("w,h,gen,leaf,src,out", _WHOLE, ids=["%dx%d-%s-%s-out%d" % (c[0], c[1], c[3], c[4], c[5]) for c in _WHOLE])
def test_whole_frames(ipa, orc, w, h, gen, leaf, src, out):
    import torch
    lgen, curve, guard, full, rotation = cov.FUSED_LEAVES[leaf]
    assert lgen == gen and full == (w >= 256 or rotation == 1)
    cid = "whole %dx%d %s %s out%d" % (w, h, leaf, src, out)
    data, _ = cov._mosaic("f32" if src == "f32" else "u16a", h, w, util.SEED + 11000 + 7 * w + out)
    cfa = XT if gen else "RGGB"
    linear = bool(curve) and out == 2
    want = _want(orc, data, cfa, guard, curve, linear, out, rotation)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so, do in _offsets(out):
            emb, g = Embedded(data, so), Guarded(w * h * 3, _tdt(out), do)
            pipe = _pipe(ipa, emb.view(), w, h, src == "f32", cfa, guard, curve, linear, rotation)
            _, fw, fh = pipe._run(out, g.view(), None)
            torch.cuda.synchronize()
            assert pipe.last_used_fused and (fh, fw, 3) == want.shape, (cid, fw, fh, want.shape)
            f.verify(g, want, "src+%d dst+%d" % (so, do))
            emb.assert_untouched(cid)
    names = [cov._exact(cov.fused_kernel(_kind(src, so, w), out, leaf)) for so in SRC_OFFS]
    if rotation:
        names.append(cov._exact("ipk::k_rotate1_%s<%s>" % ("transposed" if rotation == 1 else "rows", F32 if src == "f32" else U16)))
    f.ran(ran, names)
    f.close()


# =============================================================================================
# Row bands
# =============================================================================================
_BANDS = [(w, gen, s, o) for w in (257, 13) for gen in (False, True) for s in ("f32", "u16") for o in OUTS]


@pytest.mark.parametrize("w,gen,src,out", _BANDS, ids=["%d-%s-%s-out%d" % (c[0], "xtrans" if c[1] else "bayer", c[2], c[3]) for c in _BANDS])
def test_row_bands(ipa, orc, w, gen, src, out):
    """rows [3, 9) of a 12-row frame: the source is the band's rows with their halo rows, 2..9, and nothing else of the frame"""
    import torch
    h, (r0, r1) = 12, (3, 9)
    s0, s1 = r0 - 1, r1 + 1
    leaf = ("gen-" if gen else "") + ("common" if w >= 256 else "narrow")
    curve = cov.FUSED_LEAVES[leaf][1]
    cid = "band %dx%d %s %s out%d" % (w, h, leaf, src, out)
    data, _ = cov._mosaic("f32" if src == "f32" else "u16a", h, w, util.SEED + 11500 + w + out)
    cfa = XT if gen else "RGGB"
    linear = out == 2                                   # as output_16bit sets it, whatever the curve
    want = _want(orc, data, cfa, False, curve, linear, out)[r0:r1]
    plan = ipa.FusedPlan(width=w, height=h, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa=cfa, wb_coeffs=util.WB,
                         cam_to_xyz_normalized=util.cam_matrix(), points=curve, linear=linear, out_type=out, band=(s0, s1 - s0, r0, r1 - r0))
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so, do in _offsets(out):
            emb, g = Embedded(data[s0:s1], so), Guarded((r1 - r0) * w * 3, _tdt(out), do)
            plan.run(emb.view(), g.view())
            torch.cuda.synchronize()
            f.verify(g, want, "src+%d dst+%d" % (so, do))
            emb.assert_untouched(cid)
    f.ran(ran, [cov._exact(cov.fused_kernel(_kind(src, so, w), out, leaf)) for so in SRC_OFFS])
    f.close()


# =============================================================================================
# Regions
# =============================================================================================
RW, RH = 300, 24
# (x, y, w, h)
REGIONS = [(1, 2, 1, 5), (2, 3, 3, 4), (3, 1, 255, 6), (43, 0, 256, 5), (44, 5, 256, 3), (23, 18, 277, 6), (297, 20, 3, 4)]
assert {r[0] % 4 for r in REGIONS} == {0, 1, 2, 3} and {r[2] for r in REGIONS} == {1, 3, 255, 256, 277}
assert any(r[0] + r[2] == RW and r[1] + r[3] == RH for r in REGIONS)
_REGION_FRAMES = {}


def _region_frame(orc, gen, src, out):
    key = (gen, src, out)
    if key not in _REGION_FRAMES:
        data, _ = cov._mosaic("f32" if src == "f32" else "u16a", RH, RW, util.SEED + 12000 + 3 * out + gen)
        _REGION_FRAMES[key] = (data, _want(orc, data, XT if gen else "RGGB", False, cov.CURVE3, out == 2, out))
    return _REGION_FRAMES[key]


_REGION_CASES = [(r, gen, s, o) for r in REGIONS for gen in (False, True) for s in ("f32", "u16") for o in OUTS]


@pytest.mark.parametrize("region,gen,src,out", _REGION_CASES,
                         ids=["x%d-y%d-%dx%d-%s-%s-out%d" % (c[0] + ("xtrans" if c[1] else "bayer", c[2], c[3])) for c in _REGION_CASES])
def test_regions(ipa, orc, region, gen, src, out):
    import torch
    x, y, rw, rh = region
    cid = "region %r %s %s out%d" % (region, "xtrans" if gen else "bayer", src, out)
    data, whole = _region_frame(orc, gen, src, out)
    want = whole[y: y + rh, x: x + rw]
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so, do in _offsets(out):
            emb, g = Embedded(data, so), Guarded(rw * rh * 3, _tdt(out), do)
            pipe = _pipe(ipa, emb.view(), RW, RH, src == "f32", XT if gen else "RGGB", False, cov.CURVE3, out == 2)
            pipe.run_region(x, y, rw, rh, out_type=out, out=g.view())
            torch.cuda.synchronize()
            assert pipe.last_region_windowed, cid
            f.verify(g, want, "src+%d dst+%d" % (so, do))
            emb.assert_untouched(cid)
    S = F32 if src == "f32" else U16
    f.ran(ran, [r"^ipk::k_fused_bayer_window<%s, %s, %d, " % (S, cov._b(S == F32), out)])
    f.close()


# =============================================================================================
# Batch
# =============================================================================================
_BATCH = [(lay, s, o) for lay in ("packed", "gapped") for s in ("f32", "u16") for o in OUTS]


@pytest.mark.parametrize("layout,src,out", _BATCH, ids=["%s-%s-out%d" % c for c in _BATCH])
def test_batch_into_one_allocation(ipa, orc, layout, src, out):
    import torch
    w, h, nf = 257, 11, 3
    n = w * h * 3
    assert n % 2 == 1                                   # packed: frame 1 starts at an odd byte (u8) / an odd element (u16, f32)
    gap = util.GUARD_BAND if layout == "gapped" else 0
    stride = n + gap
    cid = "batch %s %s out%d" % (layout, src, out)
    frames = [cov._mosaic("f32" if src == "f32" else "u16a", h, w, util.SEED + 12500 + 5 * k + out)[0] for k in range(nf)]
    want = np.concatenate([_want(orc, d, "RGGB", False, cov.CURVE3, out == 2, out).ravel() for d in frames])
    plan = ipa.FusedPlan(width=w, height=h, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa="RGGB", wb_coeffs=util.WB,
                         cam_to_xyz_normalized=util.cam_matrix(), points=cov.CURVE3, linear=out == 2, out_type=out)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so, do in _offsets(out):
            embs = [Embedded(d, so) for d in frames]
            g = Guarded(nf * n + (nf - 1) * gap, _tdt(out), do)
            ipa.FusedBatchPlan(plan, [e.view() for e in embs], [g.view(k * stride, n) for k in range(nf)]).run()
            torch.cuda.synchronize()
            f.verify(g, want, "src+%d dst+%d" % (so, do), gaps=[(k * stride + n, gap) for k in range(nf - 1)] if gap else ())
            for e in embs:
                e.assert_untouched(cid)
    S = F32 if src == "f32" else U16
    f.ran(ran, [cov._exact("ipk::k_fused_bayer_batch<%s, %s, %d, false>" % (S, cov._b(S == F32), out))])
    f.close()


# =============================================================================================
# Resample and near-full-size preview
# =============================================================================================
# name -> (width, height, filter, R9 index | size limit)
RESAMPLE = {"crop-uneven": (47, 61, "GRBG", 1), "rot.2": (47, 61, XT, 3), "rot.77": (47, 61, "GRBG", 5),
            "131x97@87": (131, 97, XT, dict(maxwidth=87)), "101x103@51": (101, 103, "RGGB", dict(maxwidth=51))}


def _resample_geometry(orc, name):
    """-> (corners as the oracle's transform takes them, scaled?)"""
    w, h, _cfa, how = RESAMPLE[name]
    if isinstance(how, dict):
        nw, nh = sdf._negotiated(orc, w, h, sdf.NOCROP, how)
        return ((0, 0), (w - 1, 0), (0, h - 1), nw, nh), True          # scale_down_opbuf's corners
    corners = orc.rotatecrop_corners(rcf.R9[how], w, h)
    assert corners is not None
    return corners, False


_RESAMPLE_CASES = [(n, s, o) for n in RESAMPLE for s in ("f32", "u16") for o in OUTS]


@pytest.mark.parametrize("name,src,out", _RESAMPLE_CASES, ids=["%s-%s-out%d" % c for c in _RESAMPLE_CASES])
def test_resampled_and_scaled(ipa, orc, name, src, out):
    import torch
    w, h, cfa, _ = RESAMPLE[name]
    cid = "resample %s %s out%d" % (name, src, out)
    corners, scaled = _resample_geometry(orc, name)
    tl, tr, bl, nw, nh = corners
    data = rcf._mosaic(util.SEED + 13000 + len(name) + out, h, w, src == "f32")
    otype = [rcf.F32, rcf.U8, rcf.U16][out]
    want = rcf._oracle_ops(orc, data, (0, 0, 0, 0), cfa, util.BLACK, util.WHITE, corners, util.WB, util.cam_matrix(), 0.0, cov.CURVE3, out == 2, otype)
    assert want.shape == (nh, nw, 3)
    kw = dict(width=w, height=h, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa=cfa, wb_coeffs=util.WB,
              cam_to_xyz_normalized=util.cam_matrix(), points=cov.CURVE3, linear=out == 2, out_type=out)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so, do in _offsets(out):
            emb, g = Embedded(data, so), Guarded(nw * nh * 3, _tdt(out), do)
            if scaled:
                ipa.raw_to_srgb_scaled(emb.view(), nw, nh, out=g.view(), **kw)
            else:
                ipa.raw_to_srgb_resampled(emb.view(), (tl[0], tl[1], tr[0], tr[1], bl[0], bl[1]), nw, nh, out=g.view(), **kw)
            torch.cuda.synchronize()
            f.verify(g, want, "src+%d dst+%d" % (so, do))
            emb.assert_untouched(cid)
    f.ran(ran, [r"^ipk::k_fused_resample<%s, %d>\[fast_ok=1%s\]" % (F32 if src == "f32" else U16, out, ",axis=1" if scaled else "")])
    f.close()


def test_resample_cases_have_odd_and_even_output_widths(orc):
    """an odd width ends every row -- the last one too -- on a lane whose second pixel does not exist; an even one on a lane that stores both"""
    widths = {name: _resample_geometry(orc, name)[0][3] for name in RESAMPLE}
    assert {w % 2 for w in widths.values()} == {0, 1}, widths
    assert any(w % 2 for n, w in widths.items() if isinstance(RESAMPLE[n][3], dict)) and any(w % 2 for n, w in widths.items() if not isinstance(RESAMPLE[n][3], dict)), widths


# =============================================================================================
# Demosaic only (OUT == 3) and the stream probe (OUT == 4)
# =============================================================================================
_DEMOSAIC = [c for c in cov._DEMOSAIC if c[0] != "RGBE"]


@pytest.mark.parametrize("cfa,w,kernel", _DEMOSAIC, ids=["%s-%d" % (c[0][:4], c[1]) for c in _DEMOSAIC])
def test_demosaic_only(ipa, orc, cfa, w, kernel):
    import torch
    h = 11
    cid = "demosaic %s %d" % (cfa[:4], w)
    buf = util.uniform_f32(util.SEED + 13500 + w, h * w, -0.05, 1.0).reshape(h, w)
    buf.ravel()[w + 1: w + 1 + util.SPECIALS.size] = util.SPECIALS
    buf[h // 2, w // 2] = np.nan; buf[h - 2, 2] = -np.inf
    want = orc.demosaic_full(cfa, buf)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so in SRC_OFFS:
            for do in (1, 3):
                emb, g = Embedded(buf, so), Guarded(h * w * 4, torch.float32, do)
                assert ipa.lib().ipk_demosaic_full(emb.ptr, w, h, cfa.encode(), g.ptr, None) == 0, ipa.lib().ipk_last_error()
                torch.cuda.synchronize()
                f.verify(g, want, "src+%d dst+%d" % (so, do))
                emb.assert_untouched(cid)
    f.ran(ran, [cov._exact(kernel)], nothing_staged=False)
    f.close()


@pytest.mark.parametrize("src", ["f32", "u16"])
def test_stream_probe(ipa, orc, src):
    import torch
    w, h = 262, 11
    cid = "probe %s" % src
    data, _ = cov._mosaic("u16a", h, w, util.SEED + 13600)
    if src == "f32":
        data = data.astype(np.float32) + np.float32(0.25)
    plan = ipa.FusedPlan(width=w, height=h, is_float=src == "f32", black0=util.BLACK, white0=util.WHITE, cfa="BGGR", wb_coeffs=util.WB,
                         cam_to_xyz_normalized=util.cam_matrix())
    want = np.ascontiguousarray(orc.demosaic_full("BGGR", orc.gofloat_cfa(data, 0, 0, w, h, util.BLACK, util.WHITE))[:, :, :3])
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so in SRC_OFFS:
            for do in (1, 3):
                emb, g = Embedded(data, so), Guarded(h * w * 3, torch.float32, do)
                plan.probe(emb.view(), g.view())
                torch.cuda.synchronize()
                f.verify(g, want, "src+%d dst+%d" % (so, do))
                emb.assert_untouched(cid)
    S = F32 if src == "f32" else U16
    f.ran(ran, [cov._exact("ipk::k_fused_bayer<%s, %s, 4, true, false, false, 1, false>" % (S, cov._b(S == F32)))])
    f.close()


# =============================================================================================
# The staged driver, and the staged point-wise tail at a destination one element off
# =============================================================================================
_STAGED_RUNS = [(w, cfa, s, o) for w in (13, 257) for cfa in ("RGGB", "RGBE") for s in ("f32", "u16") for o in OUTS]


@pytest.mark.parametrize("w,cfa,src,out", _STAGED_RUNS, ids=["%d-%s-%s-out%d" % c for c in _STAGED_RUNS])
def test_staged_driver(ipa, orc, w, cfa, src, out):
    """ipk_pipeline_run on its staged route -- a four-colour filter, which has no one-launch route, and a Bayer frame with allow_fused = 0: the first
    stage (k_gofloat_cfa*) reads the embedded, offset source, the last one writes the guarded, offset destination"""
    import torch
    h = 11
    cid = "staged %dx%d %s %s out%d" % (w, h, cfa, src, out)
    data, _ = cov._mosaic("f32" if src == "f32" else "u16a", h, w, util.SEED + 13650 + w + out)
    want = _want(orc, data, cfa, False, cov.CURVE3, out == 2, out)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        for so, do in _offsets(out):
            emb, g = Embedded(data, so), Guarded(w * h * 3, _tdt(out), do)
            pipe = _pipe(ipa, emb.view(), w, h, src == "f32", cfa, False, cov.CURVE3, out == 2)
            pipe.allow_fused = cfa == "RGBE"                              # (nothing to allow there)
            pipe._run(out, g.view(), None)
            torch.cuda.synchronize()
            assert pipe.last_used_fused is False, cid
            f.verify(g, want, "src+%d dst+%d" % (so, do))
            emb.assert_untouched(cid)
    f.ran(ran, [r"^ipk::k_gofloat_cfa(_v4)?<%s" % (F32 if src == "f32" else U16)], nothing_staged=False)
    f.close()



@pytest.mark.parametrize("out", OUTS, ids=["f32", "u8", "u16"])
def test_pointwise_chain_out_offset_destination(ipa, orc, out):
    import torch
    npix = 64 * 96 + 3
    cid = "chain out%d" % out
    buf = np.ascontiguousarray(cov._rgbe(npix, util.SEED + 13700)).reshape(1, npix, 4)
    cm, points = util.cam_matrix(), cov.CURVE3
    src = cov._upload(ipa, buf)
    g = Guarded(npix * 3, _tdt(out), 1)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        rc = ipa.lib().ipk_pointwise_chain_out(src.data_ptr(), npix, 1, 0, cov._fa(util.WB), cov._fa(cm), 0.0, cov._fa([c for p in points for c in p]),
                                               len(points), 0, out, g.ptr, None)
        assert rc == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    f.verify(g, cov._chain_want(orc, buf, cm, points, False, out), "dst+1")
    f.ran(ran, [cov._exact("ipk::k_pointwise_chain_small" if out == 0 else "ipk::k_raster_chain<ipk::Rgbe32, %d>" % out)], nothing_staged=False)
    f.close()


_RASTER = [(b, o) for b in (8, 16) for o in OUTS]


@pytest.mark.parametrize("bits,out", _RASTER, ids=["u%d-out%d" % c for c in _RASTER])
def test_raster_to_srgb_offset_destination(ipa, orc, bits, out):
    import torch
    h, w = 7, 333
    cid = "raster u%d out%d" % (bits, out)
    img = (util.splitmix64(util.SEED + 13800 + bits, h * w * 3) & np.uint64((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16).reshape(h, w, 3)
    img.ravel()[:6] = [0, 1, (1 << bits) - 1, 2, (1 << bits) - 2, 128]
    cm, points = util.cam_matrix(), cov.CURVE3
    src = cov._upload(ipa, img)
    g = Guarded(h * w * 3, _tdt(out), 1)
    f = Findings(cid)
    with ipa.launch_log() as ran:
        rc = ipa.lib().ipk_raster_to_srgb(src.data_ptr(), 2 if bits == 8 else 3, w, h, cov._fa(util.WB), cov._fa(cm), 0.0, cov._fa([c for p in points for c in p]),
                                          len(points), 0, out, g.ptr, None)
        assert rc == 0, ipa.lib().ipk_last_error()
        torch.cuda.synchronize()
    f.verify(g, cov._chain_want(orc, orc.gofloat_other(img, 0, 0, w, h), cm, points, False, out), "dst+1")
    f.ran(ran, [cov._exact("ipk::k_raster_chain<%s, %d>" % ("unsigned char" if bits == 8 else U16, out))], nothing_staged=False)
    f.close()
