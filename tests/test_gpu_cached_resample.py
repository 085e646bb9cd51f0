"""ipk_pipeline_run_cached_region under IPK_FUSED_CACHED_RESAMPLE on the GPU: with the rotatecrop buffer (hash 2) missing, a region is resampled from
the cached demosaic buffer by ONE launch of k_fused_resample's cached-buffer source mode, bit for bit the same rectangle of the CPU oracle's
pipeline_run / output_8bit / output_16bit; what enters the cache, what is launched, and that nothing outside the destination is written."""
import re

import numpy as np
import pytest

import util
from util import assert_bits_equal
from test_gpu_cached_region import _build, _apply, _raw_pipe, _want, _host, _same, CROPS

pytestmark = pytest.mark.gpu

F32, U8, U16 = 0, 1, 2
RGBE_LAUNCH = r"^ipk::k_fused_resample<float, [012]>\[.*rgbe=1.*\]$"
ANGLES = [0.0, 0.03, 0.3, 0.5, 1.0]
# kind -> (sensor width, height, extra ops)
KINDS = {"rggb_u16": (342, 75, {}), "rggb_f32": (200, 120, {}), "xtrans_f32": (342, 75, dict(maxwidth=100)), "rgb8": (200, 120, {}),
         "mono_u16": (200, 120, {}), "rgbe_u16": (342, 75, {})}


@pytest.fixture(scope="module")
def ipa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _rc(angle):
    return (0.1, 0.05, 0.2, 0.0, angle)


def _make(ipa, orc, kind, angle, seed=0, bit=True, **ops):
    sw, sh, extra = KINDS[kind]
    pipe, desc = _build(ipa, orc, kind, sw=sw, sh=sh, seed=16000 + seed, rotatecrop=_rc(angle), **dict(extra, **ops))
    pipe.resample_cached = bit
    return pipe, desc


def _regions(fw, fh):
    """the whole area; 1x1 at two corners; one row, one column; an odd offset with an odd width (the window's first column is odd and the last lane has
    one pixel); rectangles wider and taller than a 64x32 / 32x32 tile (tiles are laid from the window's origin: they straddle tile borders wherever they
    start); rectangles touching each edge"""
    cand = [(0, 0, fw, fh), (0, 0, 1, 1), (fw - 1, fh - 1, 1, 1), (0, fh // 2, fw, 1), (fw // 3, 0, 1, fh), (3, 5, 37, 9), (1, 1, fw - 2, fh - 3),
            (5, 2, 71, 35), (fw - 67, fh - 34, 67, 34), (31, 3, 66, 33), (0, 3, 9, 11), (fw - 9, 2, 9, 13), (4, 0, 11, 7), (6, fh - 7, 13, 7)]
    return [(x, y, w, h) for x, y, w, h in cand if x >= 0 and y >= 0 and w > 0 and h > 0 and x + w <= fw and y + h <= fh]


def _run(ipa, pipe, cache, reg, out_type, log=False):
    import torch
    x, y, w, h = reg
    if not log:
        got = pipe.run_region(x, y, w, h, out_type, cache=cache)
        torch.cuda.synchronize()
        return _host(got, out_type, h, w), None
    with ipa.launch_log() as ran:
        got = pipe.run_region(x, y, w, h, out_type, cache=cache)
        torch.cuda.synchronize()
    return _host(got, out_type, h, w), sorted(ran)


def _check(ipa, pipe, cache, want, out_type, regions):
    for reg in regions:
        x, y, w, h = reg
        got, _ = _run(ipa, pipe, cache, reg, out_type)
        assert pipe.last_region_windowed, reg
        _same(got, want[y:y + h, x:x + w], out_type, "region %r out %d" % (reg, out_type))


def _only_the_resample(ran, normal=True):
    hits = [e for e in ran if re.match(RGBE_LAUNCH, e)]
    assert len(hits) == 1 and not any("k_transform_buffer" in e or "gather=1" in e for e in ran), ran
    rest = [e for e in ran if e not in hits]
    if normal:
        assert rest == [], ran
    else:
        assert len(rest) == 1 and "k_rotate" in rest[0], ran


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("kind", list(KINDS))
def test_regions_of_every_kind_and_angle(ipa, orc, kind, angle):
    pipe, desc = _make(ipa, orc, kind, angle, seed=1)
    _, (fw, fh) = pipe.sizes()
    admitted = pipe.resamples_cached_region()
    if kind == "rgbe_u16":
        assert not admitted
    elif angle in (0.0, 0.03):
        assert admitted, (kind, angle)
    cache = ipa.PipelineCache(1 << 28)
    regions = _regions(fw, fh)
    assert (0, 0, fw, fh) in regions
    for out_type in (F32, U8, U16):
        assert pipe.resamples_cached_region(out_type) == admitted
        _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, regions)
        assert cache.contains(pipe.hashes(out_type)[2]) == (not admitted), "hash 2 is filled on the parent's route alone"
    # what ran: the one launch where the route is admitted (hash 1 present, hash 2 absent: OpDemosaic's own scale_down_opbuf, which is
    # k_transform_buffer too, does not run again); OpRotateCrop over the whole frame and the gather launch on a fresh cache where it is not
    fresh = ipa.PipelineCache(1 << 28)
    _, ran = _run(ipa, pipe, cache if admitted else fresh, (0, 0, fw, fh), F32, log=True)
    if admitted:
        _only_the_resample(ran)
    else:
        assert not any("rgbe=1" in e for e in ran) and any("gather=1" in e for e in ran), ran
        if kind == "rgbe_u16":
            assert any(e.startswith("ipk::k_transform_buffer<float>") for e in ran), ran
    fresh.close()
    cache.close()


# Normal, Rotate180, Rotate90, and Rotate90 / Rotate270 with a horizontal flip (Transpose and Transverse between them)
@pytest.mark.parametrize("rot,fliph", [(0, False), (2, False), (1, False), (1, True), (3, True)])
def test_orientations_all_outputs(ipa, orc, rot, fliph):
    pipe, desc = _make(ipa, orc, "rggb_u16", 0.03, seed=2, rotation=rot, fliph=fliph)
    assert pipe.resamples_cached_region()
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    regions = [(0, 0, fw, fh), (3, 5, 37, 31), (fw - 33, fh - 21, 33, 21), (fw - 1, 0, 1, fh), (0, fh - 1, 5, 1), (0, 0, 1, 1)]
    for out_type in (F32, U8, U16):
        _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, regions)
        assert pipe.last_ops_run & 0x84 == (0x04 if (rot, fliph) == (0, False) else 0x84)
        got, ran = _run(ipa, pipe, cache, (3, 5, 37, 31), out_type, log=True)
        _only_the_resample(ran, normal=(rot, fliph) == (0, False))
    cache.close()


def test_more_tiles_than_compute_units(ipa, orc):
    """the kernel's tile loop and its prefetch: a block takes several tiles"""
    import torch
    sw, sh = 1210, 620
    raw = util.noise_u16(util.SEED + 16003, sh, sw)
    pipe = _raw_pipe(ipa, raw, "RGGB", False)
    _apply(pipe, dict(rotatecrop=_rc(0.03)))
    pipe.resample_cached = True
    desc = orc.make_pipeline(raw, cfa=orc.cfa_shift("RGGB", CROPS[3], CROPS[0]), crops=CROPS, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                             wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), rotatecrop=_rc(0.03))
    _, (fw, fh) = pipe.sizes()
    assert fw * fh > 2048 * ipa.lib().ipk_device_cus()
    assert pipe.resamples_cached_region()
    cache = ipa.PipelineCache(1 << 30)
    _run(ipa, pipe, cache, (0, 0, 2, 2), F32)                                # the cache up to op 1
    for out_type in (F32, U8):
        got, ran = _run(ipa, pipe, cache, (0, 0, fw, fh), out_type, log=True)
        _only_the_resample(ran)
        _same(got, _want(orc, desc, out_type), out_type, "whole area, out %d" % out_type)
    cache.close()


@pytest.mark.parametrize("angle", [0.0, 0.03])
def test_special_values(ipa, orc, angle):
    """util.SPECIALS rows and lone +-inf / NaN samples in an f32 mosaic, inside, just outside and on the border of the region's source footprint: taps of
    weight 0 over inf give the oracle's NaN, and specials outside every window do not leak in"""
    sw, sh = 342, 75
    raw = util.noise_u16(util.SEED + 16004, sh, sw).astype(np.float32)
    with np.errstate(over="ignore"):
        raw[26:28, :] = np.resize(util.SPECIALS * np.float32(util.WHITE), 2 * sw).reshape(2, sw)
    pipe = _raw_pipe(ipa, raw, "RGGB", True)
    _apply(pipe, dict(rotatecrop=_rc(angle)))
    pipe.resample_cached = True
    _, (fw, fh) = pipe.sizes()
    # region (x, y, w, h) of the result; rotatecrop's crops shift it by about (0, 0.1 * 72) in the cropped frame, the sensor crops by (5, 1) more
    x, y, w, h = 101, 21, 130, 16
    sx, sy = x + 5, y + 1 + 7
    for k, v in enumerate([np.inf, -np.inf, np.nan]):
        for dy, dx in ((-3, 9 * k), (-2, 40 + 9 * k), (-1, 80 + 9 * k), (0, 20 + 9 * k), (h - 1, 30 + 11 * k), (h, 60 + 11 * k), (h + 1, 90 + 11 * k),
                       (h + 3, 11 * k), (3 + k, -3), (6 + k, -2), (9 + k, -1), (12 + k, 0), (2 + k, w - 1), (5 + k, w), (8 + k, w + 1), (11 + k, w + 3),
                       (5 + k, 40 + 30 * k)):
            raw_y, raw_x = sy + dy, sx + dx
            if 0 <= raw_y < sh and 0 <= raw_x < sw:
                raw[raw_y, raw_x] = v
    pipe = _raw_pipe(ipa, raw, "RGGB", True)
    _apply(pipe, dict(rotatecrop=_rc(angle)))
    pipe.resample_cached = True
    assert pipe.resamples_cached_region()
    desc = orc.make_pipeline(raw, cfa=orc.cfa_shift("RGGB", CROPS[3], CROPS[0]), crops=CROPS, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                             wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), rotatecrop=_rc(angle))
    cache = ipa.PipelineCache(1 << 28)
    regions = [(x, y, w, h), (0, 14, fw, 9), (0, 0, fw, fh), (x + 1, y + 1, w - 2, h - 2), (x - 2, y - 2, w + 5, h + 4)]
    for out_type in (F32, U8, U16):
        _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, regions)
    assert not cache.contains(pipe.hashes()[2])
    cache.close()


def _keys(cache, hs):
    return [cache.contains(k) for k in hs]


@pytest.mark.parametrize("out_type", [F32, U8, U16])
def test_cache_contract(ipa, orc, out_type):
    pipe, desc = _make(ipa, orc, "rggb_u16", 0.03, seed=5, rotation=2)
    _, (fw, fh) = pipe.sizes()
    reg = (5, 3, 201, 31)
    x, y, w, h = reg
    want = _want(orc, desc, out_type)[y:y + h, x:x + w]
    # the parent's route on a cache of its own: its mask is the yardstick for bits 3..7
    pipe.resample_cached = False
    parent = ipa.PipelineCache(1 << 28)
    got, ran = _run(ipa, pipe, parent, reg, out_type, log=True)
    _same(got, want, out_type, "bit clear")
    parent_mask = pipe.last_ops_run
    assert parent_mask & 7 == 7
    assert any(e.startswith("ipk::k_transform_buffer<float>") for e in ran) and any("gather=1" in e for e in ran) and not any("rgbe=1" in e for e in ran), ran
    assert _keys(parent, pipe.hashes(out_type)) == [True, True, True, False, False, False, False, False]
    # the bit on an empty cache: ops 0..1 whole-frame and stored, the rectangle resampled, hash 2 absent
    pipe.resample_cached = True
    cache = ipa.PipelineCache(1 << 28)
    got, ran = _run(ipa, pipe, cache, reg, out_type, log=True)
    _same(got, want, out_type, "bit set, empty cache")
    assert pipe.last_region_windowed and pipe.last_ops_run == parent_mask
    assert sum(bool(re.match(RGBE_LAUNCH, e)) for e in ran) == 1 and not any("gather=1" in e for e in ran), ran
    hs = pipe.hashes(out_type)
    assert _keys(cache, hs) == [True, True, False, False, False, False, False, False]
    for k in (0, 1):                                                         # stored as ipk_pipeline_run_cached's staged ops store them
        assert_bits_equal(cache.get(hs[k]), parent.get(hs[k]), "cached buffer %d" % k)
    before = cache.stats()
    # again: nothing whole-frame, ONE launch and the permutation, the cache keeps its entries
    got, ran = _run(ipa, pipe, cache, reg, out_type, log=True)
    _same(got, want, out_type, "bit set, hash 1 present")
    _only_the_resample(ran, normal=False)
    assert pipe.last_region_windowed and pipe.last_ops_run == (parent_mask & ~3) and pipe.last_ops_run & 4
    after = cache.stats()
    assert (after["entries"], after["bytes"]) == (before["entries"], before["bytes"]) == (2, after["bytes"])
    assert _keys(cache, hs)[:3] == [True, True, False]
    # hash 2 present (a region call that leaves the bit out fills it): the gather launch runs, one tap per pixel
    pipe.resample_cached = False
    _run(ipa, pipe, cache, reg, out_type)
    assert _keys(cache, hs)[:3] == [True, True, True]
    pipe.resample_cached = True
    got, ran = _run(ipa, pipe, cache, reg, out_type, log=True)
    _same(got, want, out_type, "bit set, hash 2 present")
    assert any("gather=1" in e for e in ran) and not any("rgbe=1" in e or "k_transform_buffer" in e for e in ran), ran
    assert pipe.last_ops_run == (parent_mask & ~7)
    # hash 7 present: the rectangle is copied out
    import torch
    whole, _, _ = pipe._run(out_type, cache=cache)
    torch.cuda.synchronize()
    assert cache.contains(hs[7])
    got, ran = _run(ipa, pipe, cache, reg, out_type, log=True)
    _same(got, want, out_type, "bit set, hash 7 present")
    assert not pipe.last_region_windowed and pipe.last_ops_run == 0 and not any("rgbe=1" in e or "gather=1" in e for e in ran), ran
    cache.close()
    parent.close()


@pytest.mark.parametrize("kind,angle", [("rggb_u16", 0.03), ("xtrans_f32", 0.0), ("mono_u16", 0.3)])
def test_equal_bits_with_the_cached_run_and_between_overlapping_regions(ipa, orc, kind, angle):
    import torch
    pipe, desc = _make(ipa, orc, kind, angle, seed=6)
    if not pipe.resamples_cached_region():
        pytest.fail("the case is meant to take the route")
    _, (fw, fh) = pipe.sizes()
    for out_type in (F32, U8, U16):
        other = ipa.PipelineCache(1 << 28)
        whole, _, _ = pipe._run(out_type, cache=other)
        torch.cuda.synchronize()
        whole = _host(whole, out_type, fh, fw)
        other.close()
        cache = ipa.PipelineCache(1 << 28)
        a, b = (2, 1, min(90, fw - 2), min(30, fh - 1)), (41, 13, min(75, fw - 41), min(25, fh - 13))
        ga, _ = _run(ipa, pipe, cache, a, out_type)
        gb, _ = _run(ipa, pipe, cache, b, out_type)
        assert not cache.contains(pipe.hashes(out_type)[2])
        for (x, y, w, h), g in ((a, ga), (b, gb)):
            _same(g, whole[y:y + h, x:x + w], out_type, "against ipk_pipeline_run_cached, %r" % ((x, y, w, h),))
        ox0, oy0, ox1, oy1 = max(a[0], b[0]), max(a[1], b[1]), min(a[0] + a[2], b[0] + b[2]), min(a[1] + a[3], b[1] + b[3])
        assert ox1 > ox0 and oy1 > oy0
        _same(ga[oy0 - a[1]:oy1 - a[1], ox0 - a[0]:ox1 - a[0]], gb[oy0 - b[1]:oy1 - b[1], ox0 - b[0]:ox1 - b[0]], out_type, "the overlap")
        cache.close()


@pytest.mark.parametrize("out_type,off,reg", [(U8, 3, (7, 3, 51, 7)), (F32, 1, (1, 2, 63, 11)), (U16, 1, (9, 1, 65, 33))])
def test_nothing_outside_the_destination_is_written(ipa, orc, out_type, off, reg):
    import torch
    pipe, desc = _make(ipa, orc, "rggb_u16", 0.03, seed=9)
    assert pipe.resamples_cached_region(out_type)
    cache = ipa.PipelineCache(1 << 28)
    x, y, w, h = reg
    g = util.Guarded(w * h * 3, {U8: torch.uint8, F32: torch.float32, U16: torch.int16}[out_type], off=off)
    with ipa.launch_log() as ran:
        pipe.run_region(x, y, w, h, out_type, out=g.view(), cache=cache)
        torch.cuda.synchronize()
    assert any(re.match(RGBE_LAUNCH, e) for e in ran), sorted(ran)
    got = g.result("region %r" % (reg,))
    got = (got.view(np.uint16) if out_type == U16 else got).reshape(h, w, 3)
    _same(got, _want(orc, desc, out_type)[y:y + h, x:x + w], out_type, "guarded destination")
    cache.close()
