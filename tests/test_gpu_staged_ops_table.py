"""The eight ops of Pipeline::run as the two staged drivers run them -- ipk_pipeline_run's scratch-buffer driver and ipk_pipeline_run_cached's cache
driver -- crossed over what makes an op a no-op, what chooses its launch and where its output goes: four sources (a mosaic through plain gofloat and
demosaic::full, a mosaic through the one scaling pass, a monochrome f32 raw, a cropped RGB8 raster), a no-op or two-point curve, linear or not, Normal
or Rotate90, the three output types, and a frame above (24x18) or below (17x15) the point-wise chain's 256-pixel floor.
Bar: bit-exact against the CPU oracle; the stage labels, ops_run and the cache's contents are pinned with it."""
import ctypes as C
import itertools

import numpy as np
import pytest

import util
import test_gpu_staged_paths as sp
from test_gpu_staged_paths import F32, U8, U16

pytestmark = pytest.mark.gpu

CODES = {F32: 0, U8: 1, U16: 2}
SOURCES = ["bayer_plain", "bayer_one_pass", "mono_f32", "rgb8_cropped"]
SIZES = [(24, 18), (17, 15)]                                               # 432 and 255 pixels in front of OpTransform
CURVES = {"flat": [], "two": [(0.3, 0.2), (0.7, 0.85)]}
BAYER = dict(cfa="RGGB", cpp=1, is_float=False, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4)


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _build(ipa, orc, source, w, h, ops):
    """(pipeline with the source's allow_fused, a maker of fresh oracle descriptors)"""
    import torch
    seed = util.SEED + 21000 + 16 * SOURCES.index(source) + w
    if source == "rgb8_cropped":
        data = (util.splitmix64(seed, (h + 2) * (w + 2) * 3) & np.uint64(255)).astype(np.uint8).reshape(h + 2, w + 2, 3)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(w + 2, h + 2, torch.from_numpy(data.ravel()).cuda(), bits=8))
        g = pipe.ops.gofloat
        g.crop_top = g.crop_right = g.crop_bottom = g.crop_left = 1
        sp._apply(pipe, ops)
        return pipe, lambda: orc.make_pipeline(data, crops=(1, 1, 1, 1), **ops)
    if source == "mono_f32":
        data, src = sp._source("mono_f32", h, w, seed)
    elif source == "bayer_plain":
        data, src = util.noise_u16(seed, h, w), BAYER
    else:
        data, src = util.noise_u16(seed, 2 * h, 2 * w), BAYER
        ops = dict(ops, maxwidth=h if ops["rotation"] else w)             # half the result's width: OpDemosaic's scale is exactly 2, its minscale
    pipe = sp._pipeline(ipa, data, src, (0, 0, 0, 0), ops)
    pipe.allow_fused = source != "bayer_plain"
    return pipe, lambda: sp._oracle_desc(orc, data, src, (0, 0, 0, 0), dict(ops, wb_coeffs=util.WB, cam_to_xyz_normalized=sp._cam4()))


def _shape(a, out_type, fw, fh):
    a = a.cpu().numpy()
    return (a.view(np.uint16) if out_type == U16 else a).reshape(fh, fw, 3)


def _labels(linear, rotated, out_type):
    names = ["gofloat", "demosaic", "rotatecrop", "to_lab", "basecurve", "from_lab"] + ([] if linear else ["gamma"])
    if rotated:
        names.append("transform" if out_type == F32 else "quantise+transform")
    elif out_type != F32:
        names.append("quantise")
    return names


def _entry_ptr(ipa, cache, key):
    p, w, h, c, m = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    assert ipa.lib().ipk_cache_get(cache.handle, key, C.byref(p), C.byref(w), C.byref(h), C.byref(c), C.byref(m)) == 0
    return p.value


@pytest.mark.parametrize("out_type", [F32, U8])
def test_an_active_rotatecrop_through_both_drivers(ipa, orc, out_type):
    """the one op the matrix below leaves a no-op: a crop with an angle on the plain mosaic, its buffer a new one under its own key"""
    w, h = 40, 30
    rc = tuple(float(np.float32(v)) for v in (0.1, 0.05, 0.08, 0.12, 0.3))
    ops = dict(points=CURVES["two"], exposure=0.0, linear=False, rotation=1, rotatecrop=rc)
    pipe, desc = _build(ipa, orc, "bayer_plain", w, h, ops)
    code = CODES[out_type]
    _, (fw, fh) = pipe.sizes()
    want = sp._want(orc, desc(), out_type)
    assert want.shape == (fh, fw, 3) and (fw, fh) != (h, w)
    sp._same(sp._out(pipe, out_type), want, "ipk_pipeline_run")
    cache = ipa.PipelineCache(1 << 26)
    try:
        hs = pipe.hashes(code)
        cold, _, _ = pipe._run(code, cache=cache)
        sp._same(_shape(cold, out_type, fw, fh), want, "cold cache")
        assert pipe.last_ops_run == 0xFF and all(cache.contains(k) for k in hs)
        assert _entry_ptr(ipa, cache, hs[2]) != _entry_ptr(ipa, cache, hs[1])
        warm, _, _ = pipe._run(code, cache=cache)
        sp._same(_shape(warm, out_type, fw, fh), want, "warm cache")
        assert pipe.last_ops_run == 0
    finally:
        cache.close()
    _, stages = pipe.run_timed(code)
    assert [name for name, _ in stages] == _labels(False, True, out_type), stages


@pytest.mark.parametrize("size", SIZES, ids=["%dx%d" % s for s in SIZES])
@pytest.mark.parametrize("source", SOURCES)
def test_the_two_drivers_over_the_switch_matrix(ipa, orc, source, size):
    w, h = size
    one_pass = source == "bayer_one_pass"
    for n, (curve, linear, rotation, out_type) in enumerate(itertools.product(CURVES, (False, True), (0, 1), (F32, U8, U16))):
        ops = dict(points=CURVES[curve], exposure=0.0, linear=linear, rotation=rotation)
        tag = "%s %dx%d curve %s linear %d rotation %d -> %s" % (source, w, h, curve, linear, rotation, out_type)
        code = CODES[out_type]
        pipe, desc = _build(ipa, orc, source, w, h, ops)
        fw, fh = (h, w) if rotation else (w, h)
        assert pipe.sizes()[1] == (fw, fh), tag
        want = sp._want(orc, desc(), out_type)
        fused = pipe.allow_fused
        # output_8bit forces linear = false, output_16bit linear = true (pipeline.rs:405, :452)
        lin = {F32: linear, U8: False, U16: True}[out_type]

        sp._same(sp._out(pipe, out_type), want, tag + ": ipk_pipeline_run")
        assert pipe.last_used_fused is False, tag
        if out_type == F32:
            # the op that writes straight into dst writes nothing else: sentinels on both sides of a destination at an odd float offset
            for allow in sorted({fused, False}):
                pipe.allow_fused = allow
                g = util.Guarded(fw * fh * 3, np.dtype(np.float32), 1 + 2 * (n % 2))
                assert g.ptr % 8 == 4
                pipe.run(out=g.view())
                sp._same(g.result(tag).reshape(fh, fw, 3), want, tag + ": guarded destination, allow_fused %s" % allow)
            pipe.allow_fused = fused

        cache = ipa.PipelineCache(1 << 26)
        try:
            hs = pipe.hashes(code)
            cold, _, _ = pipe._run(code, cache=cache)
            sp._same(_shape(cold, out_type, fw, fh), want, tag + ": cold cache")
            assert pipe.last_ops_run == 0xFF and pipe.last_used_fused is False, (tag, hex(pipe.last_ops_run))
            # every op visited enters the cache under its hash; op 0's buffer never exists where the one pass ran
            assert [cache.contains(k) for k in hs] == [not one_pass] + [True] * 7, tag
            # a no-op's key holds its input's buffer; every other op made one of its own
            noop = {1: source in ("mono_f32", "rgb8_cropped"), 2: True, 3: False, 4: curve == "flat", 5: False, 6: lin, 7: rotation == 0}
            ptrs = [None if (i == 0 and one_pass) else _entry_ptr(ipa, cache, hs[i]) for i in range(8)]
            for i in range(2 if one_pass else 1, 8):
                assert (ptrs[i] == ptrs[i - 1]) == noop[i], (tag, i, ptrs)
            warm, _, _ = pipe._run(code, cache=cache)
            sp._same(_shape(warm, out_type, fw, fh), want, tag + ": warm cache")
            assert pipe.last_ops_run == 0, (tag, hex(pipe.last_ops_run))
        finally:
            cache.close()

        pipe.allow_fused = False
        timed, stages = pipe.run_timed(code)
        assert [name for name, _ in stages] == _labels(lin, rotation == 1, out_type), (tag, stages)
        sp._same(_shape(timed, out_type, fw, fh), want, tag + ": run_timed, allow_fused False")
