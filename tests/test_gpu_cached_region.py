"""ipk_pipeline_run_cached_region on the GPU: every region is bit for bit the same rectangle of the CPU oracle's pipeline_run / output_8bit /
output_16bit, computed by ONE gather launch over the buffer memoised behind OpRotateCrop; what enters the cache, what is launched, and that nothing
outside the destination is written."""
import re

import numpy as np
import pytest

import util
from util import assert_bits_equal

pytestmark = pytest.mark.gpu

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
CROPS = (1, 3, 2, 5)
F32, U8, U16 = 0, 1, 2
GATHER_F32_SMALL = r"^ipk::k_pointwise_chain_small\[.*gather=1\]$"
GATHER_F32_LONG = r"^ipk::k_pointwise_chain<false>\[.*gather=1\]$"
GATHER_U8 = r"^ipk::k_raster_chain<ipk::Rgbe32, 1>\[.*gather=1\]$"


@pytest.fixture(scope="module")
def ipa():
    import torch
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _raw_pipe(ipa, data, cfa, is_float, crops=CROPS, cpp=1):
    import torch
    h, w = data.shape[:2]
    dev = torch.from_numpy(np.ascontiguousarray(data, np.float32).ravel()).cuda() if is_float else ipa.upload_u16(data)
    return ipa.Pipeline.new_from_source(ipa.RawImage(width=w, height=h, data=dev, cfa=cfa, is_float=is_float, crops=crops, cpp=cpp,
                                                     blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                                                     cam_to_xyz_normalized=util.cam_matrix()))


def _build(ipa, orc, kind, sw=342, sh=75, seed=0, crops=CROPS, **ops):
    """(pipeline, oracle descriptor) of one source kind; ops: exposure, rotation, fliph, flipv, maxwidth, rotatecrop"""
    import torch
    raw = util.noise_u16(util.SEED + 15000 + seed, sh, sw)
    okw = dict(crops=crops, **ops)
    if kind == "rgb8":
        data = (util.noise_u16(util.SEED + 15001 + seed, sh, sw * 3) & 255).astype(np.uint8).reshape(sh, sw, 3)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(sw, sh, torch.from_numpy(data.ravel()).cuda(), bits=8))
        g = pipe.ops.gofloat
        g.crop_top, g.crop_right, g.crop_bottom, g.crop_left = crops
        ops.setdefault("exposure", 0.5); okw["exposure"] = ops["exposure"]                       # not the default ops: no fast path
        desc = orc.make_pipeline(data, **okw)
    else:
        cfa = {"rggb_u16": "RGGB", "xtrans_f32": XT, "rgbe_u16": "RGBE", "mono_u16": "", "rggb_f32": "RGGB"}[kind]
        is_float = kind.endswith("f32")
        data = raw.astype(np.float32) if is_float else raw
        pipe = _raw_pipe(ipa, data, cfa, is_float, crops)
        desc = orc.make_pipeline(data, cfa=orc.cfa_shift(cfa, crops[3], crops[0]) if cfa else "", blacklevels=[util.BLACK] * 4,
                                 whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), **okw)
    _apply(pipe, ops)
    return pipe, desc


def _apply(pipe, ops):
    for k, v in ops.items():
        if k == "exposure":
            pipe.ops.basecurve.exposure = v
        elif k in ("rotation", "fliph", "flipv"):
            setattr(pipe.ops.transform, k, v)
        elif k == "maxwidth":
            pipe.globals.settings.maxwidth = v
        elif k == "rotatecrop":
            rc = pipe.ops.rotatecrop
            rc.crop_top, rc.crop_right, rc.crop_bottom, rc.crop_left, rc.rotation = v
        else:
            raise KeyError(k)


def _want(orc, desc, out_type):
    return [orc.pipeline_run, orc.pipeline_output_8bit, orc.pipeline_output_16bit][out_type](desc)


def _host(t, out_type, h, w):
    a = t.cpu().numpy()
    if out_type == U16:
        a = a.view(np.uint16)
    return a.reshape(h, w, 3)


def _same(got, want, out_type, what):
    if out_type == F32:
        assert_bits_equal(got, want, what)
    else:
        assert got.shape == want.shape and np.array_equal(got, want), what


def _check(ipa, pipe, cache, want, out_type, regions, windowed=True):
    import torch
    for x, y, w, h in regions:
        got = pipe.run_region(x, y, w, h, out_type, cache=cache)
        torch.cuda.synchronize()
        assert pipe.last_region_windowed == windowed, (x, y, w, h)
        _same(_host(got, out_type, h, w), want[y:y + h, x:x + w], out_type, "region %r out %d" % ((x, y, w, h), out_type))


def _strip_regions(fw, fh):
    """widths around the launches' geometry (4-pixel lanes, 64-pixel strides, 128- / 256-pixel chunks) at odd and even offsets, touching each edge;
    pixel counts 1, 255, 256, 257 (the quantised launch's floor) and the whole area"""
    out = [(0, 0, 1, 1), (fw - 1, fh - 1, 1, 1), (7, 3, 255, 1), (10, 4, 256, 1), (1, fh - 1, 257, 1), (0, 0, 51, 5), (fw - 64, 1, 64, 4), (0, 0, fw, fh)]
    rows = [(0, 5), (fh - 3, 3), (11, 17), (1, 1), (0, fh)]
    for i, wd in enumerate([1, 2, 3, 4, 5, 63, 255, 256, 257, 300]):
        for j, x in enumerate([0, fw - wd, 7, 10, (fw - wd) // 2 | 1]):
            if 0 <= x and x + wd <= fw:
                y, h = rows[(i + j) % len(rows)]
                out.append((x, y, wd, h))
    return out


@pytest.mark.parametrize("kind", ["rggb_u16", "xtrans_f32", "rgbe_u16", "mono_u16", "rgb8"])
def test_strip_geometry_regions_all_outputs(ipa, orc, kind):
    pipe, desc = _build(ipa, orc, kind, sw=341 if kind == "rggb_u16" else 342, seed=1)
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    regions = _strip_regions(fw, fh)
    assert {1, 255, 256, 257, fw * fh} <= {w * h for _, _, w, h in regions}
    for out_type in (F32, U8, U16):
        _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, regions)
    if kind == "mono_u16":
        assert cache.get(pipe.hashes()[2]) is not None
    cache.close()


ORIENTS = [(r, f) for r in range(4) for f in (False, True)]


@pytest.mark.parametrize("rot,fliph", ORIENTS)
def test_all_orientations(ipa, orc, rot, fliph):
    pipe, desc = _build(ipa, orc, "rggb_u16", seed=2, rotation=rot, fliph=fliph)
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    regions = [(0, 0, fw, fh), (3, 5, 41, 30), (fw - 33, fh - 21, 33, 21), (fw - 1, 0, 1, fh), (0, fh - 1, 5, 1)]
    for out_type in (F32, U8, U16):
        _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, regions)
        assert pipe.last_ops_run & 0x80 == (0 if (rot, fliph) == (0, False) else 0x80)
    cache.close()


@pytest.mark.parametrize("ops", [dict(rotatecrop=(0.1, 0.05, 0.2, 0.0, 0.3), rotation=1), dict(maxwidth=30, rotation=3, fliph=True)], ids=["angle", "maxwidth"])
def test_rotatecrop_angle_and_scaled_one_pass(ipa, orc, ops):
    pipe, desc = _build(ipa, orc, "rggb_u16", seed=3, **ops)
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    regions = [(0, 0, fw, fh), (1, 2, fw - 3, fh - 4), (fw - 1, fh - 1, 1, 1), (2, 1, 7, 40)]
    for out_type in (F32, U8, U16):
        _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, [r for r in regions if r[0] + r[2] <= fw and r[1] + r[3] <= fh])
    if "maxwidth" in ops:                                                    # gofloat + demosaic as the one scaling pass: op 0's buffer never exists
        assert (fw, fh) == (30, 139)                                         # (the transposed width is what maxwidth limits: scale 2.4)
        for out_type in (F32, U8, U16):
            assert [cache.contains(k) for k in pipe.hashes(out_type)[:3]] == [False, True, True]
    cache.close()


def test_special_values(ipa, orc):
    """util.SPECIALS and lone +-inf / NaN samples in an f32 mosaic: the region's own samples come out as the oracle's, and the specials that lie
    next to a region's border (in the mosaic and, through demosaic's one-pixel reach, in the buffer the launch reads) do not leak in"""
    import torch
    sw, sh = 342, 75
    raw = util.noise_u16(util.SEED + 15004, sh, sw).astype(np.float32)
    with np.errstate(over="ignore"):                                         # 3.4e38 * white is one more +inf
        raw[20:22, :] = np.resize(util.SPECIALS * np.float32(util.WHITE), 2 * sw).reshape(2, sw)
    x, y, w, h = 101, 31, 130, 20                                            # region of the result; the crop shifts it by (5, 1) in the sensor
    for k, v in enumerate([np.inf, -np.inf, np.nan]):
        raw[y + 1 - 2, x + 5 + 9 * k] = v; raw[y + 1 + h + 1, x + 5 + 11 * k] = v; raw[y + 1 + 3 * k, x + 5 - 2] = v; raw[y + 1 + 2 * k, x + 5 + w + 1] = v
        raw[y + 1 + 5 + k, x + 5 + 40 + 30 * k] = v
    for ops in (dict(), dict(rotation=1)):
        pipe = _raw_pipe(ipa, raw, "RGGB", True)
        _apply(pipe, ops)
        desc = orc.make_pipeline(raw, cfa=orc.cfa_shift("RGGB", CROPS[3], CROPS[0]), crops=CROPS, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                                 wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), **ops)
        _, (fw, fh) = pipe.sizes()
        cache = ipa.PipelineCache(1 << 28)
        # Normal: the region the specials surround, the rows of util.SPECIALS, the whole result; Rotate90: the same pixels as columns
        regions = [(x, y, w, h), (0, 15, fw, 9), (0, 0, fw, fh)] if not ops else [(fw - y - h, x, h, w), (3, 7, 41, 200), (0, 0, fw, fh)]
        for out_type in (F32, U8, U16):
            _check(ipa, pipe, cache, _want(orc, desc, out_type), out_type, regions)
        cache.close()


def _keys(cache, hs):
    return [cache.contains(k) for k in hs]


@pytest.mark.parametrize("out_type", [F32, U8])
def test_cache_contract_and_launches(ipa, orc, out_type):
    import torch
    pipe, desc = _build(ipa, orc, "rggb_u16", seed=5, rotation=2)
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    reg = (5, 3, 301, 41)
    x, y, w, h = reg
    # an empty cache: ops 0..2 over the whole frame, stored as ipk_pipeline_run_cached stores them; nothing of the rectangle is stored
    want = _want(orc, desc, out_type)
    _check(ipa, pipe, cache, want, out_type, [reg])
    hs = pipe.hashes(out_type)
    assert _keys(cache, hs) == [True, True, True, False, False, False, False, False]
    assert pipe.last_ops_run == 0xFF                                         # curve, gamma (u8 forces it; f32: linear is off) and a 180-degree transform all run
    rgbe = cache.get(hs[2])
    assert rgbe.shape == (fh, fw, 4)
    before = cache.stats()
    assert before["entries"] == 3
    # an exposure edit: nothing whole-frame runs, ONE launch, the cache keeps its entries
    pipe.ops.basecurve.exposure = 0.3
    desc.exposure = 0.3
    want = _want(orc, desc, out_type)
    with ipa.launch_log() as ran:
        got = pipe.run_region(x, y, w, h, out_type, cache=cache)
        torch.cuda.synchronize()
    _same(_host(got, out_type, h, w), want[y:y + h, x:x + w], out_type, "after the edit")
    assert pipe.last_ops_run & 7 == 0 and pipe.last_ops_run == 0xF8 and pipe.last_region_windowed
    assert len(ran) == 1 and re.match(GATHER_F32_SMALL if out_type == F32 else GATHER_U8, next(iter(ran))), sorted(ran)
    after = cache.stats()
    assert (after["entries"], after["bytes"]) == (before["entries"], before["bytes"]) and after["hits"] > before["hits"]
    hs = pipe.hashes(out_type)
    assert _keys(cache, hs) == [True, True, True, False, False, False, False, False]
    # no-ops of the reference are not counted: no curve, linear, no transform
    pipe.ops.basecurve.exposure, pipe.ops.basecurve.points = 0.0, []
    pipe.ops.transform.rotation = 0
    pipe.globals.settings.linear = True
    pipe.run_region(x, y, w, h, out_type, cache=cache)
    # f32: `linear` is part of the settings every hash covers, so ops 0..2 run again (0x07) beside to_lab and from_lab; output_8bit forces the gamma
    # whatever the setting says, its hashes stand and only the rectangle's ops run
    assert pipe.last_ops_run == (0x2F if out_type == F32 else 0x68)
    cache.close()


def test_small_u8_region_takes_the_f32_launch_and_the_quantiser(ipa, orc):
    import torch
    pipe, desc = _build(ipa, orc, "rggb_u16", seed=6, fliph=True)
    cache = ipa.PipelineCache(1 << 28)
    pipe.run_region(0, 0, 4, 4, U8, cache=cache)                             # fills the cache
    x, y, w, h = 9, 4, 51, 5                                                 # 255 pixels
    with ipa.launch_log() as ran:
        got = pipe.run_region(x, y, w, h, U8, cache=cache)
        torch.cuda.synchronize()
    assert pipe.last_region_windowed and pipe.last_ops_run & 7 == 0
    assert len(ran) == 2 and any(re.match(GATHER_F32_SMALL, e) for e in ran) and any(e.startswith("ipk::k_output8") for e in ran), sorted(ran)
    assert np.array_equal(_host(got, U8, h, w), orc.pipeline_output_8bit(desc)[y:y + h, x:x + w])
    cache.close()


@pytest.mark.parametrize("out_type", [F32, U8, U16])
def test_final_buffer_memoised_is_cut_not_launched(ipa, orc, out_type):
    import torch
    pipe, desc = _build(ipa, orc, "rggb_u16", seed=7, rotation=1)
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    whole, _, _ = pipe._run(out_type, cache=cache)                           # the whole run(cache): hash 7 is memoised
    torch.cuda.synchronize()
    want = _want(orc, desc, out_type)
    _same(_host(whole, out_type, fh, fw), want, out_type, "whole cached run")
    before = cache.stats()
    for x, y, w, h in [(3, 5, 41, 100), (0, 0, fw, fh), (fw - 1, fh - 1, 1, 1)]:
        with ipa.launch_log() as ran:
            got = pipe.run_region(x, y, w, h, out_type, cache=cache)
            torch.cuda.synchronize()
        assert not any("gather=1" in e for e in ran), sorted(ran)
        assert not pipe.last_region_windowed and pipe.last_ops_run == 0
        _same(_host(got, out_type, h, w), want[y:y + h, x:x + w], out_type, "cut from the final buffer")
    after = cache.stats()
    assert (after["entries"], after["bytes"]) == (before["entries"], before["bytes"])
    cache.close()


@pytest.mark.parametrize("out_type", [U8, U16])
def test_fast_path_descriptor_is_cut_from_the_fast_path_result(ipa, orc, out_type):
    """an RGB8 raster with the default ops and use_fastpath: the reference returns before it consults the cache, so the region is the rectangle of the
    integer fast path's result and nothing enters the cache"""
    import torch
    sw, sh = 91, 61
    img = (util.noise_u16(util.SEED + 15010, sh, sw * 3) & 255).astype(np.uint8).reshape(sh, sw, 3)
    pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(sw, sh, torch.from_numpy(img.ravel()).cuda(), bits=8))
    pipe.globals.settings.use_fastpath = True
    assert ipa.lib().ipk_pipeline_takes_fastpath(pipe.desc(), out_type) == 1
    want = _want(orc, orc.make_pipeline(img, use_fastpath=True), out_type)
    assert want.shape == (sh, sw, 3)
    cache = ipa.PipelineCache(1 << 28)
    for x, y, w, h in [(0, 0, 1, 1), (7, 3, 41, 30), (sw - 1, sh - 1, 1, 1), (0, 0, sw, sh)]:
        got = pipe.run_region(x, y, w, h, out_type, cache=cache)
        torch.cuda.synchronize()
        assert not pipe.last_region_windowed and pipe.last_ops_run == 0, (x, y, w, h)
        _same(_host(got, out_type, h, w), want[y:y + h, x:x + w], out_type, "fast-path region %r out %d" % ((x, y, w, h), out_type))
    assert cache.stats()["entries"] == 0
    cache.close()


def test_run_cached_after_regions_is_unchanged(ipa, orc):
    import torch
    pipe, desc = _build(ipa, orc, "xtrans_f32", seed=8, rotation=3)
    _, (fw, fh) = pipe.sizes()
    cache = ipa.PipelineCache(1 << 28)
    want = orc.pipeline_run(desc)
    _check(ipa, pipe, cache, want, F32, [(0, 0, 30, 20), (fw - 9, 2, 9, 200)])
    _check(ipa, pipe, cache, orc.pipeline_output_8bit(desc), U8, [(1, 1, 40, 40)])
    whole, _, _ = pipe._run(F32, cache=cache)
    torch.cuda.synchronize()
    assert_bits_equal(_host(whole, F32, fh, fw), want, "ipk_pipeline_run_cached after the region calls")
    assert pipe.last_ops_run == 0xF8                                         # resumed behind rotatecrop: ops 3..7, its usual mask
    assert all(cache.contains(k) for k in pipe.hashes())
    cache.close()


def test_long_form_whole_area(ipa):
    """above launch_pointwise_chain's switch to the four-pixel form: the region is the whole result, against ipk_pipeline_run_cached's staged kernels"""
    import torch
    W, H = 3072, 2100
    cus = ipa.lib().ipk_device_cus()
    threshold = cus * 16 * 256 * 6
    if W * H < threshold:
        pytest.skip("this device has %d CUs: the long form starts at %d pixels, the frame has %d" % (cus, threshold, W * H))
    g = torch.Generator(device="cuda"); g.manual_seed(util.SEED)
    data = torch.randint(0, 16384, (H * W,), device="cuda", generator=g, dtype=torch.int32).to(torch.float32)
    pipe = ipa.Pipeline.new_from_source(ipa.RawImage(width=W, height=H, data=data, cfa="RGGB", is_float=True, blacklevels=[util.BLACK] * 4,
                                                     whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix()))
    cache = ipa.PipelineCache(1 << 31)
    for rot in (0, 1):
        pipe.ops.transform.rotation = rot
        _, (fw, fh) = pipe.sizes()
        with ipa.launch_log() as ran:
            got = pipe.run_region(0, 0, fw, fh, F32, cache=cache)
            torch.cuda.synchronize()
        assert pipe.last_region_windowed
        assert any(re.match(GATHER_F32_LONG, e) for e in ran) and not any("k_pointwise_chain_small" in e for e in ran), sorted(ran)
        whole, _, _ = pipe._run(F32, cache=cache)                            # resumes behind rotatecrop: to_lab .. transform as staged kernels
        torch.cuda.synchronize()
        assert pipe.last_ops_run == (0xF8 if rot == 0 else 0x80)             # Rotate90 finds the gamma buffer of the run before it: k_rotate alone
        assert torch.equal(whole.view(torch.int32), got.view(torch.int32)), rot
        del whole, got
    cache.close()


@pytest.mark.parametrize("out_type,off,reg", [(U8, 3, (7, 3, 51, 7)), (F32, 1, (1, 2, 63, 11))])
def test_nothing_outside_the_destination_is_written(ipa, orc, out_type, off, reg):
    import torch
    pipe, desc = _build(ipa, orc, "rggb_u16", seed=9, rotation=1, fliph=True)
    cache = ipa.PipelineCache(1 << 28)
    x, y, w, h = reg
    g = util.Guarded(w * h * 3, torch.uint8 if out_type == U8 else torch.float32, off=off)
    pipe.run_region(x, y, w, h, out_type, out=g.view(), cache=cache)
    torch.cuda.synchronize()
    got = g.result("region %r" % (reg,)).reshape(h, w, 3)
    _same(got, _want(orc, desc, out_type)[y:y + h, x:x + w], out_type, "guarded destination")
    cache.close()
