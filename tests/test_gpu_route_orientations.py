"""Every one-launch route behind a non-Normal orientation, through every driver that shares the launch-then-orient step (run_route, ipk_api.cpp):
the plain run, the cold cached run, the warm hit, run_region of the whole result and of (3, 5, 17, 9) cut to the image.  The route tests'
test_drivers_agree run the cached driver with a Normal orientation only; here OpTransform is active, so each driver launches into scratch and
permutes.  Bar: bit-exact against the CPU oracle (0 ULP, any NaN == any NaN; equality for u8).  Each case also asserts which route ran:
last_used_fused, last_ops_run, what entered the cache, last_region_windowed, and -- for the three raw routes -- run_timed's stage names.
Frames are 96x120 with odd sensor crops and 131x97: several tiles of every kernel, a partial last one."""
import ctypes as C

import numpy as np
import pytest

import test_gpu_staged_paths as sp
import util
from test_gpu_rotatecrop_fused import R9, SENSOR_CROPS, STAGE as RESAMPLE_STAGE
from test_gpu_scaledown_fused import STAGE as SCALEDOWN_STAGE

pytestmark = pytest.mark.gpu

F32, U8 = sp.F32, sp.U8
NOCROP = (0, 0, 0, 0)
WB4 = (2.0, 1.0, 1.5, 1.3)
RAW_STAGE = "fused gofloat+demosaic+to_lab+basecurve+from_lab+gamma(+transform)"
ORIENTATIONS = {"rot1": dict(rotation=1, fliph=False), "rot2-fliph": dict(rotation=2, fliph=True)}


def _raw(cfa, is_float):
    return dict(cfa=cfa, cpp=1, is_float=is_float, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4)


# name -> (width, height, sensor crops, source (None: an RGB16 raster), ops, Pipeline flags, windowed regions, stage names of a whole f32 run)
ROUTES = {
    "raw": (96, 120, SENSOR_CROPS, _raw("RGGB", False), {}, {}, True, [RAW_STAGE]),
    "raw-four-colour": (96, 120, SENSOR_CROPS, _raw("RGBE", True), {}, dict(fuse_four_colour=True), True, [RAW_STAGE]),
    "resample": (96, 120, SENSOR_CROPS, _raw("GRBG", True), dict(rotatecrop=R9[3]), dict(fuse_rotatecrop=True), True, [RESAMPLE_STAGE]),
    "crop-only": (96, 120, SENSOR_CROPS, _raw("RGGB", False), dict(rotatecrop=R9[1]), dict(fuse_rotatecrop=True), True, [RESAMPLE_STAGE]),
    "scaledown": (131, 97, NOCROP, _raw("RGGB", False), dict(maxwidth=87), dict(fuse_scaledown=True), True, [SCALEDOWN_STAGE, "transform"]),
    "raster": (96, 120, NOCROP, None, {}, {}, False, None),
}
REPORTS = {"raw-four-colour": "fuses_four_colour", "resample": "fuses_rotatecrop", "crop-only": "fuses_rotatecrop", "scaledown": "fuses_scaledown"}


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _case(ipa, orc, route, orientation):
    """(pipeline, a function that builds a fresh oracle descriptor)"""
    w, h, crops, src, ops, flags, _, _ = ROUTES[route]
    ops = dict(ops, **ORIENTATIONS[orientation])
    seed = util.SEED + 14000 + 16 * list(ROUTES).index(route) + list(ORIENTATIONS).index(orientation)
    if src is None:
        data = util.noise_u16(seed, h, w * 3, 65535).reshape(h, w, 3)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(w, h, ipa.upload_u16(data), bits=16))
        sp._apply(pipe, ops)
        pipe.globals.settings.use_fastpath = False
        desc = lambda: orc.make_pipeline(data, use_fastpath=False, **ops)
    else:
        data = util.noise_u16(seed, h, w)
        if src["is_float"]:
            data = data.astype(np.float32) + util.uniform_f32(seed + 1, data.size, -0.5, 0.5).reshape(data.shape)
        wb = WB4 if route == "raw-four-colour" else util.WB   # the fourth colour needs a multiplier of its own
        pipe = sp._pipeline(ipa, data, src, crops, ops, wb=wb)
        desc = lambda: sp._oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=wb, cam_to_xyz_normalized=sp._cam4()))
    for k, v in flags.items():
        setattr(pipe, k, v)
    pipe.window_regions = True
    return pipe, desc


def _np(t, h, w):
    return t.cpu().numpy().reshape(h, w, 3)


@pytest.mark.parametrize("out_type", [F32, U8])
@pytest.mark.parametrize("orientation", list(ORIENTATIONS))
@pytest.mark.parametrize("route", list(ROUTES))
def test_drivers_agree_behind_an_orientation(ipa, orc, route, orientation, out_type):
    pipe, desc = _case(ipa, orc, route, orientation)
    code = {F32: ipa.OUT_F32, U8: ipa.OUT_U8}[out_type]
    one_launch_cached = route != "raster"                     # the cached driver takes the raw routes' one launch; a raster source fills the cache op by op
    tag = "%s %s %s" % (route, orientation, out_type)
    assert pipe.sizes() == orc.pipeline_sizes(desc()), tag
    want = sp._want(orc, desc(), out_type)
    fh, fw = want.shape[:2]
    if route in REPORTS:
        assert getattr(pipe, REPORTS[route])(code) is True, tag
    assert ipa.lib().ipk_pipeline_takes_fastpath(C.byref(pipe.desc()), code) == 0, tag

    sp._same(sp._out(pipe, out_type), want, tag + " run")
    assert pipe.last_used_fused is True, tag + ": the run left the one-launch route"

    cache = ipa.PipelineCache(1 << 28)
    try:
        out, _, _ = pipe._run(code, None, cache)
        sp._same(_np(out, fh, fw), want, tag + " cold cached run")
        assert pipe.last_ops_run == 0xFF and pipe.last_used_fused is one_launch_cached, tag
        hs = pipe.hashes(code)
        assert cache.contains(hs[7]), tag
        if one_launch_cached:
            assert cache.stats()["entries"] == 1 and not any(cache.contains(k) for k in hs[:7]), tag + ": only the final buffer enters the cache"
        else:
            assert cache.contains(hs[0]) and cache.stats()["entries"] > 1, tag
        out, _, _ = pipe._run(code, None, cache)
        sp._same(_np(out, fh, fw), want, tag + " warm hit")
        assert pipe.last_ops_run == 0, tag
    finally:
        cache.close()

    for x, y, w, h in ((0, 0, fw, fh), (3, 5, min(17, fw - 3), min(9, fh - 5))):
        got = _np(pipe.run_region(x, y, w, h, code), h, w)
        assert pipe.last_region_windowed is ROUTES[route][6], "%s region %r" % (tag, (x, y, w, h))
        sp._same(got, want[y:y + h, x:x + w], "%s region %r" % (tag, (x, y, w, h)))


def _timed_region(ipa, pipe, x, y, w, h):
    from imagepipe_amd import _lib
    _lib.check(ipa.lib().ipk_timing_begin(), "ipk_timing_begin")
    pipe.run_region(x, y, w, h)
    arr = (_lib.StageTime * 16)()
    n = C.c_int(0)
    _lib.check(ipa.lib().ipk_timing_end(arr, 16, C.byref(n)), "ipk_timing_end")
    return [arr[i].name.decode() for i in range(min(n.value, 16))]


@pytest.mark.parametrize("route", ["raw", "resample", "scaledown"])
def test_stage_names_behind_an_orientation(ipa, orc, route):
    """scaledown marks its stage and then "transform"; raw and resample show one label ending in "(+transform)"; a windowed region shows one
    "fused region ..." label and no "region copy" """
    pipe, desc = _case(ipa, orc, route, "rot1")
    out, stages = pipe.run_timed()
    assert [s[0] for s in stages] == ROUTES[route][7] and all(s[1] > 0.0 for s in stages), stages
    want = orc.pipeline_run(desc())
    util.assert_bits_equal(out.cpu().numpy().reshape(want.shape), want, route + " timed run")
    names = _timed_region(ipa, pipe, 3, 5, 17, 9)
    assert names == ["fused region " + ROUTES[route][7][0][len("fused "):] + ("" if route != "scaledown" else "(+transform)")], names
