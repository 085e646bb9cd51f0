"""GPU parity of ipk_plain_to_srgb -- the rectangle and raw-level modes of k_raster_chain<uint8_t | uint16_t, OUT> -- and of the route that uses it
under IPK_FUSED_PLAIN (Pipeline.fuse_plain): cropped RGB8 / RGB16 rasters, u16 monochrome and three-sample raws as one launch, regions of every
frame on that launch windowed.  Bar: bit-exact against the CPU oracle (f32 bit patterns, any NaN == any NaN; equal u8 / u16).  At the C ABI the
reference is the oracle's gofloat + point-wise stages on the rectangle; at pipeline level the oracle's pipeline and the staged route.  Every case
asserts by the launch log which kernel ran, with which mode keys, and that nothing else did."""
import ctypes as C

import numpy as np
import pytest

import util
import test_gpu_staged_paths as sp
from test_gpu_staged_paths import F32, U8, U16

pytestmark = pytest.mark.gpu

UNSUPPORTED, INVALID = -5, -2
RASTER, RGB, MONO = 0, 1, 2                                               # ipk_plain_kind
KINDS = ("rgb8", "rgb16", "cpp3", "mono")
KIND_OF = {"rgb8": RASTER, "rgb16": RASTER, "cpp3": RGB, "mono": MONO}
SRC_TYPE = {"rgb8": 2, "rgb16": 3, "cpp3": 0, "mono": 0}
SYMBOL = {"rgb8": "unsigned char", "rgb16": "unsigned short", "cpp3": "unsigned short", "mono": "unsigned short"}
NP_OUT = [np.dtype(np.float32), np.dtype(np.uint8), np.dtype(np.uint16)]
CODES = {F32: 0, U8: 1, U16: 2}
B3, W3 = (64.0, 128.0, 256.0, 0.0), (1023.0, 4095.0, 16383.0, 0.0)        # a three-sample raw's levels: different per channel
BM, WM = (util.BLACK,) * 4, (util.WHITE,) * 4
CURVE_GRID = [(0.2, 0.1), (0.4, 0.5), (0.6, 0.55), (0.8, 0.9)]            # six knots with the end points, one per grid cell at most
CURVE7 = [(0.1, 0.07), (0.25, 0.2), (0.3, 0.33), (0.5, 0.6), (0.7, 0.78), (0.85, 0.9), (0.9, 0.93)]
CURVES = {"none": [], "one": [(0.5, 0.6)], "grid": CURVE_GRID, "seven": CURVE7}


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _fa(v):
    v = [float(x) for x in np.asarray(v, np.float32).ravel()]
    return (C.c_float * max(1, len(v)))(*v)


def _image(kind, h, w, seed):
    """noise over the whole range of the element type: a raw's samples lie below its black level and above its white level, too"""
    if kind == "rgb8":
        return (util.splitmix64(seed, h * w * 3) & np.uint64(255)).astype(np.uint8).reshape(h, w, 3)
    if kind == "mono":
        return util.noise_u16(seed, h, w, 20000)
    return util.noise_u16(seed, h, w * 3, 65535 if kind == "rgb16" else 20000).reshape(h, w, 3)


def _levels(kind):
    return (BM, WM) if kind == "mono" else (B3, W3)


def _gofloat(orc, kind, img, x, y, w, h, levels=None):
    b, wh = levels or _levels(kind)
    with np.errstate(all="ignore"):
        if kind == "mono":
            return orc.gofloat_mono(img, x, y, w, h, b[0], wh[0])
        if kind == "cpp3":
            return orc.gofloat_rgb(img, x, y, w, h, b, wh)
        return orc.gofloat_other(img, x, y, w, h)


def _pointwise(orc, kind, buf4, cm, points, exposure, linear, out):
    with np.errstate(all="ignore"):
        want = orc.gamma(orc.fromlab(orc.basecurve(orc.tolab(buf4, util.WB, cm, monochrome=kind == "mono"), exposure, points)), linear)
    return want if out == 0 else (orc.output8bit(want) if out == 1 else orc.output16bit(want))


def _source(kind, img, off):
    """the image in a guarded allocation, `off` elements past a 256-byte boundary"""
    import torch
    g = util.Guarded(img.size, img.dtype, off)
    flat = np.ascontiguousarray(img).ravel()
    g.view().copy_(torch.from_numpy(flat.view(np.int16) if flat.dtype == np.uint16 else flat))
    return g


def _tag(kind, out, w, ow, fast_ok=1):
    keys = ["fast_ok=%d" % fast_ok] + (["rect=1"] if w != ow else []) + (["levels=%d" % KIND_OF[kind]] if KIND_OF[kind] else [])
    return "ipk::k_raster_chain<%s, %d>[%s]" % (SYMBOL[kind], out, ",".join(keys))


def _plain(ipa, kind, src_ptr, ow, x, y, w, h, cm, points, exposure, linear, out, dst_ptr, levels=None, src_type=None):
    b, wh = levels or _levels(kind)
    pts = [c for p in points for c in p]
    return ipa.lib().ipk_plain_to_srgb(src_ptr, SRC_TYPE[kind] if src_type is None else src_type, KIND_OF[kind], ow, x, y, w, h, _fa(b), _fa(wh), _fa(util.WB), _fa(cm),
                                       exposure, _fa(pts), len(points), int(linear), out, dst_ptr, None)


def _run_rect(ipa, orc, kind, img, x, y, w, h, out, tag, points=((0.5, 0.6),), exposure=0.0, linear=False, cm=None, fast_ok=1, off=1, want=None, levels=None):
    """one call over the rectangle: guarded source and destination, the one log entry, the oracle's stages on the rectangle"""
    import torch
    cm = util.cam_matrix() if cm is None else cm
    points = list(points)
    oh, ow = img.shape[:2]
    src = _source(kind, img, off)
    dst = util.Guarded(w * h * 3, NP_OUT[out], off)
    with ipa.launch_log() as ran:
        rc = _plain(ipa, kind, src.ptr, ow, x, y, w, h, cm, points, exposure, linear, out, dst.ptr, levels)
        assert rc == 0, (tag, ipa.lib().ipk_last_error())
        torch.cuda.synchronize()
    assert ran == {_tag(kind, out, w, ow, fast_ok)}, (tag, sorted(ran))
    got = dst.result(tag).reshape(h, w, 3)
    assert np.array_equal(src.result(tag + " (source)"), np.ascontiguousarray(img).ravel()), tag + ": the source was written"
    if want is None:
        want = _pointwise(orc, kind, _gofloat(orc, kind, img, x, y, w, h, levels), cm, points, exposure, linear, out)
    sp._same(got, want, tag)
    return got


# ---------------------------------------------------------------------------------------------
# rectangle geometry at the C ABI
# ---------------------------------------------------------------------------------------------
RECTS = [(1, 256), (2, 129), (3, 86), (4, 65), (5, 52), (63, 5), (64, 4), (65, 4), (255, 2), (256, 1), (257, 1), (300, 7)]


@pytest.mark.parametrize("rect", RECTS, ids=["%dx%d" % r for r in RECTS])
def test_rectangles_vs_oracle(ipa, orc, rect):
    """every source kind on every rectangle, at odd x, y = 3, in a source of odd pitch x + w + 5 that starts one element past a 256-byte boundary; the
    output type rotates with the kind and the rectangle"""
    w, h = rect
    x, y = 7, 3
    ow, oh = x + w + 5, y + h + 2
    for k, kind in enumerate(KINDS):
        img = _image(kind, oh, ow, util.SEED + 15000 + 8 * RECTS.index(rect) + k)
        out = (RECTS.index(rect) + k) % 3
        _run_rect(ipa, orc, kind, img, x, y, w, h, out, "%s %dx%d at (%d, %d) of %d -> %s" % (kind, w, h, x, y, ow, NP_OUT[out]))


@pytest.mark.parametrize("kind", KINDS)
def test_a_full_width_rectangle_is_the_flat_walk(ipa, orc, kind):
    """x = 0, w = owidth = 300, y = 2: an offset pointer -- no rect key; a raster's entry is ipk_raster_to_srgb's own"""
    img = _image(kind, 11, 300, util.SEED + 15200 + len(kind))
    for out in (0, 1, 2):
        _run_rect(ipa, orc, kind, img, 0, 2, 300, 7, out, "%s contiguous -> %s" % (kind, NP_OUT[out]), off=0)
        _run_rect(ipa, orc, kind, img, 0, 2, 300, 7, out, "%s contiguous, odd base -> %s" % (kind, NP_OUT[out]), off=1)


@pytest.mark.parametrize("npix", [256, 257, 511, 512, 513])
def test_one_row_rectangles_around_the_chunk_size(ipa, orc, npix):
    """the shifted last chunk: one row of npix pixels inside a wider row (rectangle mode) and as the whole row (flat)"""
    for k, kind in enumerate(KINDS):
        img = _image(kind, 3, npix + 9, util.SEED + 15300 + npix + k)
        _run_rect(ipa, orc, kind, img, 5, 1, npix, 1, (npix + k) % 3, "%s one row of %d in %d" % (kind, npix, npix + 9))
        _run_rect(ipa, orc, kind, img[:, :npix], 0, 2, npix, 1, (npix + k + 1) % 3, "%s one whole row of %d" % (kind, npix))


def test_more_chunks_than_waves(ipa, orc):
    """1061 x 1031 mono u16 -> u8 out of a 1073-wide frame: 4273 chunks of 256 pixels, more than the 4096 waves of a 256-block launch"""
    w, h, x, y = 1061, 1031, 7, 3
    img = _image("mono", h + 5, w + 12, util.SEED + 15400)
    assert (w * h + 255) // 256 > 256 * 16
    _run_rect(ipa, orc, "mono", img, x, y, w, h, 1, "mono 1061x1031")


# ---------------------------------------------------------------------------------------------
# sample values
# ---------------------------------------------------------------------------------------------
_ALL = {}


def _all_values(orc, kind):
    """(image, its gofloat buffer): mono 256 x 256 holds every u16 value once; cpp3 256 x 258 every value in every channel (each at its own pixel)"""
    if kind not in _ALL:
        v = np.arange(65536, dtype=np.uint32)
        if kind == "mono":
            img = ((v * 40503) & 0xFFFF).astype(np.uint16).reshape(256, 256)          # an odd multiplier: a permutation of the values
            assert np.unique(img).size == 65536
        else:
            n = 256 * 258
            i = np.arange(n, dtype=np.uint32)
            img = np.stack([((i * 40503 + c * 21845) & 0xFFFF) for c in range(3)], axis=1).astype(np.uint16).reshape(258, 256, 3)
            assert all(np.unique(img[:, :, c]).size == 65536 for c in range(3))
        h, w = img.shape[:2]
        buf = _gofloat(orc, kind, img, 0, 0, w, h)
        assert (buf[:, :, :3] < 0).any() and (buf[:, :, :3] == 1.0).any() and not buf[:, :, 3].any(), "samples below black and above white are present"
        _ALL[kind] = (img, buf)
    return _ALL[kind]


@pytest.mark.parametrize("curve", list(CURVES))
@pytest.mark.parametrize("kind", ["mono", "cpp3"])
def test_every_sample_value(ipa, orc, kind, curve):
    img, buf = _all_values(orc, kind)
    h, w = img.shape[:2]
    cm = util.cam_matrix()
    for out in (0, 1, 2):
        for linear in (False, True):
            want = _pointwise(orc, kind, buf, cm, CURVES[curve], 0.0, linear, out)
            _run_rect(ipa, orc, kind, img, 0, 0, w, h, out, "%s all values, curve %s, linear %d -> %s" % (kind, curve, linear, NP_OUT[out]),
                      points=CURVES[curve], linear=linear, want=want, off=0)


@pytest.mark.parametrize("kind", ["mono", "cpp3", "rgb16"])
def test_hostile_and_guarded_matrices(ipa, orc, kind):
    """a matrix entry of 2^21 (PointwisePrep's sane(): fast_ok = 0, every pixel takes the literal form) and one of 2^-13 (ordinary for sane(), fast_ok
    stays 1, the per-pixel guards decide), with an exposure, over every sample value / in rectangle mode.  A monochrome buffer's matrix is the sRGB
    one whatever the caller passes (colorspaces.rs:90-101): its launches keep fast_ok = 1"""
    img = _all_values(orc, kind)[0] if kind != "rgb16" else _image(kind, 40, 77, util.SEED + 15500)
    h, w = img.shape[:2]
    for entry, value, fast_ok in (((1, 1), 2.0 ** 21, 0), ((2, 0), 2.0 ** -13, 1)):
        cm = util.cam_matrix()
        cm[entry] = np.float32(value)
        fast_ok = 1 if kind == "mono" else fast_ok
        for out in (0, 1, 2):
            if kind == "rgb16":
                _run_rect(ipa, orc, kind, img, 3, 1, 71, 33, out, "rgb16 rect matrix %g -> %s" % (value, NP_OUT[out]), exposure=0.7, cm=cm, fast_ok=fast_ok)
            else:
                _run_rect(ipa, orc, kind, img, 0, 0, w, h, out, "%s matrix %g -> %s" % (kind, value, NP_OUT[out]), exposure=0.7, cm=cm, fast_ok=fast_ok, off=0)


@pytest.mark.parametrize("kind", ["mono", "cpp3"])
def test_a_white_level_equal_to_the_black_level_gives_the_staged_result(ipa, orc, kind):
    """range 0: every division is by zero.  ipk_gofloat_mono_u16 / _rgb_u16 accept such levels, so the one launch must give what they and
    ipk_pointwise_chain (+ the quantisation) give"""
    import torch
    L = ipa.lib()
    w, h, x, y, ow = 65, 9, 3, 1, 73
    img = _image(kind, h + 3, ow, util.SEED + 15600)
    img[y + 1, x + 2] = 512
    levels = ((512.0,) * 4, (512.0,) * 4) if kind == "mono" else ((64.0, 512.0, 256.0, 0.0), (1023.0, 512.0, 256.0, 0.0))
    dev = ipa.upload_u16(img)
    buf4 = torch.empty(w * h * 4, dtype=torch.float32, device="cuda")
    if kind == "mono":
        assert L.ipk_gofloat_mono_u16(dev.data_ptr(), ow, x, y, w, h, levels[0][0], levels[1][0], buf4.data_ptr(), None) == 0, L.ipk_last_error()
    else:
        assert L.ipk_gofloat_rgb_u16(dev.data_ptr(), ow, x, y, w, h, _fa(levels[0]), _fa(levels[1]), buf4.data_ptr(), None) == 0, L.ipk_last_error()
    cm = util.cam_matrix()
    for out in (0, 1, 2):
        staged = torch.empty(w * h * 3, dtype=[torch.float32, torch.uint8, torch.int16][out], device="cuda")
        rc = L.ipk_pointwise_chain_out(buf4.data_ptr(), w, h, int(kind == "mono"), _fa(util.WB), _fa(cm), 0.0, _fa([0.5, 0.6]), 1, 0, out, staged.data_ptr(), None)
        assert rc == 0, L.ipk_last_error()
        torch.cuda.synchronize()
        want = staged.cpu().numpy()
        want = (want.view(np.uint16) if out == 2 else want).reshape(h, w, 3)
        _run_rect(ipa, orc, kind, img, x, y, w, h, out, "%s white == black -> %s" % (kind, NP_OUT[out]), want=want, levels=levels)


# ---------------------------------------------------------------------------------------------
# the log of the untouched entry point, and refusals
# ---------------------------------------------------------------------------------------------
def test_raster_to_srgb_keeps_its_log_entry(ipa, orc):
    import torch
    for kind in ("rgb8", "rgb16"):
        img = _image(kind, 7, 333, util.SEED + 15700)
        dev = torch.from_numpy(img.ravel()).cuda() if kind == "rgb8" else ipa.upload_u16(img)
        for out in (0, 1, 2):
            dst = util.Guarded(7 * 333 * 3, NP_OUT[out])
            with ipa.launch_log() as ran:
                rc = ipa.lib().ipk_raster_to_srgb(dev.data_ptr(), SRC_TYPE[kind], 333, 7, _fa(util.WB), _fa(util.cam_matrix()), 0.0, _fa([0.5, 0.6]), 1, 0, out, dst.ptr, None)
                assert rc == 0, ipa.lib().ipk_last_error()
                torch.cuda.synchronize()
            assert ran == {"ipk::k_raster_chain<%s, %d>[fast_ok=1]" % (SYMBOL[kind], out)}, sorted(ran)
            sp._same(dst.result().reshape(7, 333, 3), _pointwise(orc, kind, orc.gofloat_other(img, 0, 0, 333, 7), util.cam_matrix(), [(0.5, 0.6)], 0.0, False, out), kind)


def test_refusals_write_nothing(ipa):
    import torch
    L = ipa.lib()
    src = torch.zeros(64 * 64 * 3, dtype=torch.float32, device="cuda")
    dst = torch.full((64 * 64 * 3,), 7.0, dtype=torch.float32, device="cuda")
    cm = util.cam_matrix()
    with ipa.launch_log() as ran:
        for kind in ("cpp3", "mono"):
            assert _plain(ipa, kind, src.data_ptr(), 64, 0, 0, 64, 64, cm, [], 0.0, False, 0, dst.data_ptr(), src_type=1) == UNSUPPORTED     # IPK_SRC_F32
            assert _plain(ipa, kind, src.data_ptr(), 64, 3, 1, 51, 5, cm, [], 0.0, False, 0, dst.data_ptr()) == UNSUPPORTED                 # 255 pixels
            assert _plain(ipa, kind, src.data_ptr(), 64, 3, 1, 62, 5, cm, [], 0.0, False, 0, dst.data_ptr()) == INVALID                     # x + width > owidth
            assert _plain(ipa, kind, src.data_ptr(), 64, 0, 0, 64, 64, cm, [], 0.0, False, 0, dst.data_ptr(), src_type=2) == INVALID        # a raster type
        for kind in ("rgb8", "rgb16"):
            assert _plain(ipa, kind, src.data_ptr(), 64, 0, 0, 64, 64, cm, [], 0.0, False, 0, dst.data_ptr(), src_type=1) == UNSUPPORTED
            assert _plain(ipa, kind, src.data_ptr(), 64, 3, 1, 51, 5, cm, [], 0.0, False, 0, dst.data_ptr()) == UNSUPPORTED
            assert _plain(ipa, kind, src.data_ptr(), 64, 0, 0, 64, 64, cm, [], 0.0, False, 0, dst.data_ptr(), src_type=0) == INVALID        # a raw type
        assert L.ipk_plain_to_srgb(src.data_ptr(), 0, 3, 64, 0, 0, 64, 64, _fa(BM), _fa(WM), _fa(util.WB), _fa(cm), 0.0, _fa([]), 0, 0, 0, dst.data_ptr(), None) == INVALID
        assert L.ipk_plain_to_srgb(src.data_ptr(), 0, MONO, 64, 0, 0, 64, 64, None, None, _fa(util.WB), _fa(cm), 0.0, _fa([]), 0, 0, 0, dst.data_ptr(), None) == INVALID
        torch.cuda.synchronize()
    assert not ran, sorted(ran)
    assert bool((dst == 7.0).all()), "a refused call wrote to dst"


# ---------------------------------------------------------------------------------------------
# pipeline level
# ---------------------------------------------------------------------------------------------
CROPS = (3, 1, 2, 5)
SOURCES = {"rgb8": None, "rgb16": None, "mono_u16": "mono_u16", "rgb3_u16": "rgb3_u16"}
ORIENTS = {"normal": {}, "rot90-fliph": dict(rotation=1, fliph=True)}


def _build(ipa, orc, name, w, h, seed, ops, crops=CROPS):
    """(pipeline, a maker of fresh oracle descriptors, host data)"""
    import torch
    if name in ("rgb8", "rgb16"):
        data = _image(name, h, w, seed)
        dev = torch.from_numpy(data.ravel()).cuda() if name == "rgb8" else ipa.upload_u16(data)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(w, h, dev, bits=8 if name == "rgb8" else 16))
        g = pipe.ops.gofloat
        g.crop_top, g.crop_right, g.crop_bottom, g.crop_left = crops
        ops = dict(ops, exposure=0.5)                                         # not the default ops: no fast path
        sp._apply(pipe, ops)
        return pipe, (lambda: orc.make_pipeline(data, crops=crops, **ops)), data
    data, src = sp._source(name, h, w, seed)
    pipe = sp._pipeline(ipa, data, src, crops, ops)
    return pipe, (lambda: sp._oracle_desc(orc, data, src, crops, dict(ops, wb_coeffs=util.WB, cam_to_xyz_normalized=sp._cam4()))), data


def _kernels(ran, *parts):
    return sorted(e for e in ran if any(p in e for p in parts))


@pytest.mark.parametrize("orient", list(ORIENTS))
@pytest.mark.parametrize("shape", [(37, 29), (96, 120)], ids=["37x29", "96x120"])
@pytest.mark.parametrize("name", list(SOURCES))
def test_pipeline_vs_oracle_and_staged(ipa, orc, name, shape, orient):
    import torch
    w, h = shape
    pipe, desc, _ = _build(ipa, orc, name, w, h, util.SEED + 15800 + w, ORIENTS[orient])
    for out_type in (F32, U8, U16):
        tag = "%s %dx%d %s %s" % (name, w, h, orient, out_type)
        want = sp._want(orc, desc(), out_type)
        pipe.allow_fused, pipe.fuse_plain = True, True
        assert pipe.fuses_plain(CODES[out_type]), tag
        with ipa.launch_log() as ran:
            got = sp._out(pipe, out_type)
            torch.cuda.synchronize()
        sp._same(got, want, tag + " with the bit")
        assert pipe.last_used_fused is True, tag
        chain = _kernels(ran, "k_raster_chain")
        assert len(chain) == 1 and "Rgbe32" not in chain[0] and ("rect=1" in chain[0]) and not _kernels(ran, "k_gofloat", "k_pointwise_chain"), (tag, sorted(ran))
        assert ("levels=" in chain[0]) == (name in ("mono_u16", "rgb3_u16")), (tag, chain)
        others = sorted(set(ran) - set(chain))
        assert (not others) if orient == "normal" else (len(others) == 1 and "k_rotate" in others[0]), (tag, sorted(ran))
        # without the bit: the staged kernels of today
        pipe.fuse_plain = False
        with ipa.launch_log() as ran0:
            got0 = sp._out(pipe, out_type)
            torch.cuda.synchronize()
        sp._same(got0, want, tag + " without the bit")
        assert pipe.last_used_fused is False and _kernels(ran0, "k_gofloat") and not [e for e in ran0 if "rect=" in e or "levels=" in e], (tag, sorted(ran0))
        assert _kernels(ran0, "k_pointwise_chain", "k_raster_chain<ipk::Rgbe32"), (tag, sorted(ran0))
        # ... and the staged driver
        pipe.allow_fused = False
        sp._same(sp._out(pipe, out_type), want, tag + " allow_fused = False")
        assert pipe.last_used_fused is False


@pytest.mark.parametrize("name", ["mono_f32", "rgb3_f32"])
def test_f32_plain_raws_stay_staged_with_the_bit(ipa, orc, name):
    import torch
    data, src = sp._source(name, 29, 37, util.SEED + 15900)
    pipe = sp._pipeline(ipa, data, src, CROPS, {})
    desc = lambda: sp._oracle_desc(orc, data, src, CROPS, dict(wb_coeffs=util.WB, cam_to_xyz_normalized=sp._cam4()))
    for out_type in (F32, U8, U16):
        logs = []
        for bit in (False, True):
            pipe.fuse_plain = bit
            assert not pipe.fuses_plain()
            with ipa.launch_log() as ran:
                got = sp._out(pipe, out_type)
                torch.cuda.synchronize()
            sp._same(got, sp._want(orc, desc(), out_type), "%s %s bit %d" % (name, out_type, bit))
            assert pipe.last_used_fused is False and _kernels(ran, "k_gofloat") and not [e for e in ran if "rect=" in e or "levels=" in e], sorted(ran)
            logs.append(ran)
            assert pipe.region(0, 0, 20, 20)[0] == 0
        assert logs[0] == logs[1]


def test_cached_and_host_drivers(ipa, orc):
    """the cached driver fills its cache from the staged ops (nothing memoised: every op runs, the result is the oracle's); the host driver reads
    the same route as ipk_pipeline_run"""
    import torch
    from imagepipe_amd import _lib
    pipe, desc, data = _build(ipa, orc, "rgb3_u16", 96, 120, util.SEED + 16000, {})
    pipe.fuse_plain = True
    cache = ipa.PipelineCache(64 << 20)
    try:
        with ipa.launch_log() as ran:
            got = pipe.run(cache=cache).numpy()
            torch.cuda.synchronize()
        sp._same(got, orc.pipeline_run(desc()), "cached")
        assert pipe.last_ops_run == 0xFF and pipe.last_used_fused is False and not [e for e in ran if "levels=" in e], sorted(ran)
    finally:
        cache.close()
    for name in ("mono_u16", "rgb8"):
        pipe, desc, data = _build(ipa, orc, name, 96, 120, util.SEED + 16001, {})
        pipe.fuse_plain = True
        want = orc.pipeline_output_8bit(desc())
        host = np.zeros(want.shape, np.uint8)
        used = C.c_int(-1)
        d = pipe.desc()
        src = np.ascontiguousarray(data)
        with ipa.launch_log() as ran:
            _lib.check(ipa.lib().ipk_host_pipeline_run(C.byref(d), src.ctypes.data, host.ctypes.data, 1, C.byref(used)), "ipk_host_pipeline_run")
        sp._same(host, want, name + " host")
        assert used.value == 1 and len(_kernels(ran, "rect=1")) == 1 and not _kernels(ran, "k_gofloat"), sorted(ran)


# ---------------------------------------------------------------------------------------------
# regions
# ---------------------------------------------------------------------------------------------
def _windows(fw, fh):
    """the corners, a full row and a full column (windowed where they have 256 pixels), an interior 19 x 17, the whole result, a 15 x 15 (route 0)"""
    return [(0, 0, 16, 16), (fw - 17, 0, 17, 16), (0, fh - 16, 16, 16), (fw - 16, fh - 17, 16, 17), (0, fh // 2, fw, 1), (fw // 3, 0, 1, fh),
            (5, 4, 19, 17), (0, 0, fw, fh), (2, 3, 15, 15)]


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (False, True)])
def test_regions_all_orientations(ipa, orc, rot, fh):
    """device and host forms against the rectangle cut from the whole result (itself the oracle's); *windowed equals the plan.  96 x 120 cropped, the
    source kind rotating with the orientation, and a 300 x 40 frame whose full rows (or, transposed, full columns: one-pixel-wide sensor
    rectangles) have 256 pixels and more"""
    import torch
    from imagepipe_amd import _lib
    k = 2 * rot + int(fh)
    names = list(SOURCES)
    for name, (w, h), crops in ((names[k % 4], (96, 120), CROPS), (names[(k + 1) % 4], (300, 40), CROPS), (names[k % 2], (96, 120), (0, 0, 0, 0))):
        pipe, desc, data = _build(ipa, orc, name, w, h, util.SEED + 16100 + k, dict(rotation=rot, fliph=fh), crops)
        pipe.fuse_plain = True
        _, (fw, fhh) = pipe.sizes()
        seen = set()
        for out_type in ((F32, U8, U16)[k % 3], (F32, U8, U16)[(k + 1) % 3]):
            code = CODES[out_type]
            whole = sp._want(orc, desc(), out_type)
            assert whole.shape[:2] == (fhh, fw)
            d = pipe.desc()
            src = np.ascontiguousarray(data)
            for win in _windows(fw, fhh):
                x, y, rw, rh = win
                tag = "%s %dx%d rot %d fliph %d %s region %r" % (name, w, h, rot, fh, out_type, win)
                plan, (sx, sy, sw, sh) = pipe.region(x, y, rw, rh, code)
                assert plan == int(rw * rh >= 256), tag
                seen.add(plan)
                if plan:
                    assert sw * sh == rw * rh and sx >= crops[3] and sy >= crops[0] and sx + sw <= w - crops[1] and sy + sh <= h - crops[2], (tag, sx, sy, sw, sh)
                with ipa.launch_log() as ran:
                    got = pipe.run_region(x, y, rw, rh, code)
                    torch.cuda.synchronize()
                assert pipe.last_region_windowed is bool(plan), tag
                got = got.cpu().numpy()
                sp._same((got.view(np.uint16) if out_type == U16 else got).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw], tag)
                chain = _kernels(ran, "k_raster_chain")
                assert len(chain) == 1 and not _kernels(ran, "k_gofloat", "k_pointwise_chain"), (tag, sorted(ran))
                if plan:
                    assert ("rect=1" in chain[0]) == (sw != w), (tag, chain, (sx, sy, sw, sh))
                host = np.zeros((rh, rw, 3), NP_OUT[code])
                flag = C.c_int(-1)
                _lib.check(ipa.lib().ipk_host_pipeline_run_region(C.byref(d), src.ctypes.data, x, y, rw, rh, host.ctypes.data, code, C.byref(flag)), "ipk_host_pipeline_run_region")
                assert flag.value == plan, tag
                sp._same(host, whole[y:y + rh, x:x + rw], tag + " (host form)")
        assert seen == {0, 1}


def test_region_reads_only_the_reported_rectangle(ipa, orc):
    """everything outside the rectangle ipk_pipeline_region reports is 0xFFFF / 0xFF: the device form on a poisoned frame and the host form, which
    uploads the rectangle's rows alone, give the clean frame's region"""
    import torch
    from imagepipe_amd import _lib
    for name, ops in (("mono_u16", dict(rotation=3)), ("rgb8", {}), ("rgb3_u16", dict(rotation=1, fliph=True))):
        clean, desc, data = _build(ipa, orc, name, 96, 120, util.SEED + 16200, ops)
        clean.fuse_plain = True
        _, (fw, fhh) = clean.sizes()
        whole = sp._want(orc, desc(), U8)
        for win in ((3, 5, 40, 30), (0, 0, 16, 16), (fw - 20, fhh - 20, 20, 20)):
            x, y, rw, rh = win
            plan, (sx, sy, sw, sh) = clean.region(x, y, rw, rh, 1)
            assert plan == 1
            bad = np.full_like(data, 0xFF if data.dtype == np.uint8 else 0xFFFF)
            bad[sy:sy + sh, sx:sx + sw] = data[sy:sy + sh, sx:sx + sw]
            assert not np.array_equal(bad, data)
            dev = torch.from_numpy(bad.ravel()).cuda() if name == "rgb8" else ipa.upload_u16(bad)
            clean.globals.image.data = dev
            got = clean.run_region(x, y, rw, rh, 1)
            torch.cuda.synchronize()
            sp._same(got.cpu().numpy().reshape(rh, rw, 3), whole[y:y + rh, x:x + rw], "%s region %r from a poisoned device frame" % (name, win))
            host = np.zeros((rh, rw, 3), np.uint8)
            flag = C.c_int(-1)
            d = clean.desc()
            _lib.check(ipa.lib().ipk_host_pipeline_run_region(C.byref(d), bad.ctypes.data, x, y, rw, rh, host.ctypes.data, 1, C.byref(flag)), "ipk_host_pipeline_run_region")
            assert flag.value == 1
            sp._same(host, whole[y:y + rh, x:x + rw], "%s region %r through the host form" % (name, win))


@pytest.mark.parametrize("off", [0, 1])
def test_region_writes_only_the_region(ipa, orc, off):
    import torch
    for name, ops, out_type in (("rgb16", dict(rotation=1), U8), ("mono_u16", {}, F32), ("rgb3_u16", dict(rotation=2), U16)):
        pipe, desc, _ = _build(ipa, orc, name, 96, 120, util.SEED + 16300, ops)
        pipe.fuse_plain = True
        code = CODES[out_type]
        whole = sp._want(orc, desc(), out_type)
        _, (fw, fhh) = pipe.sizes()
        for x, y, rw, rh in ((3, 5, 17, 16), (fw - 16, fhh - 16, 16, 16), (fw // 2, 0, 3, fhh)):
            g = util.Guarded(rw * rh * 3, NP_OUT[code], off)
            pipe.run_region(x, y, rw, rh, code, out=g.view())
            torch.cuda.synchronize()
            assert pipe.last_region_windowed is True
            tag = "%s %s off %d region %r" % (name, out_type, off, (x, y, rw, rh))
            sp._same(g.result(tag).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw], tag)
