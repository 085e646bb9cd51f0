"""GPU parity of the window launches of the scale-in-one-pass kernels (k_raw_scaled_demosaic, _w8, _w8m, k_raster_scale_down): at op level
ipk_raw_scaled_demosaic_window / ipk_raster_scale_down_window against the same rectangle of the CPU oracle's whole-frame result, and at pipeline level
regions of downscaled previews under IPK_FUSED_WINDOW_PREVIEWS (Pipeline.window_previews), from device and from host memory.  Bar: bit-exact f32 (any
NaN == any NaN), equal u8 / u16.  Every case asserts by the launch log which kernel ran and that it ran as a window launch.  The frames are the
smallest at which each kernel is selected (the shapes of the kernel-coverage table), plus two results wider than one block."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_gpu_rotatecrop_fused as rcf
import test_gpu_scaledown_fused as sdf
from test_gpu_rotatecrop_fused import XT, F32, U8, U16, SENSOR_CROPS, _mosaic, _upload, _np, _same, _oracle_desc, _want
from test_gpu_scaledown_fused import CODES

pytestmark = pytest.mark.gpu

NOCROP = (0, 0, 0, 0)
INVALID = -2
NP_OUT = {F32: np.dtype(np.float32), U8: np.dtype(np.uint8), U16: np.dtype(np.uint16)}
SCALERS = ("k_raw_scaled_demosaic", "k_raster_scale_down")
W16x12 = "16x12:" + "".join("RGB"[(3 * r + c * c + r * c) % 3] for r in range(12) for c in range(16))     # 192 cells: no LDS cell table, the w8 kernel


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _scalers(ran):
    return sorted(e for e in ran if any(k in e for k in SCALERS))


def _assert_window_only(ran, tag):
    s = _scalers(ran)
    assert s and all(e.endswith(",win=1]") or e.endswith("[win=1]") for e in s), "%s: not a window launch alone: %r" % (tag, sorted(ran))


# ---------------------------------------------------------------------------------------------
# op level
# ---------------------------------------------------------------------------------------------
# (cfa, w, h, nw, nh, kernel): the coverage table's shapes, one result with a second 256-column block (w8m) and one with a third 128-column block
# (the general kernel, skip 8.02)
RSD_SHAPES = [
    (XT, 150, 100, 100, 40, "w8m<%s, 2u, false>"), (XT, 150, 100, 50, 40, "w8m<%s, 3u, false>"), (XT, 150, 100, 30, 40, "w8m<%s, 5u, false>"),
    ("RGBE", 150, 100, 100, 40, "w8m<%s, 2u, true>"), ("RGBE", 150, 100, 50, 40, "w8m<%s, 3u, true>"), ("RGBE", 150, 100, 30, 40, "w8m<%s, 5u, true>"),
    (W16x12, 150, 100, 50, 40, "w8<%s>"), ("RGGB", 150, 100, 15, 40, "<%s>"), ("RGGB", 7, 30, 3, 10, "<%s>"),
    (XT, 700, 30, 330, 12, "w8m<%s, 3u, false>"), (W16x12, 700, 30, 330, 12, "w8<%s>"), ("RGGB", 2400, 24, 300, 3, "<%s>"),
]
RSD = [(s,) + c for s in ("f32", "u16") for c in RSD_SHAPES]
RSD_IDS = ["%s-%s-%dx%d-%dx%d" % (c[0], c[1][:5], c[2], c[3], c[4], c[5]) for c in RSD]


def _op_windows(nw, nh):
    """interior; touching the left, right, top and bottom edge; 1x1; one column; one row; the whole result; and, in a result of 300 columns and
    more, one that starts beyond column 256 (the second block column of the window-8 kernels, the third of the general kernel)"""
    a, b = max(1, nw // 3), max(1, nh // 3)
    wins = [(min(1, nw - 1), min(1, nh - 1), max(1, nw - 2), max(1, nh - 2)), (0, b, a, b), (nw - a, b, a, b), (a, 0, a, b), (a, nh - b, a, b),
            (nw // 2, nh // 2, 1, 1), (nw // 3, 0, 1, nh), (0, nh // 2, nw, 1), (0, 0, nw, nh)]
    if nw >= 300:
        wins += [(259, 1, nw - 259, nh - 1), (257, 0, 7, nh)]
    return wins


def _raw_frame(src, w, h, nw, x=3, y=1):
    """the coverage table's frame: noise, an unused margin, sensor offset (3, 1), and for f32 the planted specials"""
    oh, ow = h + y + 2, w + x + 3
    raw = util.noise_u16(util.SEED + 9600 + w * h + nw, oh, ow)
    if src == "f32":
        raw = raw.astype(np.float32) + util.uniform_f32(util.SEED + 9601, oh * ow).reshape(oh, ow)
        with np.errstate(over="ignore"):
            sp = util.SPECIALS * np.float32(16383.0)
        raw[y + 2, x: x + min(w, sp.size)] = sp[: min(w, sp.size)]
        raw[y + h // 2, x + w // 2] = -np.inf; raw[y + h - 2, x + 1] = np.nan
    return raw, ow, x, y


def _symbol(entry):
    return entry.split("[")[0]


@pytest.mark.parametrize("case", RSD, ids=RSD_IDS)
def test_raw_scaled_demosaic_window_vs_oracle(ipa, orc, case):
    import torch
    src, cfa, w, h, nw, nh, kernel = case
    raw, ow, x, y = _raw_frame(src, w, h, nw)
    dev = _upload(ipa, raw)
    with np.errstate(all="ignore"):
        want = orc.scaled_demosaic(cfa, orc.gofloat_cfa(raw, x, y, w, h, util.BLACK, util.WHITE), nw, nh)
    L = ipa.lib()
    whole = torch.empty(nh * nw * 4, dtype=torch.float32, device="cuda")
    with ipa.launch_log() as ran0:
        assert L.ipk_raw_scaled_demosaic(dev.data_ptr(), 1 if src == "f32" else 0, ow, x, y, w, h, util.BLACK, util.WHITE, cfa.encode(), nw, nh, whole.data_ptr(), None) == 0
    sel = _scalers(ran0)
    assert len(sel) == 1 and re.search(r"^ipk::k_raw_scaled_demosaic_?" + re.escape(kernel % ("float" if src == "f32" else "unsigned short")) + r"\[", sel[0]) \
        and "win=" not in sel[0], sel
    _same(whole.cpu().numpy().reshape(nh, nw, 4), want, "whole frame")
    for win in _op_windows(nw, nh):
        wx, wy, ww, wh = win
        tag = "%s window %r" % (RSD_IDS[RSD.index(case)], win)
        with ipa.launch_log() as ran:
            got = ipa.raw_scaled_demosaic_window(dev, ow, x, y, w, h, util.BLACK, util.WHITE, cfa, nw, nh, win)
            torch.cuda.synchronize()
        _same(got.cpu().numpy().reshape(wh, ww, 4), want[wy:wy + wh, wx:wx + ww], tag)
        s = _scalers(ran)
        assert len(s) == 1 and _symbol(s[0]) == _symbol(sel[0]) and s[0].endswith(",win=1]"), "%s: %r, whole frame %r" % (tag, s, sel)
        assert re.sub(r"xcd=\d", "xcd=0", s[0]) == re.sub(r"xcd=\d", "xcd=0", sel[0])[:-1] + ",win=1]", (tag, s, sel)


@pytest.mark.parametrize("bits", [8, 16])
def test_raster_scale_down_window_vs_oracle(ipa, orc, bits):
    import torch
    shapes = [(83, 57, 29, 19, 3, 2), (2400, 24, 300, 3, 1, 1)]
    for w, h, nw, nh, cx, cy in shapes:
        oh, ow = h + cy + 1, w + cx + 2
        img = (util.splitmix64(util.SEED + 9710 + bits + w, oh * ow * 3) & np.uint64((1 << bits) - 1)).astype(np.uint8 if bits == 8 else np.uint16).reshape(oh, ow, 3)
        dev = torch.from_numpy(img.ravel()).cuda() if bits == 8 else ipa.upload_u16(img)
        want = orc.scale_down_opbuf(orc.gofloat_other(img, cx, cy, w, h), nw, nh)
        sym = "ipk::k_raster_scale_down<%s>" % ("unsigned char" if bits == 8 else "unsigned short")
        for win in _op_windows(nw, nh):
            wx, wy, ww, wh = win
            with ipa.launch_log() as ran:
                got = ipa.raster_scale_down_window(dev, ow, cx, cy, w, h, nw, nh, win)
                torch.cuda.synchronize()
            _same(got.cpu().numpy().reshape(wh, ww, 4), want[wy:wy + wh, wx:wx + ww], "raster u%d %dx%d window %r" % (bits, w, h, win))
            assert _scalers(ran) == [sym + "[win=1]"], (win, sorted(ran))
        whole = torch.empty(nh * nw * 4, dtype=torch.float32, device="cuda")
        with ipa.launch_log() as ran:
            assert ipa.lib().ipk_raster_scale_down(dev.data_ptr(), 2 if bits == 8 else 3, ow, cx, cy, w, h, nw, nh, whole.data_ptr(), None) == 0
        assert _scalers(ran) == [sym], sorted(ran)                                 # whole frames carry no tag
        _same(whole.cpu().numpy().reshape(nh, nw, 4), want, "raster whole frame")


@pytest.mark.parametrize("src", ["f32", "u16"])
def test_xcd_grouping_follows_the_window_rows(ipa, orc, src):
    """a 33 x 110 result (100x330 at maxheight 110): windows of 31, 32 and 41 rows -- no grouping, grouping, grouping with leftover rows"""
    import torch
    cfa, w, h, nw, nh = XT, 100, 330, 33, 110
    raw, ow, x, y = _raw_frame(src, w, h, nw)
    dev = _upload(ipa, raw)
    with np.errstate(all="ignore"):
        want = orc.scaled_demosaic(cfa, orc.gofloat_cfa(raw, x, y, w, h, util.BLACK, util.WHITE), nw, nh)
    for rows, xcd in ((31, 0), (32, 1), (41, 2)):
        for wy in (0, 37, nh - rows):
            win = (2, wy, 29, rows)
            with ipa.launch_log() as ran:
                got = ipa.raw_scaled_demosaic_window(dev, ow, x, y, w, h, util.BLACK, util.WHITE, cfa, nw, nh, win)
                torch.cuda.synchronize()
            _same(got.cpu().numpy().reshape(rows, 29, 4), want[wy:wy + rows, 2:31], "xcd %s window %r" % (src, win))
            s = _scalers(ran)
            assert len(s) == 1 and "w8m<" in s[0] and s[0].endswith(",xcd=%d,win=1]" % xcd), (win, s)


@pytest.mark.parametrize("off", [0, 1])
def test_window_writes_only_its_samples(ipa, orc, off):
    """guard bands around a destination that starts 0 / 1 element past a 256-byte boundary: ww * wh * 4 floats, nothing else (one element past it the
    raw form selects the general kernel, as for whole frames)"""
    import torch
    L = ipa.lib()
    for src, (cfa, w, h, nw, nh, _k) in (("f32", RSD_SHAPES[1]), ("u16", RSD_SHAPES[6]), ("u16", RSD_SHAPES[7]), ("f32", RSD_SHAPES[9])):
        raw, ow, x, y = _raw_frame(src, w, h, nw)
        dev = _upload(ipa, raw)
        with np.errstate(all="ignore"):
            want = orc.scaled_demosaic(cfa, orc.gofloat_cfa(raw, x, y, w, h, util.BLACK, util.WHITE), nw, nh)
        for wx, wy, ww, wh in ((nw - 1, nh - 1, 1, 1), (3, 1, nw - 5, nh - 3), (nw // 3, 0, 1, nh), (0, nh // 2, nw, 1)):
            g = util.Guarded(ww * wh * 4, NP_OUT[F32], off)
            rc = L.ipk_raw_scaled_demosaic_window(dev.data_ptr(), 1 if src == "f32" else 0, ow, x, y, w, h, util.BLACK, util.WHITE, cfa.encode(), nw, nh,
                                                  wx, wy, ww, wh, g.ptr, None)
            assert rc == 0, L.ipk_last_error()
            torch.cuda.synchronize()
            tag = "%s %s off %d window %r" % (src, cfa[:5], off, (wx, wy, ww, wh))
            _same(g.result(tag).reshape(wh, ww, 4), want[wy:wy + wh, wx:wx + ww], tag)
    w, h, nw, nh, cx, cy = 83, 57, 29, 19, 3, 2
    img = (util.splitmix64(util.SEED + 9720, (h + 3) * (w + 5) * 3) & np.uint64(255)).astype(np.uint8).reshape(h + 3, w + 5, 3)
    dev = torch.from_numpy(img.ravel()).cuda()
    want = orc.scale_down_opbuf(orc.gofloat_other(img, cx, cy, w, h), nw, nh)
    for wx, wy, ww, wh in ((nw - 1, nh - 1, 1, 1), (3, 1, 20, 15), (0, nh // 2, nw, 1)):
        g = util.Guarded(ww * wh * 4, NP_OUT[F32], off)
        assert L.ipk_raster_scale_down_window(dev.data_ptr(), 2, w + 5, cx, cy, w, h, nw, nh, wx, wy, ww, wh, g.ptr, None) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
        tag = "raster off %d window %r" % (off, (wx, wy, ww, wh))
        _same(g.result(tag).reshape(wh, ww, 4), want[wy:wy + wh, wx:wx + ww], tag)


def test_window_refusals_write_nothing(ipa):
    import torch
    L = ipa.lib()
    raw, ow, x, y = _raw_frame("u16", 150, 100, 50)
    dev = _upload(ipa, raw)
    img = torch.zeros(60 * 90 * 3, dtype=torch.uint8, device="cuda")
    out = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    nw, nh = 50, 40
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (nw - 1, 0, 2, 1), (0, nh - 1, 1, 2), (nw, 0, 1, 1), (0, nh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        assert L.ipk_raw_scaled_demosaic_window(dev.data_ptr(), 0, ow, x, y, 150, 100, util.BLACK, util.WHITE, XT.encode(), nw, nh, *win, out.data_ptr(), None) == INVALID, win
        assert L.ipk_raster_scale_down_window(img.data_ptr(), 2, 90, 3, 2, 83, 57, nw, nh, *win, out.data_ptr(), None) == INVALID, win
    # admission is that of the whole-frame forms
    raw_args = (ow, x, y, 150, 100, util.BLACK, util.WHITE, XT.encode(), nw, nh)
    assert L.ipk_raw_scaled_demosaic_window(dev.data_ptr(), 2, *raw_args, 0, 0, 2, 2, out.data_ptr(), None) == INVALID          # a raster type
    assert L.ipk_raw_scaled_demosaic(dev.data_ptr(), 2, *raw_args, out.data_ptr(), None) == INVALID
    assert L.ipk_raw_scaled_demosaic_window(None, 0, *raw_args, 0, 0, 2, 2, out.data_ptr(), None) == INVALID
    assert L.ipk_raw_scaled_demosaic_window(dev.data_ptr(), 0, ow, x, y, 150, 100, util.BLACK, util.WHITE, b"RGGBX", nw, nh, 0, 0, 2, 2, out.data_ptr(), None) < 0
    assert L.ipk_raster_scale_down_window(img.data_ptr(), 0, 90, 3, 2, 83, 57, nw, nh, 0, 0, 2, 2, out.data_ptr(), None) == INVALID   # a raw type
    assert L.ipk_raster_scale_down_window(img.data_ptr(), 2, 80, 3, 2, 83, 57, nw, nh, 0, 0, 2, 2, out.data_ptr(), None) == INVALID   # wider than the pitch
    assert L.ipk_raster_scale_down(img.data_ptr(), 2, 80, 3, 2, 83, 57, nw, nh, out.data_ptr(), None) == INVALID
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to dst"


# ---------------------------------------------------------------------------------------------
# pipeline level
# ---------------------------------------------------------------------------------------------
# name -> (cfa or None for a raster, is_float / bits, (w, h, crops), ops, the kernel's symbol part, (demosaic size))
FRAMES = {
    "rggb-131x97@40": ("RGGB", False, (131, 97, NOCROP), dict(maxwidth=40), "w8m<unsigned short, 3u, false>", (40, 29)),
    "rgbe-131x97@40": ("RGBE", True, (131, 97, NOCROP), dict(maxwidth=40), "w8m<float, 3u, true>", (40, 29)),
    "xtrans-150x100@40": (XT, True, (150, 100, NOCROP), dict(maxwidth=40), "w8m<float, 3u, false>", (40, 26)),
    "xtrans-150x100@30": (XT, False, (150, 100, NOCROP), dict(maxwidth=30), "w8m<unsigned short, 5u, false>", (30, 20)),
    "rggb-150x100@15": ("RGGB", False, (150, 100, NOCROP), dict(maxwidth=15), "demosaic<unsigned short>", (15, 10)),
    "grbg-cropped-96x120@h40": ("GRBG", True, (96, 120, SENSOR_CROPS), dict(maxheight=40), "w8m<float, 3u, false>", (31, 40)),
    "raster-rgb8-83x57@29": (None, 8, (83, 57, NOCROP), dict(maxwidth=29, exposure=0.5), "k_raster_scale_down<unsigned char>", (29, 19)),
    "raster-rgb16-83x57@29": (None, 16, (83, 57, NOCROP), dict(maxwidth=29, exposure=0.5), "k_raster_scale_down<unsigned short>", (29, 19)),
}


def _build(ipa, orc, name, seed, extra=None, data=None):
    """(pipeline, oracle descriptor, host data)"""
    import torch
    cfa, kind, (w, h, crops), ops, _sym, _size = FRAMES[name]
    ops = {**ops, **(extra or {})}
    if ops.get("rotation", 0) % 2:                         # the size limit applies behind OpTransform: on the other axis the same preview is negotiated
        ops = {{"maxwidth": "maxheight", "maxheight": "maxwidth"}.get(k, k): v for k, v in ops.items()}
    if cfa is None:
        if data is None:
            data = (util.splitmix64(seed, h * w * 3) & np.uint64((1 << kind) - 1)).astype(np.uint8 if kind == 8 else np.uint16).reshape(h, w, 3)
        dev = torch.from_numpy(data.ravel()).cuda() if kind == 8 else ipa.upload_u16(data)
        pipe = ipa.Pipeline.new_from_source(ipa.OtherImage(w, h, dev, bits=kind))
        pipe.globals.settings.maxwidth, pipe.globals.settings.maxheight = ops.get("maxwidth", 0), ops.get("maxheight", 0)
        pipe.ops.basecurve.exposure = ops["exposure"]
        for k in ("rotation", "fliph", "flipv"):
            if k in ops:
                setattr(pipe.ops.transform, k, ops[k])
        return pipe, orc.make_pipeline(data, **ops), data
    if data is None:
        data = _mosaic(seed, h, w, kind)
    return sdf._pipeline(ipa, data, cfa, crops, ops), _oracle_desc(orc, data, cfa, crops, ops), data


def _regions(fw, fh):
    """one under 256 pixels and one of 256 and more where the result has them (the two forms of the tail), a corner pixel, the whole result"""
    small = (min(3, fw - 1), min(5, fh - 1), min(17, fw - min(3, fw - 1)), min(9, fh - min(5, fh - 1)))
    return [small, (1, 2, fw - 3, fh - 3), (fw - 1, fh - 1, 1, 1), (0, 0, fw, fh)]


def _timed_region(ipa, pipe, x, y, w, h, code):
    from imagepipe_amd import _lib
    L = ipa.lib()
    _lib.check(L.ipk_timing_begin(), "ipk_timing_begin")
    with ipa.launch_log() as ran:
        got = pipe.run_region(x, y, w, h, code)
    arr = (_lib.StageTime * 16)()
    n = C.c_int(0)
    _lib.check(L.ipk_timing_end(arr, 16, C.byref(n)), "ipk_timing_end")
    return got, ran, [arr[i].name.decode() for i in range(min(n.value, 16))]


def _check_frame(ipa, orc, name, seed, out_types, extra=None):
    pipe, desc, _ = _build(ipa, orc, name, seed, extra)
    sym, size = FRAMES[name][4], FRAMES[name][5]
    (dw, dh), (fw, fh) = pipe.sizes()
    assert (dw, dh) == size, (name, dw, dh)
    oriented = any((extra or {}).values())                 # OpTransform permutes: the quantisation cannot be the chain's last step
    sizes = set()
    for out_type in out_types:
        code = CODES[out_type]
        want = _want(orc, desc, out_type)
        assert want.shape[:2] == (fh, fw), name
        pipe.window_previews = True
        assert pipe.windows_preview(code), name
        for reg in _regions(fw, fh):
            x, y, w, h = reg
            sizes.add(w * h >= 256)
            t = "%s %s region %r" % (name, out_type, reg)
            pipe.window_previews = True
            assert pipe.region(x, y, w, h, code)[0] == 1, t
            got, ran, stages = _timed_region(ipa, pipe, x, y, w, h, code)
            assert pipe.last_region_windowed is True, t
            _same(_np(got, out_type, h, w), want[y:y + h, x:x + w], t)
            _assert_window_only(ran, t)
            assert any(sym in e for e in _scalers(ran)), (t, _scalers(ran))
            assert stages[0] == "region gofloat+demosaic" and "region copy" not in stages, (t, stages)
            if out_type != F32 and not oriented and w * h >= 256:
                assert stages[1:] == ["to_lab+basecurve+from_lab+gamma+quantise"], (t, stages)
            else:
                assert stages[1] == "to_lab+basecurve+from_lab+gamma", (t, stages)
            with_bit = _np(got, out_type, h, w).copy()
            pipe.window_previews = False
            assert pipe.region(x, y, w, h, code)[0] == 0, t
            got, ran, stages = _timed_region(ipa, pipe, x, y, w, h, code)
            assert pipe.last_region_windowed is False, t
            assert "region copy" in stages and not [e for e in ran if "win=1" in e] and any(sym in e for e in _scalers(ran)), (t, stages, sorted(ran))
            _same(_np(got, out_type, h, w), want[y:y + h, x:x + w], t + " without the bit")
            _same(_np(got, out_type, h, w), with_bit, t + ": the two settings")
    return sizes


@pytest.mark.parametrize("name", list(FRAMES))
def test_preview_regions_vs_oracle(ipa, orc, name):
    sizes = _check_frame(ipa, orc, name, util.SEED + 14000 + len(name), (F32, U8, U16))
    assert sizes == ({False} if name == "rggb-150x100@15" else {False, True}), "both forms of the tail (the 15 x 10 result has 150 pixels: one)"


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (False, True)])
def test_preview_regions_all_orientations(ipa, orc, rot, fh):
    name = "rggb-131x97@40" if fh else "xtrans-150x100@40"
    _check_frame(ipa, orc, name, util.SEED + 14100 + 2 * rot + fh, (F32, U8, U16), dict(rotation=rot, fliph=fh))


def test_raster_preview_regions_oriented(ipa, orc):
    _check_frame(ipa, orc, "raster-rgb8-83x57@29", util.SEED + 14200, (F32, U8), dict(rotation=1, flipv=True))


# ---------------------------------------------------------------------------------------------
# the launch reads only the window it reports
# ---------------------------------------------------------------------------------------------
READ_CASES = {"xtrans-150x100@40": None, "rgbe-131x97@40": None, "rggb-131x97@40": dict(rotation=3), "rggb-150x100@15": None,
              "grbg-cropped-96x120@h40": dict(rotation=1, fliph=True), "xtrans-150x100@30": None, "raster-rgb8-83x57@29": None}


def _poisoned(data, sx, sy, sw, sh):
    poison = np.nan if data.dtype == np.float32 else (0xFF if data.dtype == np.uint8 else 0xFFFF)
    out = np.full_like(data, poison)
    out[sy:sy + sh, sx:sx + sw] = data[sy:sy + sh, sx:sx + sw]
    return out


@pytest.mark.parametrize("case", list(READ_CASES))
def test_region_reads_only_the_reported_window(ipa, orc, case):
    """everything outside the window ipk_pipeline_region reports is NaN (f32) / 0xFFFF (u16) / 0xFF (RGB8): the inputs are noise, so a stray read
    changes the result -- for f32 sources even one with weight zero.  From device memory and through ipk_host_pipeline_run_region"""
    import torch
    from imagepipe_amd import _lib
    extra = READ_CASES[case]
    w, h, _crops = FRAMES[case][2]
    clean, _desc, data = _build(ipa, orc, case, util.SEED + 14300 + len(case), extra)
    clean.window_previews = True
    _, (fw, fh) = clean.sizes()
    L = ipa.lib()
    wholes = {t: rcf._out(clean, t) for t in (F32, U8, U16)}
    regs = _regions(fw, fh)[:3] + [(0, 0, 1, 1), (fw - 1, 0, 1, fh), (0, fh // 2, fw, 1)]
    for i, reg in enumerate(regs):
        x, y, rw, rh = reg
        out_type = [F32, U8, U16][i % 3]
        code = CODES[out_type]
        whole = wholes[out_type]
        win, (sx, sy, sw, sh) = clean.region(x, y, rw, rh, code)
        assert win == 1 and sw > 0 and sh > 0 and sx + sw <= w and sy + sh <= h, (case, reg)
        bad = _poisoned(data, sx, sy, sw, sh)
        assert not np.array_equal(bad.view(np.uint8), data.view(np.uint8)), "nothing is poisoned: the case tests nothing"
        pipe, _, _ = _build(ipa, orc, case, 0, extra, data=bad)
        pipe.window_previews = True
        got = pipe.run_region(x, y, rw, rh, code)
        torch.cuda.synchronize()
        assert pipe.last_region_windowed is True
        _same(_np(got, out_type, rh, rw), whole[y:y + rh, x:x + rw], "%s region %r %s from a poisoned device frame (window %r)" % (case, reg, out_type, (sx, sy, sw, sh)))
        host = np.zeros((rh, rw, 3), NP_OUT[out_type])
        wflag = C.c_int(-1)
        d = pipe.desc()
        _lib.check(L.ipk_host_pipeline_run_region(C.byref(d), bad.ctypes.data, x, y, rw, rh, host.ctypes.data, code, C.byref(wflag)), "ipk_host_pipeline_run_region")
        assert wflag.value == 1
        _same(host, whole[y:y + rh, x:x + rw], "%s region %r %s through the host form" % (case, reg, out_type))


@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("out_type", [F32, U8, U16])
def test_pipeline_region_writes_only_the_region(ipa, orc, out_type, off):
    import torch
    code = CODES[out_type]
    for name, extra in (("xtrans-150x100@40", None), ("rggb-131x97@40", dict(rotation=1)), ("raster-rgb8-83x57@29", None)):
        pipe, _, _ = _build(ipa, orc, name, util.SEED + 14400, extra)
        whole = rcf._out(pipe, out_type)
        pipe.window_previews = True
        _, (fw, fh) = pipe.sizes()
        for x, y, rw, rh in _regions(fw, fh)[:3]:
            g = util.Guarded(rw * rh * 3, NP_OUT[out_type], off)
            pipe.run_region(x, y, rw, rh, code, out=g.view())
            torch.cuda.synchronize()
            assert pipe.last_region_windowed is True
            tag = "%s %s off %d region %r" % (name, out_type, off, (x, y, rw, rh))
            _same(g.result(tag).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw], tag)


def test_region_refusals_write_nothing(ipa, orc):
    import torch
    pipe, _, _ = _build(ipa, orc, "rggb-131x97@40", util.SEED + 14500)
    pipe.window_previews = True
    _, (fw, fh) = pipe.sizes()
    L = ipa.lib()
    d = pipe.desc()
    out = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    flag = C.c_int(-1)
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (fw - 1, 0, 2, 1), (0, fh - 1, 1, 2), (fw, 0, 1, 1), (0, fh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        assert L.ipk_pipeline_run_region(C.byref(d), pipe.globals.image.data.data_ptr(), *win, out.data_ptr(), 0, C.byref(flag), None) == INVALID, win
    torch.cuda.synchronize()
    assert flag.value == -1 and bool((out == 7.0).all()), "a refused region wrote something"
