"""GPU parity of ipk_plain_scale_down -- the monochrome (plain=1) and three-sample (plain=3) modes of k_raw_scaled_demosaic<uint16_t | float> -- and of
the routes that use it under IPK_FUSED_PLAIN_PREVIEWS (Pipeline.scale_plain): downscaled previews of monochrome and three-sample raws in one pass over
the source, their regions as windows of that pass (bit 3), their straightened previews as two launches (bit 6), and the cached drivers.  Bar: bit-exact
(f32 bit patterns, any NaN == any NaN, all four channels at op level so that E is +0.0; equal u8 / u16).  Every case asserts by the launch log which
kernel ran in which mode, and that the staged kernels it replaces did not."""
import ctypes as C
import re

import numpy as np
import pytest

import util
import test_gpu_staged_paths as sp
from test_gpu_staged_paths import F32, U8, U16

pytestmark = pytest.mark.gpu

RGB, MONO = 1, 2                                                          # ipk_plain_kind
KIND = {"mono": MONO, "cpp3": RGB}
LAYOUT = {"mono": 1, "cpp3": 3}
CTYPE = {"u16": "unsigned short", "f32": "float"}
CODES = {F32: 0, U8: 1, U16: 2}
NP_OUT = {F32: np.dtype(np.float32), U8: np.dtype(np.uint8), U16: np.dtype(np.uint16)}
BM, WM = (util.BLACK, 7.0, 9.0, 0.0), (util.WHITE, 11.0, 13.0, 0.0)      # a monochrome raw reads pair 0 alone
B3, W3 = (64.0, 128.0, 256.0, 0.0), (1023.0, 4095.0, 16383.0, 0.0)       # a three-sample raw's levels: different per channel
STAGED = ("k_gofloat_mono", "k_gofloat_rgb", "k_transform_buffer")
CROPS = (3, 1, 2, 5)
X0, Y0 = 3, 2                                                             # the source's place inside the wider pitched frame at op level
# (width, height, nwidth, nheight): a non-integer scale near 3; skips 10.6 (far above 7: the widest windows) and 2.5; windows of one or two taps with
# zero weights present; nwidth - 1 == 1
GEOMS = [(83, 57, 29, 19), (150, 100, 15, 40), (101, 77, 100, 76), (11, 10, 2, 2)]


@pytest.fixture(scope="module")
def ipa():
    import imagepipe_amd
    imagepipe_amd.init(0)
    return imagepipe_amd


def _fa(v):
    return (C.c_float * 4)(*[float(x) for x in v])


def _levels(kind):
    return (BM, WM) if kind == "mono" else (B3, W3)


def _frame(kind, src, w, h, seed):
    """(data, owidth): noise over more than the level range, the w x h source at (X0, Y0) of a wider and taller frame; f32 frames hold util.SPECIALS scaled
    to the white level and lone non-finite samples, each alone in an ordinary neighbourhood"""
    oh, ow, spp = h + Y0 + 2, w + X0 + 4, 1 if kind == "mono" else 3
    data = util.noise_u16(seed, oh, ow * spp, 20000)
    if src == "f32":
        data = data.astype(np.float32) + util.uniform_f32(seed + 1, data.size, -0.5, 0.5).reshape(data.shape)
        with np.errstate(over="ignore"):
            spc = util.SPECIALS * np.float32(16383.0)
        for k in range(0, spc.size, w * spp):                              # inside the source: every other row until they are all placed
            part = spc[k: k + w * spp]
            data[Y0 + 1 + 2 * (k // (w * spp)), X0 * spp: X0 * spp + part.size] = part
        assert 1 + 2 * ((spc.size - 1) // (w * spp)) < h
        data[Y0 + h // 2, (X0 + w // 2) * spp] = -np.inf
        data[Y0 + h - 2, (X0 + 3) * spp + spp - 1] = np.nan
        data[Y0 + 5, (X0 + w - 2) * spp] = np.inf
    return (data if kind == "mono" else data.reshape(oh, ow, 3)), ow


def _oracle_op(orc, kind, data, w, h, nw, nh, levels=None):
    b, wh = levels or _levels(kind)
    with np.errstate(all="ignore"):
        buf = orc.gofloat_mono(data, X0, Y0, w, h, b[0], wh[0]) if kind == "mono" else orc.gofloat_rgb(data, X0, Y0, w, h, b, wh)
        return orc.scale_down_opbuf(buf, nw, nh)


def _plain_entries(ran):
    return sorted(e for e in ran if "plain=" in e)


def _assert_one_pass(ran, kind, src, tag, win=False):
    """the general kernel in its plain mode, and none of the staged kernels it replaces"""
    pat = r"^ipk::k_raw_scaled_demosaic<%s>\[norm_fast=0,norm_light=0,fast_x=[01],fast_y=[01],xcd=0%s,plain=%d\]$" % (
        re.escape(CTYPE[src]), ",win=1" if win else "", LAYOUT[kind])
    hits = [e for e in ran if re.match(pat, e)]
    assert len(hits) == 1 and _plain_entries(ran) == hits, (tag, sorted(ran))
    assert not [e for e in ran if any(k in e for k in STAGED)], (tag, sorted(ran))
    assert not [e for e in ran if "_w8" in e], (tag, sorted(ran))


def _assert_staged(ran, kind, tag):
    assert not _plain_entries(ran) and not [e for e in ran if "k_raw_scaled_demosaic" in e], (tag, sorted(ran))
    assert any(("k_gofloat_mono" if kind == "mono" else "k_gofloat_rgb") in e for e in ran), (tag, sorted(ran))
    assert any("k_transform_buffer<float>" in e for e in ran), (tag, sorted(ran))


def _call(ipa, kind, src, dev, ow, w, h, nw, nh, dst_ptr, win=None, levels=None):
    b, wh = levels or _levels(kind)
    L = ipa.lib()
    st = 1 if src == "f32" else 0
    if win is None:
        return L.ipk_plain_scale_down(dev.data_ptr(), st, KIND[kind], ow, X0, Y0, w, h, _fa(b), _fa(wh), nw, nh, dst_ptr, None)
    return L.ipk_plain_scale_down_window(dev.data_ptr(), st, KIND[kind], ow, X0, Y0, w, h, _fa(b), _fa(wh), nw, nh, *win, dst_ptr, None)


# ---------------------------------------------------------------------------------------------
# 1. entry point parity
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geom", GEOMS, ids=["%dx%d-%dx%d" % g for g in GEOMS])
@pytest.mark.parametrize("src", ["u16", "f32"])
@pytest.mark.parametrize("kind", ["mono", "cpp3"])
def test_entry_point_vs_oracle(ipa, orc, kind, src, geom):
    import torch
    w, h, nw, nh = geom
    data, ow = _frame(kind, src, w, h, util.SEED + 18000 + 16 * GEOMS.index(geom) + 2 * LAYOUT[kind] + (src == "f32"))
    dev = sp._upload(ipa, data, src == "f32")
    want = _oracle_op(orc, kind, data, w, h, nw, nh)
    # one geometry per kind has its destination 4 bytes off a 16-byte boundary: element alignment is all the entry point asks for
    offs = (0, 1) if geom == GEOMS[0] else (0,)
    for off in offs:
        tag = "%s %s %dx%d -> %dx%d, dst off %d" % (kind, src, w, h, nw, nh, off)
        g = util.Guarded(nw * nh * 4, NP_OUT[F32], off)
        assert g.ptr % 16 == 4 * off
        with ipa.launch_log() as ran:
            rc = _call(ipa, kind, src, dev, ow, w, h, nw, nh, g.ptr)
            assert rc == 0, (tag, ipa.lib().ipk_last_error())
            torch.cuda.synchronize()
        _assert_one_pass(ran, kind, src, tag)
        got = g.result(tag).reshape(nh, nw, 4)
        util.assert_bits_equal(got, want, tag)
        assert not got[..., 3].view(np.uint32).any(), tag + ": E is not +0.0"


def test_the_geometries_are_what_they_claim():
    f = np.float32
    skips = [(float((f(w - 1) - f(0)) / f(nw - 1)), float((f(h - 1) - f(0)) / f(nh - 1))) for w, h, nw, nh in GEOMS]
    assert 2.5 < skips[0][0] < 3.5 and skips[0][0] != round(skips[0][0])
    assert skips[1][0] > 10.0 and 1.0 < skips[1][1] < 7.0
    assert 1.0 < skips[2][0] < 1.02 and 1.0 < skips[2][1] < 1.02
    assert GEOMS[3][2] - 1 == 1


def test_raster_kind_forwards(ipa, orc):
    import torch
    w, h, nw, nh = 83, 57, 29, 19
    img = (util.splitmix64(util.SEED + 18100, (h + 4) * (w + 7) * 3) & np.uint64(255)).astype(np.uint8).reshape(h + 4, w + 7, 3)
    dev = torch.from_numpy(img.ravel()).cuda()
    want = orc.scale_down_opbuf(orc.gofloat_other(img, X0, Y0, w, h), nw, nh)
    L = ipa.lib()
    g = util.Guarded(nw * nh * 4, NP_OUT[F32], 0)
    with ipa.launch_log() as ran:
        assert L.ipk_plain_scale_down(dev.data_ptr(), 2, 0, w + 7, X0, Y0, w, h, None, None, nw, nh, g.ptr, None) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    assert sorted(ran) == ["ipk::k_raster_scale_down<unsigned char>"], sorted(ran)
    util.assert_bits_equal(g.result("raster").reshape(nh, nw, 4), want, "raster kind")
    g = util.Guarded(5 * 3 * 4, NP_OUT[F32], 0)
    with ipa.launch_log() as ran:
        assert L.ipk_plain_scale_down_window(dev.data_ptr(), 2, 0, w + 7, X0, Y0, w, h, None, None, nw, nh, 7, 2, 5, 3, g.ptr, None) == 0
        torch.cuda.synchronize()
    assert sorted(ran) == ["ipk::k_raster_scale_down<unsigned char>[win=1]"], sorted(ran)
    util.assert_bits_equal(g.result("raster window").reshape(3, 5, 4), want[2:5, 7:12], "raster kind, window")


def test_refusals_write_nothing(ipa):
    import torch
    L = ipa.lib()
    INVALID = -2
    w, h, nw, nh = 83, 57, 29, 19
    data, ow = _frame("mono", "u16", w, h, util.SEED + 18200)
    dev = sp._upload(ipa, data, False)
    out = torch.full((64,), 7.0, dtype=torch.float32, device="cuda")
    b, wh = _fa(BM), _fa(WM)
    args = (ow, X0, Y0, w, h, b, wh, nw, nh)
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (nw - 1, 0, 2, 1), (0, nh - 1, 1, 2), (nw, 0, 1, 1), (0, nh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        for kind in (MONO, RGB):
            assert L.ipk_plain_scale_down_window(dev.data_ptr(), 0, kind, *args, *win, out.data_ptr(), None) == INVALID, win
    assert L.ipk_plain_scale_down(dev.data_ptr(), 2, MONO, *args, out.data_ptr(), None) == INVALID                    # a raster type with a raw kind
    assert L.ipk_plain_scale_down(dev.data_ptr(), 0, 0, *args, out.data_ptr(), None) == INVALID                       # a raw type with the raster kind
    assert L.ipk_plain_scale_down(dev.data_ptr(), 0, 3, *args, out.data_ptr(), None) == INVALID                       # no such kind
    assert L.ipk_plain_scale_down(None, 0, MONO, *args, out.data_ptr(), None) == INVALID
    assert L.ipk_plain_scale_down(dev.data_ptr(), 0, MONO, *args, None, None) == INVALID
    assert L.ipk_plain_scale_down(dev.data_ptr(), 0, MONO, ow, X0, Y0, w, h, None, wh, nw, nh, out.data_ptr(), None) == INVALID
    assert L.ipk_plain_scale_down(dev.data_ptr(), 0, MONO, w + X0 - 1, X0, Y0, w, h, b, wh, nw, nh, out.data_ptr(), None) == INVALID   # wider than the pitch
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()), "a refused call wrote to dst"


# ---------------------------------------------------------------------------------------------
# 2. degenerate levels: what ipk_gofloat_* followed by ipk_scale_down_opbuf give on the device
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,src", [("mono", "u16"), ("cpp3", "f32")])
@pytest.mark.parametrize("name,levels", [("zero range", ((512.0, 100.0, 300.0, 0.0), (512.0, 100.0, 300.0, 0.0))),
                                         ("inverted", ((16383.0, 4095.0, 900.0, 0.0), (512.0, 128.0, 1000.0, 0.0)))])
def test_degenerate_levels_vs_the_two_staged_launches(ipa, kind, src, name, levels):
    import torch
    w, h, nw, nh = GEOMS[0]
    data, ow = _frame(kind, src, w, h, util.SEED + 18300 + LAYOUT[kind])
    if kind == "mono":
        data[Y0 + 7, X0 + 5: X0 + 9] = 512                                   # samples AT the black level: 0 / 0 with a zero range
    dev = sp._upload(ipa, data, src == "f32")
    L = ipa.lib()
    full = torch.empty(w * h * 4, dtype=torch.float32, device="cuda")
    want = torch.empty(nw * nh * 4, dtype=torch.float32, device="cuda")
    b, wh = levels
    if kind == "mono":
        assert L.ipk_gofloat_mono_u16(dev.data_ptr(), ow, X0, Y0, w, h, b[0], wh[0], full.data_ptr(), None) == 0, L.ipk_last_error()
    else:
        assert L.ipk_gofloat_rgb_f32(dev.data_ptr(), ow, X0, Y0, w, h, _fa(b), _fa(wh), full.data_ptr(), None) == 0, L.ipk_last_error()
    assert L.ipk_scale_down_opbuf(full.data_ptr(), w, h, nw, nh, want.data_ptr(), None) == 0, L.ipk_last_error()
    g = util.Guarded(nw * nh * 4, NP_OUT[F32], 0)
    tag = "%s %s, %s" % (kind, src, name)
    with ipa.launch_log() as ran:
        assert _call(ipa, kind, src, dev, ow, w, h, nw, nh, g.ptr, levels=levels) == 0, L.ipk_last_error()
        torch.cuda.synchronize()
    _assert_one_pass(ran, kind, src, tag)
    util.assert_bits_equal(g.result(tag), want.cpu().numpy(), tag)


# ---------------------------------------------------------------------------------------------
# 3. window form
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind,src", [("cpp3", "u16"), ("mono", "f32")])
def test_window_form(ipa, orc, kind, src):
    import torch
    w, h, nw, nh = GEOMS[0]
    data, ow = _frame(kind, src, w, h, util.SEED + 18400 + LAYOUT[kind])
    dev = sp._upload(ipa, data, src == "f32")
    want = _oracle_op(orc, kind, data, w, h, nw, nh)
    whole = torch.empty(nw * nh * 4, dtype=torch.float32, device="cuda")
    assert _call(ipa, kind, src, dev, ow, w, h, nw, nh, whole.data_ptr()) == 0
    whole = whole.cpu().numpy().reshape(nh, nw, 4)
    util.assert_bits_equal(whole, want, "whole frame")
    spp = LAYOUT[kind]
    flat = data.reshape(data.shape[0], ow * spp)
    for win in ((0, 0, 1, 1), (28, 18, 1, 1), (0, 0, 29, 19), (5, 3, 17, 9), (nw - 1, 0, 1, nh), (0, nh - 1, nw, 1)):
        wx, wy, ww, wh = win
        fx, fy, fw, fh = ipa.scaled_window_footprint(w, h, nw, nh, win)
        bad = np.full_like(flat, np.nan if src == "f32" else 0xFFFF)
        r0, c0 = Y0 + fy, (X0 + fx) * spp
        bad[r0: r0 + fh, c0: c0 + fw * spp] = flat[r0: r0 + fh, c0: c0 + fw * spp]
        if win != (0, 0, 29, 19):
            assert not np.array_equal(bad.view(np.uint8), flat.view(np.uint8)), "nothing is poisoned: the case tests nothing"
        for what, d in (("clean", dev), ("poisoned outside the footprint", sp._upload(ipa, bad, src == "f32"))):
            tag = "%s %s window %r, %s source" % (kind, src, win, what)
            g = util.Guarded(ww * wh * 4, NP_OUT[F32], 1)
            with ipa.launch_log() as ran:
                assert _call(ipa, kind, src, d, ow, w, h, nw, nh, g.ptr, win=win) == 0, (tag, ipa.lib().ipk_last_error())
                torch.cuda.synchronize()
            _assert_one_pass(ran, kind, src, tag, win=True)
            got = g.result(tag).reshape(wh, ww, 4)
            util.assert_bits_equal(got, whole[wy:wy + wh, wx:wx + ww], tag + " against the whole-frame call")
            util.assert_bits_equal(got, want[wy:wy + wh, wx:wx + ww], tag + " against the oracle")
    got = ipa.plain_scale_down_window(dev, KIND[kind], ow, X0, Y0, w, h, *_levels(kind), nw, nh, (5, 3, 17, 9))
    util.assert_bits_equal(got.cpu().numpy().reshape(9, 17, 4), want[3:12, 5:22], "the Python wrapper")
    got = ipa.plain_scale_down(dev, KIND[kind], ow, X0, Y0, w, h, *_levels(kind), nw, nh)
    util.assert_bits_equal(got.cpu().numpy().reshape(nh, nw, 4), want, "the Python wrapper, whole frame")


# ---------------------------------------------------------------------------------------------
# 4. pipeline
# ---------------------------------------------------------------------------------------------
SOURCE = {("mono", "u16"): "mono_u16", ("mono", "f32"): "mono_f32", ("cpp3", "u16"): "rgb3_u16", ("cpp3", "f32"): "rgb3_f32"}
_BUILT = {}


def _case(ipa, orc, kind, src, ops, w=131, h=113, crops=CROPS, wb=util.WB, data=None):
    """(pipeline, {out_type: the oracle's result}, host data); the oracle's results are computed once per case and shared"""
    name = SOURCE[(kind, src)]
    key = repr((name, sorted(ops.items()), w, h, crops, wb))
    fresh, s = sp._source(name, h, w, util.SEED + 18500 + len(name) + w)
    if data is None:
        data = fresh
    pipe = sp._pipeline(ipa, data, s, crops, ops, wb=wb)
    if key not in _BUILT:
        wants = {}
        for out_type in (F32, U8, U16):                                       # F32 first: the oracle's 8- and 16-bit outputs set the descriptor's `linear`
            wants[out_type] = sp._want(orc, sp._oracle_desc(orc, fresh, s, crops, dict(ops, wb_coeffs=wb, cam_to_xyz_normalized=sp._cam4())), out_type)
        _BUILT[key] = wants
    return pipe, _BUILT[key], data


def _logged(ipa, pipe, out_type):
    import torch
    with ipa.launch_log() as ran:
        got = sp._out(pipe, out_type)
        torch.cuda.synchronize()
    return got, ran


@pytest.mark.parametrize("out_type", [F32, U8, U16])
@pytest.mark.parametrize("src", ["u16", "f32"])
@pytest.mark.parametrize("kind", ["mono", "cpp3"])
def test_pipeline_vs_oracle(ipa, orc, kind, src, out_type):
    # one case per kind runs at rotation 1
    ops = dict(maxwidth=40, rotation=1) if (src, out_type) == ("f32", U8) else dict(maxwidth=40)
    pipe, wants, _ = _case(ipa, orc, kind, src, ops)
    tag = "%s %s -> %s %r" % (kind, src, out_type, ops)
    code = CODES[out_type]
    pipe.scale_plain = True
    assert pipe.scales_plain(code) and not pipe.fuses_plain(code), tag
    got, ran = _logged(ipa, pipe, out_type)
    _assert_one_pass(ran, kind, src, tag)
    sp._same(got, wants[out_type], tag + " with the bit")
    assert pipe.last_used_fused is False
    _, stages = pipe.run_timed(code)
    assert stages[0][0] == "gofloat+demosaic" and "demosaic" not in [n for n, _ in stages[1:]], (tag, stages)
    pipe.scale_plain = False
    assert not pipe.scales_plain(code), tag
    got0, ran0 = _logged(ipa, pipe, out_type)
    _assert_staged(ran0, kind, tag)
    sp._same(got0, wants[out_type], tag + " without the bit")
    _, stages = pipe.run_timed(code)
    assert [n for n, _ in stages[:2]] == ["gofloat", "demosaic"], (tag, stages)


@pytest.mark.parametrize("src", ["u16", "f32"])
def test_a_mono_preview_keeps_its_monochrome_flag(ipa, orc, src):
    """a white balance and a camera matrix that are far from neutral: the tail must read the sRGB matrix and unit multipliers for a monochrome raw, as
    the oracle does -- a colour reading of the same buffer is a plausible picture with other numbers"""
    wb = (3.0, 1.0, 0.4, float("nan"))
    pipe, wants, _ = _case(ipa, orc, "mono", src, dict(maxwidth=40), wb=wb)
    pipe.scale_plain = True
    for out_type in (F32, U8):
        got, ran = _logged(ipa, pipe, out_type)
        _assert_one_pass(ran, "mono", src, "mono %s, hostile colour settings" % src)
        sp._same(got, wants[out_type], "mono %s -> %s with a non-neutral white balance and matrix" % (src, out_type))
    # the reference: a monochrome buffer's result does not see the white balance at all
    _, neutral, _ = _case(ipa, orc, "mono", src, dict(maxwidth=40))
    util.assert_bits_equal(wants[F32], neutral[F32], "the oracle's monochrome result does not depend on the white balance")


# ---------------------------------------------------------------------------------------------
# 5. regions (bits 0 + 3 + 7)
# ---------------------------------------------------------------------------------------------
def _poisoned(data, spp, sx, sy, sw, sh):
    flat = data.reshape(data.shape[0], -1)
    out = np.full_like(flat, np.nan if data.dtype == np.float32 else 0xFFFF)
    out[sy:sy + sh, sx * spp:(sx + sw) * spp] = flat[sy:sy + sh, sx * spp:(sx + sw) * spp]
    return out.reshape(data.shape)


def _check_regions(ipa, orc, kind, src, ops, regions, out_types, w=131, h=113, crops=CROPS):
    import torch
    from imagepipe_amd import _lib
    L = ipa.lib()
    pipe, wants, data = _case(ipa, orc, kind, src, ops, w, h, crops)
    pipe.scale_plain = pipe.window_previews = True
    _, (fw, fh) = pipe.sizes()
    for i, reg in enumerate(regions(fw, fh)):
        x, y, rw, rh = reg
        out_type = out_types[i % len(out_types)]
        code = CODES[out_type]
        tag = "%s %s %r region %r -> %s" % (kind, src, ops, reg, out_type)
        whole = wants[out_type]
        assert whole.shape[:2] == (fh, fw), tag
        assert pipe.windows_preview(code), tag
        win, (sx, sy, sw, sh) = pipe.region(x, y, rw, rh, code)
        assert win == 1 and sw > 0 and sh > 0 and sx + sw <= w and sy + sh <= h, tag
        g = util.Guarded(rw * rh * 3, NP_OUT[out_type], 1)
        with ipa.launch_log() as ran:
            pipe.run_region(x, y, rw, rh, code, out=g.view())
            torch.cuda.synchronize()
        assert pipe.last_region_windowed is True, tag
        _assert_one_pass(ran, kind, src, tag, win=True)
        sp._same(g.result(tag).reshape(rh, rw, 3), whole[y:y + rh, x:x + rw], tag)
        # without bit 7 the region is cut from the whole result, as it always was
        pipe.scale_plain = False
        assert pipe.region(x, y, rw, rh, code)[0] == 0 and not pipe.windows_preview(code), tag
        pipe.scale_plain = True
        # the host form on a frame poisoned outside the reported window
        bad = _poisoned(data, LAYOUT[kind], sx, sy, sw, sh)
        if (sw, sh) != (w, h):
            assert not np.array_equal(bad.view(np.uint8), data.view(np.uint8)), "nothing is poisoned: the case tests nothing"
        host = np.zeros((rh, rw, 3), NP_OUT[out_type])
        wflag = C.c_int(-1)
        d = pipe.desc()
        _lib.check(L.ipk_host_pipeline_run_region(C.byref(d), bad.ctypes.data, x, y, rw, rh, host.ctypes.data, code, C.byref(wflag)), "ipk_host_pipeline_run_region")
        assert wflag.value == 1, tag
        sp._same(host, whole[y:y + rh, x:x + rw], tag + " through the host form, poisoned outside the window")


def _small_regions(fw, fh):
    """1 pixel, 255 and 256 pixels (the two forms of the tail), the whole area"""
    return [(fw - 1, fh - 1, 1, 1), (0, 1, 15, 17) if fw >= 15 else (1, 0, 17, 15), (2, 3, 16, 16), (0, 0, fw, fh)]


@pytest.mark.parametrize("rotation", [0, 1], ids=["normal", "rotate90"])
@pytest.mark.parametrize("kind,src", [("mono", "u16"), ("cpp3", "f32"), ("mono", "f32"), ("cpp3", "u16")])
def test_regions(ipa, orc, kind, src, rotation):
    _check_regions(ipa, orc, kind, src, dict(maxwidth=40, rotation=rotation), _small_regions, (U8, F32, U16))


@pytest.mark.parametrize("rotation", [0, 1], ids=["normal", "rotate90"])
def test_a_region_of_257_pixels(ipa, orc, rotation):
    """257 is prime: a row of 257 pixels needs a result that wide, so this frame is 1100x30 under a limit of 300 on its long side"""
    ops = dict(maxheight=300, rotation=1) if rotation else dict(maxwidth=300)
    regions = (lambda fw, fh: [(2, 3, 1, 257)]) if rotation else (lambda fw, fh: [(3, 2, 257, 1)])
    for out_type in (U8, F32):
        _check_regions(ipa, orc, "mono", "u16", ops, regions, (out_type,), w=1100, h=30, crops=(0, 0, 0, 0))


# ---------------------------------------------------------------------------------------------
# 6. cached
# ---------------------------------------------------------------------------------------------
def _cache_entry(ipa, cache, key):
    p, w, h, c, m = C.c_void_p(), C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_int()
    rc = ipa.lib().ipk_cache_get(cache.handle, key, C.byref(p), C.byref(w), C.byref(h), C.byref(c), C.byref(m))
    return None if rc != 0 else (w.value, h.value, c.value, m.value)


def test_cached_drivers(ipa, orc):
    import torch
    pipe, wants, _ = _case(ipa, orc, "mono", "u16", dict(maxwidth=40))
    pipe.scale_plain = True
    (dw, dh), (fw, fh) = pipe.sizes()
    uncached = pipe.run().numpy()
    cache = ipa.PipelineCache(1 << 26)
    try:
        hs = pipe.hashes()
        with ipa.launch_log() as ran:
            got = pipe.run(cache).numpy()
            torch.cuda.synchronize()
        _assert_one_pass(ran, "mono", "u16", "cached, cold")
        assert pipe.last_ops_run & 3 == 3, hex(pipe.last_ops_run)
        util.assert_bits_equal(got, wants[F32], "cached, cold")
        util.assert_bits_equal(got, uncached, "cached against uncached")
        assert _cache_entry(ipa, cache, hs[1]) == (dw, dh, 4, 1), _cache_entry(ipa, cache, hs[1])
        assert _cache_entry(ipa, cache, hs[0]) is None and not cache.contains(hs[0])
        with ipa.launch_log() as ran:
            again = pipe.run(cache).numpy()
            torch.cuda.synchronize()
        assert pipe.last_ops_run & 3 == 0 and not [e for e in ran if "k_raw_scaled_demosaic" in e or "k_gofloat" in e], (hex(pipe.last_ops_run), sorted(ran))
        util.assert_bits_equal(again, wants[F32], "cached, hit")
        # an edit behind the demosaic resumes from the monochrome buffer: still the oracle's monochrome result
        pipe.ops.basecurve.exposure = 0.5
        edited = pipe.run(cache).numpy()
        assert pipe.last_ops_run & 7 == 0, hex(pipe.last_ops_run)
        pipe.allow_fused = False
        util.assert_bits_equal(edited, pipe.run().numpy(), "an exposure edit from the cached buffer against the staged ops")
        pipe.allow_fused = True
        pipe.ops.basecurve.exposure = 0.0
    finally:
        cache.close()
    cache = ipa.PipelineCache(1 << 26)
    try:
        for out_type, reg in ((F32, (5, 3, 17, 9)), (U8, (2, 3, 16, 16))):
            x, y, rw, rh = reg
            with ipa.launch_log() as ran:
                got = pipe.run_region(x, y, rw, rh, CODES[out_type], cache=cache)
                torch.cuda.synchronize()
            a = got.cpu().numpy().reshape(rh, rw, 3)
            sp._same(a, wants[out_type][y:y + rh, x:x + rw], "cached region %r -> %s" % (reg, out_type))
            if out_type == F32:
                _assert_one_pass(ran, "mono", "u16", "cached region, cold")
                assert pipe.last_ops_run & 3 == 3
                assert _cache_entry(ipa, cache, pipe.hashes()[1]) == (dw, dh, 4, 1) and _cache_entry(ipa, cache, pipe.hashes()[0]) is None
            else:
                assert pipe.last_ops_run & 7 == 0 and not _plain_entries(ran), (hex(pipe.last_ops_run), sorted(ran))
    finally:
        cache.close()


# ---------------------------------------------------------------------------------------------
# 7. straightened previews (bits 0 + 6 + 7)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("out_type", [U8, F32])
@pytest.mark.parametrize("kind,src", [("mono", "u16"), ("cpp3", "f32")])
def test_straightened_previews(ipa, orc, kind, src, out_type):
    rc = tuple(float(np.float32(v)) for v in (0, 0, 0, 0, 0.02))
    pipe, wants, _ = _case(ipa, orc, kind, src, dict(maxwidth=90, rotatecrop=rc))
    code = CODES[out_type]
    tag = "%s %s straightened -> %s" % (kind, src, out_type)
    pipe.scale_plain = pipe.fuse_scaled_rotatecrop = True
    assert pipe.fuses_scaled_rotatecrop(code) and pipe.scales_plain(code), tag
    got, ran = _logged(ipa, pipe, out_type)
    _assert_one_pass(ran, kind, src, tag)
    assert len([e for e in ran if re.match(r"^ipk::k_fused_resample<float, [012]>\[.*rgbe=1.*\]$", e)]) == 1 and len(ran) == 2, (tag, sorted(ran))
    assert pipe.last_used_fused is True
    sp._same(got, wants[out_type], tag)
    _, stages = pipe.run_timed(code)
    assert [n for n, _ in stages] == ["gofloat+demosaic", "rotatecrop+to_lab+basecurve+from_lab+gamma"], (tag, stages)
    # a region of it: pass 1 over the footprint, windowed
    _, (fw, fh) = pipe.sizes()
    x, y, rw, rh = 4, 5, 19, 11
    import torch
    with ipa.launch_log() as ranr:
        reg = pipe.run_region(x, y, rw, rh, code)
        torch.cuda.synchronize()
    assert pipe.last_region_windowed is True
    _assert_one_pass(ranr, kind, src, tag + " region", win=True)
    a = reg.cpu().numpy()
    sp._same((a.view(np.uint16) if out_type == U16 else a).reshape(rh, rw, 3), wants[out_type][y:y + rh, x:x + rw], tag + " region")
    # without bit 7: the staged ops, the same result
    pipe.scale_plain = False
    assert not pipe.fuses_scaled_rotatecrop(code), tag
    got0, ran0 = _logged(ipa, pipe, out_type)
    _assert_staged(ran0, kind, tag)
    assert not [e for e in ran0 if "rgbe" in e], sorted(ran0)
    sp._same(got0, wants[out_type], tag + " without bit 7")
