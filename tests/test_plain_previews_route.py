"""Downscaled previews of monochrome and three-sample raws as one pass over the source (no GPU): which descriptors ipk_pipeline_scales_plain names
under IPK_FUSED_PLAIN_PREVIEWS (bit 7 of allow_fused), what bits 3 (regions of previews) and 6 (straightened previews) then answer for them, that
every report is what it was without the bit, and that no hash sees it."""
import ctypes as C

import numpy as np
import pytest

import test_scaledown_route as sr
from test_scaledown_route import INVALID, SENSOR_CROPS
from test_preview_regions_route import _region, _sizes, _footprint

ON, PREVIEWS, SCALED_RC, PLAIN_PREVIEWS = 1, 8, 64, 128
RC = [float(np.float32(v)) for v in (0, 0, 0, 0, 0.02)]
KINDS = {"mono": dict(cpp=1, is_cfa=0), "cpp3": dict(cpp=3, is_cfa=0)}
SRC = {"u16": 0, "f32": 1}


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _plain(kind, src, scaled, **kw):
    """131x113 with OpGoFloat crops; scaled: under maxwidth 40 (scale about 3.1), else no size limit (scale 1)"""
    return sr._desc(131, 113, "", SENSOR_CROPS, src_type=SRC[src], maxwidth=40 if scaled else 0, **KINDS[kind], **kw)


def _fast_raster(L):
    from imagepipe_amd._lib import PipelineDesc
    fast = PipelineDesc()
    fast.src_type, fast.width, fast.height, fast.cpp, fast.use_fastpath, fast.maxwidth = 2, 128, 64, 3, 1, 64
    m = (C.c_float * 12)()
    L.ipk_const_matrix(2, m)
    fast.cam_to_xyz_normalized[:] = m[:]
    fast.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    return fast


@pytest.mark.parametrize("src", list(SRC))
@pytest.mark.parametrize("kind", list(KINDS))
def test_truth_table(L, kind, src):
    for out_type in (0, 1, 2):
        for scaled in (False, True):
            for bits, taken in ((0, False), (ON, False), (ON | PLAIN_PREVIEWS, scaled), (PLAIN_PREVIEWS, False)):
                tag = (kind, src, out_type, scaled, bits)
                d = _plain(kind, src, scaled)
                d.allow_fused = bits
                assert L.ipk_pipeline_scales_plain(C.byref(d), out_type) == int(taken), tag
                # regions of the preview: bit 3 beside it, and neither bit alone
                for extra in (0, PREVIEWS):
                    d.allow_fused = bits | extra
                    assert L.ipk_pipeline_scales_plain(C.byref(d), out_type) == int(taken), tag
                    assert L.ipk_pipeline_windows_preview(C.byref(d), out_type) == int(taken and extra == PREVIEWS), (tag, extra)
                # straightened previews: bit 6 beside it
                for extra in (0, SCALED_RC):
                    r = _plain(kind, src, scaled, rotatecrop=RC)
                    r.allow_fused = bits | extra
                    dw, dh, _, _ = _sizes(L, r)
                    assert ((dw, dh) != (131 - 6, 113 - 5)) == scaled      # this small frame's size fold lands on the source without a limit: scale 1
                    on7 = scaled and bits == ON | PLAIN_PREVIEWS
                    assert L.ipk_pipeline_scales_plain(C.byref(r), out_type) == int(on7), (tag, extra)
                    assert L.ipk_pipeline_fuses_scaled_rotatecrop(C.byref(r), out_type) == int(on7 and extra == SCALED_RC), (tag, extra)
                    assert L.ipk_pipeline_windows_preview(C.byref(r), out_type) == 0, (tag, extra)      # an active rotatecrop: bit 6's ground


def test_negative_controls(L):
    """the bit changes no report of a mosaic, a raster or a fast-path raster, and names none of them"""
    builders = {"rggb": lambda: sr._desc(131, 113, "RGGB", SENSOR_CROPS, maxwidth=40),
                "rggb straightened": lambda: sr._desc(131, 113, "RGGB", SENSOR_CROPS, maxwidth=40, rotatecrop=RC),
                "rgb8": lambda: sr._desc(128, 64, "", src_type=2, cpp=3, is_cfa=0, maxwidth=64, exposure=0.1),
                "rgb8 straightened": lambda: sr._desc(128, 64, "", src_type=2, cpp=3, is_cfa=0, maxwidth=64, exposure=0.1, rotatecrop=RC),
                "fast path": lambda: _fast_raster(L)}
    reports = (L.ipk_pipeline_windows_preview, L.ipk_pipeline_fuses_scaled_rotatecrop, L.ipk_pipeline_fuses_plain, L.ipk_pipeline_fuses_scaledown,
               L.ipk_pipeline_fuses_rotatecrop, L.ipk_pipeline_takes_fastpath)
    for name, build in builders.items():
        for out_type in (0, 1, 2):
            for base in (ON, ON | PREVIEWS, ON | SCALED_RC, ON | PREVIEWS | SCALED_RC | 16):
                a, b = build(), build()
                a.allow_fused, b.allow_fused = base, base | PLAIN_PREVIEWS
                assert L.ipk_pipeline_scales_plain(C.byref(a), out_type) == 0 and L.ipk_pipeline_scales_plain(C.byref(b), out_type) == 0, (name, base)
                for rep in reports:
                    assert rep(C.byref(a), out_type) == rep(C.byref(b), out_type), (name, base, rep)
                assert _region(L, a, 1, 1, 5, 3, out_type) == _region(L, b, 1, 1, 5, 3, out_type), (name, base)
    fast = _fast_raster(L)
    fast.allow_fused = ON | PLAIN_PREVIEWS
    assert L.ipk_pipeline_takes_fastpath(C.byref(fast), 1) == 1 and L.ipk_pipeline_scales_plain(C.byref(fast), 1) == 0


def test_refusals(L):
    d = _plain("mono", "u16", True)
    d.allow_fused = ON | PLAIN_PREVIEWS
    assert L.ipk_pipeline_scales_plain(None, 0) == INVALID
    assert L.ipk_pipeline_scales_plain(C.byref(d), 3) == INVALID
    small = sr._desc(9, 9, "", is_cfa=0, maxwidth=4)                      # ipk_pipeline_sizes refuses a source under 10x10
    small.allow_fused = ON | PLAIN_PREVIEWS
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(small), *[C.byref(v) for v in a]) < 0
    assert L.ipk_pipeline_scales_plain(C.byref(small), 0) < 0


@pytest.mark.parametrize("kind,src", [("mono", "u16"), ("cpp3", "f32")])
def test_regions_are_windowed_with_both_bits(L, orc, kind, src):
    x0, y0, cw, ch = orc.size_image(*SENSOR_CROPS, 131, 113)
    d = _plain(kind, src, True)
    d.allow_fused = ON | PREVIEWS | PLAIN_PREVIEWS
    dw, dh, fw, fh = _sizes(L, d)
    assert (fw, fh) == (dw, dh) and dw == 40
    for win in ((0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (5, 3, 17, 9), (0, 0, dw, dh)):
        gx, gy, gw, gh = _footprint(L, cw, ch, dw, dh, win)
        assert _region(L, d, *win) == (1, (x0 + gx, y0 + gy, gw, gh)), win
        for mask in (ON | PREVIEWS, ON | PLAIN_PREVIEWS, PREVIEWS | PLAIN_PREVIEWS, ON, 0):
            d0 = _plain(kind, src, True)
            d0.allow_fused = mask
            assert _region(L, d0, *win) == (0, (x0, y0, cw, ch)), (win, mask)


def test_hashes_do_not_see_the_bit(L):
    for kind in KINDS:
        for src in SRC:
            for kw in ({}, {"rotatecrop": RC}):
                a, b = _plain(kind, src, True, **kw), _plain(kind, src, True, **kw)
                a.allow_fused, b.allow_fused = ON, ON | PLAIN_PREVIEWS
                for out_type in (0, 1, 2):
                    ha, hb = C.create_string_buffer(256), C.create_string_buffer(256)
                    assert L.ipk_pipeline_hashes(C.byref(a), out_type, 5, ha) == 0 and L.ipk_pipeline_hashes(C.byref(b), out_type, 5, hb) == 0
                    assert ha.raw == hb.raw and ha.raw != bytes(256)


def test_bindings_carry_the_bit():
    import inspect
    import imagepipe_amd
    from imagepipe_amd import _lib
    assert _lib.FUSED_PLAIN_PREVIEWS == PLAIN_PREVIEWS
    src = inspect.getsource(imagepipe_amd.Pipeline)
    assert "self.scale_plain = False" in src and "d.allow_fused |= _lib.FUSED_PLAIN_PREVIEWS" in src
    assert callable(imagepipe_amd.Pipeline.scales_plain)
    for name in ("ipk_plain_scale_down", "ipk_plain_scale_down_window", "ipk_pipeline_scales_plain"):
        assert name in _lib.SIGNATURES
    for name in ("plain_scale_down", "plain_scale_down_window"):
        assert callable(getattr(imagepipe_amd, name)) and name in imagepipe_amd.__all__
