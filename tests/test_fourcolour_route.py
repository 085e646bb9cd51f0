"""The one-launch route for filters with a fourth colour (no GPU): which descriptors ipk_pipeline_fuses_four_colour sends there, that the opt-in
(bit 1 of allow_fused, IPK_FUSED_FOUR_COLOUR) changes neither the hashes nor any layout, that a region of such a descriptor is windowed over the
sensor window a Bayer frame of that geometry reads, and where ipk_fused_params.four_colour sits (the formerly reserved slot: nothing moved)."""
import ctypes as C

import pytest

import util

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
L16 = "RGBGRBGGGBGRGRBG"                                                   # sixteen letters without E: a three-colour tile
E16 = "RGBERGBEGRBEGREB"                                                   # sixteen letters, four colours
FOUR = ["RGBE", "ERBG", "8x2:" + E16, "2x8:" + E16]
THREE = ["RGGB", "GRBG", XT, "8x2:" + L16]
INVALID = -2                                                               # IPK_ERR_INVALID
ON, FOUR_COLOUR = 1, 2                                                     # IPK_FUSED_ON, IPK_FUSED_FOUR_COLOUR


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _desc(w, h, cfa="RGBE", crops=(0, 0, 0, 0), src_type=0, cpp=1, is_cfa=1, allow_fused=ON | FOUR_COLOUR, **kw):
    from imagepipe_amd._lib import PipelineDesc
    d = PipelineDesc()
    d.src_type, d.width, d.height, d.cpp, d.is_cfa = src_type, w, h, cpp, is_cfa
    d.cfa = cfa.encode()
    d.crop_top, d.crop_right, d.crop_bottom, d.crop_left = crops
    d.blacklevels[:] = [util.BLACK] * 4
    d.whitelevels[:] = [util.WHITE] * 4
    d.wb_coeffs[:] = util.WB
    d.cam_to_xyz_normalized[:] = [float(v) for v in util.cam_matrix().ravel()]
    d.allow_fused = allow_fused
    for k, v in kw.items():
        if k == "rotatecrop":
            d.rotatecrop[:] = v
        else:
            setattr(d, k, v)
    return d


def _fuses(L, d, out_type=0):
    return L.ipk_pipeline_fuses_four_colour(C.byref(d), out_type)


def _region(L, d, x, y, w, h, out_type=0):
    s = [C.c_size_t() for _ in range(4)]
    rc = L.ipk_pipeline_region(C.byref(d), out_type, x, y, w, h, *[C.byref(v) for v in s])
    return rc, tuple(v.value for v in s)


@pytest.mark.parametrize("cfa", FOUR)
def test_four_colour_filters_take_the_route_with_the_bit(L, cfa):
    for src_type in (0, 1):
        for out_type in (0, 1, 2):
            for geometry in (dict(), dict(crops=(3, 1, 2, 5)), dict(rotation=1), dict(rotation=2, fliph=1), dict(flipv=1)):
                assert _fuses(L, _desc(61, 47, cfa, src_type=src_type, **geometry), out_type) == 1, (cfa, src_type, out_type, geometry)
    assert _fuses(L, _desc(61, 47, cfa, allow_fused=FOUR_COLOUR)) == 1          # any non-zero allow_fused keeps its meaning; bit 1 adds the filters
    for allow in (0, ON):
        assert _fuses(L, _desc(61, 47, cfa, allow_fused=allow)) == 0, (cfa, allow)


def test_the_tile_shape_may_come_from_the_descriptor(L):
    assert _fuses(L, _desc(61, 47, E16, cfa_width=8, cfa_height=2)) == 1
    assert _fuses(L, _desc(61, 47, E16, cfa_width=2, cfa_height=8)) == 1


@pytest.mark.parametrize("cfa", THREE)
def test_three_colour_filters_answer_0(L, cfa):
    """their own one-launch route does not depend on the bit, and this report is about the fourth colour"""
    for allow in (0, ON, ON | FOUR_COLOUR):
        assert _fuses(L, _desc(61, 47, cfa, allow_fused=allow)) == 0
    # ... and their route is what it was: windowed regions with and without the bit
    assert _region(L, _desc(61, 47, cfa, allow_fused=ON), 3, 5, 17, 9) == _region(L, _desc(61, 47, cfa), 3, 5, 17, 9)
    assert _region(L, _desc(61, 47, cfa), 3, 5, 17, 9)[0] == 1


@pytest.mark.parametrize("kw", [dict(cpp=3, is_cfa=0), dict(is_cfa=0, cfa=""), dict(is_cfa=0), dict(src_type=2, cpp=3, is_cfa=0, cfa=""),
                                dict(src_type=3, cpp=3, is_cfa=0, cfa=""), dict(rotatecrop=(0.1, 0.05, 0.2, 0.0, 0.0)),
                                dict(rotatecrop=(0.0, 0.0, 0.0, 0.0, 0.3)), dict(maxwidth=40), dict(maxwidth=90), dict(maxheight=33)])
def test_route_refused(L, kw):
    """three samples per pixel, mono, raster sources, an active rotatecrop, a scaling demosaic (100 / 90 = 1.11 and 100 / 40 = 2.5: both branches)"""
    kw = dict(kw)
    d = _desc(100, 120, kw.pop("cfa", "RGBE"), **kw)
    assert _fuses(L, d) == 0
    assert _fuses(L, d, 1) == 0


def test_refused_descriptors_answer_a_negative_code(L):
    for d in (_desc(5, 5, maxwidth=3), _desc(61, 47, rotation=7)):
        a = [C.c_size_t() for _ in range(4)]
        want = L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a])
        assert want < 0 and _fuses(L, d) == want
    assert _fuses(L, _desc(100, 120, "RGXB")) <= 0                          # an unknown letter never takes the route
    assert _fuses(L, _desc(100, 120, E16)) <= 0                             # nor do sixteen letters without a stated shape
    assert _fuses(L, _desc(100, 120, fuse_scaledown=2)) == INVALID
    assert L.ipk_pipeline_fuses_four_colour(None, 0) == INVALID
    assert _fuses(L, _desc(100, 120), 3) == INVALID


@pytest.mark.parametrize("geometry", [dict(), dict(crops=(3, 1, 2, 5)), dict(crops=(3, 1, 2, 5), rotation=1), dict(rotation=3, fliph=1), dict(rotation=2, flipv=1)])
@pytest.mark.parametrize("cfa", FOUR)
def test_regions_are_windowed_like_a_bayer_frame_of_that_geometry(L, cfa, geometry):
    d4, d3 = _desc(61, 47, cfa, **geometry), _desc(61, 47, "RGGB", allow_fused=ON, **geometry)
    a, b, c, e = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.ipk_pipeline_sizes(C.byref(d4), C.byref(a), C.byref(b), C.byref(c), C.byref(e)) == 0
    fw, fh = c.value, e.value
    for x, y, w, h in [(0, 0, 1, 1), (fw - 1, fh - 1, 1, 1), (3, 5, 17, 9), (0, 7, fw, 1), (9, 0, 1, fh), (0, 0, fw, fh)]:
        for out_type in (0, 1, 2):
            got, want = _region(L, d4, x, y, w, h, out_type), _region(L, d3, x, y, w, h, out_type)
            assert got[0] == 1 and got == want, (x, y, w, h, out_type)
    # without the bit: the whole-frame route and the whole crop window, as before
    cr = geometry.get("crops", (0, 0, 0, 0))
    d4.allow_fused = ON
    assert _region(L, d4, 3, 5, 17, 9) == (0, (cr[3], cr[0], 61 - cr[1] - cr[3], 47 - cr[0] - cr[2]))


@pytest.mark.parametrize("cfa", FOUR + ["RGGB", XT])
def test_hashes_do_not_depend_on_the_bit(L, cfa):
    out = []
    for allow in (ON, ON | FOUR_COLOUR, 0):
        buf = C.create_string_buffer(256)
        assert L.ipk_pipeline_hashes(C.byref(_desc(61, 47, cfa, allow_fused=allow)), 0, 7, buf) == 0
        out.append(buf.raw)
    assert out[0] == out[1] == out[2] and any(out[0])


def test_the_flag_fills_the_reserved_slot_and_no_layout_moved(L):
    from imagepipe_amd._lib import FusedParams, PipelineDesc
    assert FusedParams.four_colour.offset == L.ipk_abi_sizeof(20) + 4          # behind `schedule`
    assert FusedParams._fields_[-1][0] == "four_colour" and FusedParams().four_colour == 0
    assert C.sizeof(FusedParams) == L.ipk_abi_sizeof(0) and C.sizeof(FusedParams) - FusedParams.four_colour.offset in (4, 8)
    assert C.sizeof(PipelineDesc) == L.ipk_abi_sizeof(1)
    assert PipelineDesc.schedule.offset == L.ipk_abi_sizeof(21) and PipelineDesc.allow_fused.offset == L.ipk_abi_sizeof(19) - 4


def test_python_pipeline_mirror(L):
    """Pipeline.fuse_four_colour sets the bit (only next to allow_fused) and fuses_four_colour() asks the library; no GPU, so no Pipeline.new_from_source"""
    import numpy as np
    import imagepipe_amd as ipa
    img = ipa.RawImage(width=40, height=36, data=None, cfa="RGBE", blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4, wb_coeffs=util.WB,
                       cam_to_xyz_normalized=util.cam_matrix())
    pipe = ipa.Pipeline(img)
    assert pipe.fuse_four_colour is False and pipe.desc().allow_fused == 1 and pipe.fuses_four_colour() is False
    pipe.fuse_four_colour = True
    assert pipe.desc().allow_fused == 3 and pipe.fuses_four_colour() is True and pipe.fuses_four_colour(ipa.OUT_U8) is True
    pipe.allow_fused = False
    assert pipe.desc().allow_fused == 0 and pipe.fuses_four_colour() is False
