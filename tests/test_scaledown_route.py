"""The one-launch route through OpDemosaic's `full` + scale_down_opbuf branch (no GPU): which descriptors ipk_pipeline_fuses_scaledown sends there and
the descriptor field that opts in (the third layout's last reserved slot: nothing moved).  Every expectation is derived from the CPU oracle's own size
negotiation plus the f32 skips of src/scaling.rs:69-72, so a case that changes sides fails loudly."""
import ctypes as C

import numpy as np
import pytest

import util

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
W12 = (XT[0:6] + XT[18:24] + XT[6:12] + XT[24:30] + XT[12:18] + XT[30:36]) * 2 + (XT[18:24] + XT[0:6] + XT[24:30] + XT[6:12] + XT[30:36] + XT[12:18]) * 2
W12 = (W12 * 2)[:144]
INVALID = -2                                                              # IPK_ERR_INVALID
SENSOR_CROPS = (3, 1, 2, 5)                                               # top, right, bottom, left: odd offsets
NOCROP = (0, 0, 0, 0)
MINSCALE = {2: 2.0, 6: 3.0, 12: 12.0}                                     # src/ops/demosaic.rs:33-39 by the filter's width

# (width, height, sensor crops, maxwidth, maxheight, filters)
SMALL_TAKEN = {
    "131x97@87": (131, 97, NOCROP, 87, 0, ("RGGB", "GRBG", XT, W12)),
    "96x120c@h80": (96, 120, SENSOR_CROPS, 0, 80, ("RGGB", XT)),
    # skip_x exactly 2.0: 4-wide windows below a Bayer filter's minscale.  OpDemosaic's scale is the larger of the two sides' ratios against the
    # TRUNCATED demosaic size: 101x77 negotiates 51x38, 101 / 51 = 1.98 but 77 / 38 = 2.03, so that frame is this branch's only for filters whose
    # minscale is above 2 (and scaled_demosaic's for RGGB: test_route_refused); 101x103 negotiates 51x52, scale 1.98, both skips exactly 2.0
    "101x77@51": (101, 77, NOCROP, 51, 0, (XT, W12)),
    "101x103@51": (101, 103, NOCROP, 51, 0, ("RGGB", "GRBG", XT)),
    "131x97@130": (131, 97, NOCROP, 130, 0, ("RGGB", XT)),                # skips just above 1
    "150x100xt@60": (150, 100, NOCROP, 60, 0, (XT,)),                     # skips about 2.53
}
LARGE_TAKEN = {
    "24mp@3840": (6000, 4000, NOCROP, 3840, 0, ("RGGB",)),
    "100mp@6667": (10000, 10000, NOCROP, 6667, 0, ("RGGB",)),
    "26mp-xt@3840x2160": (6240, 4160, NOCROP, 3840, 2160, (XT,)),
}


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _desc(w, h, cfa="RGGB", crops=NOCROP, src_type=0, cpp=1, is_cfa=1, fuse=1, **kw):
    from imagepipe_amd._lib import PipelineDesc
    d = PipelineDesc()
    d.src_type, d.width, d.height, d.cpp, d.is_cfa = src_type, w, h, cpp, is_cfa
    d.cfa = cfa.encode()
    d.crop_top, d.crop_right, d.crop_bottom, d.crop_left = crops
    d.blacklevels[:] = [util.BLACK] * 4
    d.whitelevels[:] = [util.WHITE] * 4
    d.wb_coeffs[:] = util.WB
    d.cam_to_xyz_normalized[:] = [float(v) for v in util.cam_matrix().ravel()]
    d.allow_fused = 1
    d.fuse_scaledown = fuse
    for k, v in kw.items():
        if k == "rotatecrop":
            d.rotatecrop[:] = v
        else:
            setattr(d, k, v)
    return d


def _fuses(L, d, out_type=0):
    return L.ipk_pipeline_fuses_scaledown(C.byref(d), out_type)


def _cfa_width(cfa):
    return {4: 2, 36: 6, 144: 12}[len(cfa)]


def _negotiated(orc, w, h, crops, maxwidth, maxheight, rc=(0, 0, 0, 0, 0)):
    """(scale, skip_x, skip_y, dw, dh) from the oracle's own negotiation; the skips are scaling.rs:69-72 in f32 for scale_down_opbuf's corners"""
    desc = orc.make_pipeline(np.zeros((h, w), np.uint16), cfa="RGGB", crops=crops, rotatecrop=rc, maxwidth=maxwidth, maxheight=maxheight)
    (dw, dh), _ = orc.pipeline_sizes(desc)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    scale = orc.calculate_scaling_total(cw, ch, dw, dh)[0]
    f = np.float32
    with np.errstate(divide="ignore", invalid="ignore"):
        sx = (f(cw - 1) - f(0)) / f(dw - 1) if dw >= 1 else f(np.nan)
        sy = (f(ch - 1) - f(0)) / f(dh - 1) if dh >= 1 else f(np.nan)
    return scale, float(sx), float(sy), dw, dh


def _oracle_says(orc, w, h, crops, maxwidth, maxheight, cfa):
    scale, sx, sy, dw, dh = _negotiated(orc, w, h, crops, maxwidth, maxheight)
    if not (1.0 < scale < MINSCALE[_cfa_width(cfa)]) or dw < 2 or dh < 2:
        return 0
    return int(all(np.isfinite(s) and 1.0 <= s < 3.0 for s in (sx, sy)) and max(w, h) < 2 ** 24)


@pytest.mark.parametrize("case", list(SMALL_TAKEN) + list(LARGE_TAKEN))
def test_route_taken(L, orc, case):
    w, h, crops, mw, mh, cfas = {**SMALL_TAKEN, **LARGE_TAKEN}[case]
    for cfa in cfas:
        assert _oracle_says(orc, w, h, crops, mw, mh, cfa) == 1, "the oracle's negotiation moved: %s %s" % (case, cfa[:6])
        for src_type in (0, 1):
            for out_type in (0, 1, 2):
                d = _desc(w, h, cfa, crops, src_type=src_type, maxwidth=mw, maxheight=mh)
                assert _fuses(L, d, out_type) == 1, (case, cfa[:6], src_type, out_type)
                # OpDemosaic scales: the rotatecrop report keeps answering 0, whatever its own flag says
                d.fuse_rotatecrop = 1
                assert L.ipk_pipeline_fuses_rotatecrop(C.byref(d), out_type) == 0
                assert _fuses(L, d, out_type) == 1
        assert _fuses(L, _desc(w, h, cfa, crops, maxwidth=mw, maxheight=mh, fuse=0)) == 0, "flag 0 is the staged route"


def test_the_cases_cover_what_they_claim(orc):
    """the properties the case list is chosen for, from the oracle's negotiation"""
    scale, sx, sy, dw, dh = _negotiated(orc, 101, 77, NOCROP, 51, 0)
    assert 2.0 < scale < 2.03 and sx == 2.0 and (dw, dh) == (51, 38)       # windows floor(2c) ..= floor(2c + 2): four wide
    scale, sx, sy, dw, dh = _negotiated(orc, 101, 103, NOCROP, 51, 0)
    assert 1.98 < scale < 2.0 and sx == 2.0 and sy == 2.0 and (dw, dh) == (51, 52)   # the same below a Bayer filter's minscale
    scale, sx, sy, _, _ = _negotiated(orc, 131, 97, NOCROP, 130, 0)
    assert 1.0 < scale < 1.02 and 1.0 < sx < 1.02 and 1.0 < sy < 1.02
    scale, sx, sy, _, _ = _negotiated(orc, 150, 100, NOCROP, 60, 0)
    assert 2.5 <= scale < 2.6 and 2.5 < sx < 2.6 and 2.5 < sy < 2.6
    assert abs(_negotiated(orc, 6000, 4000, NOCROP, 3840, 0)[0] - 1.5625) < 1e-6
    assert abs(_negotiated(orc, 10000, 10000, NOCROP, 6667, 0)[0] - 1.5) < 1e-3
    assert abs(_negotiated(orc, 6240, 4160, NOCROP, 3840, 2160)[0] - 1.926) < 1e-3


def test_route_refused(L, orc):
    w, h, mw = 131, 97, 87
    assert _fuses(L, _desc(w, h, maxwidth=mw)) == 1                                         # the control
    assert _fuses(L, _desc(w, h, maxwidth=mw, fuse=0)) == 0
    assert _fuses(L, _desc(w, h, maxwidth=mw, allow_fused=0)) == 0
    assert _fuses(L, _desc(w, h, "RGBE", maxwidth=mw)) == 0                                 # a fourth colour
    assert _fuses(L, _desc(w, h, "", is_cfa=0, maxwidth=mw)) == 0                           # a mono raw
    assert _fuses(L, _desc(w, h, "", cpp=3, is_cfa=0, maxwidth=mw)) == 0                    # a three-sample raw
    for src_type in (2, 3):                                                                 # raster sources
        assert _fuses(L, _desc(w, h, "", src_type=src_type, cpp=3, is_cfa=0, maxwidth=mw)) == 0
    # an active rotatecrop behind a scaling OpDemosaic: a second resampling, staged
    rc = tuple(float(np.float32(x)) for x in (0.05, 0.05, 0.05, 0.05, 0))
    assert _negotiated(orc, w, h, NOCROP, 80, 0, rc)[0] > 1.0
    assert _fuses(L, _desc(w, h, maxwidth=80, rotatecrop=rc)) == 0
    # scale <= 1: no size limit, and a limit above the frame
    for lim in (0, 131, 200):
        assert _oracle_says(orc, w, h, NOCROP, lim, 0, "RGGB") == 0
        assert _fuses(L, _desc(w, h, maxwidth=lim)) == 0
    # RGGB at scale >= 2 is scaled_demosaic's branch; the same size is this route's for X-Trans (minscale 3)
    assert _negotiated(orc, w, h, NOCROP, 60, 0)[0] >= 2.0 and _oracle_says(orc, w, h, NOCROP, 60, 0, "RGGB") == 0
    assert _fuses(L, _desc(w, h, maxwidth=60)) == 0
    assert _oracle_says(orc, w, h, NOCROP, 60, 0, XT) == 1 and _fuses(L, _desc(w, h, XT, maxwidth=60)) == 1
    assert _negotiated(orc, 101, 77, NOCROP, 51, 0)[0] >= 2.0 and _oracle_says(orc, 101, 77, NOCROP, 51, 0, "RGGB") == 0   # 101 / 51 < 2, but 77 / 38 > 2
    assert _fuses(L, _desc(101, 77, maxwidth=51)) == 0
    # 150x100 X-Trans at maxwidth 52: scale 2.94 (150 / 52 = 2.88, 100 / 34 = 2.94) < 3, but the rows' skip is 99 / 33 = 3.0 -- admission goes by the skips
    scale, sx, sy, dw, dh = _negotiated(orc, 150, 100, NOCROP, 52, 0)
    assert 2.88 < scale < 3.0 and sy == 3.0 and (dw, dh) == (52, 34)
    assert _oracle_says(orc, 150, 100, NOCROP, 52, 0, XT) == 0
    assert _fuses(L, _desc(150, 100, XT, maxwidth=52)) == 0
    # a negotiated height of 1 (only a 12-wide filter's minscale lets one through OpDemosaic's test)
    scale, sx, sy, dw, dh = _negotiated(orc, 44, 11, NOCROP, 0, 1)
    assert 1.0 < scale < 12.0 and dh == 1 and dw >= 2
    assert _oracle_says(orc, 44, 11, NOCROP, 0, 1, W12) == 0
    assert _fuses(L, _desc(44, 11, W12, maxheight=1)) == 0


def test_route_report_fails_like_the_size_negotiation(L):
    for d in (_desc(5, 5, maxwidth=3), _desc(131, 97, maxwidth=87, rotation=7)):
        a = [C.c_size_t() for _ in range(4)]
        want = L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a])
        assert want < 0 and _fuses(L, d) == want
    assert _fuses(L, _desc(131, 97, maxwidth=87), out_type=3) == INVALID
    assert L.ipk_pipeline_fuses_scaledown(None, 0) == INVALID


def test_flag_lives_in_the_last_reserved_slot(L):
    from imagepipe_amd._lib import PipelineDesc
    assert PipelineDesc.fuse_scaledown.offset == PipelineDesc.reserved1.offset + 4
    assert PipelineDesc.reserved1.offset == PipelineDesc.fuse_rotatecrop.offset + 4
    assert C.sizeof(PipelineDesc) == L.ipk_abi_sizeof(1)
    assert PipelineDesc._fields_[-1][0] == "fuse_scaledown" and C.sizeof(PipelineDesc) - PipelineDesc.fuse_scaledown.offset in (4, 8)   # the last field (+ tail padding)
    assert PipelineDesc().fuse_scaledown == 0                                               # a fresh descriptor keeps today's behaviour
    # an object of the second layout (it ends in front of `schedule`) with poison behind its end: the field is not read
    d = _desc(131, 97, maxwidth=87, fuse=1)
    assert _fuses(L, d) == 1
    d.struct_size = PipelineDesc.schedule.offset
    assert _fuses(L, d) == 0
    d.fuse_scaledown = 77
    assert _fuses(L, d) == 0
    # values other than 0 and 1 stay free, for this report and for the one next to it
    for v in (2, -1, 256):
        d = _desc(131, 97, maxwidth=87, fuse=v)
        assert _fuses(L, d) == INVALID
        assert L.ipk_pipeline_fuses_rotatecrop(C.byref(d), 0) == INVALID
        assert L.ipk_pipeline_hashes(C.byref(d), 0, 0, C.create_string_buffer(256)) == INVALID


def test_flag_does_not_enter_the_hashes(L):
    a, b = C.create_string_buffer(256), C.create_string_buffer(256)
    assert L.ipk_pipeline_hashes(C.byref(_desc(131, 97, maxwidth=87, fuse=0)), 0, 5, a) == 0
    assert L.ipk_pipeline_hashes(C.byref(_desc(131, 97, maxwidth=87, fuse=1)), 0, 5, b) == 0
    assert a.raw == b.raw


def test_python_pipeline_passes_the_flag():
    import inspect
    import imagepipe_amd
    src = inspect.getsource(imagepipe_amd.Pipeline)
    assert "self.fuse_scaledown = False" in src and "d.fuse_scaledown = int(self.fuse_scaledown)" in src
    assert callable(imagepipe_amd.raw_to_srgb_scaled) and callable(imagepipe_amd.Pipeline.fuses_scaledown)
