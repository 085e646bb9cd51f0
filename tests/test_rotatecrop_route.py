"""The one-launch route through an active OpRotateCrop (no GPU): which descriptors ipk_pipeline_fuses_rotatecrop sends there, the descriptor
field that opts in (the third layout's formerly reserved slot: nothing moved), and the register budget of the six k_fused_resample kernels.
Every expectation of the route report is also derived from the CPU oracle's size negotiation, so a case that changes sides fails loudly."""
import ctypes as C
import re

import numpy as np
import pytest

import util

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
W12 = (XT[0:6] + XT[18:24] + XT[6:12] + XT[24:30] + XT[12:18] + XT[30:36]) * 2 + (XT[18:24] + XT[0:6] + XT[24:30] + XT[6:12] + XT[30:36] + XT[12:18]) * 2
W12 = (W12 * 2)[:144]
INVALID = -2                                                              # IPK_ERR_INVALID
SENSOR_CROPS = (3, 1, 2, 5)                                               # top, right, bottom, left: odd offsets


def f32s(*v):
    return tuple(float(np.float32(x)) for x in v)


# (crop_top, crop_right, crop_bottom, crop_left, rotation): crop-only, small and steep angles, windows that are mostly empty (0.77, 1.0, 1.3)
R9 = [f32s(0.05, 0.05, 0.05, 0.05, 0), f32s(0.1, 0.05, 0.2, 0, 0), f32s(0, 0, 0, 0, 0.04), f32s(0.1, 0, 0, 0, 0.2), f32s(0, 0, 0, 0, 0.5),
      f32s(0.02, 0.03, 0.01, 0.02, 0.77), f32s(0, 0, 0, 0, 1.0), f32s(0, 0, 0, 0, 1.3), f32s(0.07, 0.11, 0.05, 0.02, 0.04)]
# (width, height, sensor crops): every R9 setting negotiates a demosaic size >= the cropped frame on these
VERIFIED_FRAMES = [(47, 61, (0, 0, 0, 0)), (96, 120, SENSOR_CROPS)]
LARGE_TAKEN = [(6000, 4000, (0, 0, 0, 0), f32s(0.05, 0.05, 0.05, 0.05, 0)), (6000, 4000, (0, 0, 0, 0), f32s(0, 0, 0, 0, 1.0 / 30.0)),
               (6024, 4016, (0, 0, 0, 0), f32s(0.013, 0.021, 0.017, 0.009, 0.011)), (10000, 10000, (0, 0, 0, 0), f32s(0.02, 0.03, 0.01, 0.02, 0.1))]
# the reverse size fold lands one pixel short of the source: OpDemosaic scales, the frame stays staged
ONE_SHORT = [(6000, 4000, (0, 0, 0, 0), f32s(0, 0, 0, 0, 0.05)), (6000, 4000, (0, 0, 0, 0), f32s(0.03, 0.02, 0.04, 0.01, 0.02)),
             (150, 100, (0, 0, 0, 0), f32s(0.04, 0.01, 0.03, 0.02, 0.02)),
             (131, 97, (0, 0, 0, 0), f32s(0.1, 0, 0, 0, 0.2)), (108, 72, (0, 0, 0, 0), f32s(0.1, 0.05, 0.2, 0, 0)),
             (108, 72, (0, 0, 0, 0), f32s(0.07, 0.11, 0.05, 0.02, 0.04)), (150, 100, (0, 0, 0, 0), f32s(0.02, 0.03, 0.01, 0.02, 0.77)),
             (96, 120, (0, 0, 0, 0), f32s(0.1, 0, 0, 0, 0.2)), (131, 97, SENSOR_CROPS, f32s(0.1, 0.05, 0.2, 0, 0)),
             (150, 100, SENSOR_CROPS, f32s(0.1, 0, 0, 0, 0.2)), (150, 100, SENSOR_CROPS, f32s(0.07, 0.11, 0.05, 0.02, 0.04))]


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _desc(w, h, cfa="RGGB", crops=(0, 0, 0, 0), src_type=0, cpp=1, is_cfa=1, fuse=1, **kw):
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
    d.fuse_rotatecrop = fuse
    for k, v in kw.items():
        if k == "rotatecrop":
            d.rotatecrop[:] = v
        else:
            setattr(d, k, v)
    return d


def _fuses(L, d, out_type=0):
    return L.ipk_pipeline_fuses_rotatecrop(C.byref(d), out_type)


def _oracle_says(orc, w, h, crops, rc, maxwidth=0):
    """the route from the oracle's own negotiation: OpDemosaic does not scale, OpRotateCrop accepts its crops, and the transform's windows are
    at most 3x3 (the skips of src/scaling.rs:68-71 in f32)"""
    desc = orc.make_pipeline(np.zeros((h, w), np.uint16), cfa="RGGB", crops=crops, rotatecrop=rc, maxwidth=maxwidth)
    (dw, dh), _ = orc.pipeline_sizes(desc)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    scale = orc.calculate_scaling_total(cw, ch, dw, dh)[0]
    corners = orc.rotatecrop_corners(rc, cw, ch)
    if corners is None or scale > 1.0:
        return 0
    tl, tr, bl, nw, nh = corners
    if nw < 2 or nh < 2:
        return 0
    f = np.float32
    sxx, sxy = (f(tr[0]) - f(tl[0])) / f(nw - 1), (f(tr[1]) - f(tl[1])) / f(nw - 1)
    syx, syy = (f(bl[0]) - f(tl[0])) / f(nh - 1), (f(bl[1]) - f(tl[1])) / f(nh - 1)
    return int(abs(float(sxx)) + abs(float(syx)) < 2.0 and abs(float(sxy)) + abs(float(syy)) < 2.0)


@pytest.mark.parametrize("frame", VERIFIED_FRAMES, ids=["47x61", "96x120-cropped"])
@pytest.mark.parametrize("rc", R9, ids=[str(i) for i in range(len(R9))])
def test_route_taken_on_the_verified_frames(L, orc, frame, rc):
    w, h, crops = frame
    assert _oracle_says(orc, w, h, crops, rc) == 1, "the oracle's negotiation moved: %r %r" % (frame, rc)
    for cfa in ("RGGB", "GRBG", XT, W12):
        for src_type in (0, 1):
            for out_type in (0, 1, 2):
                assert _fuses(L, _desc(w, h, cfa, crops, src_type=src_type, rotatecrop=rc), out_type) == 1, (cfa[:6], src_type, out_type)
    assert _fuses(L, _desc(w, h, "RGGB", crops, rotatecrop=rc, fuse=0)) == 0, "flag 0 is the staged route"


@pytest.mark.parametrize("case", LARGE_TAKEN, ids=["24mp-crop5", "24mp-rot1/30", "6024x4016", "100mp"])
def test_route_taken_at_full_size(L, orc, case):
    w, h, crops, rc = case
    assert _oracle_says(orc, w, h, crops, rc) == 1
    for cfa, src_type, out_type in (("RGGB", 1, 0), ("RGGB", 0, 1), (XT, 1, 0), (W12, 0, 2)):
        assert _fuses(L, _desc(w, h, cfa, crops, src_type=src_type, rotatecrop=rc), out_type) == 1


@pytest.mark.parametrize("case", ONE_SHORT, ids=["%dx%d-%d" % (c[0], c[1], i) for i, c in enumerate(ONE_SHORT)])
def test_one_pixel_short_negotiations_stay_staged(L, orc, case):
    w, h, crops, rc = case
    assert _oracle_says(orc, w, h, crops, rc) == 0, "the oracle's negotiation moved: %r" % (case,)
    desc = orc.make_pipeline(np.zeros((h, w), np.uint16), cfa="RGGB", crops=crops, rotatecrop=rc)
    (dw, dh), _ = orc.pipeline_sizes(desc)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    assert (dw, dh) != (cw, ch) and orc.calculate_scaling_total(cw, ch, dw, dh)[0] > 1.0, "it is OpDemosaic's scale that keeps the frame staged"
    for cfa in ("RGGB", XT):
        for src_type in (0, 1):
            assert _fuses(L, _desc(w, h, cfa, crops, src_type=src_type, rotatecrop=rc)) == 0


def test_route_refused(L, orc):
    rc = R9[3]
    w, h = 47, 61
    assert _fuses(L, _desc(w, h, rotatecrop=rc)) == 1                                       # the control
    assert _fuses(L, _desc(w, h, rotatecrop=rc, fuse=0)) == 0
    assert _fuses(L, _desc(w, h, rotatecrop=rc, allow_fused=0)) == 0
    assert _fuses(L, _desc(w, h, "RGBE", rotatecrop=rc)) == 0                               # a fourth colour
    assert _fuses(L, _desc(w, h, "", is_cfa=0, rotatecrop=rc)) == 0                         # a mono raw
    assert _fuses(L, _desc(w, h, "", cpp=3, is_cfa=0, rotatecrop=rc)) == 0                  # a three-sample raw
    for src_type in (2, 3):                                                                 # raster sources
        assert _fuses(L, _desc(w, h, "", src_type=src_type, cpp=3, is_cfa=0, rotatecrop=rc)) == 0
    assert _oracle_says(orc, w, h, (0, 0, 0, 0), rc, maxwidth=20) == 0
    assert _fuses(L, _desc(w, h, rotatecrop=rc, maxwidth=20)) == 0                          # OpDemosaic scales
    assert _fuses(L, _desc(w, h, rotatecrop=f32s(0, 0, 0, 0, 0))) == 0                      # a no-op rotatecrop is the plain fused route
    assert _fuses(L, _desc(w, h, rotatecrop=f32s(0, 0, 0, 0, 1e-7))) == 0
    # a crop outside the image: corners() fails, the op returns its input
    neg = f32s(0, 0, 0, -0.1, 0)
    assert orc.rotatecrop_corners(neg, 60, 40) is None and _oracle_says(orc, 60, 40, (0, 0, 0, 0), neg) == 0
    assert _fuses(L, _desc(60, 40, rotatecrop=neg)) == 0


def test_route_report_fails_like_the_size_negotiation(L):
    for d in (_desc(5, 5, rotatecrop=R9[0]), _desc(47, 61, rotatecrop=R9[0], rotation=7)):
        a = [C.c_size_t() for _ in range(4)]
        want = L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a])
        assert want < 0 and _fuses(L, d) == want
    assert _fuses(L, _desc(47, 61, rotatecrop=R9[0]), out_type=3) == INVALID
    assert L.ipk_pipeline_fuses_rotatecrop(None, 0) == INVALID


def test_flag_lives_in_the_reserved_slot(L):
    from imagepipe_amd._lib import PipelineDesc
    assert PipelineDesc.fuse_rotatecrop.offset == PipelineDesc.schedule.offset + 4
    assert PipelineDesc.reserved1.offset == PipelineDesc.fuse_rotatecrop.offset + 4
    assert C.sizeof(PipelineDesc) == L.ipk_abi_sizeof(1)
    assert L.ipk_abi_sizeof(21) == PipelineDesc.schedule.offset
    assert PipelineDesc().fuse_rotatecrop == 0                                              # a fresh descriptor keeps today's behaviour
    rc = R9[3]
    # an object of the second layout (it ends in front of `schedule`) with poison behind its end: the field is not read
    d = _desc(47, 61, rotatecrop=rc, fuse=1)
    assert _fuses(L, d) == 1
    d.struct_size = PipelineDesc.schedule.offset
    assert _fuses(L, d) == 0
    # values other than 0 and 1 stay free
    for v in (2, -1, 256):
        assert _fuses(L, _desc(47, 61, rotatecrop=rc, fuse=v)) == INVALID


def test_python_pipeline_passes_the_flag():
    import inspect
    import imagepipe_amd
    src = inspect.getsource(imagepipe_amd.Pipeline)
    assert "self.fuse_rotatecrop = False" in src and "d.fuse_rotatecrop = int(self.fuse_rotatecrop)" in src


def test_resample_kernels_fit_one_block_per_cu():
    """six kernels (u16 / f32 source x f32 / u8 / u16 output), 1024 threads each: at most 128 VGPRs, no scratch, no spills"""
    import test_kernel_resources
    ks = [k for k in test_kernel_resources._kernels() if re.search(r"k_fused_resample<", k[0])]
    names = sorted(re.sub(r"\(.*$", "", k[0].replace("void ipk::", "")) for k in ks)
    assert names == sorted("k_fused_resample<%s, %d>" % (t, o) for t in ("float", "unsigned short") for o in (0, 1, 2)), names
    for name, vgpr, scratch, spills in ks:
        assert vgpr <= 128 and scratch == 0 and spills == 0, (name, vgpr, scratch, spills)
