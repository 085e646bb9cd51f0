"""IPK_FUSED_SCALED_ROTATECROP (bit 6 of allow_fused) without a GPU: which descriptors ipk_pipeline_fuses_scaled_rotatecrop sends to the two-launch route
(the scaling gofloat + demosaic pass, then one resampling launch over its RGBE buffer), that the bit needs IPK_FUSED_ON beside it, that no other report,
no region answer outside the route and no hash depends on it, and that the sensor window a region reports is all the region depends on (CPU oracle)."""
import ctypes as C

import numpy as np
import pytest

import util
import test_scaledown_route as sr
from test_scaledown_route import XT, INVALID, NOCROP, MINSCALE

ON, SRC = 1, 64
F = lambda *v: [float(np.float32(x)) for x in v]
CROPS_RC = (0.1, 0.05, 0.2, 0.0)
SENSOR_CROPS = (1, 3, 2, 5)
ANGLES = (0.0, 0.03, 0.3)
REPORTS = ("ipk_pipeline_fuses_rotatecrop", "ipk_pipeline_fuses_scaledown", "ipk_pipeline_fuses_four_colour", "ipk_pipeline_fuses_plain",
           "ipk_pipeline_windows_preview", "ipk_pipeline_takes_fastpath", "ipk_pipeline_resamples_cached_region")


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _desc(w, h, cfa="RGGB", crops=NOCROP, mask=ON | SRC, **kw):
    d = sr._desc(w, h, cfa, crops, fuse=0, **kw)
    d.allow_fused = mask
    return d


def _raster(w, h, src_type=2, mask=ON | SRC, **kw):
    return _desc(w, h, "", src_type=src_type, cpp=3, is_cfa=0, mask=mask, **kw)


def _asks(L, d, out_type=0):
    return L.ipk_pipeline_fuses_scaled_rotatecrop(C.byref(d), out_type)


def _sizes(L, d):
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
    return (a[0].value, a[1].value), (a[2].value, a[3].value)


def _scale(orc, w, h, crops, maxwidth, rc):
    return sr._negotiated(orc, w, h, crops, maxwidth, 0, rc)


def test_the_constant_and_the_symbols(L):
    from imagepipe_amd import _lib
    assert _lib.FUSED_SCALED_ROTATECROP == 64
    for name in ("ipk_pipeline_fuses_scaled_rotatecrop", "ipk_raw_demosaic_scaled", "ipk_raw_demosaic_scaled_window"):
        assert hasattr(L, name)


@pytest.mark.parametrize("angle", [0.02, 0.05])
def test_a_straightened_24mp_frame(L, orc, angle):
    rc = F(0, 0, 0, 0, angle)
    d = _desc(6000, 4000, rotatecrop=rc)
    assert _sizes(L, d)[0] == (5999, 3999) == orc.pipeline_sizes(orc.make_pipeline(np.zeros((4000, 6000), np.uint16), cfa="RGGB", rotatecrop=rc))[0]
    for src_type in (0, 1):
        for out_type in (0, 1, 2):
            d = _desc(6000, 4000, rotatecrop=rc, src_type=src_type)
            assert _asks(L, d, out_type) == 1
            d.fuse_rotatecrop = 1                                          # OpDemosaic scales: fuse_rotatecrop's route keeps refusing the frame
            assert L.ipk_pipeline_fuses_rotatecrop(C.byref(d), out_type) == 0 and _asks(L, d, out_type) == 1
    # with crops the reverse fold lands a pixel LONG: scale <= 1 is fuse_rotatecrop's ground
    rcc = F(*CROPS_RC, angle)
    d = _desc(6000, 4000, rotatecrop=rcc)
    assert _sizes(L, d)[0] == (6001, 4001)
    assert _asks(L, d) == 0
    d.fuse_rotatecrop = 1
    assert L.ipk_pipeline_fuses_rotatecrop(C.byref(d), 0) == 1


@pytest.mark.parametrize("angle", ANGLES)
@pytest.mark.parametrize("maxwidth", [180, 150, 100])
def test_straightened_previews(L, orc, maxwidth, angle):
    rc = F(*CROPS_RC, angle)
    scale, _, _, dw, dh = _scale(orc, 342, 150, NOCROP, maxwidth, rc)
    lo, hi = {180: (1.805, 1.985), 150: (2.165, 2.395), 100: (3.0, 99.0)}[maxwidth]          # 1.81-1.98, 2.17-2.39 to two places
    assert lo <= scale <= hi, scale
    for cfa in ("RGGB", XT):
        # pass 1: the scaled_demosaic kernels from minscale up, the RGBE output mode below it (skips below 3 there: admitted)
        below = scale < MINSCALE[sr._cfa_width(cfa)]
        assert below == {(180, 2): True, (180, 6): True, (150, 2): False, (150, 6): True, (100, 2): False, (100, 6): False}[(maxwidth, sr._cfa_width(cfa))]
        for src_type in (0, 1):
            d = _desc(342, 150, cfa, rotatecrop=rc, maxwidth=maxwidth, src_type=src_type)
            assert _sizes(L, d)[0] == (dw, dh)
            for out_type in (0, 1, 2):
                assert _asks(L, d, out_type) == 1, (cfa[:4], maxwidth, angle, src_type, out_type)
            d.fuse_scaledown = d.fuse_rotatecrop = 1                       # the one-launch routes do not take these frames
            assert L.ipk_pipeline_fuses_scaledown(C.byref(d), 0) == 0 and L.ipk_pipeline_fuses_rotatecrop(C.byref(d), 0) == 0


def test_small_shapes_one_pixel_short(L, orc):
    for w, h, rc, want in ((108, 62, F(0, 0, 0, 0, 0.02), (107, 61)), (262, 140, F(*CROPS_RC, 1.0), (261, 139))):
        d = _desc(w, h, rotatecrop=rc)
        assert _sizes(L, d)[0] == want and _asks(L, d) == 1
    assert _sizes(L, _desc(262, 140, rotatecrop=F(*CROPS_RC, 1.0)))[1] == (132, 183)
    # rasters: OpGoFloat::run_other + scale_down_opbuf is the one pass
    for src_type in (2, 3):
        d = _raster(200, 120, src_type, rotatecrop=F(*CROPS_RC, 0.03), maxwidth=120, exposure=0.5)
        assert _asks(L, d) == 1


def test_refused(L, orc):
    rc = F(*CROPS_RC, 0.03)
    assert _asks(L, _desc(342, 150, rotatecrop=rc, maxwidth=180)) == 1                       # the control
    assert _asks(L, _desc(342, 150, "RGBE", rotatecrop=rc, maxwidth=180, mask=ON | SRC | 2)) == 0   # a fourth colour: E is not +0.0
    assert _asks(L, _desc(342, 150, "", is_cfa=0, rotatecrop=rc, maxwidth=180)) == 0         # a monochrome raw
    assert _asks(L, _desc(342, 150, "", cpp=3, is_cfa=0, rotatecrop=rc, maxwidth=180)) == 0  # a three-sample raw
    assert _asks(L, _desc(342, 150, maxwidth=180)) == 0                                      # a no-op rotatecrop
    assert _asks(L, _desc(342, 150, rotatecrop=rc)) == 0                                     # scale <= 1
    assert _scale(orc, 342, 150, NOCROP, 0, rc)[0] <= 1.0
    assert _asks(L, _desc(342, 150, rotatecrop=F(1.5, 0, 0, 0, 0), maxwidth=180)) == 0       # a crop past the frame: the op hands its input on
    for mask in (SRC, 0, ON, SRC | 2, SRC | 62):                                             # the bit alone, and the route without the bit
        assert _asks(L, _desc(342, 150, rotatecrop=rc, maxwidth=180, mask=mask)) == 0, mask
    fast = _raster(128, 64, use_fastpath=1)
    fast.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    m = (C.c_float * 12)()
    L.ipk_const_matrix(2, m)
    fast.cam_to_xyz_normalized[:] = m[:]
    fast.blacklevels[:] = [0.0] * 4
    fast.whitelevels[:] = [0.0] * 4
    fast.maxwidth = 64
    for out_type, fastpath in ((1, 1), (2, 1)):
        assert L.ipk_pipeline_takes_fastpath(C.byref(fast), out_type) == fastpath
        assert _asks(L, fast, out_type) == 0
    assert L.ipk_pipeline_fuses_scaled_rotatecrop(None, 0) == INVALID
    assert _asks(L, _desc(342, 150, rotatecrop=rc, maxwidth=180), 3) == INVALID
    assert _asks(L, _desc(8, 8, rotatecrop=rc)) < 0                                          # a descriptor ipk_pipeline_sizes refuses


BUILDERS = {
    "rggb-24mp-angle": lambda: _desc(6000, 4000, rotatecrop=F(0, 0, 0, 0, 0.02)),
    "rggb-preview-mode": lambda: _desc(342, 150, crops=SENSOR_CROPS, rotatecrop=F(*CROPS_RC, 0.03), maxwidth=180),
    "xtrans-f32-preview": lambda: _desc(342, 150, XT, src_type=1, rotatecrop=F(*CROPS_RC, 0.3), maxwidth=150),
    "rggb-preview-scaled": lambda: _desc(342, 150, rotatecrop=F(*CROPS_RC, 0.0), maxwidth=100),
    "rgb8-preview": lambda: _raster(200, 120, rotatecrop=F(*CROPS_RC, 0.03), maxwidth=120, exposure=0.5),
    "rgbe-preview": lambda: _desc(342, 150, "RGBE", rotatecrop=F(*CROPS_RC, 0.03), maxwidth=180),
    "mono-preview": lambda: _desc(342, 150, "", is_cfa=0, rotatecrop=F(*CROPS_RC, 0.03), maxwidth=180),
    "rggb-noop-preview": lambda: _desc(342, 150, maxwidth=100),
    "rggb-noop-near-full": lambda: _desc(131, 97, maxwidth=87, fuse_scaledown=1),
    "rggb-angle-full-size": lambda: _desc(342, 150, rotatecrop=F(*CROPS_RC, 0.03), fuse_rotatecrop=1),
    "rggb-plain": lambda: _desc(342, 150),
    "rgb8-cropped": lambda: _raster(200, 120, crops=SENSOR_CROPS, exposure=0.5),
}


@pytest.mark.parametrize("name", list(BUILDERS))
def test_the_bit_changes_nothing_else(L, name):
    """masks 0..63 with and without bit 6: every other report, every hash, and every region answer of a descriptor the new route does not take"""
    def answers(mask):
        d = BUILDERS[name]()
        d.allow_fused = mask
        out = []
        for out_type in (0, 1, 2):
            out.append(tuple(getattr(L, r)(C.byref(d), out_type) for r in REPORTS))
            hs = C.create_string_buffer(256)
            assert L.ipk_pipeline_hashes(C.byref(d), out_type, 77, hs) == 0
            out.append(hs.raw)
        takes = _asks(L, d)
        if not takes:
            (_, _), (fw, fh) = _sizes(L, d)
            for reg in ((0, 0, fw, fh), (1, 2, 7, 5), (fw - 1, fh - 1, 1, 1), (fw // 3, fh // 3, fw // 3, fh // 3)):
                s = [C.c_size_t(12345) for _ in range(4)]
                out.append((L.ipk_pipeline_region(C.byref(d), 0, *reg, *[C.byref(v) for v in s]), tuple(v.value for v in s)))
        return takes, out

    taken_somewhere = False
    for mask in range(64):
        t0, a0 = answers(mask)
        t1, a1 = answers(mask | SRC)
        assert t0 == 0, "the route needs the bit"
        assert t1 == int(bool(mask & ON) and name in ("rggb-24mp-angle", "rggb-preview-mode", "xtrans-f32-preview", "rggb-preview-scaled", "rgb8-preview")), (name, mask)
        taken_somewhere |= bool(t1)
        if t1:
            assert a0[:6] == a1[:6], (name, mask)                           # reports and hashes; the region answers are the route's own
        else:
            assert a0 == a1, (name, mask)


# ---- regions: the window reported is what the region depends on ----
def _oracle_desc(orc, kind, data, rc, lim, crops):
    """lim: {"maxwidth": n} or {"maxheight": n}"""
    if kind == "rgb8":
        return orc.make_pipeline(data, crops=crops, rotatecrop=rc, exposure=0.5, **lim)
    cfa = {"rggb": "RGGB", "xtrans": XT}[kind]
    return orc.make_pipeline(data, cfa=orc.cfa_shift(cfa, crops[3], crops[0]), crops=crops, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                             wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix(), rotatecrop=rc, **lim)


WINDOW_CASES = {
    "rggb-mode-0.03": ("rggb", 342, 150, SENSOR_CROPS, F(*CROPS_RC, 0.03), 180),
    "rggb-short-0.02": ("rggb", 108, 62, NOCROP, F(0, 0, 0, 0, 0.02), 0),
    "xtrans-mode-0.3": ("xtrans", 342, 150, NOCROP, F(*CROPS_RC, 0.3), 150),
    "rggb-scaled-0.03": ("rggb", 342, 150, NOCROP, F(*CROPS_RC, 0.03), 100),
    "rgb8-0.03": ("rgb8", 200, 120, NOCROP, F(*CROPS_RC, 0.03), 120),
}


@pytest.mark.parametrize("rot,fliph", [(0, False), (1, True)])
@pytest.mark.parametrize("case", list(WINDOW_CASES))
def test_the_reported_window_is_sufficient(L, orc, case, rot, fliph):
    kind, w, h, crops, rc, maxwidth = WINDOW_CASES[case]
    lim = {"maxheight" if rot & 1 else "maxwidth": maxwidth}               # the limit applies behind OpTransform: the same side of the sensor either way
    if kind == "rgb8":
        data = (util.noise_u16(util.SEED + 17001, h, w * 3) & 255).astype(np.uint8).reshape(h, w, 3)
        d = _raster(w, h, crops=crops, rotatecrop=rc, exposure=0.5, rotation=rot, fliph=int(fliph), **lim)
    else:
        data = util.noise_u16(util.SEED + 17000, h, w)
        d = _desc(w, h, {"rggb": "RGGB", "xtrans": XT}[kind], crops, rotatecrop=rc, rotation=rot, fliph=int(fliph), **lim)
    assert _asks(L, d) == 1
    (_, _), (fw, fh) = _sizes(L, d)
    od = _oracle_desc(orc, kind, data, rc, lim, crops)
    od.rotation, od.fliph = rot, int(fliph)
    want = orc.pipeline_run(od)
    assert want.shape == (fh, fw, 3)
    _, _, cw, ch = orc.size_image(*crops, w, h)
    interior = (fw // 3, fh // 3, max(fw // 4, 1), max(fh // 4, 1))
    for reg in (interior, (0, 0, 1, 1), (fw - 1, fh - 1, 1, 1), (0, fh // 2, fw, 1), (0, 0, fw, fh)):
        s = [C.c_size_t() for _ in range(4)]
        assert L.ipk_pipeline_region(C.byref(d), 0, *reg, *[C.byref(v) for v in s]) == 1, (case, reg)
        sx, sy, sw, sh = [v.value for v in s]
        assert sw > 0 and sh > 0
        assert crops[3] <= sx and sx + sw <= crops[3] + cw and crops[0] <= sy and sy + sh <= crops[0] + ch, "inside the crop window"
        if reg == interior:
            assert sw < cw and sh < ch, "an interior region reads less than the crop window"
        noise = (util.noise_u16(util.SEED + 17002, data.shape[0], int(np.prod(data.shape[1:]))).reshape(data.shape) & (255 if kind == "rgb8" else 16383))
        other = noise.astype(data.dtype)
        other[sy:sy + sh, sx:sx + sw] = data[sy:sy + sh, sx:sx + sw]
        assert not np.array_equal(other, data) or (sw, sh) == (cw, ch)
        od2 = _oracle_desc(orc, kind, other, rc, lim, crops)
        od2.rotation, od2.fliph = rot, int(fliph)
        got = orc.pipeline_run(od2)
        x, y, rw, rh = reg
        util.assert_bits_equal(got[y:y + rh, x:x + rw], want[y:y + rh, x:x + rw], "%s region %r: samples outside the window (%d, %d) %dx%d matter" % (
            case, reg, sx, sy, sw, sh))


def test_python_attribute():
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    img = ipa.RawImage(width=342, height=150, data=None, cfa="RGGB", crops=NOCROP, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                       wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix())
    pipe = ipa.Pipeline(img)                                                 # no device: the descriptor alone is read
    assert pipe.fuse_scaled_rotatecrop is False
    rc = pipe.ops.rotatecrop
    rc.crop_top, rc.crop_right, rc.crop_bottom, rc.crop_left, rc.rotation = F(*CROPS_RC, 0.03)
    pipe.globals.settings.maxwidth = 180
    assert pipe.desc().allow_fused == ON and not pipe.fuses_scaled_rotatecrop()
    pipe.fuse_scaled_rotatecrop = True
    assert pipe.desc().allow_fused == ON | _lib.FUSED_SCALED_ROTATECROP
    assert pipe.fuses_scaled_rotatecrop() and pipe.fuses_scaled_rotatecrop(1) and pipe.fuses_scaled_rotatecrop(2)
    pipe.allow_fused = False                                                 # the bit stands only beside IPK_FUSED_ON
    assert pipe.desc().allow_fused == 0 and not pipe.fuses_scaled_rotatecrop()
    assert callable(ipa.raw_demosaic_scaled)
