"""The one-launch route of the frames whose OpDemosaic is a pass-through (no GPU): cropped RGB8 / RGB16 rasters, u16 monochrome and u16 three-sample
raws under IPK_FUSED_PLAIN (bit 4 of allow_fused, acting beside IPK_FUSED_ON).  Which descriptors ipk_pipeline_fuses_plain reports, which regions
ipk_pipeline_region windows and the rectangle it reports -- against a brute-force index walk of rotate_buffer --, and that without the bit every
answer is the one the parent commit recorded (tests/golden/routes/route_table.npz) or the same descriptor gives with the bit cleared."""
import ctypes as C
import itertools
import os
import sys

import numpy as np
import pytest

import util
import test_scaledown_route as sr
from test_scaledown_route import SENSOR_CROPS, NOCROP, INVALID

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ON, FOUR, REGIONS, PREVIEWS, PLAIN = 1, 2, 4, 8, 16
RC = [float(np.float32(v)) for v in (0.1, 0, 0, 0, 0.2)]

# name -> (cfa, src_type, cpp, is_cfa, admitted under the bit)
SOURCES = {"rgb8": ("", 2, 3, 0, True), "rgb16": ("", 3, 3, 0, True), "mono-u16": ("", 0, 1, 0, True), "cpp3-u16": ("", 0, 3, 0, True),
           "mono-f32": ("", 1, 1, 0, False), "cpp3-f32": ("", 1, 3, 0, False), "rggb": ("RGGB", 0, 1, 1, False)}


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _desc(name, w, h, crops=NOCROP, **kw):
    cfa, src_type, cpp, is_cfa, _ = SOURCES[name]
    return sr._desc(w, h, cfa, crops, src_type=src_type, cpp=cpp, is_cfa=is_cfa, fuse=0, **kw)


def _region(L, d, x, y, w, h, out_type=0):
    s = [C.c_size_t(12345) for _ in range(4)]
    rc = L.ipk_pipeline_region(C.byref(d), out_type, x, y, w, h, *[C.byref(v) for v in s])
    return rc, tuple(v.value for v in s)


def _sizes(L, d):
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
    return tuple(v.value for v in a)


# ---------------------------------------------------------------------------------------------
# the whole-frame report
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(SOURCES))
def test_fuses_plain_truth_table(L, name):
    admitted = SOURCES[name][4]
    raster = SOURCES[name][1] in (2, 3)
    seen = set()
    for crops, rc, mw, mask in itertools.product((NOCROP, SENSOR_CROPS), (None, RC), (0, 40), (0, ON, PLAIN, ON | PLAIN)):
        kw = dict(maxwidth=mw)
        if rc is not None:
            kw["rotatecrop"] = rc
        d = _desc(name, 96, 120, crops, **kw)
        d.allow_fused = mask
        # an uncropped raster is on the launch whatever the bit says: the report is about the frames the bit adds
        want = int(admitted and mask == (ON | PLAIN) and rc is None and mw == 0 and not (raster and crops == NOCROP))
        for out_type in (0, 1, 2):
            assert L.ipk_pipeline_fuses_plain(C.byref(d), out_type) == want, (name, crops, rc, mw, mask, out_type)
            for other in (L.ipk_pipeline_fuses_rotatecrop, L.ipk_pipeline_fuses_scaledown, L.ipk_pipeline_fuses_four_colour, L.ipk_pipeline_windows_preview):
                d0 = _desc(name, 96, 120, crops, **kw)
                d0.allow_fused = mask & ~PLAIN
                assert other(C.byref(d), out_type) == other(C.byref(d0), out_type), "no other report sees the bit"
        seen.add(want)
    assert seen == ({0, 1} if admitted else {0}), name


def test_a_scale_above_one_really_is_one(L, orc):
    """the truth table's size limit: maxwidth 40 on the 96-wide frame makes OpDemosaic scale (scale > 1), cropped or not"""
    for crops in (NOCROP, SENSOR_CROPS):
        d = _desc("mono-u16", 96, 120, crops, maxwidth=40)
        dw, dh, _, _ = _sizes(L, d)
        _, _, cw, ch = orc.size_image(*crops, 96, 120)
        assert orc.calculate_scaling_total(cw, ch, dw, dh)[0] > 1.0


def test_small_frames_and_the_fast_path(L):
    # 255 pixels in the cropped rectangle: 27x20 minus crops (3, 1, 2, 5) is 21x15 = 315; 25x20 is 19x15 = 285; 23x19 is 17x14 = 238
    for w, h, want in ((27, 20, 1), (25, 20, 1), (23, 19, 0)):
        d = _desc("cpp3-u16", w, h, SENSOR_CROPS)
        d.allow_fused = ON | PLAIN
        assert L.ipk_pipeline_fuses_plain(C.byref(d), 0) == want, (w, h)
    # a frame on the fast path stays there: the default ops of a raster, 8- and 16-bit results
    from imagepipe_amd._lib import PipelineDesc
    fast = PipelineDesc()
    fast.src_type, fast.width, fast.height, fast.cpp, fast.use_fastpath = 2, 128, 64, 3, 1
    m = (C.c_float * 12)()
    L.ipk_const_matrix(2, m)
    fast.cam_to_xyz_normalized[:] = m[:]
    fast.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    fast.allow_fused = ON | PLAIN
    for out_type, fastpath in ((1, 1), (2, 1), (0, 0)):
        assert L.ipk_pipeline_takes_fastpath(C.byref(fast), out_type) == fastpath
        assert L.ipk_pipeline_fuses_plain(C.byref(fast), out_type) == 0
        # its regions: cut from the fast path's result; an f32 result never takes the fast path, and the uncropped raster's launch is windowed
        assert _region(L, fast, 3, 2, 40, 40, out_type) == ((0, (0, 0, 128, 64)) if fastpath else (1, (3, 2, 40, 40)))
    assert L.ipk_pipeline_fuses_plain(None, 0) == INVALID and L.ipk_pipeline_fuses_plain(C.byref(fast), 3) == INVALID


# ---------------------------------------------------------------------------------------------
# regions
# ---------------------------------------------------------------------------------------------
def _index_walk(orc, w, h, orientation):
    """rotate_buffer on an image whose pixel (row, col) holds (col, row, 0): result[oy, ox] -> the (col, row) it came from"""
    src = np.zeros((h, w, 3), np.float32)
    src[:, :, 0] = np.arange(w, dtype=np.float32)[None, :]
    src[:, :, 1] = np.arange(h, dtype=np.float32)[:, None]
    out = orc.rotate_buffer(src, orientation)
    return out[:, :, 0].astype(np.int64), out[:, :, 1].astype(np.int64)


def _windows(fw, fh):
    """the corners (16 x 16: 256 pixels), a one-row strip of 256+ pixels where a row has them, a one-column strip, an interior 19 x 17, the whole"""
    a = min(16, fw, fh)
    wins = [(0, 0, 16, 16), (fw - 16, 0, 16, 16), (0, fh - 16, 16, 16), (fw - 16, fh - 16, 16, 16), (5, 4, 19, 17), (0, 0, fw, fh)]
    assert a == 16
    return wins


@pytest.mark.parametrize("rot,fh", [(r, f) for r in range(4) for f in (0, 1)])
@pytest.mark.parametrize("name", ["rgb8", "rgb16", "mono-u16", "cpp3-u16"])
def test_regions_map_back_through_every_orientation(L, orc, name, rot, fh):
    """37 x 29 with sensor crops (3, 1, 2, 5): a 31 x 24 rectangle at (5, 3).  Every region of 256 pixels and more answers 1 and reports exactly the
    sensor rectangle its pixels come from, by rotate_buffer's own walk; the uncropped rasters, which the launch always took, are windowed too"""
    for crops in (SENSOR_CROPS, NOCROP):
        w, h = 37, 29
        d = _desc(name, w, h, crops, rotation=rot, fliph=fh)
        d.allow_fused = ON | PLAIN
        x0, y0, cw, ch = orc.size_image(*crops, w, h)
        _, _, fw, fhh = _sizes(L, d)
        ori = orc.transform_orientation(rot, bool(fh), False)
        cols, rows = _index_walk(orc, cw, ch, ori)
        assert cols.shape == (fhh, fw)
        for win in _windows(fw, fhh) + [(0, fhh // 2, fw, 1), (fw // 3, 0, 1, fhh)]:
            x, y, rw, rh = win
            c, r = cols[y:y + rh, x:x + rw], rows[y:y + rh, x:x + rw]
            box = (x0 + int(c.min()), y0 + int(r.min()), int(c.max() - c.min()) + 1, int(r.max() - r.min()) + 1)
            assert box[2] * box[3] == rw * rh, "a rectangle maps to a rectangle"
            for out_type in (0, 1, 2):
                got = _region(L, d, *win, out_type)
                if rw * rh >= 256:
                    assert got == (1, box), (name, crops, rot, fh, win, got, box)
                else:
                    assert got == (0, (x0, y0, cw, ch)), (name, crops, rot, fh, win, got)
        # under 256 pixels: cut from the whole result, the crop window
        assert _region(L, d, 1, 2, 15, 15) == (0, (x0, y0, cw, ch))
        assert _region(L, d, 1, 2, 17, 15) == (0, (x0, y0, cw, ch))            # 255
        assert _region(L, d, 1, 2, 16, 16)[0] == 1                             # 256


def test_long_strips_are_windowed(L, orc):
    """a one-row and a one-column strip of 256 pixels and more, on a frame that has them"""
    d = _desc("mono-u16", 300, 290, SENSOR_CROPS, rotation=1)
    d.allow_fused = ON | PLAIN
    x0, y0, cw, ch = orc.size_image(*SENSOR_CROPS, 300, 290)
    _, _, fw, fh = _sizes(L, d)
    assert (fw, fh) == (ch, cw)
    cols, rows = _index_walk(orc, cw, ch, orc.transform_orientation(1, False, False))
    for win in ((0, 7, fw, 1), (9, 0, 1, fh), (3, 11, 256, 1), (9, 2, 1, 256)):
        x, y, rw, rh = win
        c, r = cols[y:y + rh, x:x + rw], rows[y:y + rh, x:x + rw]
        assert _region(L, d, *win) == (1, (x0 + int(c.min()), y0 + int(r.min()), int(c.max() - c.min()) + 1, int(r.max() - r.min()) + 1)), win


@pytest.mark.parametrize("name", list(SOURCES))
def test_without_the_bit_regions_are_as_they_were(L, orc, name):
    """masks 0 / 1 / 16 (and the older bits): route 0 and the crop window for every source of this family; a mosaic keeps its own answers"""
    for crops, (rot, fh) in itertools.product((NOCROP, SENSOR_CROPS), ((0, 0), (1, 0), (2, 1))):
        d1 = _desc(name, 37, 29, crops, rotation=rot, fliph=fh)
        x0, y0, cw, ch = orc.size_image(*crops, 37, 29)
        _, _, fw, fhh = _sizes(L, d1)
        for mask in (0, ON, PLAIN, ON | FOUR | REGIONS | PREVIEWS):
            d1.allow_fused = mask
            for win in _windows(fw, fhh):
                got = _region(L, d1, *win)
                if name == "rggb":
                    d0 = _desc(name, 37, 29, crops, rotation=rot, fliph=fh)
                    d0.allow_fused = mask | (ON | PLAIN if mask else 0)
                    assert got == _region(L, d0, *win), "a mosaic's regions do not depend on the bit"
                else:
                    assert got == (0, (x0, y0, cw, ch)), (name, crops, mask, win, got)
    # f32 mono / three-sample raws stay whole-frame WITH the bit too: they are staged
    if name in ("mono-f32", "cpp3-f32"):
        d = _desc(name, 37, 29, SENSOR_CROPS)
        d.allow_fused = ON | PLAIN
        x0, y0, cw, ch = orc.size_image(*SENSOR_CROPS, 37, 29)
        assert _region(L, d, 0, 0, 20, 20) == (0, (x0, y0, cw, ch))


def test_rotatecrop_and_scaled_frames_stay_whole_frame_with_the_bit(L):
    for name in ("rgb8", "mono-u16", "cpp3-u16"):
        for kw in (dict(rotatecrop=RC), dict(maxwidth=87)):
            d = _desc(name, 131, 97, **kw)
            d.allow_fused = ON | PLAIN
            assert L.ipk_pipeline_fuses_plain(C.byref(d), 0) == 0
            d0 = _desc(name, 131, 97, **kw)
            _, _, fw, fh = _sizes(L, d)
            assert _region(L, d, 0, 0, fw, fh) == _region(L, d0, 0, 0, fw, fh) and _region(L, d, 0, 0, fw, fh)[0] == 0


def test_invalid_regions_and_hashes(L):
    d = _desc("cpp3-u16", 96, 120, SENSOR_CROPS)
    d.allow_fused = ON | PLAIN
    _, _, fw, fh = _sizes(L, d)
    assert _region(L, d, 0, 0, fw, fh)[0] == 1
    for win in ((0, 0, 0, 1), (0, 0, 1, 0), (fw - 1, 0, 2, 1), (0, fh - 1, 1, 2), (fw, 0, 1, 1), (0, fh, 1, 1), ((1 << 64) - 1, 0, 2, 1)):
        rc, fp = _region(L, d, *win)
        assert rc == INVALID and fp == (12345,) * 4, (win, rc, fp)
    d0 = _desc("cpp3-u16", 96, 120, SENSOR_CROPS)
    ha, hb = C.create_string_buffer(256), C.create_string_buffer(256)
    assert L.ipk_pipeline_hashes(C.byref(d0), 0, 5, ha) == 0 and L.ipk_pipeline_hashes(C.byref(d), 0, 5, hb) == 0
    assert ha.raw == hb.raw, "the bit enters no hash"


# ---------------------------------------------------------------------------------------------
# the recorded routes
# ---------------------------------------------------------------------------------------------
def test_the_recorded_descriptors_keep_their_routes_and_never_report_plain(L):
    """every descriptor of the route table, with its own mask (none carries bit 4): the recorded row, and ipk_pipeline_fuses_plain == 0"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_route_table as tool
    finally:
        sys.path.pop(0)
    from test_rotatecrop_route import _desc as rdesc
    with np.load(tool.OUT) as z:
        recorded = z["matrix"]
    assert all(not (m & PLAIN) for m in tool.ALLOW_FUSED)
    tmp = [C.c_size_t() for _ in range(4)]
    rows, plain = [], 0
    for (w, h, crops), (_, cfa, src_type, cpp, is_cfa) in itertools.product(tool.FRAMES, tool.SOURCES):
        d = rdesc(w, h, cfa, crops, src_type=src_type, cpp=cpp, is_cfa=is_cfa, fuse=0)
        rcs = tool.rotatecrops()
        for k, mw, allow, frc, fsd, rot, fh in tool.inner_axes():
            d.rotatecrop[:] = rcs[k]
            d.maxwidth, d.allow_fused, d.fuse_rotatecrop, d.fuse_scaledown, d.rotation, d.fliph = mw, allow, frc, fsd, rot, fh
            for out_type in tool.OUT_TYPES:
                rows.append(tool._row(L, d, out_type, tmp))
                plain += L.ipk_pipeline_fuses_plain(C.byref(d), out_type) != 0
    assert np.array_equal(np.array(rows, np.int32), recorded)
    assert plain == 0


def test_abi_sizes_are_unchanged(L):
    """the opt-in lives in the mask: no layout moved.  The values are those of the commit before the bit existed"""
    from imagepipe_amd import _lib
    assert [L.ipk_abi_sizeof(i) for i in (0, 1, 16, 17, 18, 19, 20, 21)] == [856, 928, 840, 900, 808, 896, 848, 908]
    assert C.sizeof(_lib.FusedParams) == 856 and C.sizeof(_lib.PipelineDesc) == 928


def test_bindings_carry_the_bit():
    import inspect
    import imagepipe_amd
    from imagepipe_amd import _lib
    assert _lib.FUSED_PLAIN == PLAIN and (_lib.PLAIN_RASTER, _lib.PLAIN_RGB, _lib.PLAIN_MONO) == (0, 1, 2)
    src = inspect.getsource(imagepipe_amd.Pipeline)
    assert "self.fuse_plain = False" in src and "d.allow_fused |= _lib.FUSED_PLAIN" in src
    assert callable(imagepipe_amd.Pipeline.fuses_plain)
    for name in ("ipk_plain_to_srgb", "ipk_pipeline_fuses_plain"):
        assert name in _lib.SIGNATURES
    assert len(_lib.SIGNATURES["ipk_plain_to_srgb"][1]) == 19
