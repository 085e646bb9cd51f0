"""ipk_pipeline_region (no GPU): the route a region takes and the sensor window the windowed route reads, against an independent
derivation -- an index image pushed through the oracle's rotate_buffer -- plus the refusals and the window kernels' register budgets."""
import ctypes as C
import re

import numpy as np
import pytest

import util

XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
W12 = (XT[0:6] + XT[18:24] + XT[6:12] + XT[24:30] + XT[12:18] + XT[30:36]) * 2 + (XT[18:24] + XT[0:6] + XT[24:30] + XT[6:12] + XT[30:36] + XT[12:18]) * 2
W12 = (W12 * 2)[:144]
INVALID = -2                                                              # IPK_ERR_INVALID
ORIENTATIONS = [(rot, fh) for rot in range(4) for fh in (0, 1)]          # the eight dihedral orientations


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _desc(w, h, cfa="RGGB", crops=(0, 0, 0, 0), src_type=0, cpp=1, is_cfa=1, **kw):
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
    for k, v in kw.items():
        if k == "rotatecrop":
            d.rotatecrop[:] = v
        else:
            setattr(d, k, v)
    return d


def _sizes(L, d):
    a, b, c, e = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    assert L.ipk_pipeline_sizes(C.byref(d), C.byref(a), C.byref(b), C.byref(c), C.byref(e)) == 0
    return c.value, e.value


def _region(L, d, x, y, w, h, out_type=0):
    s = [C.c_size_t() for _ in range(4)]
    rc = L.ipk_pipeline_region(C.byref(d), out_type, x, y, w, h, *[C.byref(v) for v in s])
    return rc, tuple(v.value for v in s)


@pytest.mark.parametrize("cfa", ["RGGB", XT, W12])
@pytest.mark.parametrize("rot,fh", ORIENTATIONS)
def test_window_is_the_source_bounding_box_plus_halo(L, orc, cfa, rot, fh):
    sw, sh, crops = 61, 47, (3, 1, 2, 5)                               # odd crop offsets: top 3, left 5
    d = _desc(sw, sh, cfa, crops=crops, rotation=rot, fliph=fh)
    W, H = sw - crops[1] - crops[3], sh - crops[0] - crops[2]
    fw, fh_ = _sizes(L, d)
    # where every result pixel comes from: cropped-frame index (exact in f32 below 2^24) through OpTransform's permutation
    idx = np.repeat(np.arange(W * H, dtype=np.float32).reshape(H, W, 1), 3, axis=2)
    src = orc.rotate_buffer(idx, orc.transform_orientation(rot, bool(fh), False))[:, :, 0].astype(np.int64)
    assert src.shape == (fh_, fw)
    regions = [(0, 0, 1, 1), (fw - 1, 0, 1, 1), (0, fh_ - 1, 1, 1), (fw - 1, fh_ - 1, 1, 1),          # the four corners
               (0, 7, fw, 1), (9, 0, 1, fh_), (3, 5, 17, 9), (fw - 13, fh_ - 11, 13, 11), (0, 0, fw, fh_)]
    for x, y, w, h in regions:
        rc, (wx, wy, ww, wh) = _region(L, d, x, y, w, h)
        assert rc == 1, (x, y, w, h)
        part = src[y:y + h, x:x + w]
        r, c = part // W, part % W
        c0, c1, r0, r1 = int(c.min()), int(c.max()) + 1, int(r.min()), int(r.max()) + 1
        # the bounding box widened by demosaic::full's one-pixel halo, clipped to the crop window, in sensor coordinates
        hx0, hx1, hy0, hy1 = max(c0 - 1, 0), min(c1 + 1, W), max(r0 - 1, 0), min(r1 + 1, H)
        assert (wx, wy, ww, wh) == (crops[3] + hx0, crops[0] + hy0, hx1 - hx0, hy1 - hy0), (x, y, w, h)
        # ... and the halo is exactly what was added
        assert (wx - crops[3] + (c0 - hx0), wy - crops[0] + (r0 - hy0)) == (c0, r0)


FUSED_FAMILIES = [dict(cfa=XT, shape=(72, 108)), dict(cfa=XT, shape=(96, 144), maxwidth=36),
                  dict(cfa="RGGB", shape=(80, 120), maxwidth=40), dict(cfa="RGGB", shape=(80, 120), maxwidth=90),
                  dict(cfa="RGGB", shape=(80, 120), maxheight=33), dict(cfa="RGBE", shape=(40, 60)),
                  dict(cfa="RGGB", shape=(60, 90), rotation=1), dict(cfa="RGGB", shape=(60, 90), rotation=3, fliph=1, maxwidth=30),
                  dict(cfa="RGGB", shape=(60, 90), rotation=2, flipv=1),
                  dict(cfa="RGGB", shape=(100, 100), rotatecrop=(0.1, 0.05, 0.2, 0.0, 0.0)),
                  dict(cfa="RGGB", shape=(100, 120), rotatecrop=(0.0, 0.0, 0.0, 0.0, 0.3), maxwidth=64),
                  dict(cfa="GRBG", shape=(64, 64), crops=(1, 1, 1, 1), maxwidth=20),
                  dict(cfa="GRBG", shape=(64, 64), crops=(1, 1, 1, 1))]


@pytest.mark.parametrize("case", FUSED_FAMILIES)
def test_route_is_windowed_exactly_where_the_run_fuses(L, case):
    """the descriptor families of test_gpu_fused.test_staged_pipeline_vs_oracle: windowed where ipk_pipeline_run fuses"""
    case = dict(case)
    h, w = case.pop("shape")
    d = _desc(w, h, case.pop("cfa"), **case)
    fusable = d.cfa != b"RGBE" and not any(k in case for k in ("maxwidth", "maxheight", "rotatecrop"))
    fw, fh = _sizes(L, d)
    rc, win = _region(L, d, 1, 2, fw - 3, fh - 4)
    assert rc == (1 if fusable else 0)
    cr = case.get("crops", (0, 0, 0, 0))
    if not fusable:
        assert win == (cr[3], cr[0], w - cr[1] - cr[3], h - cr[0] - cr[2])      # the whole crop window
    for out_type in (1, 2):
        assert _region(L, d, 0, 0, fw, fh, out_type)[0] == rc


@pytest.mark.parametrize("kw", [dict(allow_fused=0), dict(is_cfa=0, cfa=""), dict(cpp=3, is_cfa=0, cfa=""), dict(src_type=2, cpp=3, is_cfa=0, cfa=""),
                                dict(src_type=3, cpp=3, is_cfa=0, cfa="")])
def test_other_routes_take_the_whole_frame(L, kw):
    kw = dict(kw)
    d = _desc(90, 60, kw.pop("cfa", "RGGB"), **kw)
    fw, fh = _sizes(L, d)
    assert _region(L, d, 5, 5, 20, 20) == (0, (0, 0, 90, 60))


def test_invalid_regions_are_refused(L):
    d = _desc(90, 60)
    fw, fh = _sizes(L, d)
    big = (1 << 64) - 1
    for x, y, w, h in [(0, 0, 0, 1), (0, 0, 1, 0), (0, 0, fw + 1, 1), (0, 0, 1, fh + 1), (fw, 0, 1, 1), (0, fh, 1, 1), (1, 0, fw, 1),
                       (big, 0, 2, 1), (2, 0, big, 1), (0, big, 1, 2), (0, 2, 1, big), (big, big, big, big)]:
        assert _region(L, d, x, y, w, h)[0] == INVALID, (x, y, w, h)
    assert _region(L, d, 0, 0, fw, fh, 3)[0] == INVALID                             # bad out_type
    assert _region(L, _desc(8, 8), 0, 0, 1, 1)[0] == INVALID                      # a descriptor ipk_pipeline_sizes rejects
    assert _region(L, _desc(90, 60, rotation=4), 0, 0, 1, 1)[0] == INVALID
    assert _region(L, _desc(90, 60, npoints=65), 0, 0, 1, 1)[0] == INVALID        # ... and one ipk_pipeline_run rejects
    s = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_region(None, 0, 0, 0, 1, 1, *[C.byref(v) for v in s]) == INVALID


def test_window_kernels_fit_their_budget():
    """the region form of the fused kernel, read from the code object as test_kernel_resources does: at most 128 VGPRs (one 1024-thread block
    per CU), and no scratch for the common-parameter variants (CM = 1, what real sensors take) and the narrow Bayer windows.  The runtime-flag
    full-strip variants spill a few dwords, as their whole-frame counterparts do (the generic-CFA ones there too)."""
    import test_kernel_resources as tkr
    ks = [k for k in tkr._kernels() if "k_fused_bayer_window<" in k[0]]
    assert len(ks) == 42, [k[0] for k in ks]
    problems = []
    for name, vgpr, scratch, spills in ks:
        short = re.sub(r"\(.*$", "", name.replace("void ipk::", ""))
        if vgpr > 128:
            problems.append("%s: %d VGPRs > 128" % (short, vgpr))
        if re.search(r", 1>$|, false, false, true, 0>$", short) and (scratch or spills):
            problems.append("%s: %d bytes of scratch, %d spills" % (short, scratch, spills))
    assert not problems, "\n".join(problems)
