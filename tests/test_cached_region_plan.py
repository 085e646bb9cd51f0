"""ipk_pipeline_region_gather (no GPU): where a region of the result lies in the buffer OpRotateCrop hands to OpToLab, against an independent
derivation -- an index image of that buffer pushed through the oracle's rotate_buffer -- the buffer's shape against the oracle's ops, and the
refusals of the two entry points."""
import ctypes as C

import numpy as np
import pytest

import util
from test_region_plan import INVALID, ORIENTATIONS, _desc, _sizes

NOT_INIT = -1                                                             # IPK_ERR_NOT_INIT


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def _gather(L, d, x, y, w, h, out_type=0):
    bw, bh = C.c_size_t(), C.c_size_t()
    base, xs, ys = C.c_int64(), C.c_int64(), C.c_int64()
    rc = L.ipk_pipeline_region_gather(C.byref(d), out_type, x, y, w, h, C.byref(bw), C.byref(bh), C.byref(base), C.byref(xs), C.byref(ys))
    return rc, (bw.value, bh.value), base.value, xs.value, ys.value


def _regions(fw, fh):
    """every edge, the four corners as 1x1, odd interiors and the whole result"""
    out = [(0, 0, 1, 1), (fw - 1, 0, 1, 1), (0, fh - 1, 1, 1), (fw - 1, fh - 1, 1, 1), (fw // 2, fh // 3, 1, 1),
           (0, 1, fw, 1), (1, 0, 1, fh), (0, fh - 2, fw, 2), (fw - 3, 0, 3, fh), (0, 0, 5, 4), (fw - 7, fh - 5, 7, 5), (3, 2, min(17, fw - 3), min(9, fh - 2)),
           (0, 0, fw, fh)]
    return [r for r in out if r[2] >= 1 and r[3] >= 1 and r[0] >= 0 and r[1] >= 0 and r[0] + r[2] <= fw and r[1] + r[3] <= fh]


def _oracle_buffer_shape(orc, sw, sh, crops, d, rotatecrop):
    """(width, height) of what the oracle's gofloat, demosaic and rotatecrop hand to OpToLab for this descriptor"""
    a, b, c, e = C.c_size_t(), C.c_size_t(), C.c_size_t(), C.c_size_t()
    from imagepipe_amd import _lib
    assert _lib.load().ipk_pipeline_sizes(C.byref(d), C.byref(a), C.byref(b), C.byref(c), C.byref(e)) == 0
    x, y, w, h = orc.size_image(crops[0], crops[1], crops[2], crops[3], sw, sh)
    raw = util.noise_u16(util.SEED + 7, sh, sw)
    mosaic = orc.gofloat_cfa(raw, x, y, w, h, util.BLACK, util.WHITE)
    _, rgbe = orc.demosaic_run(orc.cfa_shift("RGGB", crops[3], crops[0]), mosaic, a.value, b.value)
    out = orc.rotatecrop_run(rotatecrop, rgbe)
    return out.shape[1], out.shape[0]


@pytest.mark.parametrize("rot,fh", ORIENTATIONS)
@pytest.mark.parametrize("frame", [(37, 23, (2, 1, 3, 2)), (342, 75, (1, 3, 2, 5))])
@pytest.mark.parametrize("rc_crop", [False, True])
@pytest.mark.parametrize("maxwidth", [0, 24])
def test_gather_is_rotate_buffers_walk_over_the_region(L, orc, frame, rot, fh, rc_crop, maxwidth):
    sw, sh, crops = frame
    rotatecrop = (0.1, 0.05, 0.2, 0.0, 0.0) if rc_crop else (0.0, 0.0, 0.0, 0.0, 0.0)
    d = _desc(sw, sh, "RGGB", crops=crops, rotation=rot, fliph=fh, rotatecrop=rotatecrop, maxwidth=maxwidth)
    fw, fh_ = _sizes(L, d)
    rc, (bw, bh), _, _, _ = _gather(L, d, 0, 0, 1, 1)
    assert rc == 0
    assert (bw, bh) == _oracle_buffer_shape(orc, sw, sh, crops, d, rotatecrop)
    # where every result pixel comes from: the buffer's pixel index (exact in f32 below 2^24) through OpTransform's permutation
    idx = np.repeat(np.arange(bw * bh, dtype=np.float32).reshape(bh, bw, 1), 3, axis=2)
    src = orc.rotate_buffer(idx, orc.transform_orientation(rot, bool(fh), False))[:, :, 0].astype(np.int64)
    assert src.shape == (fh_, fw)
    for x, y, w, h in _regions(fw, fh_):
        rc, shape, base, xs, ys = _gather(L, d, x, y, w, h)
        assert rc == 0 and shape == (bw, bh), (x, y, w, h)
        i, j = np.meshgrid(np.arange(w, dtype=np.int64), np.arange(h, dtype=np.int64))
        assert np.array_equal(base + i * xs + j * ys, src[y:y + h, x:x + w]), (x, y, w, h, base, xs, ys)
    for out_type in (1, 2):
        assert _gather(L, d, 0, 0, fw, fh_, out_type)[:2] == (0, (bw, bh))


def test_plain_rectangle_flips_and_transposes_have_the_stated_steps(L):
    d = _desc(90, 60)
    assert _gather(L, d, 4, 6, 20, 10) == (0, (90, 60), 6 * 90 + 4, 1, 90)
    d = _desc(90, 60, rotation=2)                                           # 180 degrees: both steps negated
    assert _gather(L, d, 0, 0, 90, 60)[2:] == (90 * 60 - 1, -1, -90)
    d = _desc(90, 60, rotation=1)                                           # a transposing orientation: the steps swap
    rc, shape, _, xs, ys = _gather(L, d, 0, 0, 60, 90)
    assert rc == 0 and shape == (90, 60) and abs(xs) == 90 and abs(ys) == 1


def test_invalid_regions_and_descriptors_are_refused(L):
    d = _desc(90, 60)
    fw, fh = _sizes(L, d)
    big = (1 << 64) - 1
    for x, y, w, h in [(0, 0, 0, 1), (0, 0, 1, 0), (0, 0, fw + 1, 1), (0, 0, 1, fh + 1), (fw, 0, 1, 1), (0, fh, 1, 1), (1, 0, fw, 1),
                       (big, 0, 2, 1), (2, 0, big, 1), (0, big, 1, 2), (0, 2, 1, big), (big, big, big, big)]:
        assert _gather(L, d, x, y, w, h)[0] == INVALID, (x, y, w, h)
    assert _gather(L, d, 0, 0, fw, fh, 3)[0] == INVALID                             # bad out_type
    assert _gather(L, _desc(8, 8), 0, 0, 1, 1)[0] == INVALID                      # a descriptor ipk_pipeline_sizes rejects
    assert _gather(L, _desc(90, 60, rotation=4), 0, 0, 1, 1)[0] == INVALID
    assert _gather(L, _desc(90, 60, npoints=65), 0, 0, 1, 1)[0] == INVALID        # ... and one ipk_pipeline_run rejects
    v = [C.c_size_t(), C.c_size_t(), C.c_int64(), C.c_int64(), C.c_int64()]
    assert L.ipk_pipeline_region_gather(None, 0, 0, 0, 1, 1, *[C.byref(a) for a in v]) == INVALID
    assert L.ipk_pipeline_region_gather(C.byref(d), 0, 0, 0, 1, 1, None, C.byref(v[1]), C.byref(v[2]), C.byref(v[3]), C.byref(v[4])) == INVALID
    # the same message as ipk_pipeline_region's
    s = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_region(C.byref(d), 0, fw, 0, 1, 1, *[C.byref(a) for a in s]) == INVALID
    want = L.ipk_last_error()
    assert _gather(L, d, fw, 0, 1, 1)[0] == INVALID
    assert L.ipk_last_error() == want and b"outside" in want


def test_run_cached_region_without_a_gpu_or_an_argument(L):
    import torch
    d = _desc(90, 60)
    cache = C.c_void_p()
    assert L.ipk_cache_new(1 << 20, C.byref(cache)) == 0
    try:
        ops, win = C.c_int(-1), C.c_int(-1)
        one = C.c_void_p(16)                                                # never dereferenced: both calls return before they touch a buffer
        args = lambda dd, src, ch, dst: (dd, src, 0, ch, 0, 0, 4, 4, dst, 0, C.byref(ops), C.byref(win), None)
        assert L.ipk_pipeline_run_cached_region(*args(None, one, cache, one)) == INVALID
        assert L.ipk_pipeline_run_cached_region(*args(C.byref(d), None, cache, one)) == INVALID
        assert L.ipk_pipeline_run_cached_region(*args(C.byref(d), one, None, one)) == INVALID
        assert L.ipk_pipeline_run_cached_region(*args(C.byref(d), one, cache, None)) == INVALID
        if not torch.cuda.is_available():                                   # no context on this thread: there is no CPU fallback
            assert L.ipk_pipeline_run_cached_region(*args(C.byref(d), one, cache, one)) == NOT_INIT
    finally:
        L.ipk_cache_free(cache)
