"""IPK_FUSED_CACHED_RESAMPLE (bit 5 of allow_fused) without a GPU: which descriptors ipk_pipeline_run_cached_region would resample straight from the cached
demosaic buffer (ipk_pipeline_resamples_cached_region), that the bit needs IPK_FUSED_ON beside it, and that no hash and no region report depends on it."""
import ctypes as C

import numpy as np
import pytest

import util
import test_scaledown_route as sr
from test_scaledown_route import XT, INVALID, NOCROP

ON, CACHED = 1, 32
RC = [float(np.float32(v)) for v in (0.1, 0.05, 0.2, 0.0, 0.3)]
CROP_ONLY = RC[:4] + [0.0]
CROPS = (1, 3, 2, 5)


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


# name -> builder of a fresh descriptor the route admits (allow_fused is set by the tests)
ADMITTED = {
    "rggb-u16-angle": lambda: sr._desc(342, 75, "RGGB", CROPS, fuse=0, rotatecrop=RC),
    "rggb-u16-crop-only": lambda: sr._desc(342, 75, "RGGB", CROPS, fuse=0, rotatecrop=CROP_ONLY),
    "xtrans-preview-crop": lambda: sr._desc(342, 75, XT, CROPS, src_type=1, fuse=0, maxwidth=100, rotatecrop=CROP_ONLY),
    "rgb8-exposure-crop": lambda: sr._desc(200, 120, "", CROPS, src_type=2, cpp=3, is_cfa=0, fuse=0, exposure=0.5, rotatecrop=CROP_ONLY),
    "mono-u16": lambda: sr._desc(200, 120, "", CROPS, src_type=0, cpp=1, is_cfa=0, fuse=0, rotatecrop=RC),
    "cpp3-u16": lambda: sr._desc(200, 120, "", CROPS, src_type=0, cpp=3, is_cfa=0, fuse=0, rotatecrop=RC),
}


def _asks(L, d, out_type=0):
    return L.ipk_pipeline_resamples_cached_region(C.byref(d), out_type)


def _fast(L):
    from imagepipe_amd._lib import PipelineDesc
    fast = PipelineDesc()
    fast.src_type, fast.width, fast.height, fast.cpp, fast.use_fastpath = 2, 128, 64, 3, 1
    m = (C.c_float * 12)()
    L.ipk_const_matrix(2, m)
    fast.cam_to_xyz_normalized[:] = m[:]
    fast.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    return fast


def test_the_constant():
    from imagepipe_amd import _lib
    assert _lib.FUSED_CACHED_RESAMPLE == 32


@pytest.mark.parametrize("name", list(ADMITTED))
def test_admitted_under_the_bit_and_under_it_alone(L, name):
    for mask in range(64):
        d = ADMITTED[name]()
        d.allow_fused = mask
        want = int(mask & (ON | CACHED) == (ON | CACHED))                   # every mask without bit 5, and bit 5 without bit 0: 0
        for out_type in (0, 1, 2):
            assert _asks(L, d, out_type) == want, (name, mask, out_type)


def test_the_preview_case_really_scales(L):
    d = ADMITTED["xtrans-preview-crop"]()
    a = [C.c_size_t() for _ in range(4)]
    assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
    assert a[0].value < 342 - 8 and a[0].value <= 100 + 30                   # the demosaic size is the preview's, not the cropped sensor's


def test_refused(L):
    on = ON | CACHED
    noop = sr._desc(342, 75, "RGGB", CROPS, fuse=0)                          # a no-op rotatecrop: the gather route's ground
    noop.allow_fused = on
    assert _asks(L, noop) == 0
    rgbe = sr._desc(342, 75, "RGBE", CROPS, fuse=0, rotatecrop=RC)           # a fourth colour: E is not +0.0 in its buffers
    rgbe.allow_fused = on | 2
    assert _asks(L, rgbe) == 0
    outside = sr._desc(342, 75, "RGGB", CROPS, fuse=0, rotatecrop=[1.5, 0.0, 0.0, 0.0, 0.0])   # a crop past the frame: the op hands its input on
    outside.allow_fused = on
    assert _asks(L, outside) == 0
    fast = _fast(L)
    fast.allow_fused = on
    for out_type, fastpath in ((1, 1), (2, 1), (0, 0)):
        assert L.ipk_pipeline_takes_fastpath(C.byref(fast), out_type) == fastpath
        assert _asks(L, fast, out_type) == 0
    assert L.ipk_pipeline_resamples_cached_region(None, 0) == INVALID
    assert _asks(L, ADMITTED["mono-u16"](), 3) == INVALID
    tiny = sr._desc(8, 8, "RGGB", fuse=0, rotatecrop=RC)                     # a descriptor ipk_pipeline_sizes refuses
    tiny.allow_fused = on
    assert _asks(L, tiny) < 0


@pytest.mark.parametrize("name", list(ADMITTED) + ["noop"])
def test_no_hash_and_no_region_report_sees_the_bit(L, name):
    build = ADMITTED.get(name, lambda: sr._desc(342, 75, "RGGB", CROPS, fuse=0))

    def reports(mask):
        d = build()
        d.allow_fused = mask
        hs = C.create_string_buffer(256)
        assert L.ipk_pipeline_hashes(C.byref(d), 0, 77, hs) == 0
        a = [C.c_size_t() for _ in range(4)]
        assert L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a]) == 0
        fw, fh = a[2].value, a[3].value
        out = [hs.raw]
        for reg in ((0, 0, fw, fh), (1, 2, 7, 5), (fw - 1, fh - 1, 1, 1)):
            s = [C.c_size_t(12345) for _ in range(4)]
            out.append((L.ipk_pipeline_region(C.byref(d), 0, *reg, *[C.byref(v) for v in s]), tuple(v.value for v in s)))
            bw, bh, base, xs, ys = C.c_size_t(), C.c_size_t(), C.c_int64(), C.c_int64(), C.c_int64()
            rc = L.ipk_pipeline_region_gather(C.byref(d), 0, *reg, C.byref(bw), C.byref(bh), C.byref(base), C.byref(xs), C.byref(ys))
            out.append((rc, bw.value, bh.value, base.value, xs.value, ys.value))
        return out

    for mask in range(64):
        assert reports(mask) == reports(mask & ~CACHED), (name, mask)
    for mask in range(32):
        assert reports(mask | CACHED) == reports(mask), (name, mask)


def test_python_attribute():
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    img = ipa.RawImage(width=342, height=75, data=None, cfa="RGGB", crops=CROPS, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4,
                       wb_coeffs=util.WB, cam_to_xyz_normalized=util.cam_matrix())
    pipe = ipa.Pipeline(img)                                                 # no device: the descriptor alone is read
    assert pipe.resample_cached is False
    rc = pipe.ops.rotatecrop
    rc.crop_top, rc.crop_right, rc.crop_bottom, rc.crop_left, rc.rotation = RC
    assert pipe.desc().allow_fused == ON and not pipe.resamples_cached_region()
    pipe.resample_cached = True
    assert pipe.desc().allow_fused == ON | _lib.FUSED_CACHED_RESAMPLE
    assert pipe.resamples_cached_region() and pipe.resamples_cached_region(1) and pipe.resamples_cached_region(2)
    pipe.allow_fused = False                                                 # the bit stands only beside IPK_FUSED_ON
    assert pipe.desc().allow_fused == 0 and not pipe.resamples_cached_region()
