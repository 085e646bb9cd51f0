"""The guarded-buffer helpers of tests/util.py, checked on numpy arrays (no GPU): a write planted one element before the destination, one element
after it, or at the far end of either band must be reported; an untouched buffer, and one whose interior alone was written, pass.  The GPU classes
(util.Guarded, util.Embedded) use exactly these functions for layout and checks."""
import numpy as np
import pytest

import util

DTYPES = [np.float32, np.uint8, np.uint16]
LAYOUTS = [(1, 0, 64), (1, 1, 64), (257 * 11 * 3, 0, 1024), (257 * 11 * 3, 1, 1024), (300, 3, 1024), (0, 1, 100)]      # (n, off, band)


@pytest.mark.parametrize("n,off,band", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8", "u16"])
def test_layout_sits_off_a_256_byte_boundary_with_whole_bands(dtype, n, off, band):
    lo, total = util.guard_layout(n, off, band)
    assert ((lo - off) * np.dtype(dtype).itemsize) % 256 == 0
    assert lo - off >= band and total - (lo + n) == band
    a = util.guard_fill(n, dtype, off, band)
    assert a.size == total and a.dtype == dtype and np.all(a == np.array(util.SENTINELS[np.dtype(dtype).name]).astype(dtype))


@pytest.mark.parametrize("n,off,band", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8", "u16"])
def test_untouched_and_interior_writes_pass(dtype, n, off, band):
    a = util.guard_fill(n, dtype, off, band)
    inner = util.guard_check(a, n, off, band, "untouched")
    assert inner.size == n and np.all(inner == a[0])                     # the interior starts out as sentinels: an unwritten sample is visible
    lo, _ = util.guard_layout(n, off, band)
    a[lo: lo + n] = 1                                                    # every interior element, the first and the last included
    inner = util.guard_check(a, n, off, band, "interior")
    assert inner.size == n and np.all(inner == 1)


@pytest.mark.parametrize("where", ["one-before", "one-after", "front-band-far-end", "back-band-far-end"])
@pytest.mark.parametrize("n,off,band", LAYOUTS)
@pytest.mark.parametrize("dtype", DTYPES, ids=["f32", "u8", "u16"])
def test_planted_band_writes_are_reported(dtype, n, off, band, where):
    a = util.guard_fill(n, dtype, off, band)
    lo, total = util.guard_layout(n, off, band)
    at = {"one-before": lo - 1, "one-after": lo + n, "front-band-far-end": 0, "back-band-far-end": total - 1}[where]
    a[at] = 1
    with pytest.raises(AssertionError, match="guard bands"):
        util.guard_check(a, n, off, band, where)


def test_a_nan_in_a_band_is_reported():
    a = util.guard_fill(12, np.float32, 1)
    a[util.guard_layout(12, 1)[0] + 12] = np.nan
    with pytest.raises(AssertionError, match="1 elements past its last"):
        util.guard_check(a, 12, 1, what="nan")


def test_a_buffer_of_the_wrong_size_is_refused():
    with pytest.raises(AssertionError):
        util.guard_check(util.guard_fill(12, np.uint8, 0), 12, 1)


@pytest.mark.parametrize("off", [0, 1, 3])
@pytest.mark.parametrize("dtype", [np.float32, np.uint16], ids=["f32", "u16"])
def test_embedded_source_is_surrounded_by_poison(dtype, off):
    data = (np.arange(11 * 13, dtype=np.uint32) % 4000).astype(dtype).reshape(11, 13)
    host, lo = util.embed_host(data, off)
    assert host.dtype == dtype and ((lo - off) * host.itemsize) % 256 == 0 and lo - off >= 1024 and host.size - (lo + data.size) >= 1024
    assert np.array_equal(host[lo: lo + data.size], data.ravel())
    outside = np.concatenate([host[:lo], host[lo + data.size:]])
    if dtype == np.float32:
        assert np.all(outside.view(np.uint32) == 0x7FC00000) and np.isnan(outside).all()
    else:
        assert np.all(outside == 0xFFFF)
