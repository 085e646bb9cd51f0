"""The row class test of the Lab out-of-table step (imagepipe_amd/csrc/ipk_lab_slots.inc): as an unsigned integer the bit pattern of an f32 is below
0x40000000 -- the bits of 2.0f -- exactly when the value lies in [+0, 2): every value >= 2, +inf, every NaN, -0 and every negative value is at or above it."""
import numpy as np

import util


def _ordinary(v):
    return np.asarray(v, np.float32).view(np.uint32) < np.uint32(0x40000000)


def _in_class(v):
    v = np.asarray(v, np.float32)
    with np.errstate(invalid="ignore"):
        return (v >= 0) & (v < 2) & ~np.signbit(v)


def test_class_predicate_on_the_special_values():
    assert np.array_equal(_ordinary(util.SPECIALS), _in_class(util.SPECIALS))
    assert not _ordinary(np.float32(-0.0)) and _ordinary(np.float32(0.0)) and not _ordinary(np.float32(2.0)) and not _ordinary(np.float32(np.nan))
    assert _ordinary(np.nextafter(np.float32(2.0), np.float32(0.0))) and _ordinary(np.float32(1e-45))


def test_class_predicate_over_every_exponent():
    """every exponent field (denormals, the normal range, inf / NaN) with the lowest, the highest and a few middle mantissas, both signs"""
    e = np.arange(256, dtype=np.uint32)[:, None] << np.uint32(23)
    m = np.array([0, 1, 0x2AAAAA, 0x400000, 0x555555, 0x7FFFFE, 0x7FFFFF], np.uint32)[None, :]
    pos = (e | m).ravel()
    bits = np.concatenate([pos, pos | np.uint32(0x80000000)])
    v = bits.view(np.float32)
    assert np.array_equal(_ordinary(v), _in_class(v))
    assert int(_ordinary(v).sum()) == 128 * 7            # exponent fields 0..127 of the positive half: [+0, 2)
