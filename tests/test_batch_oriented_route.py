"""A batch whose frames carry their own orientation (no GPU): what IPK_FUSED_BATCH_ORIENTED (allow_fused bit 9, beside bits 0 and 8) changes in
ipk_pipeline_batches_previews and in the plan of ipk_pipeline_run_batch_each, and that without it -- or without either of the bits it acts beside -- every
answer is the one of tests/test_batch_each_route.py and tests/test_batch_previews_route.py.  Written down from include/imagepipe_amd.h; the base descriptor
is those modules' thumbnail under a square box, and every size comes from ipk_pipeline_sizes and is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import test_batch_previews_route as br
from test_batch_previews_route import ON, BATCH, OUT_F32, OUT_U8, OUT_U16, thumb
from test_batch_each_route import plan, with_wb, SINGLE, UNIFORM, VARIED

ORIENTED = 512
ALL = ON | BATCH | ORIENTED
TRIPLES = [(r, h, v) for r in range(4) for h in (0, 1) for v in (0, 1)]
# ipk_orientation: Normal, HorizontalFlip, Rotate180, VerticalFlip, Transpose, Rotate90, Transverse, Rotate270, Unknown
TRANSPOSING = (4, 5, 6, 7)
# one (rotation, fliph, flipv) for each of the eight orientations, in the enum's order
ONE_OF_EACH = [(0, 0, 0), (0, 1, 0), (2, 0, 0), (0, 0, 1), (1, 0, 1), (1, 0, 0), (1, 1, 0), (3, 0, 0)]


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def boxed(triple=(0, 0, 0), allow_fused=ALL, **kw):
    """the thumbnail under the 23 x 23 box with this (rotation, fliph, flipv)"""
    args = dict(maxwidth=23, maxheight=23, rotation=triple[0], fliph=triple[1], flipv=triple[2], allow_fused=allow_fused)
    args.update(kw)
    return thumb(**args)


def test_the_enum_and_the_python_surface():
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    assert _lib.FUSED_BATCH_ORIENTED == ORIENTED == ipa.FUSED_BATCH_ORIENTED and "FUSED_BATCH_ORIENTED" in ipa.__all__
    assert "ipk_pointwise_chain_out_batch_oriented" in _lib.SIGNATURES
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "imagepipe_amd.h")).read()
    assert "IPK_FUSED_BATCH_ORIENTED = 512" in header


def test_the_triples_compose_to_the_eight_orientations(L):
    """OpTransform::run's recomposition (src/ops/transform.rs:58-66): the rotation's flips, then fliph on x and flipv on y"""
    flips = {0: (0, 0, 0), 1: (0, 1, 0), 2: (0, 1, 1), 3: (0, 0, 1), 4: (1, 0, 0), 5: (1, 0, 1), 6: (1, 1, 1), 7: (1, 1, 0)}
    base = {0: 0, 1: 5, 2: 2, 3: 7}
    back = {v: k for k, v in flips.items()}
    for r, h, v in TRIPLES:
        t, fx, fy = flips[base[r]]
        assert L.ipk_transform_orientation(r, h, v) == back[(t, fx ^ h, fy ^ v)], (r, h, v)
    assert [L.ipk_transform_orientation(*t) for t in ONE_OF_EACH] == list(range(8))


def test_the_square_box_gives_every_orientation_the_same_demosaic_size(L):
    for t in TRIPLES:
        ori = L.ipk_transform_orientation(*t)
        want = (23, 17, 17, 23) if ori in TRANSPOSING else (23, 17, 23, 17)
        assert br.sizes(L, boxed(t)) == want, (t, ori)


@pytest.mark.parametrize("out_type", [OUT_F32, OUT_U8, OUT_U16])
def test_batches_previews_for_each_orientation(L, out_type):
    for t in TRIPLES:
        ori = L.ipk_transform_orientation(*t)
        assert br.report(L, boxed(t), 4, out_type) == (1, 64, 1), (t, ori)
        # without bit 9, and with bit 9 but without bit 8 or bit 0: the parent's answer
        for bits in (ON | BATCH, ON | ORIENTED, BATCH | ORIENTED, ORIENTED):
            want = (1, 64, 1) if ori == 0 and bits == ON | BATCH else (0, 0, 0)
            assert br.report(L, boxed(t, allow_fused=bits), 4, out_type) == want, (t, ori, bits)
    assert br.report(L, boxed((1, 0, 0)), 1, out_type) == (0, 0, 0)       # n <= 1 still is not a batch


def test_an_active_rotatecrop_still_answers_0(L):
    for t in ((0, 0, 0), (1, 0, 0), (2, 1, 0)):
        for rc in ((0.1, 0.05, 0.08, 0.12, 0.0), (0.0, 0.0, 0.0, 0.0, 0.03)):
            d = boxed(t, rotatecrop=[float(np.float32(v)) for v in rc])
            assert br.report(L, d, 4) == (0, 0, 0), (t, rc)
    # and in the plan such frames go one by one, cut at every change of orientation as before
    rc = [0.0, 0.0, 0.0, 0.0, float(np.float32(0.03))]
    ds = [with_wb(boxed(t, rotatecrop=rc), k + 1) for k, t in enumerate(ONE_OF_EACH[:4])]
    assert plan(L, ds) == (0, [SINGLE] * 4, [0, 1, 2, 3])


FIVE = [ONE_OF_EACH[i] for i in (0, 5, 2, 7, 4)]                         # Normal, Rotate90, Rotate180, Rotate270, Transpose


@pytest.mark.parametrize("out_type", [OUT_F32, OUT_U8, OUT_U16])
def test_five_orientations_are_one_varied_run(L, out_type):
    """the test that fails without the feature: orientation alone varies the run"""
    assert plan(L, [boxed(t) for t in FIVE], out_type) == (0, [VARIED] * 5, [0] * 5)
    # all eight, and all sixteen triples
    assert plan(L, [boxed(t) for t in ONE_OF_EACH], out_type) == (0, [VARIED] * 8, [0] * 8)
    assert plan(L, [boxed(t) for t in TRIPLES], out_type) == (0, [VARIED] * 16, [0] * 16)


def test_without_the_bit_orientation_cuts_at_every_change(L):
    for bits in (ON | BATCH, ON | ORIENTED, BATCH | ORIENTED, ON):
        assert plan(L, [boxed(t, allow_fused=bits) for t in FIVE]) == (0, [SINGLE] * 5, [0, 1, 2, 3, 4]), bits
    # varied settings inside runs of one orientation: the parent's plan, route 2 only where the parent has it (Normal, bits 0 and 8)
    ds = [with_wb(boxed(t, allow_fused=ON | BATCH), k + 1) for k, t in enumerate([FIVE[0]] * 2 + [FIVE[1]] * 2 + [FIVE[0]] * 2)]
    assert plan(L, ds) == (0, [VARIED, VARIED, SINGLE, SINGLE, VARIED, VARIED], [0, 0, 2, 2, 4, 4])


def test_frames_equal_in_all_eight_fields_are_the_uniform_batch(L):
    for t in ONE_OF_EACH:
        assert plan(L, [boxed(t) for _ in range(3)]) == (0, [UNIFORM] * 3, [0] * 3), t
    # and a run that mixes identical neighbours with another orientation is varied as a whole, as it is for the five fields
    ds = [boxed(FIVE[1]), boxed(FIVE[1]), boxed(FIVE[0]), boxed(FIVE[0])]
    assert plan(L, ds) == (0, [VARIED] * 4, [0] * 4)


def test_orientation_and_white_balance_vary_together(L):
    ds = [with_wb(boxed(t), k + 1) for k, t in enumerate(ONE_OF_EACH)]
    assert plan(L, ds) == (0, [VARIED] * 8, [0] * 8)
    ds = [with_wb(boxed(FIVE[0]), 1), with_wb(boxed(FIVE[0]), 2), boxed(FIVE[1]), boxed(FIVE[1])]
    assert plan(L, ds) == (0, [VARIED] * 4, [0] * 4)


def test_the_demosaic_size_is_shape(L):
    """under maxwidth alone the fold swaps the sides of a frame with rotation 1 or 3 before the clamp (transform.rs:75-84 reads `rotation`, never the
    flips), so such a frame negotiates another demosaic size than its Normal neighbour and cuts the run; frames that differ in the flips alone, or in
    rotation 0 against 2, or 1 against 3, agree under any limit"""
    one = lambda t, k=0: with_wb(boxed(t, maxheight=0), k)
    normal, rot90 = br.sizes(L, one((0, 0, 0))), br.sizes(L, one((1, 0, 0)))
    assert normal == (23, 17, 23, 17) and rot90[:2] != normal[:2] and rot90[2:] == (rot90[1], rot90[0]), (normal, rot90)
    assert br.report(L, one((1, 0, 0)), 3)[:2] == (1, 64)
    assert plan(L, [one((0, 0, 0)), one((1, 0, 0)), one((0, 0, 0))]) == (0, [SINGLE] * 3, [0, 1, 2])
    # Transpose is rotation 1 with flipv: the fold swaps for it as for Rotate90, so it shares a run with Rotate90 and Rotate270, not with Normal
    assert L.ipk_transform_orientation(1, 0, 1) == 4 and br.sizes(L, one((1, 0, 1))) == rot90
    assert plan(L, [one((0, 0, 0)), one((1, 0, 1))]) == (0, [SINGLE] * 2, [0, 1])
    assert plan(L, [one((1, 0, 0)), one((1, 0, 1)), one((3, 0, 0)), one((3, 1, 0))]) == (0, [VARIED] * 4, [0] * 4)
    # the non-transposing ones agree with Normal
    assert plan(L, [one((0, 0, 0)), one((0, 1, 0)), one((2, 0, 0)), one((0, 0, 1))]) == (0, [VARIED] * 4, [0] * 4)
    # varied settings on both sides of the cut
    ds = [one((0, 0, 0), 1), one((0, 1, 0), 2), one((1, 0, 0), 3), one((3, 0, 0), 4)]
    assert plan(L, ds) == (0, [VARIED] * 4, [0, 0, 2, 2])


def test_allow_fused_is_shape(L):
    """two neighbours of which only one carries bit 9 cut"""
    ds = [boxed(FIVE[0]), boxed(FIVE[1], allow_fused=ON | BATCH), boxed(FIVE[0])]
    assert plan(L, ds) == (0, [SINGLE] * 3, [0, 1, 2])
    ds = [with_wb(boxed(FIVE[0]), 1), with_wb(boxed(FIVE[0], allow_fused=ON | BATCH), 2)]
    assert plan(L, ds) == (0, [SINGLE] * 2, [0, 1])


def test_a_preview_under_256_pixels_keeps_its_cuts(L):
    ds = [boxed(t, maxwidth=15, maxheight=15) for t in FIVE]
    dw, dh = br.sizes(L, ds[0])[:2]
    assert dw * dh < 256 and br.report(L, ds[1], 3) == (0, 0, 0)
    assert plan(L, ds) == (0, [SINGLE] * 5, [0, 1, 2, 3, 4])


def test_the_bit_moves_no_other_report(L):
    regions = [(1, 1, 5, 4)]
    for t in FIVE:
        a, b = boxed(t, allow_fused=ON | BATCH), boxed(t)
        assert br.everything_else(L, a, OUT_U8, regions) == br.everything_else(L, b, OUT_U8, regions), t
        assert br.sizes(L, a) == br.sizes(L, b)
