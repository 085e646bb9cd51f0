"""A batch whose frames negotiate their own preview size (no GPU): what IPK_FUSED_BATCH_SIZES (allow_fused bit 11, beside bits 0 and 8, and only with bit 9
or bit 10) changes in the plan of ipk_pipeline_run_batch_each -- the "one demosaic size" condition of bits 9 and 10 is waived for a pair of descriptors
that both carry the bit, would both batch their own previews and both select the general scaling kernel -- the chunks such a run is executed in
(ipk_pipeline_batch_each_chunks), and that without the bit every answer is the parent's.  Written down from include/imagepipe_amd.h; the base descriptor is
the route tests' cropped thumbnail under maxwidth 19, and every size comes from ipk_pipeline_sizes and is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import util
import test_batch_previews_route as br
from test_batch_previews_route import ON, BATCH, OUT_F32, OUT_U8, OUT_U16, XT
from test_batch_each_route import plan, with_wb, SINGLE, UNIFORM, VARIED
from test_batch_sensor_route import skips

ORIENTED, SENSOR, SIZES = 512, 1024, 2048
ROT = ON | BATCH | ORIENTED | SIZES
SEN = ON | BATCH | SENSOR | SIZES
BOTH = ON | BATCH | ORIENTED | SENSOR | SIZES


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def thumb(rotation=0, **kw):
    """211x157 RGGB, crops (2, 3, 4, 5) -> 203x151, maxwidth 19: Normal 19x14, Rotate90 demosaic 25x19 (final 19x25)"""
    args = dict(maxwidth=19, allow_fused=ROT, rotation=rotation)
    args.update(kw)
    return br.thumb(**args)


def body(**kw):
    """a 200x160 sensor (5:4 beside the thumbnail's 4:3): 19x15 under maxwidth 19"""
    args = dict(maxwidth=19, allow_fused=SEN)
    args.update(kw)
    return br.make_desc(200, 160, args.pop("cfa", "RGGB"), **args)


def chunks(L, descs, out_type=OUT_U8):
    """-> (rc, [chunk_first]); the output starts from a sentinel"""
    from imagepipe_amd._lib import PipelineDesc
    n = len(descs)
    dp = (C.POINTER(PipelineDesc) * max(n, 1))(*[C.pointer(d) if d is not None else None for d in descs])
    first = (C.c_size_t * max(n, 1))(*[77] * max(n, 1))
    rc = L.ipk_pipeline_batch_each_chunks(dp, n, out_type, first)
    return rc, list(first)[:n]


def test_the_enum_and_the_surfaces():
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    assert _lib.FUSED_BATCH_SIZES == SIZES == ipa.FUSED_BATCH_SIZES and "FUSED_BATCH_SIZES" in ipa.__all__
    for name in ("ipk_scaled_demosaic_batch_sized", "ipk_pointwise_chain_out_batch_sized", "ipk_pipeline_batch_each_chunks"):
        assert name in _lib.SIGNATURES, name
    for name in ("scaled_demosaic_batch_sized", "pointwise_chain_out_batch_sized", "batch_each_chunks"):
        assert name in ipa.__all__ and callable(getattr(ipa, name)), name
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    header = open(os.path.join(root, "include", "imagepipe_amd.h")).read()
    assert "IPK_FUSED_BATCH_SIZES = 2048" in header
    for name in ("ipk_scaled_demosaic_batch_sized", "ipk_pointwise_chain_out_batch_sized", "ipk_pipeline_batch_each_chunks"):
        assert name in header and name in open(os.path.join(root, "include", "imagepipe_amd.hpp")).read(), name


def test_the_sizes_by_hand(L):
    """the shapes of this module, each with both skips above 7 (pass1_batched = 1) and at least 256 pixels"""
    for d, want in ((thumb(0), (19, 14, 19, 14)), (thumb(1), (25, 19, 19, 25)), (thumb(2), (19, 14, 19, 14)), (thumb(3), (25, 19, 19, 25)),
                    (body(), (19, 15, 19, 15))):
        assert br.sizes(L, d) == want
        dw, dh = want[:2]
        sx, sy = skips(d, dw, dh)
        assert sx > 7.0 and sy > 7.0 and dw * dh >= 256, (want, sx, sy)
        for out_type in (OUT_F32, OUT_U8, OUT_U16):
            assert br.report(L, d, 3, out_type) == (1, 64, 1), want
    assert 19 * 14 == 266 and br.cropped(thumb()) == (203, 151)


@pytest.mark.parametrize("out_type", [OUT_F32, OUT_U8, OUT_U16])
def test_normal_and_rotate90_alternating_are_one_run(L, out_type):
    """the test that fails without the feature: on the parent 19x14 beside 25x19 cuts every pair"""
    for n in (2, 3, 5):
        ds = [thumb(i % 2) for i in range(n)]
        assert plan(L, ds, out_type) == (0, [VARIED] * n, [0] * n), n
        assert chunks(L, ds, out_type) == (0, [0] * n), n
    # all four rotations and a flip, with their own colours
    ds = [with_wb(thumb(i % 4, fliph=(i // 4) % 2), i + 1) for i in range(8)]
    assert plan(L, ds, out_type) == (0, [VARIED] * 8, [0] * 8)


def test_two_sensor_sizes_are_one_run(L):
    ds = [thumb(allow_fused=SEN) if i % 2 == 0 else body() for i in range(5)]
    assert br.sizes(L, ds[0])[:2] == (19, 14) and br.sizes(L, ds[1])[:2] == (19, 15)
    assert plan(L, ds) == (0, [VARIED] * 5, [0] * 5)
    # an X-Trans body of a third size joins
    xt = br.make_desc(216, 192, XT, maxwidth=19, allow_fused=SEN)
    assert br.sizes(L, xt)[:2] == (19, 16) and br.report(L, xt, 2) == (1, 64, 1)
    assert plan(L, ds + [xt]) == (0, [VARIED] * 6, [0] * 6)


def test_orientation_and_sensor_size_together(L):
    ds = [thumb(0, allow_fused=BOTH), body(rotation=1, allow_fused=BOTH), thumb(1, allow_fused=BOTH), body(rotation=2, fliph=1, allow_fused=BOTH)]
    assert [br.sizes(L, d)[:2] for d in ds] == [(19, 14), (23, 19), (25, 19), (19, 15)]
    for d in ds:
        assert br.report(L, d, 2) == (1, 64, 1)
    assert plan(L, ds) == (0, [VARIED] * 4, [0] * 4)
    assert chunks(L, ds) == (0, [0] * 4)


def test_both_sides_need_the_bit(L):
    no = ON | BATCH | ORIENTED
    assert plan(L, [thumb(0), thumb(1, allow_fused=no), thumb(0)]) == (0, [SINGLE] * 3, [0, 1, 2])
    assert plan(L, [thumb(0, allow_fused=no), thumb(1), thumb(0)]) == (0, [SINGLE, VARIED, VARIED], [0, 1, 1])
    no = ON | BATCH | SENSOR
    assert plan(L, [thumb(allow_fused=SEN), body(allow_fused=no), thumb(allow_fused=SEN)]) == (0, [SINGLE] * 3, [0, 1, 2])


def test_the_bit_needs_bit_9_or_bit_10(L):
    alone = ON | BATCH | SIZES
    assert plan(L, [thumb(i % 2, allow_fused=alone) for i in range(4)]) == (0, [SINGLE] * 4, [0, 1, 2, 3])
    assert plan(L, [thumb(allow_fused=alone), body(allow_fused=alone)]) == (0, [SINGLE] * 2, [0, 1])
    # bit 9 lets the orientation differ, not the sensor; bit 10 the sensor, not the orientation
    assert plan(L, [thumb(allow_fused=ROT), body(allow_fused=ROT)]) == (0, [SINGLE] * 2, [0, 1])
    assert plan(L, [thumb(0, allow_fused=SEN), thumb(1, allow_fused=SEN)]) == (0, [SINGLE] * 2, [0, 1])
    # and neither of bits 0 and 8 may be missing
    for bits in (BATCH | ORIENTED | SIZES, ON | ORIENTED | SIZES):
        assert plan(L, [thumb(i % 2, allow_fused=bits) for i in range(3)]) == (0, [SINGLE] * 3, [0, 1, 2]), bits


def test_a_window_8_frame_cuts(L):
    """a frame whose skip is at most 7 (pass1_batched = 0) has no sized launch: 203x151 under maxwidth 60, Normal 60x44, Rotate90 80x60"""
    n8, r8 = thumb(0, maxwidth=60), thumb(1, maxwidth=60)
    assert br.sizes(L, n8)[:2] == (60, 44) and br.sizes(L, r8)[:2] == (80, 60)
    assert max(skips(n8, 60, 44)) <= 7.0 and br.report(L, n8, 2) == (1, 64, 0) and br.report(L, r8, 2) == (1, 64, 0)
    assert plan(L, [n8, r8, n8]) == (0, [SINGLE] * 3, [0, 1, 2])
    # one side alone: under maxwidth 28 the Normal frame (28x20, skips 7.5) selects the general kernel, the Rotate90 frame (37x28, skip 5.6) does not
    a, b = thumb(0, maxwidth=28), thumb(1, maxwidth=28)
    assert br.sizes(L, a)[:2] == (28, 20) and br.sizes(L, b)[:2] == (37, 28)
    assert br.report(L, a, 2) == (1, 64, 1) and br.report(L, b, 2) == (1, 64, 0) and min(skips(a, 28, 20)) > 7.0 and skips(b, 37, 28)[0] <= 7.0
    assert plan(L, [a, b, a]) == (0, [SINGLE] * 3, [0, 1, 2])
    assert plan(L, [b, a, a, b]) == (0, [SINGLE, UNIFORM, UNIFORM, SINGLE], [0, 1, 1, 3])


def test_maxwidth_and_four_still_count(L):
    assert plan(L, [thumb(0), thumb(1, maxwidth=21), thumb(0)]) == (0, [SINGLE] * 3, [0, 1, 2])
    assert br.sizes(L, thumb(1, maxwidth=21))[:2] == (28, 21)
    assert plan(L, [thumb(0), thumb(1, maxheight=40)]) == (0, [SINGLE] * 2, [0, 1])
    rgbe = body(cfa="RGBE")
    assert br.sizes(L, rgbe)[:2] == (19, 15) and br.report(L, rgbe, 2) == (1, 64, 1)
    assert plan(L, [thumb(allow_fused=SEN), rgbe, thumb(allow_fused=SEN)]) == (0, [SINGLE] * 3, [0, 1, 2])
    assert plan(L, [rgbe, body(cfa="RGBE", crops=(0, 0, 0, 0), blacklevels=[util.BLACK + 1.0] * 4)])[1] == [VARIED] * 2


def test_everything_equal_is_route_1_and_equal_sizes_take_the_old_run(L):
    assert plan(L, [thumb(1) for _ in range(4)]) == (0, [UNIFORM] * 4, [0] * 4)
    assert chunks(L, [thumb(1) for _ in range(4)]) == (0, [0] * 4)
    # rotations of one demosaic size: the run bit 9 gave without bit 11
    ds = [thumb(0), thumb(2), thumb(0, fliph=1)]
    assert plan(L, ds) == (0, [VARIED] * 3, [0] * 3)


def test_without_the_bit_the_plan_does_not_move(L):
    for bits in (ON | BATCH | ORIENTED, ON | BATCH | SENSOR, ON | BATCH | ORIENTED | SENSOR, ON | BATCH, ON, 0):
        ds = [thumb(i % 2, allow_fused=bits) for i in range(4)]
        assert plan(L, ds) == (0, [SINGLE] * 4, [0, 1, 2, 3]), bits
        assert chunks(L, ds) == (0, [0, 1, 2, 3]), bits
        ds = [thumb(allow_fused=bits), body(allow_fused=bits), thumb(allow_fused=bits)]
        assert plan(L, ds) == (0, [SINGLE] * 3, [0, 1, 2]), bits
    # under a square box bit 9 alone keeps its run
    box = lambda rot: br.thumb(maxwidth=23, maxheight=23, rotation=rot, allow_fused=ON | BATCH | ORIENTED)
    assert plan(L, [box(i % 4) for i in range(5)]) == (0, [VARIED] * 5, [0] * 5)


def test_the_bit_moves_no_other_report(L):
    regions = [(1, 1, 5, 4)]
    for mk in (lambda: thumb(0), lambda: thumb(1), body):
        a, b = mk(), mk()
        a.allow_fused &= ~SIZES
        assert br.everything_else(L, a, OUT_U8, regions) == br.everything_else(L, b, OUT_U8, regions)
        assert br.sizes(L, a) == br.sizes(L, b) and br.report(L, a, 3) == br.report(L, b, 3)
    full = lambda bits: br.make_desc(211, 157, "RGGB", crops=(2, 3, 4, 5), allow_fused=bits)
    assert br.everything_else(L, full(SIZES), OUT_U8, regions) == br.everything_else(L, full(ON), OUT_U8, regions)


# ---------------------------------------------------------------------------------------------
# chunks
# ---------------------------------------------------------------------------------------------
def test_67_equal_sized_frames_are_64_and_3(L):
    ds = [with_wb(thumb(0), i + 1) for i in range(67)]
    assert plan(L, ds) == (0, [VARIED] * 67, [0] * 67)
    assert chunks(L, ds) == (0, [0] * 64 + [64] * 3)
    # the uniform batch of previews reports the same cut
    assert chunks(L, [thumb(0) for _ in range(67)]) == (0, [0] * 64 + [64] * 3)


def test_mixed_sizes_cut_at_64(L):
    ds = [thumb(i % 2) for i in range(67)]
    assert plan(L, ds) == (0, [VARIED] * 67, [0] * 67)
    assert chunks(L, ds) == (0, [0] * 64 + [64] * 3)
    ds = [thumb(i % 2) for i in range(130)]
    assert chunks(L, ds) == (0, [0] * 64 + [64] * 64 + [128] * 2)


def big(rot, **kw):
    """a 60000x40000 sensor under maxwidth 3000: Normal 3000x2000 (6 MP, 91.6 MiB of RGBE), Rotate90 4500x3000 (13.5 MP, 206 MiB); skips 20 and 13.3"""
    args = dict(maxwidth=3000, allow_fused=ROT, rotation=rot)
    args.update(kw)
    return br.make_desc(60000, 40000, "RGGB", **args)


def test_large_frames_cut_at_the_256_mib_sum(L):
    """hostile sizes, nothing allocated: the report is host arithmetic alone"""
    assert br.sizes(L, big(0))[:2] == (3000, 2000) and br.sizes(L, big(1))[:2] == (4500, 3000)
    assert br.report(L, big(0), 5) == (1, 2, 1) and br.report(L, big(1), 5) == (1, 1, 1)
    mib = lambda wh: wh[0] * wh[1] * 16 / 2.0 ** 20
    assert mib((3000, 2000)) < 92 and 205 < mib((4500, 3000)) < 207
    # N N R N N N R R N: 91.6 + 91.6 | 206 | 91.6 + 91.6 | 91.6 | 206 | 206 | 91.6  (N + R is 297.6 MiB: cut)
    rots = [0, 0, 1, 0, 0, 0, 1, 1, 0]
    ds = [big(r) for r in rots]
    assert plan(L, ds) == (0, [VARIED] * 9, [0] * 9)
    assert chunks(L, ds) == (0, [0, 0, 2, 3, 3, 5, 6, 7, 8])
    # equal sizes reproduce ipk_pipeline_batches_previews' chunk: 2 for the Normal frames, 1 for the rotated ones
    ds = [with_wb(big(0), i + 1) for i in range(5)]
    assert chunks(L, ds) == (0, [0, 0, 2, 2, 4])
    ds = [with_wb(big(1), i + 1) for i in range(3)]
    assert chunks(L, ds) == (0, [0, 1, 2])
    # previews that alone exceed 256 MiB (5500x3666 is 308 MiB of RGBE, 8250x5500 692 MiB; skips 10.9 and 7.3): one run, every frame a chunk of its own
    over = [big(r, maxwidth=5500) for r in (0, 1, 0, 0)]
    assert [br.sizes(L, d)[:2] for d in over[:2]] == [(5500, 3666), (8250, 5500)] and 5500 * 3666 > 1 << 24
    assert br.report(L, over[0], 5) == (1, 1, 1) and br.report(L, over[1], 5) == (1, 1, 1)
    assert plan(L, over) == (0, [VARIED] * 4, [0] * 4) and chunks(L, over) == (0, [0, 1, 2, 3])
    # a small frame behind a large one does not join it, and two small ones behind that share a chunk
    # (maxwidth 3500: Normal 3500x2333, 124.6 MiB; Rotate90 5250x3500, 18.4 MP, alone above the cut)
    m = [big(r, maxwidth=3500) for r in (1, 0, 0, 1, 0)]
    assert [br.sizes(L, d)[:2] for d in m[:2]] == [(5250, 3500), (3500, 2333)] and 5250 * 3500 > 1 << 24 > 2 * 3500 * 2333
    assert plan(L, m) == (0, [VARIED] * 5, [0] * 5) and chunks(L, m) == (0, [0, 1, 1, 3, 4])
    # previews of 2^36 x 2^35 pixels, whose byte count leaves 64 bits: ipk_pipeline_batches_previews answers 0 for them, so they never share a
    # scratch -- single frames, or a uniform run that does not batch -- and every frame is its own chunk
    huge = lambda rot: br.make_desc(1 << 40, 1 << 39, "RGGB", maxwidth=1 << 36, allow_fused=ROT, rotation=rot)
    ds = [huge(0), huge(1), huge(0), huge(0)]
    assert br.sizes(L, ds[0])[:2] == (1 << 36, 1 << 35) and br.report(L, ds[0], 3) == (0, 0, 0) and br.report(L, ds[1], 3) == (0, 0, 0)
    assert plan(L, ds) == (0, [SINGLE, SINGLE, UNIFORM, UNIFORM], [0, 1, 2, 2]) and chunks(L, ds) == (0, [0, 1, 2, 3])


@pytest.mark.parametrize("wh_mw", [((203, 151), 19), ((2048, 1366), 1024), ((8640, 5760), 2160), ((6000, 4000), 3000)])
def test_runs_of_equal_size_reproduce_the_report(L, wh_mw):
    (w, h), mw = wh_mw
    d = lambda k: with_wb(br.make_desc(w, h, "RGGB", maxwidth=mw, allow_fused=ROT), k)
    rc, chunk, p1 = br.report(L, d(0), 200)
    dw, dh = br.sizes(L, d(0))[:2]
    assert rc == 1 and chunk == br.chunk_of(dw, dh)
    n = 2 * chunk + 1
    ds = [d(k + 1) for k in range(n)]
    assert plan(L, ds) == (0, [VARIED] * n, [0] * n)
    assert chunks(L, ds) == (0, [i // chunk * chunk for i in range(n)])


def test_routes_0_and_1_report_themselves(L):
    full = lambda k: with_wb(br.make_desc(211, 157, "RGGB", crops=(2, 3, 4, 5), allow_fused=ROT), k)
    assert chunks(L, [full(1), full(2), full(3)]) == (0, [0, 1, 2])
    # a uniform run that does not batch previews (full-size frames) has no scratch to share
    assert plan(L, [full(0), full(0), full(0)])[1] == [UNIFORM] * 3
    assert chunks(L, [full(0), full(0), full(0)]) == (0, [0, 1, 2])
    assert chunks(L, []) == (0, [])


def test_invalid_input_names_its_index(L):
    err = lambda: L.ipk_last_error().decode()
    ds = [thumb(i % 2) for i in range(4)]
    rc, first = chunks(L, ds[:2] + [None] + ds[2:])
    assert rc == -2 and "index 2" in err() and first == [77] * 5, err()
    bad = [thumb(i % 2) for i in range(4)]
    bad[3].fuse_scaledown = 5
    rc, first = chunks(L, bad)
    assert rc == -2 and "descriptor 3" in err() and first == [77] * 4, err()
    assert plan(L, bad)[0] == -2 and "descriptor 3" in err()
    bad = [thumb(i % 2) for i in range(4)]
    bad[1].npoints = 65
    assert chunks(L, bad)[0] == -2 and "descriptor 1" in err(), err()
    assert chunks(L, [thumb()], 3)[0] == -2
