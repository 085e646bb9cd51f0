"""A batch whose frames carry their own colour settings (no GPU): the plan ipk_pipeline_batch_each_plan reports for ipk_pipeline_run_batch_each -- the runs
of same-shaped descriptors and each frame's route (0 single, 1 uniform, 2 varied previews) -- written down from include/imagepipe_amd.h.  The base
descriptor is the thumbnail of tests/test_batch_previews_route.py; sizes come from ipk_pipeline_sizes and are asserted."""
import ctypes as C

import numpy as np
import pytest

import util
import test_batch_previews_route as br
from test_batch_previews_route import ON, BATCH, OUT_F32, OUT_U8, OUT_U16, thumb

SINGLE, UNIFORM, VARIED = 0, 1, 2


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def plan(L, descs, out_type=OUT_U8):
    """-> (rc, [route], [run_first]); the outputs start from a sentinel"""
    from imagepipe_amd._lib import PipelineDesc
    n = len(descs)
    dp = (C.POINTER(PipelineDesc) * max(n, 1))(*[C.pointer(d) if d is not None else None for d in descs])
    route, first = (C.c_int * max(n, 1))(*[77] * max(n, 1)), (C.c_size_t * max(n, 1))(*[77] * max(n, 1))
    rc = L.ipk_pipeline_batch_each_plan(dp, n, out_type, route, first)
    return rc, list(route)[:n], list(first)[:n]


def with_wb(d, k):
    """descriptor d with the k-th of a family of different white balances (k = 0: as it is)"""
    if k:
        d.wb_coeffs[:] = [util.WB[0] * (1.0 + 0.03125 * k), util.WB[1], util.WB[2] * (1.0 - 0.015625 * k), util.WB[3]]
    return d


def varied(n, **kw):
    return [with_wb(thumb(**kw), i + 1) for i in range(n)]


def test_the_base_descriptor(L):
    d = thumb()
    assert br.sizes(L, d) == (23, 17, 23, 17) and br.cropped(d) == (203, 151) and d.allow_fused == 1 | 256
    assert br.report(L, d, 5) == (1, 64, 1)


@pytest.mark.parametrize("out_type", [OUT_F32, OUT_U8, OUT_U16])
def test_five_white_balances(L, out_type):
    assert plan(L, varied(5), out_type) == (0, [VARIED] * 5, [0] * 5)
    # the same with the bit clear: frame by frame
    assert plan(L, varied(5, allow_fused=ON), out_type) == (0, [SINGLE] * 5, [0] * 5)
    # and the bit without bit 0 is nothing
    assert plan(L, varied(5, allow_fused=BATCH), out_type) == (0, [SINGLE] * 5, [0] * 5)


def test_each_of_the_five_fields_varies_a_run(L):
    def changed(field):
        d = thumb()
        if field == "cam":
            d.cam_to_xyz_normalized[5] = d.cam_to_xyz_normalized[5] * 1.5
        elif field == "exposure":
            d.exposure = 0.5
        elif field == "npoints":
            d.npoints = 2
            d.points[2], d.points[3] = 0.8, 0.85
        elif field == "points":
            d.points[1] = 0.625
        else:
            with_wb(d, 3)
        return d
    for field in ("wb", "cam", "exposure", "npoints", "points"):
        assert plan(L, [thumb(), changed(field), thumb()]) == (0, [VARIED] * 3, [0] * 3), field


def test_identical_descriptors_are_the_uniform_batch(L):
    assert plan(L, [thumb() for _ in range(5)]) == (0, [UNIFORM] * 5, [0] * 5)
    assert plan(L, [thumb(allow_fused=ON) for _ in range(5)]) == (0, [UNIFORM] * 5, [0] * 5)
    assert plan(L, [thumb(allow_fused=0) for _ in range(2)]) == (0, [UNIFORM] * 2, [0] * 2)


def test_a_run_mixing_identical_and_varied_descriptors(L):
    ds = [thumb(), thumb(), with_wb(thumb(), 1), thumb(), with_wb(thumb(), 2), with_wb(thumb(), 2)]
    assert plan(L, ds) == (0, [VARIED] * 6, [0] * 6)
    # with the bit clear the same run keeps its identical neighbours as uniform sub-runs
    for d in ds:
        d.allow_fused = ON
    assert plan(L, ds) == (0, [UNIFORM, UNIFORM, SINGLE, SINGLE, UNIFORM, UNIFORM], [0] * 6)


CUTS = {
    "maxwidth": dict(maxwidth=29),
    "linear": dict(linear=1),
    "crop": dict(crops=(2, 3, 4, 7)),
    "orientation": dict(rotation=1, maxheight=23),
    "rotatecrop": dict(rotatecrop=[0.0, 0.0, 0.0, 0.0, float(np.float32(0.03))]),
    "blacklevel": dict(blacklevels=[util.BLACK + 1.0] + [util.BLACK] * 3),
    "allow_fused": dict(allow_fused=ON | BATCH | 8),
    "schedule": dict(schedule=1),
    "cfa": dict(cfa="GRBG"),
}


@pytest.mark.parametrize("what", list(CUTS))
def test_a_change_of_shape_cuts_the_run(L, what):
    """frames 0-2 the thumbnail, 3-5 the other shape, 6-7 the thumbnail again: three runs, whatever the settings inside them"""
    def other(k):
        kw = dict(CUTS[what])
        cfa = kw.pop("cfa", "RGGB")
        args = dict(crops=(2, 3, 4, 5), maxwidth=23)
        args.update(kw)
        return with_wb(br.make_desc(211, 157, cfa, **args), k)
    takes = br.report(L, other(0), 3)[0] == 1
    if what in ("orientation", "rotatecrop"):
        assert not takes                                                    # out of the route's scope: they go frame by frame
    else:
        assert takes
    first = [0, 0, 0, 3, 3, 3, 6, 6]
    ds = [with_wb(thumb(), k + 1) for k in range(3)] + [other(k + 1) for k in range(3)] + [with_wb(thumb(), k + 1) for k in range(2)]
    mid = VARIED if takes else SINGLE
    assert plan(L, ds) == (0, [VARIED] * 3 + [mid] * 3 + [VARIED] * 2, first), what
    # identical settings inside every run: the uniform batch, for the orientation and rotatecrop runs as well
    ds = [thumb() for _ in range(3)] + [other(0) for _ in range(3)] + [thumb() for _ in range(2)]
    assert plan(L, ds) == (0, [UNIFORM] * 8, first), what
    # one such frame in the middle of a varied batch is a run of its own
    ds = varied(2) + [other(5)] + varied(2)
    assert plan(L, ds) == (0, [VARIED, VARIED, SINGLE, VARIED, VARIED], [0, 0, 2, 3, 3]), what


def test_struct_size_counts_as_shape(L):
    from imagepipe_amd._lib import PipelineDesc
    ds = varied(4)
    ds[2].struct_size = PipelineDesc.schedule.offset                        # the second published layout: its tail reads as zeros, which it holds anyway
    assert plan(L, ds) == (0, [VARIED, VARIED, SINGLE, SINGLE], [0, 0, 2, 3])


def test_padding_and_cfa_spelling_are_not_compared(L):
    a, b = with_wb(thumb(), 1), with_wb(thumb(), 2)
    b.cfa = b"2x2:RGGB"                                                     # folds to the plain letters
    raw = (C.c_char * C.sizeof(b)).from_buffer(b)
    from imagepipe_amd._lib import PipelineDesc
    pad = PipelineDesc.fuse_scaledown.offset + 4                            # the struct's tail padding
    assert C.sizeof(PipelineDesc) == pad + 4
    raw[pad: pad + 4] = b"\xa5" * 4
    c = with_wb(thumb(), 3)
    c.cfa_width, c.cfa_height = 2, 2                                        # stated through the fields: folded as well
    assert plan(L, [a, b, c]) == (0, [VARIED] * 3, [0] * 3)


def test_full_size_frames(L):
    """no size limit: the one-launch raw route.  Varied settings go frame by frame (the persistent batch launch keeps one parameter set); identical ones
    are the uniform batch"""
    full = lambda k: with_wb(br.make_desc(211, 157, "RGGB", crops=(2, 3, 4, 5)), k)
    assert br.sizes(L, full(0)) == (203, 151, 203, 151) and br.report(L, full(0), 3) == (0, 0, 0)
    assert plan(L, [full(k + 1) for k in range(3)]) == (0, [SINGLE] * 3, [0] * 3)
    assert plan(L, [full(0) for _ in range(3)]) == (0, [UNIFORM] * 3, [0] * 3)
    assert plan(L, [full(1), full(1), full(2), full(3), full(3), full(3)]) == (0, [UNIFORM, UNIFORM, SINGLE, UNIFORM, UNIFORM, UNIFORM], [0] * 6)


def test_a_preview_under_256_pixels_is_never_varied(L):
    ds = varied(4, maxwidth=15)
    dw, dh = br.sizes(L, ds[0])[:2]
    assert dw * dh < 256
    assert plan(L, ds) == (0, [SINGLE] * 4, [0] * 4)
    ds = varied(4, maxwidth=19)                                             # 19 x 14 = 266: in
    assert br.sizes(L, ds[0])[:2] == (19, 14) and plan(L, ds)[1] == [VARIED] * 4


def test_invalid_input(L):
    err = lambda: L.ipk_last_error().decode()
    assert plan(L, []) == (0, [], [])
    assert L.ipk_pipeline_batch_each_plan(None, 0, OUT_U8, None, None) == 0
    assert L.ipk_pipeline_batch_each_plan(None, 3, OUT_U8, None, None) == -2
    ds = varied(4)
    rc, route, first = plan(L, ds[:2] + [None] + ds[2:])
    assert rc == -2 and "index 2" in err() and route == [77] * 5 and first == [77] * 5, err()
    bad = varied(4)
    bad[3].fuse_scaledown = 5
    rc, route, first = plan(L, bad)
    assert rc == -2 and "descriptor 3" in err() and "fuse_scaledown" in err() and route == [77] * 4, err()
    bad = varied(4)
    bad[1].npoints = 65
    assert plan(L, bad)[0] == -2 and "descriptor 1" in err(), err()
    bad = varied(4)
    bad[0].struct_size = 0
    assert plan(L, bad)[0] == -2 and "descriptor 0" in err(), err()
    assert plan(L, ds, 3)[0] == -2
    # the outputs are optional
    from imagepipe_amd._lib import PipelineDesc
    dp = (C.POINTER(PipelineDesc) * 4)(*[C.pointer(d) for d in ds])
    assert L.ipk_pipeline_batch_each_plan(dp, 4, OUT_U8, None, None) == 0
    route = (C.c_int * 4)()
    assert L.ipk_pipeline_batch_each_plan(dp, 4, OUT_U8, route, None) == 0 and list(route) == [VARIED] * 4


def test_the_plan_moves_no_other_report(L):
    ds = varied(3) + [thumb(rotation=1, maxheight=23), thumb(maxwidth=0)]
    regions = [(1, 1, 5, 4)]
    before = [(bytes((C.c_char * C.sizeof(d)).from_buffer(d)), br.everything_else(L, d, OUT_U8, regions), br.report(L, d, 3)) for d in ds]
    assert plan(L, ds)[0] == 0
    after = [(bytes((C.c_char * C.sizeof(d)).from_buffer(d)), br.everything_else(L, d, OUT_U8, regions), br.report(L, d, 3)) for d in ds]
    assert before == after


def test_the_python_surface():
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    for name in ("ipk_pipeline_run_batch_each", "ipk_pipeline_batch_each_plan", "ipk_pointwise_chain_out_batch"):
        assert name in _lib.SIGNATURES
    assert C.sizeof(_lib.ChainParams) == 4 + 4 * (4 + 12 + 1 + 1 + 128) == 588 and _lib.ChainParams().struct_size == 588
    p = ipa.chain_params(util.WB, util.cam_matrix(), 0.5, [(0.5, 0.6)])
    assert p.npoints == 1 and p.points[1] == np.float32(0.6) and p.exposure == 0.5
    for name in ("run_batch_each", "batch_each_plan", "pointwise_chain_out_batch", "chain_params"):
        assert name in ipa.__all__ and callable(getattr(ipa, name))


# ---------------------------------------------------------------------------------------------
# rasters: the fast path is decided by the five fields themselves
# ---------------------------------------------------------------------------------------------
def raster(L, exposure=0.0, use_fastpath=1, allow_fused=ON | BATCH, src_type=br.RGB8):
    """a 131x113 raster under maxwidth 40 with Pipeline::default_ops of a raster source, but for the exposure: exposure 0 is the descriptor that
    output_8bit / output_16bit send down the integer fast path"""
    from imagepipe_amd._lib import PipelineDesc
    d = PipelineDesc()
    d.src_type, d.width, d.height, d.cpp, d.maxwidth, d.use_fastpath, d.allow_fused = src_type, 131, 113, 3, 40, use_fastpath, allow_fused
    d.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
    m = (C.c_float * 12)()
    assert L.ipk_const_matrix(2, m) == 0                                    # SRGB_D65_43
    d.cam_to_xyz_normalized[:] = list(m)
    d.exposure = exposure
    return d


def fastpath(L, ds, out_type):
    return [L.ipk_pipeline_takes_fastpath(C.byref(d), out_type) for d in ds]


@pytest.mark.parametrize("src_type", [br.RGB8, br.RGB16])
def test_a_default_raster_among_edited_ones(L, src_type):
    mk = lambda *es: [raster(L, e, src_type=src_type) for e in es]
    assert br.report(L, raster(L, 0.25, src_type=src_type), 3, OUT_U8)[0] == 1 and br.report(L, raster(L, 0.0, src_type=src_type), 3, OUT_U8)[0] == 0
    for out_type in (OUT_U8, OUT_U16):
        # an edited, a default and an edited raster: the default one takes the fast path, so it shares no run with its neighbours
        ds = mk(0.25, 0.0, 0.5)
        assert fastpath(L, ds, out_type) == [0, 1, 0]
        assert plan(L, ds, out_type) == (0, [SINGLE] * 3, [0, 1, 2]), out_type
        # the same whichever comes first
        assert plan(L, mk(0.0, 0.25, 0.5), out_type) == (0, [SINGLE, VARIED, VARIED], [0, 1, 1]), out_type
        ds = mk(0.25, 0.5, 0.0, 0.0, 0.25, 0.5)
        assert plan(L, ds, out_type) == (0, [VARIED, VARIED, UNIFORM, UNIFORM, VARIED, VARIED], [0, 0, 2, 2, 4, 4]), out_type
    # run() has no fast path: one run, all varied
    ds = mk(0.25, 0.0, 0.5)
    assert fastpath(L, ds, OUT_F32) == [0, 0, 0] and plan(L, ds, OUT_F32) == (0, [VARIED] * 3, [0] * 3)
    # nor has a caller who switched it off
    ds = [raster(L, e, use_fastpath=0, src_type=src_type) for e in (0.25, 0.0, 0.5)]
    assert fastpath(L, ds, OUT_U8) == [0, 0, 0] and plan(L, ds, OUT_U8) == (0, [VARIED] * 3, [0] * 3)
    # without the bit the edited ones go frame by frame, the default ones as the uniform batch's loop
    ds = [raster(L, e, allow_fused=ON, src_type=src_type) for e in (0.25, 0.5, 0.0, 0.0)]
    assert plan(L, ds, OUT_U8) == (0, [SINGLE, SINGLE, UNIFORM, UNIFORM], [0, 0, 2, 2])
