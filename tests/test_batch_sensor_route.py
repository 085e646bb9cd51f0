"""A batch whose frames carry their own sensor settings (no GPU): what IPK_FUSED_BATCH_SENSOR (allow_fused bit 10, beside bits 0 and 8) changes in the plan
of ipk_pipeline_run_batch_each -- width, height, cfa, cfa_width, cfa_height, the four crops, blacklevels and whitelevels may differ inside a run whose
frames select the general scaling kernel and negotiate one demosaic size -- and that without it, or without either of the bits it acts beside, every
answer is the one of tests/test_batch_each_route.py.  Written down from include/imagepipe_amd.h; the base descriptor is those modules' thumbnail, and every
size comes from ipk_pipeline_sizes and is asserted."""
import ctypes as C
import os

import numpy as np
import pytest

import util
import test_batch_previews_route as br
from test_batch_previews_route import ON, BATCH, PLAIN_PREVIEWS, OUT_F32, OUT_U8, OUT_U16, XT, U16, F32
from test_batch_each_route import plan, with_wb, SINGLE, UNIFORM, VARIED

ORIENTED, SENSOR = 512, 1024
ALL = ON | BATCH | SENSOR


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def thumb(**kw):
    """the thumbnail of the route tests with bits 0, 8 and 10: 211x157 RGGB, crops (2, 3, 4, 5) -> 203x151, maxwidth 23 -> 23x17"""
    args = dict(allow_fused=ALL)
    args.update(kw)
    cfa = args.pop("cfa", None)
    d = br.thumb(**args)
    if cfa is not None:
        d.cfa = cfa
    return d


def other(w, h, cfa="RGGB", crops=(0, 0, 0, 0), **kw):
    args = dict(maxwidth=23, allow_fused=ALL)
    args.update(kw)
    return br.make_desc(w, h, cfa, crops=crops, **args)


def skips(d, nw, nh):
    """the launcher's f32 skips (src/scaling.rs:69-72) of the cropped frame"""
    w, h = br.cropped(d)
    f = np.float32
    return float((f(w - 1) - f(0)) / f(nw - 1)), float((f(h - 1) - f(0)) / f(nh - 1))


# the eight sensor fields, each varied alone against the thumbnail
def _cfa_width():
    d = thumb()
    d.cfa_width, d.cfa_height = 2, 2                                        # folded into cfa: the same filter, stated through the fields
    d.cfa = b"GRBG"
    return d


def _cfa_height():
    d = thumb()
    d.cfa = b"2x2:BGGR"
    return d


FIELDS = {
    "width": lambda: thumb(width=213, crops=(2, 5, 4, 5)),                   # 213 - 10 = 203: the cropped size stays, the pitch moves
    "height": lambda: thumb(height=159, crops=(2, 3, 6, 5)),
    "cfa": lambda: thumb(cfa=b"GRBG"),
    "cfa_width": _cfa_width,
    "cfa_height": _cfa_height,
    "crop_top": lambda: thumb(crops=(1, 3, 4, 5)),                           # 203x152: still 23x17 (a crop that shrinks the height negotiates 23x16)
    "crop_right": lambda: thumb(crops=(2, 4, 4, 5)),                         # 202x151
    "crop_bottom": lambda: thumb(crops=(2, 3, 2, 5)),
    "crop_left": lambda: thumb(crops=(2, 3, 4, 6)),
    "blacklevels": lambda: thumb(blacklevels=[util.BLACK + 1.0] + [util.BLACK] * 3),
    "whitelevels": lambda: thumb(whitelevels=[util.WHITE - 100.0] * 4),
}


def test_the_enum_and_the_python_surface():
    import imagepipe_amd as ipa
    from imagepipe_amd import _lib
    assert _lib.FUSED_BATCH_SENSOR == SENSOR == ipa.FUSED_BATCH_SENSOR and "FUSED_BATCH_SENSOR" in ipa.__all__
    assert "ipk_scaled_demosaic_batch_each" in _lib.SIGNATURES
    for name in ("scaled_frame", "scaled_demosaic_batch_each"):
        assert name in ipa.__all__ and callable(getattr(ipa, name))
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "imagepipe_amd.h")).read()
    assert "IPK_FUSED_BATCH_SENSOR = 1024" in header
    # ipk_scaled_frame: a uint32 (padded to 8), five size_t, eight floats, 160 chars
    assert C.sizeof(_lib.ScaledFrame) == 8 + 5 * 8 + 8 * 4 + 160 == 240 and _lib.ScaledFrame().struct_size == 240
    f = ipa.scaled_frame(216, 5, 2, 203, 151, 64.0, [1000.0, 1001.0, 1002.0], "RGGB")
    assert (f.owidth, f.x, f.y, f.width, f.height) == (216, 5, 2, 203, 151) and f.cfa == b"RGGB"
    assert list(f.black4) == [64.0, 0.0, 0.0, 0.0] and list(f.white4) == [1000.0, 1001.0, 1002.0, 0.0]


def test_the_base_descriptor(L):
    d = thumb()
    assert br.sizes(L, d) == (23, 17, 23, 17) and br.cropped(d) == (203, 151) and d.allow_fused == 1 | 256 | 1024
    assert br.report(L, d, 5) == (1, 64, 1)
    sx, sy = skips(d, 23, 17)
    assert sx > 7.0 and sy > 7.0


@pytest.mark.parametrize("field", list(FIELDS))
@pytest.mark.parametrize("out_type", [OUT_F32, OUT_U8, OUT_U16])
def test_each_sensor_field_alone_varies_a_run(L, field, out_type):
    """the test that fails without the feature: on the parent every one of these cuts the run"""
    d = FIELDS[field]()
    assert br.sizes(L, d) == (23, 17, 23, 17) and br.report(L, d, 3, out_type) == (1, 64, 1), field
    for n in (2, 3, 5):
        ds = [thumb() if i % 2 == 0 else FIELDS[field]() for i in range(n)]
        assert plan(L, ds, out_type) == (0, [VARIED] * n, [0] * n), (field, n)


def joiners():
    return [other(230, 170), other(216, 162, XT), other(211, 157, "GRBG", crops=(2, 4, 4, 4))]


def test_other_bodies_join_the_run(L):
    """a larger sensor, an X-Trans body and a frame whose odd crop_left made its filter GRBG: all negotiate 23 x 17 with both skips above 7"""
    for d in joiners():
        assert br.sizes(L, d) == (23, 17, 23, 17), br.cropped(d)
        sx, sy = skips(d, 23, 17)
        assert sx > 7.0 and sy > 7.0 and br.report(L, d, 2) == (1, 64, 1), (sx, sy)
    assert br.cropped(joiners()[2]) == (203, 151) and joiners()[2].crop_left % 2 == 0 and thumb().crop_left % 2 == 1
    ds = [thumb()] + joiners() + [thumb()]
    assert plan(L, ds) == (0, [VARIED] * 5, [0] * 5)
    # with their own colours too
    ds = [with_wb(d, k + 1) for k, d in enumerate([thumb()] + joiners() + [thumb()])]
    assert plan(L, ds) == (0, [VARIED] * 5, [0] * 5)
    # and each of them next to itself alone is the uniform batch
    for k in range(3):
        assert plan(L, [joiners()[k], joiners()[k]]) == (0, [UNIFORM] * 2, [0] * 2), k


MONO = dict(cpp=1, is_cfa=0)
CUTS = {
    "size 23x16": lambda: other(204, 150),
    "window-8 kernel": lambda: thumb(maxwidth=60),
    "src_type": lambda: thumb(src_type=F32),
    "mono": lambda: br.make_desc(211, 157, "", crops=(2, 3, 4, 5), maxwidth=23, allow_fused=ALL | PLAIN_PREVIEWS, **MONO),
    "rgbe": lambda: thumb(cfa=b"RGBE"),
    "maxwidth": lambda: thumb(maxwidth=29),
    "rotatecrop": lambda: thumb(rotatecrop=[0.0, 0.0, 0.0, 0.0, float(np.float32(0.03))]),
    "no bit 10": lambda: thumb(allow_fused=ON | BATCH),
    "no bit 8": lambda: thumb(allow_fused=ON | SENSOR),
    "no bit 0": lambda: thumb(allow_fused=BATCH | SENSOR),
}


def test_the_cutting_frames_are_what_they_claim(L):
    assert br.sizes(L, CUTS["size 23x16"]())[:2] == (23, 16) and br.report(L, CUTS["size 23x16"](), 2) == (1, 64, 1)
    d = CUTS["window-8 kernel"]()
    dw, dh = br.sizes(L, d)[:2]
    assert not br.general_kernel(203, 151, dw, dh) and br.report(L, d, 2) == (1, 64, 0), (dw, dh)
    assert br.sizes(L, CUTS["src_type"]()) == (23, 17, 23, 17) and br.report(L, CUTS["src_type"](), 2) == (1, 64, 1)
    assert br.sizes(L, CUTS["mono"]()) == (23, 17, 23, 17) and br.report(L, CUTS["mono"](), 2) == (1, 64, 1)
    assert br.sizes(L, CUTS["rgbe"]()) == (23, 17, 23, 17) and br.report(L, CUTS["rgbe"](), 2) == (1, 64, 1)
    assert br.report(L, CUTS["rotatecrop"](), 2) == (0, 0, 0)


@pytest.mark.parametrize("what", list(CUTS))
def test_these_cut_the_run(L, what):
    """frames 0-1 the thumbnail with its own black levels, frame 2 the cutting one, frames 3-4 thumbnails again: three runs"""
    lv = lambda k: thumb(blacklevels=[util.BLACK + float(k)] * 4)
    ds = [lv(1), lv(2), CUTS[what](), lv(3), lv(4)]
    assert plan(L, ds) == (0, [VARIED, VARIED, SINGLE, VARIED, VARIED], [0, 0, 2, 3, 3]), what
    # the same whichever side states the difference: two of the cutting kind in the middle
    ds = [lv(1), lv(2), CUTS[what](), CUTS[what](), lv(3)]
    rc, route, first = plan(L, ds)
    assert rc == 0 and first == [0, 0, 2, 2, 4] and route[:2] == [VARIED, VARIED] and route[4] == SINGLE, what


def test_both_sides_need_the_bit(L):
    lv = lambda k, bits=ALL: thumb(blacklevels=[util.BLACK + float(k)] * 4, allow_fused=bits)
    assert plan(L, [lv(1), lv(2, ON | BATCH), lv(3)]) == (0, [SINGLE] * 3, [0, 1, 2])
    assert plan(L, [lv(1, ON | BATCH), lv(2), lv(3)]) == (0, [SINGLE, VARIED, VARIED], [0, 1, 1])


def test_mono_frames_with_their_own_levels_under_bit_7(L):
    mono = lambda k, src_type=U16: br.make_desc(211, 157, "", crops=(2, 3, 4, 5), maxwidth=23, allow_fused=ALL | PLAIN_PREVIEWS, src_type=src_type,
                                                blacklevels=[util.BLACK + float(k)] * 4, **MONO)
    assert br.report(L, mono(0), 3) == (1, 64, 1)
    assert plan(L, [mono(k) for k in range(4)]) == (0, [VARIED] * 4, [0] * 4)
    # without bit 7 a monochrome raw is no preview batch at all
    ds = [br.make_desc(211, 157, "", crops=(2, 3, 4, 5), maxwidth=23, allow_fused=ALL, blacklevels=[util.BLACK + float(k)] * 4, **MONO) for k in range(3)]
    assert plan(L, ds) == (0, [SINGLE] * 3, [0, 1, 2])
    # three-sample raws likewise
    rgb = lambda k: br.make_desc(211, 157, "", crops=(2, 3, 4, 5), maxwidth=23, allow_fused=ALL | PLAIN_PREVIEWS, cpp=3, is_cfa=0,
                                 whitelevels=[util.WHITE - float(k)] * 4)
    assert plan(L, [rgb(k) for k in range(3)]) == (0, [VARIED] * 3, [0] * 3)
    assert plan(L, [mono(0), mono(1), rgb(0), rgb(1)]) == (0, [VARIED] * 4, [0, 0, 2, 2])


def test_sensor_fields_equal_and_colours_varied_is_route_2(L):
    assert plan(L, [with_wb(thumb(), k + 1) for k in range(4)]) == (0, [VARIED] * 4, [0] * 4)


def test_everything_equal_is_route_1(L):
    assert plan(L, [thumb() for _ in range(4)]) == (0, [UNIFORM] * 4, [0] * 4)
    # identical neighbours inside a run that varies elsewhere: the whole run is varied, as for the five fields
    assert plan(L, [thumb(), thumb(), FIELDS["blacklevels"](), FIELDS["blacklevels"]()]) == (0, [VARIED] * 4, [0] * 4)


def test_orientation_and_sensor_vary_together_under_bits_9_and_10(L):
    box = lambda t, **kw: thumb(maxwidth=23, maxheight=23, rotation=t[0], fliph=t[1], flipv=t[2], allow_fused=ALL | ORIENTED, **kw)
    ds = [box((0, 0, 0)), box((1, 0, 0), blacklevels=[util.BLACK + 2.0] * 4), box((2, 0, 0), crops=(1, 3, 4, 5)), box((3, 1, 0), cfa=b"GRBG")]
    for d in ds:
        assert br.sizes(L, d)[:2] == (23, 17)
    assert plan(L, ds) == (0, [VARIED] * 4, [0] * 4)
    # bit 10 without bit 9: the orientation still cuts
    for d in ds:
        d.allow_fused = ALL
    assert plan(L, ds)[2] == [0, 1, 2, 3]


def test_without_the_bit_the_plan_does_not_move(L):
    for bits in (ON | BATCH, ON | SENSOR, BATCH | SENSOR, ON, SENSOR):
        for field in FIELDS:
            d = FIELDS[field]()
            d.allow_fused = bits
            ds = [thumb(allow_fused=bits), d, thumb(allow_fused=bits)]
            assert plan(L, ds) == (0, [SINGLE] * 3, [0, 1, 2]), (bits, field)
    # varied colours inside runs of one sensor setting: the parent's plan
    lv = lambda k, c: with_wb(thumb(blacklevels=[util.BLACK + float(k)] * 4, allow_fused=ON | BATCH), c)
    assert plan(L, [lv(0, 1), lv(0, 2), lv(1, 3), lv(1, 4), lv(0, 5)]) == (0, [VARIED, VARIED, VARIED, VARIED, SINGLE], [0, 0, 2, 2, 4])


def test_the_bit_moves_no_other_report(L):
    regions = [(1, 1, 5, 4)]
    for mk in [thumb] + [FIELDS[f] for f in FIELDS]:
        a, b = mk(), mk()
        a.allow_fused = ON | BATCH
        assert br.everything_else(L, a, OUT_U8, regions) == br.everything_else(L, b, OUT_U8, regions)
        assert br.sizes(L, a) == br.sizes(L, b) and br.report(L, a, 3) == br.report(L, b, 3)
    ds = [thumb()] + joiners()
    before = [(bytes((C.c_char * C.sizeof(d)).from_buffer(d)), br.everything_else(L, d, OUT_U8, regions), br.report(L, d, 3)) for d in ds]
    assert plan(L, ds)[0] == 0
    after = [(bytes((C.c_char * C.sizeof(d)).from_buffer(d)), br.everything_else(L, d, OUT_U8, regions), br.report(L, d, 3)) for d in ds]
    assert before == after
    # allow_fused = 1024 alone still means "on" to the older routes: the full-size frame's reports are those of allow_fused = 1
    full = lambda bits: br.make_desc(211, 157, "RGGB", crops=(2, 3, 4, 5), allow_fused=bits)
    assert br.everything_else(L, full(SENSOR), OUT_U8, regions) == br.everything_else(L, full(ON), OUT_U8, regions)


def test_invalid_input_names_its_index(L):
    err = lambda: L.ipk_last_error().decode()
    ds = [thumb()] + joiners()
    rc, route, first = plan(L, ds[:2] + [None] + ds[2:])
    assert rc == -2 and "index 2" in err() and route == [77] * 5 and first == [77] * 5, err()
    bad = [thumb()] + joiners()
    bad[3].fuse_scaledown = 5
    rc, route, first = plan(L, bad)
    assert rc == -2 and "descriptor 3" in err() and route == [77] * 4, err()
    bad = [thumb()] + joiners()
    bad[1].npoints = 65
    assert plan(L, bad)[0] == -2 and "descriptor 1" in err(), err()
    bad = [thumb()] + joiners()
    bad[2].struct_size = 0
    assert plan(L, bad)[0] == -2 and "descriptor 2" in err(), err()
