"""The nine route switches crossed (no GPU): the seven opt-in bits of ipk_pipeline_desc.allow_fused beside IPK_FUSED_ON and the flags fuse_rotatecrop
and fuse_scaledown, every combination of them -- 1024 settings -- over 70 descriptors (ten sources x seven geometries).  include/imagepipe_amd.h gives
every switch the same contract: it changes no result and enters no hash.  Here: no setting moves a size, a hash or the fast-path report; every region
plan stays inside the frame; every report reads only the switches the header names for it (DEPENDS, written down from the header's text); a mask
without IPK_FUSED_ON means what the header says it means (canonical); and every switch does move some report on some case, so the matrix is not
vacuous.  tests/test_gpu_switch_matrix.py runs the same cases and settings on the GPU and takes the cases, the settings and S260 from here."""
import ctypes as C

import numpy as np
import pytest

import util
import test_gpu_staged_paths as sp
import test_scaledown_route as sr

W, H = 131, 113                                                           # tests/test_gpu_plain_previews.py's frame
ON, FOUR, REGIONS, PREVIEWS, PLAIN, CACHED, SCALED_RC, PLAIN_PREVIEWS = 1, 2, 4, 8, 16, 32, 64, 128
# a setting is (allow_fused, fuse_rotatecrop, fuse_scaledown), indexed allow_fused | fuse_rotatecrop << 8 | fuse_scaledown << 9
FRC, FSD = 1 << 8, 1 << 9
N_SETTINGS = 1024
SWITCHES = {"FOUR_COLOUR": FOUR, "WINDOW_REGIONS": REGIONS, "WINDOW_PREVIEWS": PREVIEWS, "PLAIN": PLAIN, "CACHED_RESAMPLE": CACHED,
            "SCALED_ROTATECROP": SCALED_RC, "PLAIN_PREVIEWS": PLAIN_PREVIEWS, "fuse_rotatecrop": FRC, "fuse_scaledown": FSD}
ALL_ON = ON | sum(SWITCHES.values())
SOURCES = list(sp.SOURCES) + ["rgb8", "rgb16"]
RASTERS = ("rgb8", "rgb16")
RASTER_EXPOSURE = 0.25                                                    # not the default ops: no fast path; and not the 0.5 of the GPU module's exposure edit
# name -> (sensor crops, rotatecrop, _place_scale's branch)
ANGLE = lambda a: (0.0, 0.0, 0.0, 0.0, a)
GEOMETRIES = [("G0", "zero", None, "le1"), ("G1", "crop", sp.ROTATECROPS["crop"], "le1"), ("G2", "zero", ANGLE(0.03), "le1"),
              ("G3", "zero", None, "mid"), ("G4", "zero", None, "ge"), ("G5", "zero", ANGLE(0.03), "mid"), ("G6", "crop", ANGLE(0.3), "ge")]
CASES = [(i, j) for i in range(len(SOURCES)) for j in range(len(GEOMETRIES))]
CASE_IDS = ["%s-%s" % (SOURCES[i], GEOMETRIES[j][0]) for i, j in CASES]


def setting(s):
    return s & 255, (s >> 8) & 1, (s >> 9) & 1


def _popcount(v):
    return bin(v).count("1")


# at most three of the nine switches on beside bit 0, or at most three off: every pair and triple, both ways
S260 = [s for s in range(N_SETTINGS) if s & ON and (_popcount(s & ~ON) <= 3 or _popcount(s & ~ON) >= 6)]
assert len(S260) == 260 and ALL_ON in S260 and ON in S260


def out_type_of(i, j):
    return (i + j) % 3


def source_fields(name):
    """the RawImage fields of sp._source, or a raster's: (cfa, cpp, is_float)"""
    if name in RASTERS:
        return "", 3, False
    _, src = sp._source(name, 12, 12, 1)
    return src["cfa"], src["cpp"], src["is_float"]


_OPS = {}


def case_ops(orc, i, j):
    """(sensor crops, ops) of case (source i, geometry j): the rotatecrop, the orientation of the odd-numbered geometries and the maxwidth that
    sp._place_scale finds for the branch.  The negotiation reads the frame's shape and the filter's width alone, so zeros stand in for the samples."""
    cfa = source_fields(SOURCES[i])[0]
    key = (sp._minscale(cfa), j)
    if key not in _OPS:
        _, crops, rc, branch = GEOMETRIES[j]
        ops = {}
        if rc is not None:
            ops["rotatecrop"] = tuple(float(np.float32(v)) for v in rc)
        if j % 2:
            ops.update(sp.ORIENTS["rotflip"])
        src = dict(cfa=cfa, cpp=1, is_float=False, blacklevels=[util.BLACK] * 4, whitelevels=[util.WHITE] * 4)
        sp._place_scale(orc, np.zeros((H, W), np.uint16), src, sp.CROPS[crops], ops, branch)
        _OPS[key] = (sp.CROPS[crops], ops)
    crops, ops = _OPS[key]
    return crops, dict(ops)


def regions_of(fw, fh):
    """the two regions of a fw x fh result: an interior one with x % 4 != 0 and fewer than 256 pixels, and one of at least 256 pixels that ends on
    the result's last row and column"""
    small = (5, 3, min(13, fw - 7), min(9, fh - 5))
    bw = min(fw, 20)
    bh = -(-256 // bw)
    big = (fw - bw, fh - bh, bw, bh)
    assert small[2] >= 1 and small[3] >= 1 and small[2] * small[3] < 256 and small[0] % 4 and small[0] + small[2] < fw and small[1] + small[3] < fh, (fw, fh)
    assert bh <= fh and bw * bh >= 256, (fw, fh)
    return small, big


@pytest.fixture(scope="module")
def L():
    from imagepipe_amd import _lib
    return _lib.load()


def build_desc(orc, i, j):
    """the descriptor of a case as the *_route.py tests build theirs (sr._desc), every switch off"""
    name = SOURCES[i]
    cfa, cpp, is_float = source_fields(name)
    crops, ops = case_ops(orc, i, j)
    kw = dict(maxwidth=ops.get("maxwidth", 0), rotation=ops.get("rotation", 0), fliph=int(ops.get("fliph", False)))
    if "rotatecrop" in ops:
        kw["rotatecrop"] = list(ops["rotatecrop"])
    if name in RASTERS:
        d = sr._desc(W, H, "", crops, src_type=2 if name == "rgb8" else 3, cpp=3, is_cfa=0, fuse=0, exposure=RASTER_EXPOSURE, **kw)
    else:
        shifted = orc.cfa_shift(cfa, crops[3], crops[0]) if cfa else ""
        d = sr._desc(W, H, shifted, crops, src_type=int(is_float), cpp=cpp, is_cfa=int(bool(cfa)), fuse=0, **kw)
    d.allow_fused = 0
    return d


def apply_setting(d, s):
    d.allow_fused, d.fuse_rotatecrop, d.fuse_scaledown = setting(s)
    return d


# ---------------------------------------------------------------------------------------------
# the walk: every report of every case under every setting, once
# ---------------------------------------------------------------------------------------------
REPORTS = ["fuses_rotatecrop", "fuses_scaledown", "fuses_four_colour", "windows_preview", "fuses_plain", "scales_plain", "fuses_scaled_rotatecrop",
           "resamples_cached_region"]
COLUMNS = ["fastpath"] + REPORTS + [r + k for r in ("small_", "big_") for k in ("kind", "x", "y", "w", "h")] + ["sizes_same", "hashes_same"]
COL = {c: k for k, c in enumerate(COLUMNS)}
PLAN = [COL[r + k] for r in ("small_", "big_") for k in ("kind", "x", "y", "w", "h")]


def _region(L, d, out_type, reg):
    s = [C.c_size_t(0) for _ in range(4)]
    rc = L.ipk_pipeline_region(C.byref(d), out_type, *reg, *[C.byref(v) for v in s])
    return [rc] + [v.value for v in s]


def _sizes(L, d):
    a = [C.c_size_t() for _ in range(4)]
    rc = L.ipk_pipeline_sizes(C.byref(d), *[C.byref(v) for v in a])
    return (rc,) + tuple(v.value for v in a)


def _hashes(L, d):
    out = []
    for out_type in (0, 1, 2):
        buf = C.create_string_buffer(256)
        out.append((L.ipk_pipeline_hashes(C.byref(d), out_type, 5, buf), buf.raw))
    return out


@pytest.fixture(scope="module")
def walked(L, orc):
    """T[case, setting, column] (int64), and per case the regions, the result's size and the frame's crop window"""
    T = np.zeros((len(CASES), N_SETTINGS, len(COLUMNS)), np.int64)
    info = []
    for c, (i, j) in enumerate(CASES):
        d = build_desc(orc, i, j)
        out_type = out_type_of(i, j)
        sizes0, hashes0 = _sizes(L, d), _hashes(L, d)
        assert sizes0[0] == 0 and all(rc == 0 and raw != bytes(256) for rc, raw in hashes0), CASE_IDS[c]
        regs = regions_of(sizes0[3], sizes0[4])
        info.append(dict(regions=regs, sizes=sizes0[1:]))
        for s in range(N_SETTINGS):
            apply_setting(d, s)
            row = [L.ipk_pipeline_takes_fastpath(C.byref(d), out_type)]
            row += [getattr(L, "ipk_pipeline_" + r)(C.byref(d), out_type) for r in REPORTS]
            for reg in regs:
                row += _region(L, d, out_type, reg)
            row += [int(_sizes(L, d) == sizes0), int(_hashes(L, d) == hashes0)]
            T[c, s] = row
    return T, info


def _where(T_bad):
    c, s = np.argwhere(T_bad)[0][:2]
    return "%s under allow_fused=%d fuse_rotatecrop=%d fuse_scaledown=%d" % ((CASE_IDS[c],) + setting(int(s)))


def test_no_setting_moves_a_size_a_hash_or_the_fast_path(walked):
    T, _ = walked
    for col in ("sizes_same", "hashes_same"):
        bad = T[:, :, COL[col]] != 1
        assert not bad.any(), "%s: %s" % (col, _where(bad))
    bad = T[:, :, COL["fastpath"]] != T[:, :1, COL["fastpath"]]
    assert not bad.any(), "fast path: " + _where(bad)
    bad = (T[:, :, 1:1 + len(REPORTS)] < 0) | (T[:, :, 1:1 + len(REPORTS)] > 1)
    assert not bad.any(), "a report outside {0, 1}: " + _where(bad.any(axis=2))


def test_region_plans(walked):
    """0 or 1, or the error of (0, 0, 0); the sensor window inside the frame; where the plan is `whole frame`, the window (0, 0, 0) reports"""
    T, _ = walked
    for r in ("small_", "big_"):
        kind = T[:, :, COL[r + "kind"]]
        kind0 = T[:, :1, COL[r + "kind"]]
        assert (kind0 == 0).all(), "with every switch off a region is cut from the whole result"
        bad = (kind != 0) & (kind != 1)
        assert not bad.any(), r + "region: " + _where(bad)
        x, y, w, h = (T[:, :, COL[r + k]] for k in "xywh")
        bad = (x + w > W) | (y + h > H)
        assert not bad.any(), r + "region, a window that leaves the frame: " + _where(bad)
        win = T[:, :, COL[r + "x"]: COL[r + "h"] + 1]
        bad = (kind == 0)[:, :, None] & (win != T[:, :1, COL[r + "x"]: COL[r + "h"] + 1])
        assert not bad.any(), r + "region, a whole-frame plan with another window than (0, 0, 0)'s: " + _where(bad.any(axis=2))


# Which switches a report may read, from the text of include/imagepipe_amd.h beside IPK_FUSED_ON (the declaration of each report and the field comment
# of allow_fused):
#   ipk_pipeline_fuses_rotatecrop         "1 when d->fuse_rotatecrop and d->allow_fused are set ..."
#   ipk_pipeline_fuses_scaledown          "1 when d->fuse_scaledown and d->allow_fused are set ..."
#   ipk_pipeline_fuses_four_colour        "1 when d->allow_fused has IPK_FUSED_FOUR_COLOUR set ..."
#   ipk_pipeline_windows_preview          "... IPK_FUSED_ON and IPK_FUSED_WINDOW_PREVIEWS set ... or -- with IPK_FUSED_PLAIN_PREVIEWS set as well -- ..."
#   ipk_pipeline_fuses_plain              "... IPK_FUSED_ON and IPK_FUSED_PLAIN set ..."
#   ipk_pipeline_scales_plain             "... IPK_FUSED_ON and IPK_FUSED_PLAIN_PREVIEWS set ..."
#   ipk_pipeline_fuses_scaled_rotatecrop  "... IPK_FUSED_ON and IPK_FUSED_SCALED_ROTATECROP set ... or -- with IPK_FUSED_PLAIN_PREVIEWS set as well -- ..."
#   ipk_pipeline_resamples_cached_region  "... IPK_FUSED_ON and IPK_FUSED_CACHED_RESAMPLE set ..."
#   ipk_pipeline_takes_fastpath           no switch at all
#   ipk_pipeline_region                   bit 1 ("with it: windowed"), bit 2 with either flag ("are windowed too"), bits 3, 4 and 6 (with bit 7 for the
#                                         monochrome and three-sample raws); bit 5: "no hash, no result, no region report"
DEPENDS = {
    "fastpath": (),
    "fuses_rotatecrop": ("fuse_rotatecrop",),
    "fuses_scaledown": ("fuse_scaledown",),
    "fuses_four_colour": ("FOUR_COLOUR",),
    "windows_preview": ("WINDOW_PREVIEWS", "PLAIN_PREVIEWS"),
    "fuses_plain": ("PLAIN",),
    "scales_plain": ("PLAIN_PREVIEWS",),
    "fuses_scaled_rotatecrop": ("SCALED_ROTATECROP", "PLAIN_PREVIEWS"),
    "resamples_cached_region": ("CACHED_RESAMPLE",),
    "region": ("FOUR_COLOUR", "WINDOW_REGIONS", "WINDOW_PREVIEWS", "PLAIN", "SCALED_ROTATECROP", "PLAIN_PREVIEWS", "fuse_rotatecrop", "fuse_scaledown"),
}
# The table holds beside IPK_FUSED_ON only, so the switches are flipped in the 512 settings that have it: without bit 0 any other non-zero bit (5 and 6
# aside) turns the routes on, and every report then "reads" it.  The 512 settings without bit 0 are not left out: test_masks_without_bit_0_mean_what_
# the_header_says pins each of them, report for report, to a setting with bit 0 (or to 0), and that setting is covered here.
WITH_ON = np.array([s for s in range(N_SETTINGS) if s & ON])


def _columns_of(report):
    return PLAN if report == "region" else [COL[report]]


def test_a_report_reads_only_the_switches_the_header_names(walked):
    T, _ = walked
    assert set(DEPENDS) == {"fastpath", "region"} | set(REPORTS)
    for report, may in DEPENDS.items():
        cols = _columns_of(report)
        for name, bit in SWITCHES.items():
            if name in may:
                continue
            bad = (T[:, WITH_ON][:, :, cols] != T[:, WITH_ON ^ bit][:, :, cols]).any(axis=2)
            if bad.any():
                c, k = np.argwhere(bad)[0]
                raise AssertionError("%s changes with %s: %s under allow_fused=%d fuse_rotatecrop=%d fuse_scaledown=%d" % (
                    (report, name, CASE_IDS[c]) + setting(int(WITH_ON[k]))))


def canonical(s):
    """what a mask without IPK_FUSED_ON means, from the field comment of allow_fused: bits 5 and 6 are nothing without bit 0 ("allow_fused = 32 is 0 to
    every route and report", "allow_fused = 64 is 0 ..."), alone or together; bits 3, 4 and 7 act "only together with bit 0" and alone "still mean on"
    (any non-zero value does); bits 1 and 2 count without bit 0 and, being non-zero, switch the routes on as well.  The two flags are not part of the mask."""
    allow, flags = s & 255, s & (FRC | FSD)
    if allow & ON:
        return s
    allow &= ~(CACHED | SCALED_RC)
    return flags | ((ON | (allow & (FOUR | REGIONS))) if allow else 0)


def test_the_mapping_is_the_header_table():
    assert [canonical(b) for b in (FOUR, REGIONS)] == [ON | FOUR, ON | REGIONS]
    assert [canonical(b) for b in (PREVIEWS, PLAIN, PLAIN_PREVIEWS)] == [ON] * 3
    assert [canonical(b) for b in (CACHED, SCALED_RC, CACHED | SCALED_RC)] == [0] * 3
    assert canonical(CACHED | FRC) == FRC and canonical(PLAIN | FSD) == ON | FSD and canonical(ON | CACHED) == ON | CACHED


def test_masks_without_bit_0_mean_what_the_header_says(walked):
    T, _ = walked
    off = np.array([s for s in range(N_SETTINGS) if not s & ON])
    canon = np.array([canonical(int(s)) for s in off])
    cols = [COL["fastpath"]] + [COL[r] for r in REPORTS] + PLAN
    bad = (T[:, off][:, :, cols] != T[:, canon][:, :, cols])
    if bad.any():
        c, k, col = np.argwhere(bad)[0]
        raise AssertionError("%s: column %s under allow_fused=%d fuse_rotatecrop=%d fuse_scaledown=%d is %d, under the mask it stands for (%d) %d" % (
            CASE_IDS[c], COLUMNS[cols[col]], *setting(int(off[k])), T[c, off[k], cols[col]], canon[k] & 255, T[c, canon[k], cols[col]]))


# Cases no switch reaches, with the header line that says why.  None: every source and every geometry is moved by some switch.
UNREACHED_SOURCES = {}
UNREACHED_GEOMETRIES = {}


def test_every_switch_moves_something_and_every_case_is_moved(walked):
    """a condition on the CASES, not a measurement of the library: a switch that changes no report and no plan anywhere is not exercised by this matrix"""
    T, _ = walked
    cols = [COL[r] for r in REPORTS] + PLAN
    moved_sources, moved_geometries = set(), set()
    for name, bit in SWITCHES.items():
        moved = (T[:, WITH_ON][:, :, cols] != T[:, WITH_ON ^ bit][:, :, cols]).any(axis=(1, 2))
        assert moved.any(), "%s changes no report and no region plan on any case" % name
        for c in np.flatnonzero(moved):
            moved_sources.add(SOURCES[CASES[c][0]])
            moved_geometries.add(GEOMETRIES[CASES[c][1]][0])
        # ... and with every other switch set: the setting an integrator ends on
        assert (T[:, ALL_ON][:, cols] != T[:, ALL_ON ^ bit][:, cols]).any(), "%s changes nothing beside all the others" % name
    assert set(SOURCES) - moved_sources == set(UNREACHED_SOURCES), (sorted(moved_sources), UNREACHED_SOURCES)
    assert {g[0] for g in GEOMETRIES} - moved_geometries == set(UNREACHED_GEOMETRIES), (sorted(moved_geometries), UNREACHED_GEOMETRIES)


def test_the_geometries_are_what_they_claim(L, orc):
    """the demosaic branch each geometry names, from the oracle's negotiation; every source and every geometry meets the three output types"""
    for i, j in CASES:
        crops, ops = case_ops(orc, i, j)
        cfa = source_fields(SOURCES[i])[0]
        d = build_desc(orc, i, j)
        rc, dw, dh, fw, fh = _sizes(L, d)
        _, _, cw, ch = orc.size_image(*crops, W, H)
        scale = orc.calculate_scaling_total(cw, ch, dw, dh)[0]
        branch = GEOMETRIES[j][3]
        ms = sp._minscale(cfa)
        assert {"le1": scale <= 1.0, "mid": 1.0 < scale < ms, "ge": scale >= ms}[branch], (CASE_IDS[CASES.index((i, j))], scale)
    for i in range(len(SOURCES)):
        assert {out_type_of(i, j) for j in range(len(GEOMETRIES))} == {0, 1, 2}
    for j in range(len(GEOMETRIES)):
        assert {out_type_of(i, j) for i in range(len(SOURCES))} == {0, 1, 2}
