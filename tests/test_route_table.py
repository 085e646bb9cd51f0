"""The route every descriptor takes, pinned against a recording (no GPU).  tests/golden/routes/route_table.npz was made by tools/make_route_table.py from
the library of the commit before the drivers' route decision moved into one function (choose_route, ipk_api.cpp); this test walks the same matrix
-- 57 600 descriptors x out types, the fast-path descriptors, two invalid descriptors per source family -- on the library under test and asserts
exact equality: the fast-path report, the three ipk_pipeline_fuses_* reports, the negotiated sizes, and ipk_pipeline_region's return code and
outputs for the region (1, 2, 5, 3) and for the whole result.

That every outcome occurs is a condition on the MATRIX, checked on the recording: each of the five routes, the fast path, the windowed region
kinds 0 / 1 / 2, and IPK_ERR_INVALID.  The host-side reports do not tell the raster route from the staged one (neither windows its regions), so
those two are named by construction: an uncropped RGB8 / RGB16 frame with no rotatecrop, no size limit and allow_fused set is the raster route's."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -2                                                              # IPK_ERR_INVALID


@pytest.fixture(scope="module")
def tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_route_table
    finally:
        sys.path.pop(0)
    return make_route_table


@pytest.fixture(scope="module")
def recorded(tool):
    with np.load(tool.OUT) as z:
        return {k: z[k] for k in z.files}


@pytest.fixture(scope="module")
def walked(tool):
    from imagepipe_amd import _lib
    return tool.walk(_lib.load())


def _first_difference(tool, name, want, got):
    bad = np.argwhere(want != got)
    r, c = bad[0]
    cols = tool.INVALID_COLUMNS if name == "invalid" else tool.COLUMNS
    where = tool.matrix_axes()[r] if name == "matrix" else r
    return "%s: %d of %d rows differ; first: row %r column %s recorded %d, got %d" % (
        name, len(set(bad[:, 0])), len(want), where, cols[c], want[r, c], got[r, c])


@pytest.mark.parametrize("name", ["matrix", "fast", "invalid"])
def test_routes_equal_the_recording(tool, recorded, walked, name):
    want, got = recorded[name], walked[name]
    assert want.shape == got.shape and want.dtype == got.dtype == np.int32
    assert np.array_equal(want, got), _first_difference(tool, name, want, got)


def test_every_outcome_occurs_in_the_matrix(tool, recorded):
    m, col = recorded["matrix"], {c: i for i, c in enumerate(tool.COLUMNS)}
    ax = np.array(tool.matrix_axes())
    assert len(m) == len(ax) == 4 * 10 * 4 * 3 * 5 * 4 * 3 * 2
    fi, si, rci, mw, allow = ax[:, 0], ax[:, 1], ax[:, 2], ax[:, 3], ax[:, 4]
    assert (m[:, col["sizes_rc"]] == 0).all() and (m[:, col["fastpath"]] == 0).all(), "the matrix holds valid descriptors off the fast path"
    rc, sd, four = (m[:, col[c]] == 1 for c in ("fuses_rotatecrop", "fuses_scaledown", "fuses_four_colour"))
    windowed = m[:, col["whole_rc"]] == 1
    outside = m[:, col["region_rc"]] == INVALID                           # (1, 2, 5, 3) does not fit every result: 300x20 under maxwidth 20 is 20x1
    empty = m[:, col["whole_rc"]] == INVALID                              # 300x20 cropped by its rotatecrop under maxwidth 20 negotiates 20x0: no region at all
    assert ((m[:, col["whole_rc"]] == 0) | windowed | empty).all() and ((m[:, col["region_rc"]] == m[:, col["whole_rc"]]) | outside).all()
    assert outside.any() and not outside.all() and empty.any() and (m[empty][:, col["final_h"]] == 0).all() and not (empty & (rc | sd | four)).any()
    raw = windowed & ~rc & ~sd                                            # only the raw route windows a region without one of the two reports
    raster_src = np.isin(si, [i for i, s in enumerate(tool.SOURCES) if s[2] in (2, 3)])
    raster = raster_src & (fi != 1) & (rci == 0) & (mw == 0) & (allow != 0)
    staged = ~raw & ~rc & ~sd & ~raster & ~empty
    counts = {"raw": int(raw.sum()), "raw, four colours": int((raw & four).sum()), "resample": int(rc.sum()), "scaledown": int(sd.sum()),
              "raster": int(raster.sum()), "staged": int(staged.sum()), "windowed kind 0": int(raw.sum()), "windowed kind 1": int((windowed & rc).sum()),
              "windowed kind 2": int((windowed & sd).sum()), "resample, not windowed": int((~windowed & rc).sum()),
              "scaledown, not windowed": int((~windowed & sd).sum()), "empty result (IPK_ERR_INVALID)": int(empty.sum()),
              "region outside the result (IPK_ERR_INVALID)": int((outside & ~empty).sum())}
    print(counts)
    assert all(v > 0 for v in counts.values()), counts
    assert not (raster & (windowed | rc | sd | four)).any() and not (four & ~raw).any() and not (rc & sd).any()
    assert counts["raw"] + counts["resample"] + counts["scaledown"] + counts["raster"] + counts["staged"] + int(empty.sum()) == len(m)
    # the fast path, and IPK_ERR_INVALID
    f = recorded["fast"]
    assert (f[:, col["fastpath"]] == 1).any() and (f[:, col["fastpath"]] == 0).any()
    assert ((f[:, col["fastpath"]] == 1) & (f[:, col["sizes_rc"]] == INVALID)).any(), "a fast-path frame the negotiation refuses (5x5)"
    inv, icol = recorded["invalid"], {c: i for i, c in enumerate(tool.INVALID_COLUMNS)}
    assert (inv[:, icol["fuses_rotatecrop"]] == INVALID).any() and (inv[:, icol["region_rc"]] == INVALID).all() and (inv[:, icol["hashes_rc"]] == INVALID).all()
    assert (inv[:, icol["fuses_rotatecrop"]] != INVALID).any(), "the reports leave npoints to the launch"
