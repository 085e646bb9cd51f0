#!/usr/bin/env python3
"""Records which route the pipeline drivers choose for a matrix of descriptors (no GPU): tests/golden/routes/route_table.npz.

The recording pins the route decision across refactors of the driver: it is made from the commit BEFORE the change (build that commit's library and
point IPK_SO_OVERRIDE at it), and tests/test_route_table.py walks the same matrix on the library under test and asserts equality.

    IPK_SO_OVERRIDE=/path/to/parent/libimagepipe_amd.so python tools/make_route_table.py

For every descriptor and out type one row of int32 (COLUMNS): ipk_pipeline_takes_fastpath, the three ipk_pipeline_fuses_* reports,
ipk_pipeline_sizes (return code, demosaic and final size), and ipk_pipeline_region's return code and four outputs for the region (1, 2, 5, 3) and
for the whole result.  Outputs a call left untouched keep the sentinel -1.  A second, small table (`invalid`) holds the return codes of the
host-side reports for two invalid descriptors per source family: fuse_rotatecrop = 2 and npoints = 65."""
import ctypes as C
import itertools
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

OUT = os.path.join(ROOT, "tests", "golden", "routes", "route_table.npz")
COLUMNS = ["fastpath", "fuses_rotatecrop", "fuses_scaledown", "fuses_four_colour",
           "sizes_rc", "demosaic_w", "demosaic_h", "final_w", "final_h",
           "region_rc", "region_x", "region_y", "region_w", "region_h",
           "whole_rc", "whole_x", "whole_y", "whole_w", "whole_h"]
INVALID_COLUMNS = ["fastpath", "fuses_rotatecrop", "fuses_scaledown", "fuses_four_colour", "sizes_rc", "region_rc", "hashes_rc"]
REGION = (1, 2, 5, 3)

# the axes of the matrix, slowest first
FRAMES = [(47, 61, (0, 0, 0, 0)), (96, 120, (3, 1, 2, 5)), (131, 97, (0, 0, 0, 0)), (300, 20, (0, 0, 0, 0))]
XT = "GGRGGBGGBGGRBRGRBGGGBGGRGGRGGBRBGBRG"
# (name, cfa, src_type, cpp, is_cfa)
SOURCES = [("rggb-u16", "RGGB", 0, 1, 1), ("rggb-f32", "RGGB", 1, 1, 1), ("xtrans-u16", XT, 0, 1, 1), ("xtrans-f32", XT, 1, 1, 1),
           ("rgbe-u16", "RGBE", 0, 1, 1), ("rgbe-f32", "RGBE", 1, 1, 1), ("mono-u16", "", 0, 1, 0), ("cpp3-u16", "", 0, 3, 0),
           ("rgb8", "", 2, 3, 0), ("rgb16", "", 3, 3, 0)]
MAXWIDTHS = [0, 87, 20]
ALLOW_FUSED = [0, 1, 3, 5, 7]
FUSE_FLAGS = [(0, 0), (1, 0), (0, 1), (1, 1)]                             # fuse_rotatecrop, fuse_scaledown
ORIENTATIONS = [(0, 0), (1, 0), (2, 1)]                                   # rotation, fliph
OUT_TYPES = [0, 1]                                                        # f32, u8


def rotatecrops():
    """off, and three of the route tests' R9: crop-only ("crop-uneven"), an angle ("rot.2"), crops and an angle ("crop+rot.04")"""
    from test_rotatecrop_route import R9
    return [(0.0, 0.0, 0.0, 0.0, 0.0), R9[1], R9[3], R9[8]]


def inner_axes():
    """the axes below (frame, source), in the walk's order: (rotatecrop index, maxwidth, allow_fused, fuse_rotatecrop, fuse_scaledown, rotation, fliph)"""
    return [(k, mw, allow, frc, fsd, rot, fh) for k, mw, allow, (frc, fsd), (rot, fh)
            in itertools.product(range(len(rotatecrops())), MAXWIDTHS, ALLOW_FUSED, FUSE_FLAGS, ORIENTATIONS)]


def matrix_axes():
    """one tuple per row of `matrix`: (frame index, source index, *inner_axes(), out_type)"""
    return [(fi, si) + ax + (ot,) for fi, si in itertools.product(range(len(FRAMES)), range(len(SOURCES))) for ax in inner_axes() for ot in OUT_TYPES]


def _row(L, d, out_type, tmp):
    ref = C.byref(d)
    row = [L.ipk_pipeline_takes_fastpath(ref, out_type), L.ipk_pipeline_fuses_rotatecrop(ref, out_type),
           L.ipk_pipeline_fuses_scaledown(ref, out_type), L.ipk_pipeline_fuses_four_colour(ref, out_type)]
    s = tmp
    for v in s:
        v.value = 2 ** 64 - 1
    refs = [C.byref(v) for v in s]
    rc = L.ipk_pipeline_sizes(ref, *refs)
    sizes = [v.value for v in s]
    row += [rc] + [v if v != 2 ** 64 - 1 else -1 for v in sizes]
    regions = [REGION, (0, 0, sizes[2], sizes[3]) if rc == 0 else (0, 0, 0, 0)]
    for reg in regions:
        for v in s:
            v.value = 2 ** 64 - 1
        rc = L.ipk_pipeline_region(ref, out_type, *reg, *refs)
        row += [rc] + [v.value if v.value != 2 ** 64 - 1 else -1 for v in s]
    return row


def walk(L):
    """{"matrix": (rows, len(COLUMNS)) int32 in axis order, "fast": the fast-path descriptors' rows, "invalid": (rows, len(INVALID_COLUMNS))}"""
    from test_rotatecrop_route import _desc
    tmp = [C.c_size_t() for _ in range(4)]
    rows, invalid = [], []
    hashes = C.create_string_buffer(256)
    for (w, h, crops), (_, cfa, src_type, cpp, is_cfa) in itertools.product(FRAMES, SOURCES):
        d = _desc(w, h, cfa, crops, src_type=src_type, cpp=cpp, is_cfa=is_cfa, fuse=0)
        rcs = rotatecrops()
        for k, mw, allow, frc, fsd, rot, fh in inner_axes():
            d.rotatecrop[:] = rcs[k]
            d.maxwidth, d.allow_fused, d.fuse_rotatecrop, d.fuse_scaledown, d.rotation, d.fliph = mw, allow, frc, fsd, rot, fh
            for out_type in OUT_TYPES:
                rows.append(_row(L, d, out_type, tmp))
        # the two invalid descriptors of this family: which host-side calls refuse them
        for kw in (dict(fuse_rotatecrop=2), dict(npoints=65)):
            for out_type in OUT_TYPES:
                bad = _desc(w, h, cfa, crops, src_type=src_type, cpp=cpp, is_cfa=is_cfa, fuse=1, fuse_scaledown=1, allow_fused=7, **kw)
                r = _row(L, bad, out_type, tmp)
                invalid.append(r[:5] + [r[9], L.ipk_pipeline_hashes(C.byref(bad), out_type, 7, hashes)])
    # descriptors that really take the fast path: Pipeline::default_ops for a raster source with use_fastpath, and the same with one op field moved
    fast = []
    m = (C.c_float * 12)()
    L.ipk_const_matrix(2, m)
    for (w, h), src_type, mw, use, fliph in itertools.product([(47, 61), (96, 120), (300, 20), (5, 5)], (2, 3), MAXWIDTHS, (1, 0), (0, 1)):
        d = _desc(w, h, "", src_type=src_type, cpp=3, is_cfa=0, fuse=1, fuse_scaledown=1, maxwidth=mw, use_fastpath=use, fliph=fliph)
        d.blacklevels[:] = [0.0] * 4
        d.whitelevels[:] = [0.0] * 4
        d.cam_to_xyz_normalized[:] = m[:]
        d.wb_coeffs[:] = [1.0, 1.0, 1.0, 0.0]
        for out_type in (0, 1, 2):
            fast.append(_row(L, d, out_type, tmp))
    return {"matrix": np.array(rows, np.int32), "fast": np.array(fast, np.int32), "invalid": np.array(invalid, np.int32)}


def main():
    from imagepipe_amd import _lib
    tables = walk(_lib.load())
    np.savez_compressed(OUT, **tables)
    print("%s: %d bytes from %s; %s" % (OUT, os.path.getsize(OUT), _lib.SO_PATH, ", ".join("%s %r" % (k, v.shape) for k, v in tables.items())))


if __name__ == "__main__":
    main()
