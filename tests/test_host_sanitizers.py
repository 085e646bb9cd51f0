"""The host-side code and the CPU oracle under sanitizers (no GPU, nothing sanitized is loaded into python).

`make san` (tests/cpp/Makefile, oracle/Makefile) builds stand-alone programs, each with its own main, three times: with AddressSanitizer + UBSan,
with ThreadSanitizer (the threaded ones) and plain at the shipped flags.  The sanitizer runtimes are linked statically, so the programs do not
care what a machine preloads, and this file leaves the environment exactly as it finds it.  For every program it asserts: exit status 0; no
sanitizer report on stdout or stderr; every SECTION line present with the case count computed HERE, from the axes restated in this file (a
section that silently did nothing fails); every digest equal to the plain twin's (the instrumented build computes what the shipped flags
compute).  The route-grid digests are also recomputed from tests/golden/routes/route_table.npz, which ties the C++ restatement of the grid to
the committed recording.  Leak detection stays on; no suppressions are needed (the programs never initialise the HIP runtime).

The oracle has no ThreadSanitizer flavour: libgomp is not instrumented and its barriers would be reported as races.  Its OpenMP loops are
checked by running the program with 1 and with 4 threads: all digests must agree."""
import os
import re
import subprocess
import sys
import tempfile

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")
ORACLE = os.path.join(ROOT, "oracle")
PIN = os.path.join(ROOT, "tests", "golden", "pin")
CLANGXX = "/opt/rocm/llvm/bin/clang++"
REPORTS = ("AddressSanitizer", "LeakSanitizer", "ThreadSanitizer", "runtime error:")
HOSTILE = 200000                                                          # descriptors, and argument sets
THREADS, ITERS = 8, 400


def _links(compiler, flags, suffix):
    """does a one-line program link with these sanitizer flags (is the runtime on this machine)?"""
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "probe" + suffix)
        with open(src, "w") as f:
            f.write("int main(){}\n")
        try:
            r = subprocess.run([compiler] + flags + ["-o", os.path.join(d, "probe"), src], capture_output=True, text=True, timeout=120)
        except OSError as e:
            return str(e)
        return None if r.returncode == 0 else (r.stderr.strip().splitlines() or ["exit %d" % r.returncode])[-1]


@pytest.fixture(scope="module")
def built():
    for compiler, flags, suffix in ((CLANGXX, ["-fsanitize=address,undefined"], ".cpp"), (CLANGXX, ["-fsanitize=thread"], ".cpp"),
                                    ("gcc", ["-fsanitize=address,undefined", "-static-libasan", "-static-libubsan"], ".c")):
        why = _links(compiler, flags, suffix)
        if why is not None:
            pytest.skip("no sanitizer runtime on this machine: `%s %s` does not link an empty main: %s" % (compiler, " ".join(flags), why))
    for where in (CPP, ORACLE):
        r = subprocess.run(["make", "-C", where, "-j8", "san"], capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return True


def _run(exe, *args, limit=120, env=None):
    r = subprocess.run(["timeout", "-k", "10", str(limit), exe] + [str(a) for a in args], capture_output=True, text=True, env=env)
    out = r.stdout + r.stderr
    assert r.returncode == 0, "%s exited with %d:\n%s" % (exe, r.returncode, out[-6000:])
    for word in REPORTS:
        assert word not in out, "%s reports %s:\n%s" % (exe, word, out[-6000:])
    return r.stdout


def _sections(stdout):
    found = re.findall(r"^SECTION (\S+) cases=(\d+) digest=([0-9a-f]{16})$", stdout, re.M)
    assert len({n for n, _, _ in found}) == len(found), "a section is printed twice"
    return {n: (int(c), d) for n, c, d in found}


def _check(sections, twin, expected, what):
    assert set(sections) == set(expected), "%s: sections %r, expected %r" % (what, sorted(sections), sorted(expected))
    for name, count in expected.items():
        assert sections[name][0] == count, "%s: section %s ran %d cases, expected %d" % (what, name, sections[name][0], count)
        assert sections[name][1] == twin[name][1], "%s: section %s has digest %s, its plain twin %s" % (what, name, sections[name][1], twin[name][1])
        assert twin[name][0] == count


def fnv1a64(data):
    h = 0xcbf29ce484222325
    for b in bytes(data):
        h = ((h ^ b) * 0x100000001b3) & 0xFFFFFFFFFFFFFFFF
    return "%016x" % h


# ---------------------------------------------------------------------------------------------------------------------------------
# the case counts, from the axes as this file states them
# ---------------------------------------------------------------------------------------------------------------------------------
def _tool():
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import make_route_table
    finally:
        sys.path.pop(0)
    return make_route_table


def _surface_counts():
    tool = _tool()
    divisors = [d for d in range(1, 49) if 48 % d == 0]
    assert len(divisors) == 10
    # 4, 36 and 144 letters (five 2x2 filters, X-Trans, the 12x12), the empty pattern, every "WxH:" with W, H dividing 48, three stated shapes that are also
    # inferable ones, three with leading zeros; each shifted by 0..47 in both axes and by eight negative / extreme pairs
    patterns = 5 + 1 + 1 + 1 + len(divisors) ** 2 + 3 + 3
    refused = ["RGXB", "RGGBGRBGGBRGBGGR", "5x2:RGBGRGBGRG", "2x8:RGGB", "x8:RGGBGRBGGBRGBGGR", "2x:RGGB", "2x8RGGB", "0x4:", "2x8:RGBGRBGGGBGRGRBX", "R", "2x2:",
               ":", "002x2:RGGB", "2x2:RGGB:", "96x1:R"]
    from test_rotatecrop_route import R9
    windows = 8                                                           # test_region_windows_route._windows_of
    taken = 2 * len(R9) + 2                                               # test_region_windows_route.TAKEN
    return {
        "cfa_shift": patterns * (48 * 48 + 8),
        "cfa_shift_refused": len(refused),
        "spline_new": 65 * 3,                                             # 0..64 points, three kinds of curve
        "tables": 5 + 5,                                                  # ipk_lut_table -1..3, ipk_const_matrix 0..4
        "route_grid": len(tool.matrix_axes()),
        "route_hashes": len(tool.matrix_axes()),
        "route_invalid": len(tool.FRAMES) * len(tool.SOURCES) * 2 * len(tool.OUT_TYPES),
        "route_fast": 4 * 2 * len(tool.MAXWIDTHS) * 2 * 2 * 3,
        "window_footprint": (4 + 3) * windows + 6 + 2,                    # four fixed transforms, three scaled forms; the refusals of test_footprint_refusals
        "regions": taken * 4 * 2 * windows,                               # four (filter, source type, out type) forms, with and without the bit
        "band_plan": 64 * 3 * 11,                                         # ranks 1..64, periods 2 / 6 / 12, eleven heights from 1 row
        "band_plan_scaled": 64 * 6,
        "deal_frames": 6 * sum(range(1, 9)) + 3,
        "cache": 1 + 40 + 40 + 1 + 2 + 1 + 1 + 5 + 1 + (1 + 2 + 1 + 1),
        "hostile_desc": HOSTILE,
        "hostile_args": HOSTILE,
    }


def _oracle_counts():
    pinned = [ln for ln in open(os.path.join(PIN, "cases.txt")) if ln.strip() and not ln.startswith("#")]
    for ln in pinned:
        name, _, w, h = ln.split()[:4]
        assert os.path.getsize(os.path.join(PIN, name + ".raw.u16")) == 2 * int(w) * int(h)
    return {
        "misc": 4 + 3 + 10 * (5 + 1) + 7 * 7 + 8,
        "demosaic": len(pinned) + 4 * 8,                                  # the pinned frames; four odd sizes down to 10x10, eight filters
        "transform": 4 * 3 * 3 + 3,                                       # corner sets x components x element types; the three scale_down forms
        "gofloat": 8 * 2,
        "pointwise": 3 + 4 + 2 + 1 + 1 + 2 + 1 + 3 + 3 + 12,
        "spline": 65 * 2,
        "rotatecrop": 17 * 3 * 2 + 17 + 2 + 9,
        "pipeline": 4 * 2 + 1,
    }


# ---------------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def surface(built):
    exe = lambda flavour: os.path.join(CPP, "build", "san", flavour, "host_surface")
    return {f: _sections(_run(exe(f), HOSTILE, HOSTILE)) for f in ("plain", "asan")}


def test_host_surface_under_asan_and_ubsan(surface):
    """include/imagepipe_amd.h without a GPU: exact-size buffers on valid inputs, then 200 000 hostile descriptors and 200 000 hostile argument sets"""
    _check(surface["asan"], surface["plain"], _surface_counts(), "host_surface")


@pytest.mark.parametrize("section,table,columns", [("route_grid", "matrix", 19), ("route_fast", "fast", 19), ("route_invalid", "invalid", 7)])
def test_route_sections_equal_the_recording(surface, section, table, columns):
    """the C++ restatement of tools/make_route_table.py's grid produces the committed recording, row for row: same FNV-1a fold over the int32 rows"""
    with np.load(_tool().OUT) as z:
        rows = z[table]
    assert rows.dtype == np.int32 and rows.shape[1] == columns
    want = fnv1a64(rows.astype("<i4").tobytes())
    for flavour in ("asan", "plain"):
        assert surface[flavour][section] == (len(rows), want), (flavour, section)


@pytest.mark.parametrize("flavour", ["asan", "tsan"])
def test_host_threads(built, flavour):
    """eight threads on the reports, ipk_cfa_shift, the thread-local error text, the context calls' failure paths and one shared cache"""
    exe = lambda f: os.path.join(CPP, "build", "san", f, "host_threads")
    expected = {"threads_reports": THREADS * ITERS, "threads_errors": THREADS * ITERS, "threads_cache": THREADS * ITERS}
    _check(_sections(_run(exe(flavour), ITERS)), _sections(_run(exe("plain"), ITERS)), expected, "host_threads/" + flavour)


@pytest.mark.parametrize("flavour", ["asan", "tsan"])
def test_comm_test_host_transport(built, flavour):
    """tests/cpp/comm_test.cpp in host mode (ranks are threads, a mailbox moves the bytes): test_cabi_host's shapes and one with fewer rows than ranks"""
    exe = os.path.join(CPP, "build", "san", flavour, "comm_test")
    for nranks in (2, 3, 4, 8):
        for w, h in ((64, 37), (300, 50), (300, 12), (64, 5)):
            out = _run(exe, nranks, w, h)
            assert "COMM_OK nranks=%d %dx%d host" % (nranks, w, h) in out, out


def test_oracle_surface(built):
    """every ORC_API function under ASan + UBSan with float-cast-overflow; 1 and 4 OpenMP threads, sanitized and plain: one digest per section"""
    expected = _oracle_counts()
    runs = {}
    for flavour in ("plain", "asan"):
        for threads in (1, 4):
            env = dict(os.environ, OMP_NUM_THREADS=str(threads))
            runs[flavour, threads] = _sections(_run(os.path.join(ORACLE, "build", "san", flavour, "oracle_surface"), PIN, env=env))
    for key, got in runs.items():
        _check(got, runs["plain", 1], expected, "oracle_surface/%s/%d threads" % key)
