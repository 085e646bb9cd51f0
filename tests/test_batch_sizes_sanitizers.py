"""The plan and the chunk report of ipk_pipeline_run_batch_each under IPK_FUSED_BATCH_SIZES, under AddressSanitizer + UBSan (no GPU):
tests/cpp/batch_sizes_plan.cpp -- alternating orientations and sensor sizes with the masks of bits 0, 8, 9, 10 and 11, then seeded hostile batches whose
previews' byte counts wrap or cross the 256 MiB cut -- built by the stand-alone programs' pattern rules in tests/cpp/Makefile (asked for by name, behind
`make san`), run sanitized and plain: no report, the documented number of cases, equal digests.  Nothing sanitized is loaded into python; the harness is
tests/test_host_sanitizers.py's."""
import os
import subprocess

import pytest

from test_host_sanitizers import CPP, built, _run, _sections, _check      # noqa: F401  (built: the module fixture that runs `make san`)

HOSTILE = 20000
CONTRACT = 8 * 3 * 6 * 3                                                   # masks x output types x batch sizes x kinds of alternation


@pytest.fixture(scope="module")
def plans(built):
    exe = lambda flavour: os.path.join(CPP, "build", "san", flavour, "batch_sizes_plan")
    r = subprocess.run(["make", "-C", CPP, "-j4"] + [os.path.join("build", "san", f, "batch_sizes_plan") for f in ("plain", "asan")], capture_output=True,
                       text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return {f: _sections(_run(exe(f), HOSTILE)) for f in ("plain", "asan")}


def test_batch_sizes_plan_under_asan_and_ubsan(plans):
    _check(plans["asan"], plans["plain"], {"sizes_contract": CONTRACT, "sizes_hostile": HOSTILE}, "batch_sizes_plan")
