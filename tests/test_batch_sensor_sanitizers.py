"""The plan of ipk_pipeline_run_batch_each under AddressSanitizer + UBSan (no GPU): tests/cpp/batch_plan.cpp -- batches whose frames differ in the sensor
fields IPK_FUSED_BATCH_SENSOR lets vary, with every mask of bits 0, 8, 9 and 10, through exact-size heap descriptors and outputs, then seeded hostile
batches -- built by the stand-alone programs' pattern rules in tests/cpp/Makefile (asked for by name, behind `make san`), run sanitized and plain: no report, the documented number of cases, equal digests -- and the plain build's equal to
tests/golden/batch_plan_digests.txt, the plan as recorded.  Nothing sanitized is loaded into python; the harness is tests/test_host_sanitizers.py's."""
import os
import subprocess

import pytest

from test_host_sanitizers import CPP, built, _run, _sections, _check      # noqa: F401  (built: the module fixture that runs `make san`)

HOSTILE = 20000
CONTRACT = 7 * 3 * 6 * 3                                                   # masks x output types x batch sizes x strides through the variations


@pytest.fixture(scope="module")
def plans(built):
    # the Makefile's pattern rules for the stand-alone programs build any tests/cpp/<name>.cpp on request: the program is asked for by name
    exe = lambda flavour: os.path.join(CPP, "build", "san", flavour, "batch_plan")
    r = subprocess.run(["make", "-C", CPP, "-j4"] + [os.path.join("build", "san", f, "batch_plan") for f in ("plain", "asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return {f: _sections(_run(exe(f), HOSTILE)) for f in ("plain", "asan")}


def test_batch_plan_under_asan_and_ubsan(plans):
    _check(plans["asan"], plans["plain"], {"plan_contract": CONTRACT, "plan_hostile": HOSTILE}, "batch_plan")


def test_the_plan_is_the_recorded_one(plans):
    """status, route and run_first of every case, as the plain build printed them before the plan became one record per descriptor and a list of runs"""
    recorded = _sections(open(os.path.join(os.path.dirname(CPP), "golden", "batch_plan_digests.txt")).read())
    assert plans["plain"] == recorded and set(recorded) == {"plan_contract", "plan_hostile"}, (plans["plain"], recorded)
