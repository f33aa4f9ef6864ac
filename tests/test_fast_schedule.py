"""The FAST stage's launch plan and work-unit schedule on the CPU (hyslam_amd/csrc/hs_plan_fast.hip, hs_fast.h), through two modes of the
host_sanitize driver (tests/cpp/host_sanitize/: the library's host code under AddressSanitizer + UndefinedBehaviorSanitizer on a stand-in HIP runtime;
a stand-alone program, nothing is loaded into python).  No GPU."""
import json
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp", "host_sanitize")
EXE = os.path.join(DIR, "_build", "host_sanitize")
REPORTS = ("ERROR: AddressSanitizer", "runtime error", "ERROR: LeakSanitizer")

pytestmark = pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(DIR, "Makefile")),
                                reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/ (not shipped to GPU boxes)")


def run_mode(mode, env):
    subprocess.check_call(["make", "-s", "-j4", "-C", DIR], timeout=1500)
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HS_")}
    r = subprocess.run([EXE, mode], env=dict(clean, **env), capture_output=True, text=True, timeout=300)
    out = r.stdout + r.stderr
    assert r.returncode == 0 and not any(x in out for x in REPORTS), (mode, env, out[-4000:])
    return r.stdout


def test_fast_launch_plans_match_the_recorded_ones():
    """`host_sanitize fastplan` against tests/golden/fast_launch_digests.json: for every recorded setting of the HS_FAST_* knobs (read through the knob
    table, as a handle reads them) one digest per tile width over every field of hs_fast_launch_plan's record and hs_fast_overflow_bytes — max_hcell on
    both sides of every tile-row instance, batches 1-256, 1-1904 items, the whole list and both ranges of the split — and one over the narrow / wide
    choice for batches 1-128.  The recorded lines were printed by the launcher's own configuration code of the commit before the plan function existed"""
    with open(os.path.join(ROOT, "tests", "golden", "fast_launch_digests.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 13
    for c in cases:
        assert run_mode("fastplan", c["env"]).strip().split("\n") == c["lines"], c["env"]


def test_fast_schedule_hands_out_every_unit_once():
    """`host_sanitize fastsched`: the host half of k_fast_rows' work-unit schedule (hs_fast_launch_plan: mode, queue count, magic divisors) and its device
    half (hs_fast.h: fast_queue_size, unit_decode, fast_div, compiled for the host) together — batches 1-64, 1-61 items per image, HS_FAST_NQ unset / 8 /
    16 with and without HS_FAST_IMAGE_MAJOR and HS_FAST_NO_FOLD, workgroups as planned for max_hcell 31 at both tile widths: every (item, image) exactly
    once and nothing else, fast_div(a, d, m) == a / d for every operand pair, the workgroups a multiple of the queues, all five modes reached"""
    out = run_mode("fastsched", {})
    assert "FAST SCHEDULE OK: 720 launches" in out and "FAILED" not in out, out[-4000:]
