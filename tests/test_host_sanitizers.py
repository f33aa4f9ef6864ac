"""The PRODUCT's host code under AddressSanitizer + UndefinedBehaviorSanitizer, CPU only (tests/cpp/host_sanitize/): every translation unit of
hyslam_amd/csrc compiled host-only (`hipcc --cuda-host-only`: no device code) and linked against a stand-in for the HIP runtime on host memory
(hip_stub.cpp: device calls stubbed at the hipMalloc seam, the logic runs for real).  The driver sweeps random geometries through hs_orb_create /
hs_orb_reserve / the host-pointer entry points (planners, table builders, workspace sizing, staging, the ingest tickets) and feeds the vocabulary
loaders truncated and corrupted files, then the host-pointer forms of the key-frame graph, the local map and the pose optimiser, the `_device` forms of
the tracking, reference-key-frame and key-frame stages on work areas of exactly their stated size, and the place database through both of its regrow
paths; its `refusals` mode holds every enqueue-only `_device` entry point of the resident chain to "a refused call enqueues nothing".  Any sanitizer
report aborts the driver.  The same sources build under ThreadSanitizer (`make SAN=thread`, a build directory of its own; never
both sanitizers in one binary): the driver's `threads` mode runs every section that shares something between threads, adaptor_threads the thread
code of the header-only adaptors on the same stub objects.  Stand-alone programs throughout: nothing is loaded into python under a sanitizer.  (GPU
AddressSanitizer is not available on this pool; the oracle has its own sanitizer test, tests/test_oracle_sanitizers.py.)"""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DIR = os.path.join(ROOT, "tests", "cpp", "host_sanitize")
EXE = os.path.join(DIR, "_build", "host_sanitize")
EXE_T = os.path.join(DIR, "_build_thread", "host_sanitize")
REPORTS = ("ERROR: AddressSanitizer", "runtime error", "WARNING: ThreadSanitizer", "ERROR: LeakSanitizer")

# a CPU-only build: its hipcc lines pass -fno-gpu-sanitize beside -fsanitize= (no device code is sanitized or even compiled), and it never runs on a GPU
pytestmark = pytest.mark.skipif((shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc")) or not os.path.exists(os.path.join(DIR, "Makefile")),
                                reason="needs hipcc (host-only compile) and tests/cpp/host_sanitize/ (not shipped to GPU boxes)")


def build():
    subprocess.check_call(["make", "-s", "-j4", "-C", DIR], timeout=1500)


def build_thread():
    subprocess.check_call(["make", "-s", "-j4", "-C", DIR, "SAN=thread"], timeout=1500)


def clean_run(cmd, marker, env=None, timeout=900):
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout, env=env)
    assert r.returncode == 0 and marker in r.stdout, (cmd, (r.stdout + r.stderr)[-4000:])
    assert not any(x in r.stdout + r.stderr for x in REPORTS), (cmd, (r.stdout + r.stderr)[-4000:])
    return r


def test_every_translation_unit_of_the_library_is_built():
    """the sanitizer build takes its list from hyslam_amd/csrc/Makefile's SRCS: the two are equal, and every .hip file of the directory is on it"""
    with open(os.path.join(ROOT, "hyslam_amd", "csrc", "Makefile")) as f:
        srcs = re.search(r"^SRCS\s*:=\s*(.+)$", f.read(), re.M).group(1).split()
    assert all(x.endswith(".hip") for x in srcs) and len(set(srcs)) == len(srcs) >= 25
    for flavour in ([], ["SAN=thread"]):
        listed = subprocess.run(["make", "-s", "-C", DIR, "list"] + flavour, capture_output=True, text=True, timeout=60, check=True).stdout.split()
        assert listed == [x[:-4] for x in srcs], (flavour, listed)
    on_disk = sorted(x for x in os.listdir(os.path.join(ROOT, "hyslam_amd", "csrc")) if x.endswith(".hip"))
    assert sorted(srcs) == on_disk


def test_product_host_code_is_sanitizer_clean():
    build()
    for seed, geo, voc in ((1, 150, 500), (2, 150, 500), (7, 100, 300)):
        r = subprocess.run([EXE, str(seed), str(geo), str(voc)], capture_output=True, text=True, timeout=900)
        assert r.returncode == 0 and "HOST SANITIZE OK" in r.stdout, (r.stdout + r.stderr)[-4000:]
        assert "HOST SANITIZE MAP OK" in r.stdout, (r.stdout + r.stderr)[-4000:]          # map_sweep and the place database, behind the earlier sections
        assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-4000:]


def test_no_refused_call_enqueues_anything():
    """`host_sanitize refusals` from the address / UB build: every enqueue-only `_device` entry point of the resident chain and every chain, one valid
    argument set each and one knock-out at a time (every pointer and pointer field NULL, every integer at its first refused value, alignment, sensor
    without uR, the frame_result alias).  A call returns HS_OK or HS_ERR_INVALID; across a refused one the stub counts no launch, copy, memset or
    allocation; what only a later stage of a chain reads is refused by the chain"""
    build()
    r = clean_run([EXE, "refusals"], "HOST SANITIZE REFUSALS OK: 32 entry points")
    assert "REFUSALS FAILED" not in r.stdout, r.stdout[-4000:]
    for chain, launches in (("hs_track_motion_model_device", 21), ("hs_track_local_map_device", 22), ("hs_track_frame_device", 43)):
        assert re.search(r"^%s +valid call: +%d launches; +\d+ of \d+ knock-outs refused$" % (chain, launches), r.stdout, re.M), r.stdout[-4000:]


def test_threaded_sections_are_thread_sanitizer_clean():
    """`host_sanitize threads <seed>` under ThreadSanitizer: destroy against the last borrower, the frame cache's publishers / finders / consumers, the
    two sweeps on four threads with handles of their own, handle churn beside extraction and matching, one place database under a mutex beside one
    without, the vocabulary loaders with their thread-local error text, hs_comm_available's first call from four threads.  No suppression file.  The
    same mode under AddressSanitizer + UndefinedBehaviorSanitizer: what one thread frees under another is a report there"""
    build_thread()
    build()
    for exe, seeds in ((EXE_T, (1, 2, 7)), (EXE, (1,))):
        for seed in seeds:
            clean_run([exe, "threads", str(seed)], "HOST SANITIZE THREADS OK")


def test_adaptor_thread_code_is_sanitizer_clean():
    """hip_detail::Worker (run / wait, a job that throws, destruction with a job outstanding), hip_detail::thread_handle (one per thread, destroyed
    at thread exit beside working threads) and HipFeatureMatcher's projection search over 5000 landmarks with 0, 1 and 2 gather helpers from two
    calling threads, built against the stub objects; ThreadSanitizer, then AddressSanitizer + UndefinedBehaviorSanitizer"""
    build_thread()
    build()
    clean = {k: v for k, v in os.environ.items() if k != "HYSLAM_AMD_GATHER_THREADS"}
    for flavour in ("_build_thread", "_build"):
        for helpers in (0, 1, 2):
            r = clean_run([os.path.join(DIR, flavour, "adaptor_threads")], "ADAPTOR THREADS OK", env=dict(clean, HYSLAM_AMD_GATHER_THREADS=str(helpers)))
            assert "%d gather helper threads seen per caller" % min(helpers, len(os.sched_getaffinity(0)) - 1) in r.stdout      # 4096 landmarks took the split path


def test_small_batch_pyramid_plan_is_one_launch_at_1080p():
    """the host-side plan of BASELINE's geometry: levels 1-7 of a 1920x1080 frame in ONE k_resize_chain launch for small batches (3 in the standard plan)"""
    build()
    r = subprocess.run([EXE, "plan", "1920", "1080"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "standard plan 3, small-batch plan 1 (longest chain 7 levels" in r.stdout, r.stdout


def test_plan_digests_and_refusals_match_the_recorded_ones():
    """the pure host plan (hyslam_amd/csrc/hs_plan.hip) against tests/golden/plan_digests.json: for every recorded geometry and knob setting the
    summary line and the digest of the pointer-free plan — every table, record and offset the kernels get — or the refusal's status and text"""
    build()
    with open(os.path.join(ROOT, "tests", "golden", "plan_digests.json")) as f:
        cases = json.load(f)["cases"]
    assert len(cases) == 14 + 2 * 16 + 3 + 6 + 4 + 2 + 5
    clean = {k: v for k, v in os.environ.items() if not k.startswith("HS_")}
    for c in cases:
        r = subprocess.run([EXE, "plan"] + c["args"], env=dict(clean, **c["env"]), capture_output=True, text=True, timeout=300)
        what = (c["args"], c["env"], r.stdout + r.stderr[-2000:])
        assert r.returncode == 0 and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, what
        lines = r.stdout.strip().split("\n")
        if "refused" in c:
            assert lines == ["refused: status %d: %s" % (c["refused"]["status"], c["refused"]["error"])], what
        else:
            assert lines == [c["summary"], "plan digest: " + c["digest"]], what
