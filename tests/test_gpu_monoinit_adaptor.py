"""GPU: HipMonoEstimator (hyslam_amd/host/HipMonoEstimator.h) on the cv_compat.h stand-ins against hs_monoinit_estimate on hand-gathered arrays: the
reference's constructor and Initialize signature, then identical bytes alone, in one static call over all cameras, and on a second call —
tests/cpp/test_monoinit_adaptor.cpp, built (-Wall -Wextra -Werror) and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "test_monoinit_adaptor")

pytestmark = pytest.mark.gpu


def test_cpp_mono_estimator_adaptor(gpu):
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "test_monoinit_adaptor.cpp"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])
    r = subprocess.run([EXE], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"MONOINIT ADAPTOR OK" in r.stdout, r.stdout + r.stderr
