"""GPU: HipSim3Solver (hyslam_amd/host/HipSim3Solver.h) on the cv_compat.h stand-ins against hs_sim3_iterate on hand-gathered arrays: the gathering
as the reference's constructor walks it, then identical bytes alone, in one static call over all candidates, and on a second call —
tests/cpp/test_sim3_adaptor.cpp, built and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "test_sim3_adaptor")

pytestmark = pytest.mark.gpu


def test_cpp_sim3_solver_adaptor(gpu):
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "test_sim3_adaptor.cpp"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])
    r = subprocess.run([EXE], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"SIM3 ADAPTOR OK" in r.stdout, r.stdout + r.stderr
