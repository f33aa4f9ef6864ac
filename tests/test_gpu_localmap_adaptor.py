"""GPU: HipKeyFrameGraph::localMap (hyslam_amd/host/HipKeyFrameGraph.h) on the cv_compat.h stand-ins against a literal walk written from
TrackLocalMap.cpp — tests/cpp/test_localmap_adaptor.cpp, built and run here."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, "tests", "cpp", "_build")
EXE = os.path.join(BUILD, "test_localmap_adaptor")

pytestmark = pytest.mark.gpu


def test_cpp_local_map_adaptor(gpu):
    os.makedirs(BUILD, exist_ok=True)
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-pthread",
                           os.path.join(ROOT, "tests", "cpp", "test_localmap_adaptor.cpp"), "-o", EXE,
                           "-L" + os.path.join(ROOT, "hyslam_amd"), "-lhyslam_amd", "-Wl,-rpath," + os.path.join(ROOT, "hyslam_amd")])
    r = subprocess.run([EXE], capture_output=True, timeout=300)
    assert r.returncode == 0 and b"LOCAL MAP ADAPTOR OK" in r.stdout, r.stdout + r.stderr
