"""Engine::reaches_light of the C++ host (tests/cpp/test_reach.cpp): build_host builds the binary;
on the GPU it reproduces the hand-derived pair (a face between start and target blocks, a target in
front of the face is reached), with and without a hierarchy."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_reach_bin():
    from eray_amd import build as B
    outs = B.build_host()
    exe = os.path.join(ROOT, "eray_amd", "bin", "test_reach")
    assert exe in outs and os.path.exists(exe)
    return exe


def test_build_host_builds_test_reach(test_reach_bin):
    assert os.access(test_reach_bin, os.X_OK)


@pytest.mark.gpu
def test_engine_reaches_light_gpu(test_reach_bin, tmp_path):
    r = subprocess.run([test_reach_bin], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1 tests, 0 failed checks" in r.stdout
