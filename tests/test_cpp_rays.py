"""Engine::cast_rays of the C++ host (tests/cpp/test_rays.cpp): build_host builds the binary; on
the GPU it reproduces the hand-derived one-face record and the cube's centre ray (face 1)."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_rays_bin():
    from eray_amd import build as B
    outs = B.build_host()
    exe = os.path.join(ROOT, "eray_amd", "bin", "test_rays")
    assert exe in outs and os.path.exists(exe)
    return exe


def test_build_host_builds_test_rays(test_rays_bin):
    assert os.access(test_rays_bin, os.X_OK)


@pytest.mark.gpu
def test_engine_cast_rays_gpu(test_rays_bin, tmp_path):
    r = subprocess.run([test_rays_bin, "--root", ROOT], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 tests, 0 failed checks" in r.stdout
