"""Engine::build_ray_accel of the C++ host (tests/cpp/test_accel.cpp): build_host builds the
binary; on the GPU cast_rays gives the same records with the hierarchy as without, on the cube and
on a generated sphere."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_accel_bin():
    from eray_amd import build as B
    outs = B.build_host()
    exe = os.path.join(ROOT, "eray_amd", "bin", "test_accel")
    assert exe in outs and os.path.exists(exe)
    return exe


def test_build_host_builds_test_accel(test_accel_bin):
    assert os.access(test_accel_bin, os.X_OK)


@pytest.mark.gpu
def test_engine_build_ray_accel_gpu(test_accel_bin, tmp_path):
    r = subprocess.run([test_accel_bin, "--root", ROOT], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "2 tests, 0 failed checks" in r.stdout
