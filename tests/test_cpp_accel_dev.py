"""Engine::build_ray_accel(min_faces, on_device=true) of the C++ host (tests/cpp/test_accel_dev.cpp):
build_host builds the binary; on the GPU cast_rays gives the same records through the device-built
hierarchy as without one and as through the host-built one."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_accel_dev_bin():
    from eray_amd import build as B
    outs = B.build_host()
    exe = os.path.join(ROOT, "eray_amd", "bin", "test_accel_dev")
    assert exe in outs and os.path.exists(exe)
    return exe


def test_build_host_builds_test_accel_dev(test_accel_dev_bin):
    assert os.access(test_accel_dev_bin, os.X_OK)


@pytest.mark.gpu
def test_engine_build_ray_accel_on_device_gpu(test_accel_dev_bin, tmp_path):
    r = subprocess.run([test_accel_dev_bin], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1 tests, 0 failed checks" in r.stdout
