"""Engine::build_ray_accel(min_faces, on_device, refittable) of the C++ host
(tests/cpp/test_refit_hosttree.cpp): build_host builds the binary; on the GPU an Engine builds the
host-split hierarchy refittable, moves its sphere in place, refits without a rebuild and answers
cast_rays as a freshly built Engine does."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_refit_hosttree_bin():
    from eray_amd import build as B
    outs = B.build_host()
    exe = os.path.join(ROOT, "eray_amd", "bin", "test_refit_hosttree")
    assert exe in outs and os.path.exists(exe)
    return exe


def test_build_host_builds_test_refit_hosttree(test_refit_hosttree_bin):
    assert os.access(test_refit_hosttree_bin, os.X_OK)


@pytest.mark.gpu
def test_engine_refits_a_host_built_tree_gpu(test_refit_hosttree_bin, tmp_path):
    r = subprocess.run([test_refit_hosttree_bin], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1 tests, 0 failed checks" in r.stdout
