"""Engine::update_object and Engine::refit_ray_accel of the C++ host (tests/cpp/test_update.cpp):
build_host builds the binary; on the GPU an Engine whose sphere was moved in place answers
cast_rays and render as a freshly built Engine does, with and without the refitted hierarchy."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def test_update_bin():
    from eray_amd import build as B
    outs = B.build_host()
    exe = os.path.join(ROOT, "eray_amd", "bin", "test_update")
    assert exe in outs and os.path.exists(exe)
    return exe


def test_build_host_builds_test_update(test_update_bin):
    assert os.access(test_update_bin, os.X_OK)


def test_hosts_declare_the_update_and_the_refit():
    engine = open(os.path.join(ROOT, "include", "eray", "engine.hpp")).read()
    assert "void update_object(size_t index, const Object<Built>& object);" in engine
    assert "RayAccelRefitInfo refit_ray_accel();" in engine
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "eray_scene_update_object" in text and "eray_scene_refit_ray_accel" in text


@pytest.mark.gpu
def test_engine_update_object_and_refit_gpu(test_update_bin, tmp_path):
    r = subprocess.run([test_update_bin], capture_output=True, text=True, timeout=120, cwd=tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "1 tests, 0 failed checks" in r.stdout
