"""The refit of the ray-query hierarchy that runs on the stream, without a GPU.

tests/cpp/accel_refit_async_main.cpp emulates accel_dev.hip's accel_refit_enqueue with the headers its
kernels share: scenes of two covered objects are built on meshes A and refitted to B and then to C
through one workspace that only the documented resets touch; the result must equal, byte for byte,
a synchronous-style refit from A straight to C, in the per-level order and in the order of
refit_top_levels_kernel.  One face's class is then changed in three ways: the verdict function
(accel::refit_keeps) fails that object alone, the level passes still run to their end, queries
dispatched by the records' `has` word equal the linear scan, and a refit back to B gives the bytes of
a refit that never saw the bad mesh.  The program is also compiled with -fsanitize=address,undefined
and run as a program of its own."""
import ctypes as C
import os
import re
import subprocess

import pytest

from eray_amd import capi
from eray_amd import build as B
from tests.accel_emul import SANITIZER_FLAGS, asan_build, assert_clean_sanitizer_run, figures, run_built, write_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "eray_hip.h")).read()
SOURCES = [B.REFIT_ASYNC_MAIN, *B.ACCEL_DEV_SOURCES]
REUSE = ("sphere2000", "slivers", "soup1", "soup4", "soup5", "soup65", "soup513", "soup1100")
CLASS_CHANGES = {"culled_face_scaled_until_n1_is_4": 0, "nan_vertex_on_a_culled_face": 0,
                 "unculled_face_of_the_crowded_soup_shrunk": 1}


@pytest.fixture(scope="module")
def sphere_file(tmp_path_factory):
    return write_spheres(tmp_path_factory.mktemp("accel_refit_async_meshes"), (2000,))[0]


@pytest.fixture(scope="module")
def emulation(sphere_file):
    r = run_built("accel_refit_async_main", [sphere_file, "50000"], timeout=900)
    return r, figures(r.stdout, "reuse"), figures(r.stdout, "class_change")


def test_reused_workspace_gives_the_synchronous_refits_bytes(emulation):
    r, reuse, _ = emulation
    assert set(reuse) == set(REUSE), r.stdout + r.stderr
    for name, f in reuse.items():
        assert f["objects"] == 2 and f["refits"] == 2 and f["kept"] == 1, (name, f)
        assert f["same"] == 1 and f["check"] == 1, (name, f)
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr


def test_top_levels_order_gives_the_per_level_bytes(emulation):
    _, reuse, _ = emulation
    for name, f in reuse.items():
        assert f["top"] == 1, (name, f)
    assert reuse["sphere2000"]["nodes"] > 2 * 256  # levels on both sides of the workgroup's width
    assert reuse["soup1100"]["nodes"] > 511       # ... and a pairs level 9 inside the one launch


def test_a_class_change_fails_that_object_alone_and_heals(emulation):
    r, _, changes = emulation
    assert set(changes) == set(CLASS_CHANGES), r.stdout + r.stderr
    for name, obj in CLASS_CHANGES.items():
        f = changes[name]
        assert f["face"] >= 0 and f["object"] == obj and f["kept_before"] == 1 and f["only"] == 1, (name, f)
        assert f["rays"] >= 100000 and f["mismatch"] == 0 and f["hits"] >= 10000, (name, f)
        assert f["scanned"] == f["rays"], (name, f)  # exactly one of the two objects was scanned, per ray
        assert f["healed"] == 1 and f["check"] == 1 and f["refits"] == 3, (name, f)


def test_emulation_under_asan_ubsan(sphere_file, tmp_path):
    exe = str(tmp_path / "accel_refit_async_asan")
    asan_build(SOURCES, exe, SANITIZER_FLAGS)
    r = subprocess.run([exe, sphere_file, "1500"], capture_output=True, text=True, timeout=900)
    assert_clean_sanitizer_run(r)


# ------------------------------------------------------------------ the boundary -------------
def test_header_announces_the_async_refit_and_its_status():
    assert re.search(r"^#define ERAY_HAS_RAY_ACCEL_REFIT_ASYNC 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_ABI_VERSION 6\b", HEADER, re.M)
    assert re.search(r"^int eray_scene_refit_ray_accel_async\(eray_ctx\* ctx\);", HEADER, re.M)
    assert re.search(r"^int eray_scene_ray_accel_refit_status\(eray_ctx\* ctx, eray_ray_accel_refit_status\* out\);", HEADER, re.M)
    S = capi.RayAccelRefitStatus
    assert C.sizeof(S) == 32
    assert [getattr(S, n).offset for n in ("refits", "covered", "kept", "fell_back", "workspace_bytes", "reserved")] == \
        [0, 4, 8, 12, 16, 24]


def test_null_context_is_an_error_not_a_crash():
    L = capi.lib()
    st = capi.RayAccelRefitStatus()
    assert L.eray_scene_refit_ray_accel_async(None) == capi.E_INVALID_ARGUMENT
    assert L.eray_scene_ray_accel_refit_status(None, C.byref(st)) == capi.E_INVALID_ARGUMENT
    assert L.eray_scene_ray_accel_refit_status(None, None) == capi.E_INVALID_ARGUMENT
    n = C.c_size_t()
    assert L.eray_debug_ray_accel_arrays(None, 0, None, 0, C.byref(n)) == capi.E_INVALID_ARGUMENT
    assert L.eray_debug_set_refit_top_levels(None, 1) == capi.E_INVALID_ARGUMENT
