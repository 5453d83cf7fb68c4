"""The device-side builder of the ray-query hierarchy without a GPU: tests/cpp/accel_dev_main.cpp
emulates accel_dev.hip on the CPU with the headers its kernels share (accel_margin.hpp,
accel_layout.hpp), checks the result and the host builder's with accel::check (accel_check.cpp),
walks at least 10^5 rays per mesh through the emulated tree against the linear scan, and corrupts
a valid tree in named ways that the checker must name.  The same sources compiled with
-fsanitize=address,undefined run a smaller count as a program of their own.  Then the boundary:
the header's declaration and define, the exported symbols, the Python and C++ host interfaces."""
import ctypes as C
import inspect
import os
import re
import subprocess

import pytest

from eray_amd import capi
from eray_amd import build as B
from tests.accel_emul import SANITIZER_FLAGS, asan_build, assert_clean_sanitizer_run, figures, run_built, write_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "eray_hip.h")).read()
DEBUG_HEADER = open(os.path.join(ROOT, "include", "eray_hip_debug.h")).read()
SOURCES = [os.path.join(ROOT, "tests", "cpp", "accel_dev_main.cpp"), *B.ACCEL_DEV_SOURCES]
MESHES = ("sphere2000", "sphere20000", "soup300", "cube", "slivers")
EXTRA = ("tied256", "planar200", "soup1b", "soup4b", "soup5b", "soup8b", "soup9b", "soup64b", "soup65b", "soup513b")
CORRUPTIONS = {"swapped_children", "shrunk_h", "lowered_alpha", "leaf_out_of_order", "duplicated_slot", "wrong_min_index",
               "wrong_right_min", "lowered_gamma", "unculled_into_tree"}


@pytest.fixture(scope="module")
def sphere_files(tmp_path_factory):
    return write_spheres(tmp_path_factory.mktemp("accel_dev_meshes"), (2000, 20000))


@pytest.fixture(scope="module")
def emulation(sphere_files):
    r = run_built("accel_dev_main", [*sphere_files, "50000"], timeout=900)
    return r, figures(r.stdout)


def test_emulated_build_passes_the_checker_and_so_does_the_host_build(emulation):
    r, fig = emulation
    assert set(fig) == set(MESHES) | set(EXTRA), r.stdout + r.stderr
    for name, f in fig.items():
        assert f["check_dev"] == 1 and f["check_host"] == 1, (name, f)
    assert "layout=1" in r.stdout  # node count and depth from C alone equal the recursion's, C = 0 .. 5000
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr


def test_walk_through_the_emulated_tree_equals_the_scan(emulation):
    """At least 10^5 rays per mesh (the sphere distribution, its scaled forms, the adversarial and
    non-finite rays of accel_walk_main.cpp): accel_first_face gives the linear scan's face."""
    _, fig = emulation
    for name in MESHES + ("tied256", "planar200"):
        f = fig[name]
        assert f["rays"] >= 100000 and f["mismatch"] == 0 and f["hits"] >= 10000, (name, f)
        assert f["fallback"] >= 48, name  # (the non-finite rays are among them)
    for name in EXTRA[2:]:
        assert fig[name]["mismatch"] == 0 and fig[name]["hits"] >= 100, name


def test_topology_is_the_host_builders(emulation):
    """The balanced split of the Morton order has the host build's node count, depth, unculled list
    and Object record (root, ubegin, ucount, gamma: byte for byte) on every mesh, and is the same
    tree at other node / slot bases."""
    _, fig = emulation
    for name, f in fig.items():
        assert f["same_shape"] == 1 and f["shifted"] == 1, (name, f)
    for T, depth in ((1, 1), (4, 1), (5, 2), (8, 2), (9, 3), (64, 5), (65, 6), (513, 9)):
        assert fig[f"soup{T}b"]["depth"] == depth and fig[f"soup{T}b"]["unculled"] == 0, T
    assert fig["cube"]["unculled"] == 12 and fig["cube"]["nodes"] == 0
    assert fig["slivers"]["unculled"] > 0 and fig["slivers"]["nodes"] > 0  # both kinds of face in one object


def test_checker_names_every_corruption(emulation):
    r, fig = emulation
    for name, f in fig.items():
        assert f["corruption_failed"] == 0, (name, r.stdout)
    m = re.search(r"^corruptions_named=(\S*)$", r.stdout, re.M)
    assert m and set(m.group(1).split(",")) == CORRUPTIONS, r.stdout
    assert fig["slivers"]["caught"] == len(CORRUPTIONS)  # all of them on one mesh with both kinds of face


def test_emulation_under_asan_ubsan(sphere_files, tmp_path):
    """The same sources with -fsanitize=address,undefined, run directly (its own main)."""
    exe = str(tmp_path / "accel_dev_asan")
    asan_build(SOURCES, exe, SANITIZER_FLAGS)
    r = subprocess.run([exe, *sphere_files, "1500"], capture_output=True, text=True, timeout=900)
    assert_clean_sanitizer_run(r)


# ------------------------------------------------------------------ the boundary -------------
def test_header_announces_the_device_build():
    assert re.search(r"^#define ERAY_HAS_RAY_ACCEL_DEVICE 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_ABI_VERSION 6\b", HEADER, re.M)
    assert re.search(r"^int eray_scene_build_ray_accel_device\(eray_ctx\* ctx, uint32_t min_faces, eray_ray_accel_info\* info",
                     HEADER, re.M)
    assert "round trip" in HEADER  # the one device-to-host copy is stated
    assert re.search(r"^int eray_debug_ray_accel_check\(eray_ctx\* ctx, char\* msg, uint32_t cap\);", DEBUG_HEADER, re.M)
    assert "eray_debug_ray_accel_check" not in HEADER


def test_library_exports_the_new_symbols():
    L = capi.lib()
    assert "eray_scene_build_ray_accel_device" in capi.SIGNATURES and hasattr(L, "eray_scene_build_ray_accel_device")
    assert "eray_debug_ray_accel_check" in capi.DEBUG_SIGNATURES and hasattr(L, "eray_debug_ray_accel_check")
    assert capi.SIGNATURES["eray_scene_build_ray_accel_device"] == capi.SIGNATURES["eray_scene_build_ray_accel"]
    assert "eray_scene_build_ray_accel_device" in open(os.path.join(ROOT, "INTEGRATION.md")).read()


def test_python_and_cpp_hosts_offer_the_choice():
    sig = inspect.signature(capi.Context.build_ray_accel)
    assert sig.parameters["device"].default is False and sig.parameters["min_faces"].default == 0
    engine = open(os.path.join(ROOT, "include", "eray", "engine.hpp")).read()
    assert "RayAccelInfo build_ray_accel(uint32_t min_faces = 0, bool on_device = false);" in engine


def test_null_context_is_an_error_not_a_crash():
    info = capi.RayAccelInfo()
    assert capi.lib().eray_scene_build_ray_accel_device(None, 0, C.byref(info)) == capi.E_INVALID_ARGUMENT
    assert capi.lib().eray_scene_build_ray_accel_device(None, 0, None) == capi.E_INVALID_ARGUMENT
    msg = C.create_string_buffer(64)
    assert capi.lib().eray_debug_ray_accel_check(None, msg, 64) == capi.E_INVALID_ARGUMENT
