"""The refit of a host-built ray-query hierarchy without a GPU.

tests/cpp/accel_refit_hosttree_main.cpp compares accel_layout.hpp's recursion-order numbering
(PreOrder) with a recursion that numbers as the host builder does, for every culled count up to 5,000;
builds meshes with accel_build.cpp's build_object at non-zero bases and refits them with
level_node<PreOrder>, step for step as the refit kernels run: with unmoved faces the refit is the
build byte for byte; after a deformation accel::check accepts the tree, the walk equals the linear scan
and the words that depend on face indices alone are the build's; single faces that change class make
the refit refuse; the checker names the nine corruptions on a refitted host tree.  A scene of three
objects goes through accel_build.cpp's build_scene, the code eray_scene_build_ray_accel_refittable runs
between its download and its uploads: the arrays are build_object's per covered object, the layout
records what the sizes and tree_layout give, and a refit through them reproduces the arrays.  The
program is also compiled with -fsanitize=address,undefined and run as a program of its own."""
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
SOURCES = [B.REFIT_HOSTTREE_MAIN, *B.ACCEL_DEV_SOURCES]
MESHES = ("sphere2000", "slivers3000")
# 9 .. 19: the smallest sizes at which the two halves' subtrees differ in node count
SOUPS = tuple(f"soup{T}h" for T in (1, 4, 5, 9, 10, 11, 13, 19, 65, 513))
CORRUPTIONS = {"swapped_children", "shrunk_h", "lowered_alpha", "leaf_out_of_order", "duplicated_slot", "wrong_min_index",
               "wrong_right_min", "lowered_gamma", "unculled_into_tree"}
CLASS_CHANGES = ("culled_face_scaled_until_n1_is_4", "nan_vertex_on_a_culled_face", "unculled_face_of_the_crowded_soup_shrunk")


@pytest.fixture(scope="module")
def sphere_file(tmp_path_factory):
    return write_spheres(tmp_path_factory.mktemp("accel_refit_hosttree_meshes"), (2000,))[0]


@pytest.fixture(scope="module")
def emulation(sphere_file):
    r = run_built("accel_refit_hosttree_main", [sphere_file, "50000"], timeout=900)
    return r, figures(r.stdout)


def test_arithmetic_ids_are_the_host_builders_for_every_count_to_5000(emulation):
    r, _ = emulation
    m = re.search(r"^ids=(\d+) id_errors=(\d+) range_errors=(\d+) coverage_errors=(\d+) count_errors=(\d+)$", r.stdout, re.M)
    assert m, r.stdout + r.stderr
    assert int(m.group(1)) >= 5000 and [int(g) for g in m.groups()[1:]] == [0, 0, 0, 0], m.group(0)


def test_refit_of_the_same_mesh_is_the_host_build_byte_for_byte(emulation):
    r, fig = emulation
    assert set(fig) == set(MESHES) | set(SOUPS), r.stdout + r.stderr
    for name, f in fig.items():
        assert f["identity"] == 1, (name, f)
    assert fig["slivers3000"]["unculled"] > 0 and fig["slivers3000"]["nodes"] > 0  # both kinds of face in one object
    assert fig["soup9h"]["nodes"] == 5 and fig["soup19h"]["nodes"] == 13  # halves of unlike node counts


def test_refit_of_the_moved_mesh_passes_the_checker_and_equals_the_scan(emulation):
    r, fig = emulation
    for name, f in fig.items():
        assert f["check"] == 1 and f["moved"] >= 1, (name, f)  # (the refit rewrote nodes: B is not A)
    for name in MESHES:
        f = fig[name]
        assert f["rays"] >= 100000 and f["mismatch"] == 0 and f["hits"] >= 10000 and f["fallback"] >= 48, (name, f)
    for name in SOUPS:
        assert fig[name]["rays"] >= 1024 and fig[name]["mismatch"] == 0 and fig[name]["hits"] >= 100, name
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr


def test_refit_keeps_the_index_array_and_the_index_words_of_every_node(emulation):
    _, fig = emulation
    for name, f in fig.items():
        assert f["topology"] == 1, (name, f)


def test_class_changes_are_detected(emulation):
    r, _ = emulation
    for name in CLASS_CHANGES:
        m = re.search(rf"^class_change={name} face=(-?\d+) detected=(\d)$", r.stdout, re.M)
        assert m and int(m.group(1)) >= 0 and m.group(2) == "1", (name, r.stdout)


def test_checker_names_every_corruption_of_a_refitted_host_tree(emulation):
    r, fig = emulation
    for name, f in fig.items():
        assert f["corruption_failed"] == 0, (name, r.stdout)
    m = re.search(r"^corruptions_named=(\S*)$", r.stdout, re.M)
    assert m and set(m.group(1).split(",")) == CORRUPTIONS, r.stdout
    assert fig["slivers3000"]["caught"] == len(CORRUPTIONS)


def test_scene_build_concatenates_the_objects_and_records_the_layout_a_refit_reproduces_it_from(emulation):
    r, _ = emulation
    f = figures(r.stdout, key="scene")["three_objects"]
    assert f["slices"] == 1 and f["layout"] == 1 and f["refit"] == 1, f
    # two covered objects around one below min_faces; a tree with a pairs level and one without
    assert f["objects"] == 2 and f["c0"] == 259 and f["extra0"] == 3 and f["c2"] == 256 and f["extra2"] == 0, f


def test_emulation_under_asan_ubsan(sphere_file, tmp_path):
    exe = str(tmp_path / "accel_refit_hosttree_asan")
    asan_build(SOURCES, exe, SANITIZER_FLAGS)
    r = subprocess.run([exe, sphere_file, "1500"], capture_output=True, text=True, timeout=900)
    assert_clean_sanitizer_run(r)


# ------------------------------------------------------------------ the boundary -------------
def test_header_announces_the_refittable_host_build():
    assert re.search(r"^#define ERAY_HAS_RAY_ACCEL_REFIT_HOST 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_ABI_VERSION 6\b", HEADER, re.M)
    assert re.search(r"^int eray_scene_build_ray_accel_refittable\(eray_ctx\* ctx, uint32_t min_faces, eray_ray_accel_info\* info",
                     HEADER, re.M)
    text = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert "pub fn eray_scene_build_ray_accel_refittable(ctx: *mut ErayCtx, min_faces: u32, info: *mut ErayRayAccelInfo) -> c_int;" in text
    engine = open(os.path.join(ROOT, "include", "eray", "engine.hpp")).read()
    assert "RayAccelInfo build_ray_accel(uint32_t min_faces, bool on_device, bool refittable);" in engine


def test_library_exports_the_entry_point_and_null_context_is_an_error():
    L = capi.lib()
    assert hasattr(L, "eray_scene_build_ray_accel_refittable")
    info = capi.RayAccelInfo()
    assert L.eray_scene_build_ray_accel_refittable(None, 0, C.byref(info)) == capi.E_INVALID_ARGUMENT
    assert L.eray_scene_build_ray_accel_refittable(None, 0, None) == capi.E_INVALID_ARGUMENT


def test_refittable_with_device_is_a_value_error():
    ctx = object.__new__(capi.Context)  # (the check comes before any library call: no device needed)
    with pytest.raises(ValueError):
        capi.Context.build_ray_accel(ctx, 0, device=True, refittable=True)
