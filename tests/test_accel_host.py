"""The ray-query hierarchy without a GPU: the builder (eray_amd/csrc/accel_build.cpp) and the walk
the kernel runs (accel_walk.hpp) in tests/cpp/accel_walk_main.cpp, against a linear scan with one
shared f32 predicate; the boundary's structure, announcements and NULL-context behaviour.

The program runs at least 10^5 rays per mesh (50,000 of the sphere distribution plus the scaled
and adversarial sets: grazing rays within 1e-7 .. 1e-3 rad of a face's plane, along edges, through
vertices, zero direction components, starts on coordinate planes of vertices, directions of length
1e-3 and 1e3, starts at distance 1e3, NaN and inf components) on displaced_sphere(2000 / 20000,
42), a 300-face soup, the cube and a mesh with slivers, zero-area and huge faces.  The same
sources compiled with -fsanitize=address,undefined run a smaller count as a program of their own."""
import ctypes as C
import os
import re
import subprocess

import pytest

from eray_amd import capi
from tests.accel_emul import SANITIZER_FLAGS, asan_build, assert_clean_sanitizer_run, figures, run_built, write_spheres

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "eray_hip.h")).read()
SOURCES = [os.path.join(ROOT, "tests", "cpp", "accel_walk_main.cpp"), os.path.join(ROOT, "eray_amd", "csrc", "accel_build.cpp")]


@pytest.fixture(scope="module")
def sphere_files(tmp_path_factory):
    return write_spheres(tmp_path_factory.mktemp("accel_meshes"), (2000, 20000))


@pytest.fixture(scope="module")
def walk(sphere_files):
    r = run_built("accel_walk_main", [*sphere_files, "50000"], timeout=900)
    return r, figures(r.stdout)


SUITES = ("sphere2000", "sphere20000", "soup300", "cube", "slivers")


def test_walk_equals_the_scan_and_nodes_hold_their_faces(walk):
    """(a) every ray's walk result is the scan's; (b) every (ray, face) pair the predicate passes
    has its leaf and all its ancestors pass the node test, unless the face is unculled or the ray a
    fallback ray; the slots are a permutation of the faces, byte copies of their records."""
    r, fig = walk
    assert set(fig) == set(SUITES) | set(MOVED_SUITES), r.stdout + r.stderr
    for name in SUITES:
        f = fig[name]
        assert f["rays"] >= 100000, name
        assert f["mismatch"] == 0 and f["violation"] == 0 and f["perm"] == 1, (name, f)
    assert fig["sphere2000"]["pairs"] >= 10000 and fig["slivers"]["pairs"] >= 10000  # (b) saw passing pairs
    assert fig["slivers"]["unculled"] > 0 and fig["slivers"]["nodes"] > 0  # both kinds of face in one object
    assert r.returncode == 0 and r.stdout.rstrip().endswith("OK"), r.stdout + r.stderr


def test_build_is_deterministic_and_bounded(walk):
    """(c) two builds give the same bytes; (d) a stack one level short of the tree is refused; the
    depth stays within ceil(log2(T / leaf)) + 1 and the walk's stack below the tree's depth."""
    _, fig = walk
    for name in SUITES:
        f = fig[name]
        assert f["rebuild"] == 1 and f["deep"] == 1, name
        assert f["depth"] <= f["depth_bound"] <= 32, name
        assert f["stack_high"] < max(f["depth"], 1), name


def test_honesty_caps(walk):
    """(e) conditions, not measurements: the 20,000-face sphere's mean face tests per ray of the
    sphere distribution at most T / 10; no unculled face on either sphere; no fallback ray among the
    finite rays with |d| in [1e-3, 1e3]; the cube's faces all unculled."""
    _, fig = walk
    assert fig["sphere20000"]["tests_per_ray"] <= 20000 / 10
    assert fig["sphere2000"]["unculled"] == 0 and fig["sphere20000"]["unculled"] == 0
    for name in SUITES:
        assert fig[name]["fallback_in_range"] == 0, name
        assert fig[name]["fallback"] >= 48, name  # the non-finite rays do fall back
    assert fig["cube"]["unculled"] == 12 and fig["cube"]["nodes"] == 0


MOVES = ((1, 0, 1e6), (1, 1000, 1), (1, 1000, 1e5), (1e-2, 5, 1e4), (1e-2, 0, 1))  # (s, t, k), the program's order
MOVED_SUITES = tuple(f"{mesh}_m{m}" for m in range(len(MOVES)) for mesh in ("sphere2000", "slivers"))


@pytest.mark.parametrize("name", MOVED_SUITES)
def test_moved_meshes_and_scaled_directions(walk, name):
    """sphere2000 and the sliver mesh moved to x * s + t with the rays' directions scaled by s * k:
    directions up to 5e6 long (step 5 of accel_build.hpp's margin proof) and meshes 1000 units from
    the origin (beta's |a|1 term).  20,000 rays each, all inside accel_covered's range by
    construction: none falls back, the walk equals the scan, no passing face's leaf or ancestor
    fails the node test, and faces remain under the tree (an empty tree would test nothing)."""
    r, fig = walk
    assert name in fig, r.stdout + r.stderr
    f = fig[name]
    assert f["rays"] == 20000, f
    assert f["mismatch"] == 0 and f["violation"] == 0, f
    assert f["fallback"] == 0 and f["fallback_in_range"] == 0, f
    assert f["pairs"] >= 3000, f
    assert f["unculled"] < f["faces"] and f["nodes"] > 0, f


def test_walk_program_under_asan_ubsan(sphere_files, tmp_path):
    """The same two sources with -fsanitize=address,undefined, run directly (its own main)."""
    exe = str(tmp_path / "accel_walk_asan")
    asan_build(SOURCES, exe, SANITIZER_FLAGS)
    r = subprocess.run([exe, *sphere_files, "1500"], capture_output=True, text=True, timeout=900)
    assert_clean_sanitizer_run(r)


# ------------------------------------------------------------------ the boundary -------------
def header_struct(name):
    """(size from the struct's 'NN B' comment, {field: offset} from its 'offset N' comments)."""
    m = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), HEADER, re.S)
    assert m, name
    body = m.group(1)
    size = int(re.search(r"(\d+) B \*/", body).group(1))
    offsets = {}
    for decl, first, second in re.findall(r"([^;/]*);\s*/\* offset (\d+)(?:, (\d+))?", body):
        names = [re.sub(r"\[.*", "", n.strip().split()[-1].lstrip("*")) for n in decl.split(",")]
        for n, off in zip(names, [first, second]):
            offsets[n] = int(off)
    return size, offsets


def test_info_structure_matches_the_header():
    size, offsets = header_struct("eray_ray_accel_info")
    assert size == 48 == C.sizeof(capi.RayAccelInfo)
    assert set(offsets) == {f[0] for f in capi.RayAccelInfo._fields_}
    for field, off in offsets.items():
        assert getattr(capi.RayAccelInfo, field).offset == off, field


def test_header_announces_the_hierarchy():
    assert re.search(r"^#define ERAY_HAS_RAY_ACCEL 1\b", HEADER, re.M)
    assert re.search(r"^#define ERAY_ABI_VERSION 6\b", HEADER, re.M)
    assert not re.search(r"^#define ERAY_RAYS_\w+ (?!1u|2u)", HEADER, re.M)  # no new ERAY_RAYS_* flag
    for name in ("eray_scene_build_ray_accel", "eray_scene_drop_ray_accel"):
        assert name in capi.SIGNATURES and hasattr(capi.lib(), name)
        assert name in open(os.path.join(ROOT, "INTEGRATION.md")).read()
    assert hasattr(capi.Context, "build_ray_accel") and hasattr(capi.Context, "drop_ray_accel")


def test_null_context_is_an_error_not_a_crash():
    info = capi.RayAccelInfo()
    assert capi.lib().eray_scene_build_ray_accel(None, 0, C.byref(info)) == capi.E_INVALID_ARGUMENT
    assert capi.lib().eray_scene_build_ray_accel(None, 0, None) == capi.E_INVALID_ARGUMENT
    assert capi.lib().eray_scene_drop_ray_accel(None) == capi.E_INVALID_ARGUMENT
