"""GPU parity of the device-built ray-query hierarchy (eray_scene_build_ray_accel_device;
accel_dev.hip, accel_margin.hpp, accel_layout.hpp): eray_cast_rays returns through it the records
it returns without one and through the host-built hierarchy — the first face BY INDEX that passes
Triangle::intersects in f32, with the same u, v, t bits.

Bar: byte equality of whole record arrays (and of out_rgb) between the device-built hierarchy, the
LDS tiles (before any build), ERAY_RAYS_BRUTE_FORCE and the host-built hierarchy; the same info
counts as the host build; and eray_debug_ray_accel_check (accel_check.cpp on the arrays copied
back) accepts the tree.  Meshes, rays and comparisons are those of tests/test_gpu_rays_accel.py
(imported), every build here is device=True."""
import numpy as np
import pytest

from eray_amd import capi
from tests.test_gpu_rays_accel import (adversarial_rays, assert_hits_equal, passing_faces_f64, rays_array, scene, soup,
                                       sphere_mesh, sphere_rays, true_box)

pytestmark = pytest.mark.gpu

COUNTS = ("objects", "faces", "nodes", "max_depth", "unculled_faces", "device_bytes")


@pytest.fixture(scope="module")
def sphere3000():
    rng = np.random.default_rng(21)
    mesh = sphere_mesh(3000)
    s0, d0 = sphere_rays(rng, 4096)
    s1, d1 = adversarial_rays(rng, mesh[0])
    return {"mesh": mesh, "box": true_box(mesh), "start": np.concatenate([s0, s1]), "raw": np.concatenate([d0, d1])}


def forms(gpu, rays, min_faces, what, normalize=(False, True), object=-1, want_rgb=True, expect=None):
    """three_forms of tests/test_gpu_rays_accel.py with a fourth and a fifth: tiles (no hierarchy),
    brute force, the host-built hierarchy and the device-built one, byte for byte; the checker on
    both trees; the device build's counts against the host build's.  Returns the device build's
    info and the records of the last `normalize`."""
    gpu.drop_ray_accel()
    rgb_now = want_rgb and object < 0  # (out_rgb has no single-object form)

    def cast(nz, **kw):
        return gpu.cast_rays(rays, normalize=nz, object=object, want_rgb=rgb_now, **kw)

    before = {nz: {"tiles": cast(nz), "brute force": cast(nz, brute_force=True)} for nz in normalize}
    host = gpu.build_ray_accel(min_faces)
    if host["objects"]:
        assert gpu.check_ray_accel() == "", f"{what}: the checker on the host build"
    for nz in normalize:
        before[nz]["the host-built hierarchy"] = cast(nz)
    info = gpu.build_ray_accel(min_faces, device=True)
    for k, v in (expect or {}).items():
        assert info[k] == v, (what, k, info)
    for k in COUNTS:
        assert info[k] == host[k], (what, k, info, host)
    if info["objects"]:
        assert gpu.check_ray_accel() == "", f"{what}: the checker on the device build"
    for nz in normalize:
        tree = cast(nz)
        others = dict(before[nz])
        others["brute force after the build"] = cast(nz, brute_force=True)
        for name, other in others.items():
            if rgb_now:
                assert_hits_equal(tree[0], other[0], f"{what} normalize={nz}: device-built hierarchy vs {name}")
                assert tree[0].tobytes() == other[0].tobytes(), f"{what} normalize={nz}: records vs {name}"
                assert tree[1].tobytes() == other[1].tobytes(), f"{what} normalize={nz}: out_rgb vs {name}"
            else:
                assert_hits_equal(tree, other, f"{what} normalize={nz}: device-built hierarchy vs {name}")
                assert tree.tobytes() == other.tobytes(), f"{what} normalize={nz}: records vs {name}"
    return info, (tree[0] if rgb_now else tree)


# ------------------------------------------------------------------ 1. byte equality ---------
def test_device_build_is_byte_equal_on_the_sphere(gpu, sphere3000):
    """displaced_sphere(3000, 42) with its true box: 4096 sphere rays and the adversarial set,
    stored and normalised directions, object -1 (with out_rgb) and object 0."""
    A = sphere3000
    scene(gpu, [(A["mesh"], A["box"])])
    rays = rays_array(A["start"], A["raw"])
    expect = {"objects": 1, "faces": 3000, "unculled_faces": 0}
    info, hits = forms(gpu, rays, 0, "sphere 3000, object -1", expect=expect)
    assert info["nodes"] >= 3000 // 4 and 10 <= info["max_depth"] <= 11 and info["device_bytes"] > 48 * 3000
    hit = hits["object"][:4096] >= 0
    assert hit.sum() >= 1000 and (~hit).sum() >= 500
    assert (hits["object"][4096:4096 + 960] >= 0).sum() >= 100  # adversarial rays that hit
    forms(gpu, rays, 0, "sphere 3000, object 0", object=0, expect=expect)
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 2. tree boundaries -------
@pytest.mark.parametrize("T, min_faces, objects", [(1, 1, 1), (4, 1, 1), (5, 1, 1), (8, 1, 1), (9, 1, 1), (64, 1, 1),
                                                  (65, 1, 1), (512, 1, 1), (513, 1, 1), (15, 16, 0), (16, 16, 1)])
def test_tree_and_leaf_boundaries(gpu, T, min_faces, objects):
    """Single-face, full and odd leaves, counts on a depth boundary (64 = 4 * 2^4: five levels; 65:
    one more, one pair of leaves on the last), an object of min_faces - 1 and of min_faces faces."""
    rng = np.random.default_rng(100 + T)
    mesh = soup(rng, T, spread=0.8, size=0.06)
    s, d = sphere_rays(rng, 1024)
    aim = mesh[0].reshape(T, 3, 3).mean(1)[rng.integers(T, size=512)]  # half of the rays at face centroids
    d[:512] = (aim + rng.uniform(-0.01, 0.01, (512, 3)) - s[:512]).astype(np.float32)
    scene(gpu, [(mesh, true_box(mesh))], lights=False)
    info, hits = forms(gpu, rays_array(s, d), min_faces, f"T={T}", want_rgb=False, expect={"objects": objects})
    if objects:
        assert info["faces"] == T and info["unculled_faces"] == 0
        bound = 1
        while 4 << (bound - 1) < T:
            bound += 1
        assert info["max_depth"] == bound, info
    else:
        assert info["nodes"] == 0 and info["device_bytes"] == 0
    assert (hits["object"] >= 0).sum() >= 100
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 3. order and ties --------
def test_smallest_index_wins_with_compaction(gpu, sphere3000):
    """The sphere with its face order reversed, and 600 faces crowded into a small volume (culled
    and unculled faces mixed: the compaction's order) so that a ray passes many of them."""
    A = sphere3000
    rev = tuple(x[::-1].copy() for x in A["mesh"])
    rays = rays_array(A["start"][:2048], A["raw"][:2048])
    scene(gpu, [(rev, A["box"])], lights=False)
    _, hits = forms(gpu, rays, 0, "reversed sphere", want_rgb=False, expect={"objects": 1, "unculled_faces": 0})
    assert (hits["object"] >= 0).sum() >= 500
    rng = np.random.default_rng(33)
    crowd = soup(rng, 600, spread=0.25, size=0.15)
    s, d = sphere_rays(rng, 2048)
    d = (np.float32(rng.uniform(-0.3, 0.3, (2048, 3))) - s).astype(np.float32)  # targets in the crowded volume
    assert (passing_faces_f64(crowd[0], s, d) >= 5).sum() >= 500  # many faces pass per ray
    scene(gpu, [(crowd, true_box(crowd))], lights=False)
    info, hits = forms(gpu, rays_array(s, d), 0, "crowded soup", want_rgb=False, expect={"objects": 1})
    assert 0 < info["unculled_faces"] < 300 and info["nodes"] > 0
    assert (hits["object"] >= 0).sum() >= 500


def test_tied_keys_and_a_flat_axis(gpu):
    """256 faces in groups of 8 on one triangle each (vertices rotated, b and c swapped, and exact
    copies: equal centroids, equal Morton keys, the index decides), and a planar mesh whose
    centroids have no extent in z (that axis' code is 0)."""
    rng = np.random.default_rng(44)
    base = soup(rng, 32, spread=0.8, size=0.25)[0].reshape(32, 3, 3)
    perms = [(0, 1, 2), (1, 2, 0), (2, 0, 1), (0, 2, 1), (2, 1, 0), (1, 0, 2), (0, 1, 2), (1, 2, 0)]
    pos = np.stack([base[g][list(p)] for g in range(32) for p in perms]).reshape(256, 9).astype(np.float32)
    tied = (pos, rng.normal(size=(256, 9)).astype(np.float32), rng.uniform(0, 1, (256, 6)).astype(np.float32))
    s, d = sphere_rays(rng, 2048)
    aim = pos.reshape(256, 3, 3).mean(1)[rng.integers(256, size=1024)]
    d[:1024] = (aim + rng.uniform(-0.02, 0.02, (1024, 3)) - s[:1024]).astype(np.float32)
    scene(gpu, [(tied, true_box(tied))], lights=False)
    info, hits = forms(gpu, rays_array(s, d), 1, "tied centroids", want_rgb=False, expect={"objects": 1, "faces": 256})
    assert info["nodes"] > 0 and (hits["object"] >= 0).sum() >= 300
    flat = soup(rng, 200, spread=0.8, size=0.2)
    flat[0].reshape(200, 3, 3)[:, :, 2] = np.float32(0.25)
    scene(gpu, [(flat, true_box(flat))], lights=False)
    info, hits = forms(gpu, rays_array(s, d), 1, "planar mesh", want_rgb=False, expect={"objects": 1, "faces": 200})
    assert info["nodes"] > 0 and (hits["object"] >= 0).sum() >= 100
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 4. no tree, no faces, no rays
def test_all_unculled_empty_scene_and_no_rays(gpu):
    rng = np.random.default_rng(8)
    big = soup(rng, 40, spread=1.0, size=3.0)  # |n| of the order of 10: no margin, every face unculled
    s, d = sphere_rays(rng, 1024)
    rays = rays_array(s, d)
    scene(gpu, [(big, true_box(big))])
    info, hits = forms(gpu, rays, 1, "all unculled", expect={"objects": 1, "faces": 40, "unculled_faces": 40, "nodes": 0,
                                                             "max_depth": 0})
    assert (hits["object"] >= 0).sum() >= 200
    assert gpu.check_ray_accel() == ""  # (root == kNoNode is what it requires of an object without a culled face)
    assert gpu.cast_rays(rays[:0]).shape == (0,)  # count == 0 with a device-built hierarchy
    gpu.scene_reset()
    info = gpu.build_ray_accel(device=True)
    assert info["objects"] == 0 and info["nodes"] == 0 and info["faces"] == 0 and info["device_bytes"] == 0
    hits = gpu.cast_rays(rays[:300])
    assert (hits["object"] == -1).all() and not hits["position"].view(np.uint32).any()
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 5. several objects -------
def test_several_objects_share_the_arrays(gpu, cube, sphere3000):
    """The cube, the sphere and a shifted copy with min_faces 0 (the cube keeps the tiles) and 1
    (three covered objects, the cube all unculled between the spheres' node and slot bases); then
    40 soups of 16 faces, every one covered."""
    A = sphere3000
    shift = np.float32([0.6, 0.1, -0.2])
    moved = ((A["mesh"][0].reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(np.float32), A["mesh"][1], A["mesh"][2])
    cube_box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    objects = [(A["mesh"], A["box"]), (cube, cube_box), (moved, true_box(moved))]
    scene(gpu, objects, centre=(0.5, 4.0, 1.0))
    rays = rays_array(A["start"], A["raw"])
    _, hits = forms(gpu, rays, 0, "mixed scene", normalize=(True,), expect={"objects": 2, "faces": 6000, "unculled_faces": 0})
    for k in range(3):
        assert (hits["object"] == k).sum() >= 50, k
    forms(gpu, rays, 1, "mixed scene, min_faces 1", normalize=(True,),
          expect={"objects": 3, "faces": 6012, "unculled_faces": 12})
    rng = np.random.default_rng(55)
    small = []
    for k in range(40):
        m = soup(rng, 16, spread=0.12, size=0.08)
        centre = np.float32([(k % 5 - 2) * 0.4, (k // 5 % 4 - 1.5) * 0.4, (k // 20 - 0.5) * 0.5])
        m = ((m[0].reshape(-1, 3, 3) + centre).reshape(-1, 9).astype(np.float32), m[1], m[2])
        small.append((m, true_box(m)))
    scene(gpu, small, lights=False)
    s, d = sphere_rays(rng, 2048)
    cents = np.concatenate([m[0].reshape(-1, 3, 3).mean(1) for m, _ in small])
    aim = cents[rng.integers(640, size=1024)]  # half of the rays at face centroids
    d[:1024] = (aim + rng.uniform(-0.01, 0.01, (1024, 3)) - s[:1024]).astype(np.float32)
    info, hits = forms(gpu, rays_array(s, d), 1, "40 soups of 16 faces", normalize=(True,), want_rgb=False,
                       expect={"objects": 40, "faces": 640, "max_depth": 3})
    assert info["nodes"] == 40 * 7 and len(np.unique(hits["object"][hits["object"] >= 0])) >= 20
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 6. a larger mesh ---------
def test_more_than_one_sort_block_and_workgroup(gpu):
    """displaced_sphere(20000, 42): 79 workgroups in the margin and key passes, a sort beyond one
    block, 14 levels."""
    rng = np.random.default_rng(66)
    mesh = sphere_mesh(20000)
    s, d = sphere_rays(rng, 8192)
    scene(gpu, [(mesh, true_box(mesh))], lights=False)
    info, hits = forms(gpu, rays_array(s, d), 0, "sphere 20000", normalize=(True,), want_rgb=False,
                       expect={"objects": 1, "faces": 20000, "unculled_faces": 0, "max_depth": 14})
    assert (hits["object"] >= 0).sum() >= 2000
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 7. lifecycle -------------
def test_lifecycle_of_a_device_build(gpu, sphere3000):
    A = sphere3000
    rng = np.random.default_rng(9)
    rays = rays_array(A["start"][:2048], A["raw"][:2048])
    small = soup(rng, 600, spread=0.9, size=0.1)
    scene(gpu, [(A["mesh"], A["box"])])
    brute1 = gpu.cast_rays(rays, normalize=True, brute_force=True)
    host = gpu.build_ray_accel()
    first = gpu.build_ray_accel(device=True)  # a build of either kind replaces the other
    assert first["objects"] == 1 and first["faces"] == 3000 and first["nodes"] == host["nodes"]
    assert gpu.check_ray_accel() == ""
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute1.tobytes()
    gpu.add_object(*small, *true_box(small))  # a geometry change: the hierarchy is gone, silently
    stale = gpu.cast_rays(rays, normalize=True)
    brute = gpu.cast_rays(rays, normalize=True, brute_force=True)
    assert stale.tobytes() == brute.tobytes() and stale.tobytes() != brute1.tobytes()
    second = gpu.build_ray_accel(device=True)
    assert second["objects"] == 2 and second["faces"] == 3600 and second["nodes"] > first["nodes"]
    assert gpu.check_ray_accel() == ""
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    again = gpu.build_ray_accel(device=True)  # twice: the same tree
    assert {k: again[k] for k in COUNTS} == {k: second[k] for k in COUNTS}
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    third = gpu.build_ray_accel(1000)  # the host build replaces the device build
    assert third["objects"] == 1 and third["nodes"] == first["nodes"]
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    gpu.build_ray_accel(device=True)
    gpu.drop_ray_accel()
    gpu.drop_ray_accel()  # (nothing to drop: still fine)
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    gpu.build_ray_accel(device=True)
    gpu.scene_reset()  # a reset drops it too
    assert (gpu.cast_rays(rays[:64])["object"] == -1).all()


def test_captured_cast_rays_with_a_device_built_hierarchy_replays(sphere3000):
    """As test_captured_cast_rays_with_a_hierarchy_replays (a fresh context on its own stream): the
    query against a device-built hierarchy is one kernel with no host round trip, captured into a
    graph and replayed twice."""
    import torch
    A = sphere3000
    st = torch.cuda.Stream()
    gpu = capi.Context(0)
    gpu.set_stream(st.cuda_stream)
    rays_h = rays_array(A["start"], A["raw"])
    n = rays_h.shape[0]
    scene(gpu, [(A["mesh"], A["box"])])
    rays = gpu.to_device(rays_h)
    hit, rgb = gpu.empty((n,), capi.HIT_DTYPE), gpu.empty((n, 3), np.float32)
    try:
        gpu.cast_rays_device(rays.ptr, n, hit.ptr, rgb.ptr, flags=capi.RAYS_NORMALIZE)  # tiles
        gpu.synchronize()
        want_hit, want_rgb = hit.numpy(), rgb.numpy()
        assert (want_hit["object"] >= 0).sum() >= 1000
        assert gpu.build_ray_accel(device=True)["objects"] == 1
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            gpu.cast_rays_device(rays.ptr, n, hit.ptr, rgb.ptr, flags=capi.RAYS_NORMALIZE)
        for replay in range(2):
            gpu.memset(hit.ptr, 0xFF, hit.nbytes)
            gpu.memset(rgb.ptr, 0xFF, rgb.nbytes)
            gpu.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert hit.numpy().tobytes() == want_hit.tobytes(), f"replay {replay}: records"
            assert rgb.numpy().tobytes() == want_rgb.tobytes(), f"replay {replay}: rgb"
    finally:
        for a in (rays, hit, rgb):
            a.free()
        gpu.close()
