"""GPU parity of the ray-query hierarchy (eray_scene_build_ray_accel; rays.hip rays_accel_kernel,
accel_walk.hpp, accel_build.hpp): with a hierarchy eray_cast_rays returns the records it returns
without one — the first face BY INDEX that passes Triangle::intersects in f32 (object.rs:63-78),
with the same u, v, t bits.

Bar: byte equality of whole record arrays (and of out_rgb) between the hierarchy, the LDS tiles
(before the build, or after a drop) and ERAY_RAYS_BRUTE_FORCE; for the mixed scene also the
oracle's records (oracle.cast_rays: Object::intersects per object and cast_ray's selection)."""
import numpy as np
import pytest

from eray_amd import capi, meshgen
from tests import ray_refs as R
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu


def assert_hits_equal(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(got["object"], want["object"]), f"{what}: object"
    assert np.array_equal(got["face"], want["face"]), f"{what}: face"
    for name in ("position", "normal", "uv", "u", "v"):
        assert_bit_equal(got[name], want[name], f"{what}: {name}")


# ------------------------------------------------------------------ inputs -------------------
def soup(rng, T, spread=1.0, size=0.2):
    centre = rng.uniform(-spread, spread, (T, 1, 3))
    pos = (centre + rng.uniform(-size, size, (T, 3, 3))).reshape(T, 9).astype(np.float32)
    nrm = rng.normal(size=(T, 9)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (T, 6)).astype(np.float32)
    return pos, nrm, uv


def sphere_rays(rng, n):
    """n rays from the radius-3 sphere toward targets uniform in [-1, 1]^3 (dir not normalised)."""
    v = rng.normal(size=(n, 3))
    start = (3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    target = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    return start, (target - start).astype(np.float32)


def rays_array(start, d):
    return np.ascontiguousarray(np.concatenate([start, d], axis=1), np.float32)


def sphere_mesh(T, seed=42):
    v, n, t, F, _, _ = meshgen.displaced_sphere(T, seed)
    return (v[F].reshape(T, 9).astype(np.float32), n[F].reshape(T, 9).astype(np.float32),
            t[F].reshape(T, 6).astype(np.float32))


def true_box(mesh):
    p = mesh[0].reshape(-1, 3)
    return tuple(p.min(0)), tuple(p.max(0))


def adversarial_rays(rng, pos):
    """Rays built from the mesh's own faces (computed in f64, stored as f32): within 1e-7 .. 1e-3 rad
    of a face's plane and through a point of it, along an edge, through a vertex, with one or two
    zero direction components, from a vertex's coordinate plane with that component zero; each at
    direction scales 1, 1e-3 and 1e3; then starts inside the mesh and non-finite components."""
    T = pos.shape[0]
    S, D = [], []
    for i in range(960):
        p = pos[rng.integers(T)].astype(np.float64)
        a, e1, e2 = p[0:3], p[3:6] - p[0:3], p[6:9] - p[0:3]
        n = np.cross(e1, e2)
        n /= np.linalg.norm(n)
        bu, bv = rng.uniform(0, 1, 2)
        if bu + bv > 1:
            bu, bv = 1 - bu, 1 - bv
        P = a + bu * e1 + bv * e2
        kind, scale = i % 8, (1.0, 1e-3, 1e3)[(i // 8) % 3]
        if kind <= 2:
            ang = (1e-7, 1e-6, 1e-5, 1e-4, 1e-3)[(i // 24) % 5] * (-1.0 if kind == 2 else 1.0)
            t = rng.uniform(0, 1) * e1 + rng.uniform(0, 1) * e2
            t /= np.linalg.norm(t)
            d = np.cos(ang) * t - np.sin(ang) * n
            s = P - rng.uniform(0.5, 3.0) * d
        elif kind == 3:
            d = e1 / np.linalg.norm(e1)
            s = a - rng.uniform(0.5, 3.0) * d
        elif kind == 4:
            v = rng.normal(size=3)
            s = 3.0 * v / np.linalg.norm(v)
            d = a + e1 - s
        elif kind == 5:
            d = rng.choice([-1.0, 1.0], 3)
            d[rng.integers(3)] = 0.0
            if i % 16 >= 8:
                d[rng.integers(3)] = 0.0
            s = P - 2.5 * d
        elif kind == 6:
            ax = rng.integers(3)
            d = rng.uniform(-1, 1, 3)
            d[ax] = 0.0
            s = P - 3.0 * d
            s[ax] = a[ax]
        else:
            v = rng.normal(size=3)
            s = 1e3 * v / np.linalg.norm(v)
            d = (P - s) / 1e3
        S.append(s)
        D.append(d * scale)
    S.extend(rng.uniform(-0.3, 0.3, (200, 3)))  # starts inside the mesh
    D.extend(rng.normal(size=(200, 3)))
    for k, bad in enumerate((np.nan, np.inf, -np.inf)):
        for j in range(6):
            s, d = np.array([0.1, 0.2, 3.0]), np.array([0.01, -0.02, -1.0])
            (s if j < 3 else d)[j % 3] = bad
            S.append(s)
            D.append(d)
    S.append(np.array([0.0, 0.0, 3.0]))
    D.append(np.zeros(3))
    return np.float32(S), np.float32(D)


@pytest.fixture(scope="module")
def sphere3000():
    rng = np.random.default_rng(21)
    mesh = sphere_mesh(3000)
    s0, d0 = sphere_rays(rng, 4096)
    s1, d1 = adversarial_rays(rng, mesh[0])
    return {"mesh": mesh, "box": true_box(mesh), "start": np.concatenate([s0, s1]), "raw": np.concatenate([d0, d1])}


def scene(gpu, objects, centre=(0.0, 0.0, 5.0), lights=True):
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera(centre, (60.0, 60.0), 64, 1.0))
    for mesh, (lo, hi) in objects:
        gpu.add_object(*mesh, tuple(lo), tuple(hi))
    if lights:
        gpu.add_light(capi.make_light((1.0, 1.0, 2.0), "point"))
        gpu.add_light(capi.make_light((0.0, 2.0, 0.0), "ambient", brightness=0.2))


def three_forms(gpu, rays, min_faces, what, normalize=(False, True), object=-1, want_rgb=True, expect=None):
    """Tiles (no hierarchy), brute force and the hierarchy, byte for byte; returns the build's info
    and the records of the last `normalize`."""
    gpu.drop_ray_accel()
    rgb_now = want_rgb and object < 0  # (out_rgb has no single-object form)
    before = {}
    for nz in normalize:
        tiles = gpu.cast_rays(rays, normalize=nz, object=object, want_rgb=rgb_now)
        brute = gpu.cast_rays(rays, normalize=nz, object=object, want_rgb=rgb_now, brute_force=True)
        before[nz] = (tiles, brute)
    info = gpu.build_ray_accel(min_faces)
    if expect is not None:
        for k, v in expect.items():
            assert info[k] == v, (what, k, info)
    for nz in normalize:
        tiles, brute = before[nz]
        tree = gpu.cast_rays(rays, normalize=nz, object=object, want_rgb=rgb_now)
        brute2 = gpu.cast_rays(rays, normalize=nz, object=object, want_rgb=rgb_now, brute_force=True)
        for name, other in (("tiles", tiles), ("brute force", brute), ("brute force after the build", brute2)):
            if rgb_now:
                assert_hits_equal(tree[0], other[0], f"{what} normalize={nz}: hierarchy vs {name}")
                assert tree[0].tobytes() == other[0].tobytes(), f"{what} normalize={nz}: records vs {name}"
                assert tree[1].tobytes() == other[1].tobytes(), f"{what} normalize={nz}: out_rgb vs {name}"
            else:
                assert_hits_equal(tree, other, f"{what} normalize={nz}: hierarchy vs {name}")
                assert tree.tobytes() == other.tobytes(), f"{what} normalize={nz}: records vs {name}"
    return info, (tree[0] if rgb_now else tree)


# ------------------------------------------------------------------ 1. the three forms -------
def test_three_forms_are_byte_equal(gpu, sphere3000):
    """displaced_sphere(3000, 42) with its true box as the only object: 4096 sphere rays, the
    adversarial set and 200 starts inside the mesh, stored and normalised directions."""
    A = sphere3000
    scene(gpu, [(A["mesh"], A["box"])])
    rays = rays_array(A["start"], A["raw"])
    expect = {"objects": 1, "faces": 3000, "unculled_faces": 0}
    info, hits = three_forms(gpu, rays, 0, "sphere 3000, object -1", expect=expect)
    assert info["nodes"] >= 3000 // 4 and 10 <= info["max_depth"] <= 11 and info["device_bytes"] > 48 * 3000
    hit = hits["object"][:4096] >= 0
    assert hit.sum() >= 1000 and (~hit).sum() >= 500
    assert (hits["object"][4096:4096 + 960] >= 0).sum() >= 100  # adversarial rays that hit
    three_forms(gpu, rays, 0, "sphere 3000, object 0", object=0, expect=expect)
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 2. index order -----------
def passing_faces_f64(pos, start, d):
    """How many faces each ray passes (Moller-Trumbore in f64, front faces): a condition of test 2
    on its own input, not a reference."""
    p = pos.astype(np.float64).reshape(-1, 3, 3)
    a, e1, e2 = p[:, 0], p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]
    n = np.cross(e1, e2)
    s, d = start.astype(np.float64), d.astype(np.float64)
    det = -(d @ n.T)
    ao = s[:, None, :] - a[None]
    dao = np.cross(ao, d[:, None, :])
    with np.errstate(divide="ignore", invalid="ignore"):
        u = (dao * e2[None]).sum(-1) / det
        v = -(dao * e1[None]).sum(-1) / det
        t = (ao * n[None]).sum(-1) / det
    return ((det > 1e-6) & (u >= 0) & (v >= 0) & (u + v <= 1) & (t >= 0)).sum(1)


def test_smallest_index_wins(gpu, sphere3000):
    """The sphere with its face order reversed, and 600 faces crowded into a small volume so that a
    ray passes many of them: the smallest passing index is returned, as by the tiles."""
    A = sphere3000
    rev = tuple(x[::-1].copy() for x in A["mesh"])
    rays = rays_array(A["start"][:2048], A["raw"][:2048])
    scene(gpu, [(rev, A["box"])], lights=False)
    _, hits = three_forms(gpu, rays, 0, "reversed sphere", want_rgb=False, expect={"objects": 1, "unculled_faces": 0})
    scene(gpu, [(A["mesh"], A["box"])], lights=False)
    fwd = gpu.cast_rays(rays, normalize=True)
    both = (hits["object"] >= 0) & (fwd["object"] >= 0)
    assert both.sum() >= 500 and (hits["face"][both] != 2999 - fwd["face"][both]).sum() >= 50  # not just relabelled
    rng = np.random.default_rng(33)
    crowd = soup(rng, 600, spread=0.25, size=0.15)
    s, d = sphere_rays(rng, 2048)
    d = (np.float32(rng.uniform(-0.3, 0.3, (2048, 3))) - s).astype(np.float32)  # targets in the crowded volume
    many = passing_faces_f64(crowd[0], s, d)
    assert (many >= 5).sum() >= 500  # many faces pass per ray
    scene(gpu, [(crowd, true_box(crowd))], lights=False)
    info, hits = three_forms(gpu, rays_array(s, d), 0, "crowded soup", want_rgb=False, expect={"objects": 1})
    assert info["unculled_faces"] < 300 and info["nodes"] > 0
    assert (hits["object"] >= 0).sum() >= 500


# ------------------------------------------------------------------ 3. mixed scene -----------
def test_mixed_scene_selects_by_the_cameras_centre(gpu, oracle, cube, sphere3000):
    """The cube (below min_faces: LDS tiles), the sphere and a shifted copy (hierarchies), object =
    -1: records equal the pre-build ones, and on every ray the oracle's (each object alone, the
    selection of engine.rs:116-126 restated in numpy over those, and the oracle's own selection)."""
    A = sphere3000
    centre = (0.5, 4.0, 1.0)
    shift = np.float32([0.6, 0.1, -0.2])
    moved = ((A["mesh"][0].reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(np.float32), A["mesh"][1], A["mesh"][2])
    cube_box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    objects = [(cube, cube_box), (A["mesh"], A["box"]), (moved, true_box(moved))]
    scene(gpu, objects, centre=centre)
    rays = rays_array(A["start"], A["raw"])
    info, hits = three_forms(gpu, rays, 0, "mixed scene", normalize=(True,),
                             expect={"objects": 2, "faces": 6000, "unculled_faces": 0})
    for k in range(3):
        assert (hits["object"] == k).sum() >= 50, k
    s = oracle.Scene()
    for m, (lo, hi) in objects:
        s.add_object(*m, tuple(lo), tuple(hi))
    cam = oracle.camera(centre, (60.0, 60.0), 64, 1.0)
    per = [oracle.cast_rays(s, cam, rays, normalize=True, object=k) for k in range(3)]
    want = R.closest_by_centre(per, centre)
    R.assert_records_equal(oracle.cast_rays(s, cam, rays, normalize=True), want, "the oracle's selection and the numpy one")
    R.assert_records_equal(gpu.cast_rays(rays, normalize=True).view(oracle.HIT_DTYPE), want, "mixed scene vs the oracle")
    for k in range(3):
        R.assert_records_equal(gpu.cast_rays(rays, normalize=True, object=k).view(oracle.HIT_DTYPE), per[k], f"object {k} vs the oracle")
    # the cube among the hierarchies (every face unculled) changes nothing
    three_forms(gpu, rays, 1, "mixed scene, min_faces 1", normalize=(True,),
                expect={"objects": 3, "faces": 6012, "unculled_faces": 12})
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 4. tree boundaries -------
@pytest.mark.parametrize("T, min_faces, objects", [(15, 16, 0), (16, 16, 1), (1, 1, 1), (5, 1, 1), (9, 1, 1), (64, 1, 1),
                                                  (65, 1, 1), (257, 0, 0), (512, 0, 1), (513, 0, 1)])
def test_tree_boundaries(gpu, T, min_faces, objects):
    """Objects of min_faces - 1 and min_faces faces (explicit and the default 512), single-face and
    odd leaves, counts on a depth boundary (64 = 4 * 2^4: five levels; 65: one more)."""
    rng = np.random.default_rng(100 + T)
    mesh = soup(rng, T, spread=0.8, size=0.06)
    s, d = sphere_rays(rng, 1024)
    aim = mesh[0].reshape(T, 3, 3).mean(1)[rng.integers(T, size=512)]  # half of the rays at face centroids
    d[:512] = (aim + rng.uniform(-0.01, 0.01, (512, 3)) - s[:512]).astype(np.float32)
    scene(gpu, [(mesh, true_box(mesh))], lights=False)
    info, hits = three_forms(gpu, rays_array(s, d), min_faces, f"T={T}", want_rgb=False, expect={"objects": objects})
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


def test_all_unculled_empty_scene_and_no_rays(gpu):
    rng = np.random.default_rng(8)
    big = soup(rng, 40, spread=1.0, size=3.0)  # |n| of the order of 10: no margin, every face unculled
    s, d = sphere_rays(rng, 1024)
    rays = rays_array(s, d)
    scene(gpu, [(big, true_box(big))])
    info, hits = three_forms(gpu, rays, 1, "all unculled", expect={"objects": 1, "faces": 40, "unculled_faces": 40, "nodes": 0})
    assert (hits["object"] >= 0).sum() >= 200
    assert gpu.cast_rays(rays[:0]).shape == (0,)  # count == 0 with a hierarchy
    gpu.scene_reset()
    info = gpu.build_ray_accel()
    assert info["objects"] == 0 and info["nodes"] == 0 and info["faces"] == 0 and info["device_bytes"] == 0
    hits = gpu.cast_rays(rays[:300])
    assert (hits["object"] == -1).all() and not hits["position"].view(np.uint32).any()
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 5. invalidation ----------
def test_geometry_changes_drop_the_hierarchy(gpu, sphere3000):
    A = sphere3000
    rng = np.random.default_rng(9)
    rays = rays_array(A["start"][:2048], A["raw"][:2048])
    small = soup(rng, 600, spread=0.9, size=0.1)
    scene(gpu, [(A["mesh"], A["box"])])
    first = gpu.build_ray_accel()
    assert first["objects"] == 1 and first["faces"] == 3000
    gpu.add_light(capi.make_light((-2.0, 1.0, 1.0), "point"))  # lights, materials, camera: kept
    gpu.set_camera(capi.make_camera((0.0, 1.0, 5.0), (60.0, 60.0), 64, 1.0))
    one = gpu.cast_rays(rays, normalize=True)
    gpu.add_object(*small, *true_box(small))  # a geometry change: the hierarchy is gone, silently
    stale = gpu.cast_rays(rays, normalize=True)
    brute = gpu.cast_rays(rays, normalize=True, brute_force=True)
    assert stale.tobytes() == brute.tobytes()
    assert (stale["object"] == 1).sum() >= 20 and stale.tobytes() != one.tobytes()
    second = gpu.build_ray_accel()
    assert second["objects"] == 2 and second["faces"] == 3600 and second["nodes"] > first["nodes"]
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    third = gpu.build_ray_accel(1000)  # a second build replaces the first
    assert third["objects"] == 1 and third["faces"] == 3000 and third["nodes"] == first["nodes"]
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    gpu.drop_ray_accel()
    gpu.drop_ray_accel()  # (nothing to drop: still fine)
    assert gpu.cast_rays(rays, normalize=True).tobytes() == brute.tobytes()
    gpu.build_ray_accel()
    gpu.scene_reset()  # a reset drops it too
    assert (gpu.cast_rays(rays[:64])["object"] == -1).all()


# ------------------------------------------------------------------ 6. graph capture ---------
def test_captured_cast_rays_with_a_hierarchy_replays(sphere3000):
    """eray_cast_rays with a hierarchy still enqueues one kernel and makes no host round trip: it
    is captured into a graph on the context's stream and replayed twice."""
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
        assert gpu.build_ray_accel()["objects"] == 1
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
