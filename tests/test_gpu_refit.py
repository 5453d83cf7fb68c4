"""GPU parity of eray_scene_refit_ray_accel (accel_dev.hip accel_refit_device): after
eray_scene_update_object moved an object, the refit keeps the device build's topology and rewrites
every margin, box, min_index and record copy — queries return the first passing face by index with
the same u, v, t bits as brute force, the LDS tiles and a fresh device build.

Bar: byte equality of whole record arrays and of out_rgb; eray_debug_ray_accel_check accepts the
refitted tree; the counts are the build's.  Meshes and rays are those of tests/test_gpu_rays_accel.py."""
import numpy as np
import pytest

from tests.test_gpu_rays_accel import adversarial_rays, rays_array, scene, soup, sphere_mesh, sphere_rays, true_box
from tests.test_gpu_rays_accel_dev import COUNTS

pytestmark = pytest.mark.gpu


def displaced(mesh, frac=0.03, radius=1.0):
    """A smooth displacement of `frac` of the mesh radius, per vertex position."""
    p = mesh[0].astype(np.float64).reshape(-1, 3)
    q = p + frac * radius * np.sin(2.5 * p[:, [1, 2, 0]] + 0.3)
    return q.reshape(-1, 9).astype(np.float32), mesh[1], mesh[2]


def casts(gpu, rays, want_rgb=True, **kw):
    """The records (and sums) with stored and with normalised directions, as bytes."""
    out = b""
    for nz in (False, True):
        r = gpu.cast_rays(rays, normalize=nz, want_rgb=want_rgb, **kw)
        out += (r[0].tobytes() + r[1].tobytes()) if want_rgb else r.tobytes()
    return out


def update(gpu, index, mesh, device=True):
    held = [gpu.to_device(a) for a in mesh] if device else list(mesh)
    try:
        gpu.update_object(index, positions=held[0], bbox=true_box(mesh))
        gpu.synchronize()
    finally:
        if device:
            for a in held:
                a.free()


def refit_equals_everything(gpu, rays, min_faces, what, want_rgb=True, refitted=1):
    """With the hierarchy just invalidated by an update: the queries run without it; the refit keeps
    the topology; its tree passes the checker and answers as brute force, the tiles and a fresh
    device build do.  Returns the refit's info."""
    brute = casts(gpu, rays, want_rgb, brute_force=True)
    assert casts(gpu, rays, want_rgb) == brute, f"{what}: between the update and the refit"
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 0 and info["refitted"] == refitted, (what, info)
    assert gpu.check_ray_accel() == "", what
    tree = casts(gpu, rays, want_rgb)
    assert tree == brute, f"{what}: the refitted tree vs brute force"
    built = gpu.build_ray_accel(min_faces, device=True)
    for k in COUNTS:
        assert info[k] == built[k], (what, k, info, built)
    assert casts(gpu, rays, want_rgb) == tree, f"{what}: vs a fresh device build"
    gpu.drop_ray_accel()
    assert casts(gpu, rays, want_rgb) == tree, f"{what}: vs the tiles"
    return info


@pytest.fixture(scope="module")
def moving_sphere():
    rng = np.random.default_rng(21)
    mesh = sphere_mesh(3000)
    new = displaced(mesh)
    s0, d0 = sphere_rays(rng, 4096)
    s1, d1 = adversarial_rays(rng, new[0])
    return {"mesh": mesh, "new": new, "rays": rays_array(np.concatenate([s0, s1]), np.concatenate([d0, d1]))}


# ------------------------------------------------------------------ 6. the topology is kept
def test_refit_keeps_the_topology_on_the_sphere(gpu, moving_sphere):
    A = moving_sphere
    scene(gpu, [(A["new"], true_box(A["new"]))])
    assert gpu.build_ray_accel()["unculled_faces"] == 0  # (the independent builder, on the new geometry)
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    first = gpu.build_ray_accel(device=True)
    old = casts(gpu, A["rays"])
    update(gpu, 0, A["new"])
    info = refit_equals_everything(gpu, A["rays"], 0, "sphere 3000")
    for k in COUNTS:
        assert info[k] == first[k], (k, info, first)
    hits = gpu.cast_rays(A["rays"][:4096], normalize=True)
    assert (hits["object"] >= 0).sum() >= 1000 and (hits["object"] < 0).sum() >= 500
    assert casts(gpu, A["rays"]) != old


@pytest.mark.parametrize("T", [1, 4, 5, 65, 513])
def test_refit_at_leaf_and_level_boundaries(gpu, T):
    rng = np.random.default_rng(100 + T)
    mesh = soup(rng, T, spread=0.8, size=0.06)
    new = displaced(mesh, 0.05)
    s, d = sphere_rays(rng, 1024)
    aim = new[0].reshape(T, 3, 3).mean(1)[rng.integers(T, size=512)]  # half of the rays at face centroids
    d[:512] = (aim + rng.uniform(-0.01, 0.01, (512, 3)) - s[:512]).astype(np.float32)
    rays = rays_array(s, d)
    scene(gpu, [(mesh, true_box(mesh))])  # (with lights: out_rgb's shadow rays search the refitted tree too)
    first = gpu.build_ray_accel(1, device=True)
    assert first["objects"] == 1 and first["unculled_faces"] == 0
    update(gpu, 0, new)
    info = refit_equals_everything(gpu, rays, 1, f"T={T}")
    assert info["nodes"] == first["nodes"] and info["max_depth"] == first["max_depth"]
    assert (gpu.cast_rays(rays, normalize=True)["object"] >= 0).sum() >= 100


def test_refit_of_the_middle_of_three_covered_objects(gpu, cube, moving_sphere):
    """The mixed scene — the sphere, the cube (every face unculled, between the spheres' node and slot
    bases) and a shifted sphere, all covered with min_faces 1 — with only the cube updated."""
    A = moving_sphere
    shift = np.float32([0.6, 0.1, -0.2])
    far = ((A["mesh"][0].reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(np.float32), A["mesh"][1], A["mesh"][2])
    cube2 = ((cube[0].reshape(-1, 3, 3) * np.float32(1.125) + np.float32([0.25, -0.125, 0.0])).reshape(-1, 9).astype(np.float32),
             cube[1], cube[2])
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))

    def objects(c):
        return [(A["mesh"], true_box(A["mesh"])), (c, box if c is cube else true_box(c)), (far, true_box(far))]

    rays = A["rays"][:4096]
    scene(gpu, objects(cube2), centre=(0.5, 4.0, 1.0))
    assert gpu.build_ray_accel(1)["unculled_faces"] == 12  # (the independent builder, on the new geometry)
    scene(gpu, objects(cube), centre=(0.5, 4.0, 1.0))
    first = gpu.build_ray_accel(1, device=True)
    assert first["objects"] == 3 and first["faces"] == 6012 and first["unculled_faces"] == 12
    old = casts(gpu, rays)
    update(gpu, 1, cube2)
    info = refit_equals_everything(gpu, rays, 1, "mixed scene", refitted=3)
    for k in COUNTS:
        assert info[k] == first[k], (k, info, first)
    hits = gpu.cast_rays(rays, normalize=True)
    for k in range(3):
        assert (hits["object"] == k).sum() >= 50, k
    assert casts(gpu, rays) != old


# ------------------------------------------------------------------ 7. the refit falls back
def test_a_class_change_rebuilds(gpu, moving_sphere):
    """(a) one face of the updated sphere scaled about its centroid until |n|1 >= 4: it has no
    provable margin any more, the unculled list would change, so the call rebuilds."""
    A = moving_sphere
    pos = A["new"][0].astype(np.float64).reshape(-1, 3, 3).copy()
    c = pos[7].mean(0)
    pos[7] = c + (pos[7] - c) * 40.0
    big = (pos.reshape(-1, 9).astype(np.float32), A["new"][1], A["new"][2])
    e1, e2 = pos[7, 1] - pos[7, 0], pos[7, 2] - pos[7, 0]
    assert np.abs(np.cross(e1, e2)).sum() >= 4.0
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    assert gpu.build_ray_accel(device=True)["unculled_faces"] == 0
    update(gpu, 0, big)
    brute = casts(gpu, A["rays"], brute_force=True)
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["refitted"] == 0 and info["unculled_faces"] == 1 and info["objects"] == 1, info
    assert gpu.check_ray_accel() == ""
    assert casts(gpu, A["rays"]) == brute
    # ... and back: the face becomes cullable again, the other direction of a class change
    update(gpu, 0, A["new"])
    brute = casts(gpu, A["rays"], brute_force=True)
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["unculled_faces"] == 0, info
    assert gpu.check_ray_accel() == "" and casts(gpu, A["rays"]) == brute
    gpu.drop_ray_accel()


def test_an_object_below_min_faces_added_since_the_build_rebuilds(gpu, moving_sphere):
    """(c) with an object the hierarchy does not cover: the covered objects, their places and face
    counts are the build's, but the per-object records were sized for the build's scene — the refit
    must rebuild, and queries (which read a record per object) equal brute force.  The same after a
    reset that re-adds the covered mesh with more small objects."""
    A = moving_sphere
    rays = A["rays"][:2048]
    rng = np.random.default_rng(12)

    def small(k):
        m = soup(rng, 40, spread=0.3, size=0.3)
        return ((m[0].reshape(-1, 3, 3) + np.float32([1.2 * k - 1.8, 0.4, 0.2])).reshape(-1, 9).astype(np.float32), m[1], m[2])

    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    first = gpu.build_ray_accel(device=True)
    assert first["objects"] == 1
    extra = [small(k) for k in range(4)]
    gpu.add_object(*extra[0], *true_box(extra[0]))  # 40 faces < 512: not covered
    brute = casts(gpu, rays, brute_force=True)
    assert casts(gpu, rays) == brute
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["refitted"] == 0 and info["objects"] == 1 and info["faces"] == 3000, info
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == brute
    hits = gpu.cast_rays(rays, normalize=True)
    assert (hits["object"] == 1).sum() >= 20  # the added object is seen
    again = gpu.refit_ray_accel()  # two objects at the build and now: kept
    assert again["rebuilt"] == 0 and again["refitted"] == 1, again
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))] + [(m, true_box(m)) for m in extra])  # reset, 5 objects
    brute = casts(gpu, rays, brute_force=True)
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["objects"] == 1, info
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == brute
    gpu.drop_ray_accel()


def test_host_builds_new_objects_and_no_change(gpu, moving_sphere):
    A = moving_sphere
    rays = A["rays"][:2048]
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    host = gpu.build_ray_accel()
    update(gpu, 0, A["new"], device=False)
    brute = casts(gpu, rays, brute_force=True)
    info = gpu.refit_ray_accel()  # (b) after a host build: a device build
    assert info["rebuilt"] == 1 and info["refitted"] == 0 and info["nodes"] == host["nodes"], info
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == brute
    again = gpu.refit_ray_accel()  # (d) nothing changed: the topology is kept, the same results
    assert again["rebuilt"] == 0 and again["refitted"] == 1, again
    for k in COUNTS:
        assert again[k] == info[k], (k, again, info)
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == brute
    small = soup(np.random.default_rng(9), 600, spread=0.9, size=0.1)
    gpu.add_object(*small, *true_box(small))
    brute = casts(gpu, rays, brute_force=True)
    info = gpu.refit_ray_accel()  # (c) the covered set changed
    assert info["rebuilt"] == 1 and info["objects"] == 2 and info["faces"] == 3600, info
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == brute
    gpu.update_object(0, normals=A["new"][1] * np.float32(0.5))  # normals alone: the hierarchy stays valid
    assert gpu.check_ray_accel() == ""
    brute = casts(gpu, rays, brute_force=True)
    assert casts(gpu, rays) == brute
    gpu.drop_ray_accel()
