"""GPU parity of the refits of a HOST-built ray-query hierarchy (eray_scene_build_ray_accel_refittable;
accel_dev.hip's refit kernels in their recursion-order instantiation): the build is the host build
byte for byte; a refit of unmoved geometry reproduces it; a refit of moved geometry keeps the host
split's topology and answers as brute force and the tiles do; fallbacks stay on the host builder; the
async refit runs on the stream and inside a graph; the plain host build behaves as before.

Bar: byte equality of the hierarchy's four device arrays, of whole record arrays and of out_rgb.
Meshes, rays and helpers are those of tests/test_gpu_rays_accel.py, test_gpu_refit.py and
test_gpu_refit_async.py."""
import numpy as np
import pytest

from eray_amd import capi
from tests.test_gpu_rays_accel import rays_array, scene, soup, sphere_rays, true_box
from tests.test_gpu_rays_accel_dev import COUNTS
from tests.test_gpu_refit import casts, displaced, moving_sphere, update  # noqa: F401 (moving_sphere: a fixture)
from tests.test_gpu_refit_async import PREFIX, WIDE, Replayed, brute_answers, other, same_arrays, targets_of  # noqa: F401 (other: a fixture)

pytestmark = pytest.mark.gpu

# 1: one leaf; 4, 5: a full leaf and one face more; 9, 13: halves whose subtrees differ in node count (a
# second child that is not the first's id + 1); 65: a level more; 513: a pairs level inside the one-launch
# kernel; "sphere": 3,000 faces, full = 10, so levels 9 and 10 run as launches of their own below it
SIZES = [1, 4, 5, 9, 13, 65, 513, "sphere"]


def case(A, size):
    """(mesh, moved mesh, rays, min_faces) of one size."""
    if size == "sphere":
        return A["mesh"], displaced(A["mesh"], 0.05), A["rays"], 1
    T = size
    rng = np.random.default_rng(100 + T)
    mesh = soup(rng, T, spread=0.8, size=0.06)
    new = displaced(mesh, 0.05)
    s, d = sphere_rays(rng, 1024)
    aim = new[0].reshape(T, 3, 3).mean(1)[rng.integers(T, size=512)]  # half of the rays at face centroids
    d[:512] = (aim + rng.uniform(-0.01, 0.01, (512, 3)) - s[:512]).astype(np.float32)
    return mesh, new, rays_array(s, d), 1


def index_words(arrays):
    """left, right, min_index, right_min of every node: they depend on face indices alone."""
    return np.frombuffer(arrays["nodes"], np.uint32).reshape(-1, 12)[:, 8:12].tobytes()


# ------------------------------------------------------------------ 1. the build is the host build
@pytest.mark.parametrize("size", [9, "sphere"])
def test_refittable_build_is_the_host_build_byte_for_byte(gpu, moving_sphere, size):
    mesh, _, rays, min_faces = case(moving_sphere, size)
    scene(gpu, [(mesh, true_box(mesh))])
    plain = gpu.build_ray_accel(min_faces)
    want = gpu.ray_accel_arrays()
    tree = casts(gpu, rays)
    info = gpu.build_ray_accel(min_faces, refittable=True)
    for k in COUNTS:
        assert info[k] == plain[k], (k, info, plain)
    same_arrays(gpu.ray_accel_arrays(), want, f"{size}: refittable vs plain host build")
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == tree
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 2. unmoved geometry: the refit is the build
@pytest.mark.parametrize("size", SIZES)
def test_refit_of_unmoved_geometry_is_the_build(gpu, moving_sphere, size):
    mesh, _, _, min_faces = case(moving_sphere, size)
    scene(gpu, [(mesh, true_box(mesh))])
    first = gpu.build_ray_accel(min_faces, refittable=True)
    assert first["objects"] == 1 and first["unculled_faces"] == 0
    if size == "sphere":
        assert first["max_depth"] == 11  # levels 0 .. 10 complete
    want = gpu.ray_accel_arrays()
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 0 and info["refitted"] == 1, info
    for k in COUNTS:
        assert info[k] == first[k], (k, info, first)
    same_arrays(gpu.ray_accel_arrays(), want, f"{size}: the synchronous refit")
    if size in (513, "sphere"):  # the refit on the stream, its top levels in one launch and in a launch each
        try:
            for n, top in enumerate((True, False)):
                gpu.set_refit_top_levels(top)
                gpu.refit_ray_accel_async()
                st = gpu.refit_status()
                assert st["refits"] == n + 1 and st["kept"] == st["covered"] == 1 and st["fell_back"] == 0, (top, st)
                same_arrays(gpu.ray_accel_arrays(), want, f"{size}: the async refit, top levels {top}")
        finally:
            gpu.set_refit_top_levels(True)
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 3. moved geometry: the topology is kept
@pytest.mark.parametrize("size", SIZES)
def test_refit_of_moved_geometry_keeps_the_host_split(gpu, moving_sphere, size):
    mesh, new, rays, min_faces = case(moving_sphere, size)
    scene(gpu, [(mesh, true_box(mesh))])
    first = gpu.build_ray_accel(min_faces, refittable=True)
    built = gpu.ray_accel_arrays()
    old = casts(gpu, rays)
    update(gpu, 0, new)
    brute = casts(gpu, rays, brute_force=True)
    assert casts(gpu, rays) == brute, "between the update and the refit"
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 0 and info["refitted"] == 1, info
    for k in COUNTS:
        assert info[k] == first[k], (k, info, first)
    assert gpu.check_ray_accel() == ""
    got = gpu.ray_accel_arrays()
    assert got["index"] == built["index"] and index_words(got) == index_words(built)
    assert got["nodes"] != built["nodes"] and got["hot"] != built["hot"]  # (the refit did work)
    tree = casts(gpu, rays)
    assert tree == brute, "the refitted host tree vs brute force"
    assert tree != old
    hits = gpu.cast_rays(rays[:4096], normalize=True)
    if size == "sphere":
        assert (hits["object"] >= 0).sum() >= 1000 and (hits["object"] < 0).sum() >= 500
    else:
        assert (hits["object"] >= 0).sum() >= 100
    gpu.drop_ray_accel()
    assert casts(gpu, rays) == tree, "vs the tiles"


# ------------------------------------------------------------------ 4. non-zero bases in recursion order
def test_refit_of_the_middle_of_three_covered_objects(gpu, cube, moving_sphere):
    """The sphere, the cube (every face unculled, between the spheres' node and slot bases) and a shifted
    sphere, all covered with min_faces 1, with only the cube updated."""
    A = moving_sphere
    shift = np.float32([0.6, 0.1, -0.2])
    far = ((A["mesh"][0].reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(np.float32), A["mesh"][1], A["mesh"][2])
    cube2 = ((cube[0].reshape(-1, 3, 3) * np.float32(1.125) + np.float32([0.25, -0.125, 0.0])).reshape(-1, 9).astype(np.float32),
             cube[1], cube[2])
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    rays = A["rays"][:4096]
    scene(gpu, [(A["mesh"], true_box(A["mesh"])), (cube, box), (far, true_box(far))], centre=(0.5, 4.0, 1.0))
    first = gpu.build_ray_accel(1, refittable=True)
    assert first["objects"] == 3 and first["faces"] == 6012 and first["unculled_faces"] == 12
    built = gpu.ray_accel_arrays()
    old = casts(gpu, rays)
    update(gpu, 1, cube2)
    brute = casts(gpu, rays, brute_force=True)
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 0 and info["refitted"] == 3, info
    for k in COUNTS:
        assert info[k] == first[k], (k, info, first)
    assert gpu.check_ray_accel() == ""
    got = gpu.ray_accel_arrays()
    assert got["nodes"] == built["nodes"] and got["index"] == built["index"]  # (the spheres did not move; the cube has no node)
    assert got["hot"] != built["hot"]
    tree = casts(gpu, rays)
    assert tree == brute and tree != old
    hits = gpu.cast_rays(rays, normalize=True)
    for k in range(3):
        assert (hits["object"] == k).sum() >= 50, k
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 5. fallbacks keep the builder
def stays_host_split_and_refittable(gpu, min_faces, rays, what):
    """After a refit that had to rebuild: the arrays are the refittable host build's of the geometry as
    it stands, and a following refit keeps them."""
    brute = casts(gpu, rays, brute_force=True)
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == brute, what
    rebuilt = gpu.ray_accel_arrays()
    again = gpu.refit_ray_accel()
    assert again["rebuilt"] == 0 and again["refitted"] == again["objects"], (what, again)
    same_arrays(gpu.ray_accel_arrays(), rebuilt, f"{what}: the refit after the rebuild")
    gpu.build_ray_accel(min_faces, refittable=True)
    same_arrays(gpu.ray_accel_arrays(), rebuilt, f"{what}: vs a fresh refittable host build")


def test_fallbacks_rebuild_with_the_host_builder(gpu, moving_sphere):
    A = moving_sphere
    rays = A["rays"][:2048]
    pos = A["new"][0].astype(np.float64).reshape(-1, 3, 3).copy()
    c = pos[7].mean(0)
    pos[7] = c + (pos[7] - c) * 40.0  # one face scaled about its centroid until |n|1 >= 4: unculled
    assert np.abs(np.cross(pos[7, 1] - pos[7, 0], pos[7, 2] - pos[7, 0])).sum() >= 4.0
    big = (pos.reshape(-1, 9).astype(np.float32), A["new"][1], A["new"][2])
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    assert gpu.build_ray_accel(refittable=True)["unculled_faces"] == 0
    update(gpu, 0, big)
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["refitted"] == 0 and info["unculled_faces"] == 1 and info["objects"] == 1, info
    stays_host_split_and_refittable(gpu, 0, rays, "a class change")
    # an object added since the build (40 faces < 512: not covered, but the records were sized without it)
    small = soup(np.random.default_rng(12), 40, spread=0.3, size=0.3)
    gpu.add_object(*small, *true_box(small))
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["refitted"] == 0 and info["objects"] == 1 and info["faces"] == 3000, info
    stays_host_split_and_refittable(gpu, 0, rays, "an object added")
    gpu.refit_ray_accel_async()  # (and the stream's refit accepts it)
    st = gpu.refit_status()
    assert st["refits"] == 1 and st["kept"] == st["covered"] == 1, st
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 6. on the stream and in a graph
class ReplayedHostTree(Replayed):
    """tests/test_gpu_refit_async.py's Replayed with the hierarchy built by the refittable host build."""

    def __init__(self, objects, index, min_faces, rays_h, centre=(0.0, 0.0, 5.0)):
        import torch
        self.torch = torch
        self.st = torch.cuda.Stream()
        self.gpu = gpu = capi.Context(0)
        gpu.set_stream(self.st.cuda_stream)
        self.held = []
        scene(gpu, objects, centre=centre)
        self.first = gpu.build_ray_accel(min_faces, refittable=True)
        n = self.n = rays_h.shape[0]
        self.T = objects[index][0][0].shape[0]
        self.rays = self.hold(gpu.to_device(rays_h))
        self.targets = self.hold(gpu.to_device(targets_of(rays_h)))
        self.verts = self.hold(gpu.to_device(objects[index][0][0]))
        self.hit = [self.hold(gpu.empty((n,), capi.HIT_DTYPE)) for _ in range(2)]
        self.rgb = [self.hold(gpu.empty((n, 3), np.float32)) for _ in range(2)]
        self.reach = self.hold(gpu.empty((n,), np.uint32))
        self.index = index
        self.enqueue()  # (the scene is uploaded, the refit's workspace made)
        gpu.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(self.graph, stream=self.st):
            self.enqueue()


def test_captured_update_refit_and_queries_replay_on_a_host_tree(other, moving_sphere):
    A = moving_sphere
    mesh, rays_h = A["mesh"], A["rays"][:4096]
    good = [displaced(mesh, f)[0] for f in (0.01, 0.05)]
    nan = good[1].copy()
    nan[1234, 4] = np.nan
    R = ReplayedHostTree([(mesh, WIDE)], 0, 0, rays_h)
    try:
        gpu = R.gpu
        assert R.first["objects"] == 1 and R.first["max_depth"] == 11
        built = gpu.ray_accel_arrays()
        assert gpu.refit_status()["refits"] == 1
        seen = []
        for k, pos in enumerate(good):
            got = R.replay(pos)
            assert got == brute_answers(other, [((pos, mesh[1], mesh[2]), WIDE)], rays_h), f"replay {k}"
            seen.append(got)
        st = gpu.refit_status()
        assert st["refits"] == 3 and st["kept"] == st["covered"] == 1 and st["fell_back"] == 0, st
        assert seen[0] != seen[1]
        assert gpu.check_ray_accel() == ""
        now = gpu.ray_accel_arrays()
        assert now["index"] == built["index"] and index_words(now) == index_words(built) and now["nodes"] != built["nodes"]
        # a NaN vertex: the object falls back to the scan, the records stay exact
        got = R.replay(nan)
        st = gpu.refit_status()
        assert st["fell_back"] == 1 and st["kept"] == 0 and st["refits"] == 4, st
        assert got == brute_answers(other, [((nan, mesh[1], mesh[2]), WIDE)], rays_h), "NaN vertex"
        # ... and good positions heal it, to the bytes of a refit that never saw the bad mesh
        got = R.replay(good[0])
        st = gpu.refit_status()
        assert st["fell_back"] == 0 and st["kept"] == 1 and st["refits"] == 5, st
        assert got == seen[0] and gpu.check_ray_accel() == ""
        scene(other, [(mesh, WIDE)])
        other.build_ray_accel(0, refittable=True)
        update(other, 0, (good[0], mesh[1], mesh[2]))
        info = other.refit_ray_accel()
        assert info["rebuilt"] == 0, info
        same_arrays(gpu.ray_accel_arrays(), other.ray_accel_arrays(), "healed")
        other.drop_ray_accel()
    finally:
        R.close()


# ------------------------------------------------------------------ 7. the plain host build is untouched
def test_plain_host_build_still_rebuilds_on_the_device_and_refuses_the_async_refit(gpu, moving_sphere):
    A = moving_sphere
    rays = A["rays"][:2048]
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    gpu.build_ray_accel()
    st = capi.lib().eray_scene_refit_ray_accel_async(gpu.handle)
    assert st == capi.E_INVALID_ARGUMENT
    assert capi.last_error(gpu.handle) == PREFIX + "the hierarchy was built on the host (only a device build is refitted)"
    host = gpu.ray_accel_arrays()
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["refitted"] == 0, info
    assert gpu.ray_accel_arrays()["nodes"] != host["nodes"]  # (the device's split, numbered level by level)
    assert gpu.check_ray_accel() == "" and casts(gpu, rays) == casts(gpu, rays, brute_force=True)
    with pytest.raises(ValueError):
        gpu.build_ray_accel(device=True, refittable=True)
    gpu.drop_ray_accel()
