"""GPU parity of eray_scene_refit_ray_accel_async (accel_dev.hip accel_refit_enqueue): the kept-topology
refit enqueued on the context's stream, the device taking the verdict per covered object — directly,
and captured into one graph with the update before it and the queries after it.

Bar: byte equality everywhere — hit records and out_rgb with stored and with normalised directions,
reach words, and the hierarchy's four device arrays against those eray_scene_refit_ray_accel leaves
for the same geometry on a second context built the same way.  Meshes, rays and helpers are those
of tests/test_gpu_refit.py and tests/test_gpu_rays_accel.py."""
import numpy as np
import pytest

from eray_amd import capi
from tests.test_gpu_rays_accel import rays_array, scene, soup, sphere_rays, true_box
from tests.test_gpu_rays_accel_dev import COUNTS
from tests.test_gpu_refit import casts, displaced, moving_sphere, update  # noqa: F401 (moving_sphere: a fixture)

pytestmark = pytest.mark.gpu

PREFIX = "eray_scene_refit_ray_accel_async: "
WIDE = ((-9.0, -9.0, -9.0), (9.0, 9.0, 9.0))  # a box that holds every version of a replayed object
LIGHT = np.float32([1.0, 1.0, 2.0])


@pytest.fixture(scope="module")
def other():
    """A second context: the synchronous refit's arrays for the same geometry."""
    ctx = capi.Context(0)
    yield ctx
    ctx.close()


def targets_of(rays):
    """Each ray's light position: the scene's point light, every fourth ray a point beyond the mesh."""
    t = np.tile(LIGHT, (rays.shape[0], 1))
    t[::4] = rays[::4, :3] + 4.0 * rays[::4, 3:]
    return np.ascontiguousarray(t, np.float32)


def answers(ctx, rays, **kw):
    """Records and sums with stored and with normalised directions, and the reach words, as bytes."""
    out = casts(ctx, rays, True, **kw)
    tg = targets_of(rays)
    for nz in (False, True):
        out += ctx.rays_reach_light(rays, tg, normalize=nz, **kw).tobytes()
    return out


def same_arrays(got, want, what):
    assert got.keys() == want.keys()
    for k in got:
        assert len(got[k]) == len(want[k]) and got[k] == want[k], f"{what}: the {k} array"


def sync_arrays(other, objects, index, new, min_faces, centre=(0.0, 0.0, 5.0)):
    """What eray_scene_refit_ray_accel leaves on a context built the same way."""
    scene(other, objects, centre=centre)
    other.build_ray_accel(min_faces, device=True)
    update(other, index, new)
    info = other.refit_ray_accel()
    assert info["rebuilt"] == 0, info
    return other.ray_accel_arrays(), info


def async_equals_sync(gpu, other, objects, index, new, min_faces, rays, what, covered=1, centre=(0.0, 0.0, 5.0)):
    """Build on `objects`, move object `index` to `new`, refit on the stream: the status, the checker,
    the queries against brute force, the arrays against the synchronous refit's."""
    scene(gpu, objects, centre=centre)
    first = gpu.build_ray_accel(min_faces, device=True)
    assert first["objects"] == covered
    old = gpu.ray_accel_arrays()
    update(gpu, index, new)
    brute = answers(gpu, rays, brute_force=True)
    gpu.refit_ray_accel_async()
    st = gpu.refit_status()
    assert st["refits"] == 1 and st["covered"] == covered and st["kept"] == covered and st["fell_back"] == 0, (what, st)
    assert st["workspace_bytes"] > 0
    assert gpu.check_ray_accel() == "", what
    assert answers(gpu, rays) == brute, f"{what}: the refitted tree vs brute force"
    got = gpu.ray_accel_arrays()
    want, info = sync_arrays(other, objects, index, new, min_faces, centre)
    same_arrays(got, want, what)
    for k in COUNTS:
        assert info[k] == first[k], (what, k, info, first)
    return first, old, got


# ------------------------------------------------------------------ 1. the direct call
def test_direct_call_on_the_sphere(gpu, other, moving_sphere):
    A = moving_sphere
    first, old, got = async_equals_sync(gpu, other, [(A["mesh"], true_box(A["mesh"]))], 0, A["new"], 0, A["rays"], "sphere 3000")
    assert first["max_depth"] > 10  # levels on both sides of the one-launch kernel's reach
    assert got["nodes"] != old["nodes"] and got["index"] == old["index"]
    hits = gpu.cast_rays(A["rays"][:4096], normalize=True)
    assert (hits["object"] >= 0).sum() >= 1000 and (hits["object"] < 0).sum() >= 500
    # the same bytes with a launch per level, and a second refit through the same workspace
    gpu.set_refit_top_levels(False)
    try:
        gpu.refit_ray_accel_async()
        st = gpu.refit_status()
        assert st["refits"] == 2 and st["kept"] == 1, st
        same_arrays(gpu.ray_accel_arrays(), got, "a launch per level")
    finally:
        gpu.set_refit_top_levels(True)
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 2. boundaries
@pytest.mark.parametrize("T", [1, 4, 5, 65, 513, 1100])
def test_leaf_level_and_block_boundaries(gpu, other, T):
    """1: a single leaf; 4, 5: a full leaf and one face more; 65: a level more; 513: three workgroups
    of faces; 1100: 256 nodes on level 8 and a pairs level below them, all inside the one launch."""
    rng = np.random.default_rng(100 + T)
    mesh = soup(rng, T, spread=0.8, size=0.06)
    new = displaced(mesh, 0.05)
    s, d = sphere_rays(rng, 1024)
    aim = new[0].reshape(T, 3, 3).mean(1)[rng.integers(T, size=512)]  # half of the rays at face centroids
    d[:512] = (aim + rng.uniform(-0.01, 0.01, (512, 3)) - s[:512]).astype(np.float32)
    rays = rays_array(s, d)
    first, _, _ = async_equals_sync(gpu, other, [(mesh, true_box(mesh))], 0, new, 1, rays, f"T={T}")
    assert first["unculled_faces"] == 0
    if T == 1100:
        assert first["max_depth"] == 10 and first["nodes"] == 511 + 2 * (1100 - 1024)
    assert (gpu.cast_rays(rays, normalize=True)["object"] >= 0).sum() >= 100
    gpu.drop_ray_accel()


def test_pairs_level_beside_a_deeper_tree(gpu, other, moving_sphere):
    """The soup of 1100 (its pairs level is level 9) beside the sphere of 3000 (complete levels 9 and 10):
    level 9 then runs as a launch of its own for both; the soup is the object that moves."""
    A = moving_sphere
    rng = np.random.default_rng(1100)
    mesh = soup(rng, 1100, spread=0.8, size=0.06)
    new = displaced(mesh, 0.05)
    objects = [(A["mesh"], true_box(A["mesh"])), (mesh, true_box(mesh))]
    async_equals_sync(gpu, other, objects, 1, new, 1, A["rays"][:4096], "soup 1100 beside the sphere", covered=2)
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 3. the middle of three
def mixed(A, cube):
    shift = np.float32([0.6, 0.1, -0.2])
    far = ((A["mesh"][0].reshape(-1, 3, 3) + shift).reshape(-1, 9).astype(np.float32), A["mesh"][1], A["mesh"][2])
    return far, ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))


def test_middle_of_three_covered_objects(gpu, other, cube, moving_sphere):
    A = moving_sphere
    far, box = mixed(A, cube)
    cube2 = ((cube[0].reshape(-1, 3, 3) * np.float32(1.125) + np.float32([0.25, -0.125, 0.0])).reshape(-1, 9).astype(np.float32),
             cube[1], cube[2])
    objects = [(A["mesh"], true_box(A["mesh"])), (cube, box), (far, true_box(far))]
    rays = A["rays"][:4096]
    first, _, _ = async_equals_sync(gpu, other, objects, 1, cube2, 1, rays, "mixed scene", covered=3, centre=(0.5, 4.0, 1.0))
    assert first["faces"] == 6012 and first["unculled_faces"] == 12
    hits = gpu.cast_rays(rays, normalize=True)
    for k in range(3):
        assert (hits["object"] == k).sum() >= 50, k
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 4., 5. capture
class Replayed:
    """A fresh context on its own stream whose object `index` is rewritten by a graph that holds
    update_object_device -> refit_ray_accel_async -> cast_rays (stored and normalised directions,
    records and rgb) -> rays_reach_light, after one warm call of each outside the capture."""

    def __init__(self, objects, index, min_faces, rays_h, centre=(0.0, 0.0, 5.0)):
        import torch
        self.torch = torch
        self.st = torch.cuda.Stream()
        self.gpu = gpu = capi.Context(0)
        gpu.set_stream(self.st.cuda_stream)
        self.held = []
        scene(gpu, objects, centre=centre)
        self.first = gpu.build_ray_accel(min_faces, device=True)
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

    def hold(self, a):
        self.held.append(a)
        return a

    def enqueue(self):
        gpu = self.gpu
        gpu.update_object_device(self.index, self.verts.ptr, None, None, self.T)
        gpu.refit_ray_accel_async()
        for k, flags in enumerate((0, capi.RAYS_NORMALIZE)):
            gpu.cast_rays_device(self.rays.ptr, self.n, self.hit[k].ptr, self.rgb[k].ptr, flags=flags)
        gpu.rays_reach_light_device(self.rays.ptr, self.targets.ptr, self.n, self.reach.ptr, flags=capi.RAYS_NORMALIZE)

    def replay(self, positions):
        gpu = self.gpu
        self.verts.upload(positions)
        for a in (*self.hit, *self.rgb, self.reach):
            gpu.memset(a.ptr, 0xFF, a.nbytes)
        gpu.synchronize()
        self.graph.replay()
        self.torch.cuda.synchronize()
        out = b""
        for k in range(2):
            out += self.hit[k].numpy().tobytes() + self.rgb[k].numpy().tobytes()
        return out + self.reach.numpy().tobytes()

    def close(self):
        for a in self.held:
            a.free()
        self.gpu.close()


def brute_answers(ctx, objects, rays_h, centre=(0.0, 0.0, 5.0)):
    """The same outputs from another context that received the scene as it now stands, by brute force."""
    scene(ctx, objects, centre=centre)
    out = casts(ctx, rays_h, True, brute_force=True)
    return out + ctx.rays_reach_light(rays_h, targets_of(rays_h), normalize=True, brute_force=True).tobytes()


def test_captured_update_refit_and_queries_replay(other, moving_sphere):
    A = moving_sphere
    mesh, rays_h = A["mesh"], A["rays"]
    versions = [displaced(mesh, f)[0] for f in (0.01, 0.03, 0.05)]
    R = Replayed([(mesh, WIDE)], 0, 0, rays_h)
    try:
        gpu = R.gpu
        before = gpu.refit_status()["refits"]
        assert before == 1
        seen = []
        for k, pos in enumerate(versions):
            got = R.replay(pos)
            want = brute_answers(other, [((pos, mesh[1], mesh[2]), WIDE)], rays_h)
            assert got == want, f"replay {k}"
            st = gpu.refit_status()
            assert st["kept"] == st["covered"] == 1 and st["fell_back"] == 0, (k, st)
            seen.append(got)
        assert gpu.refit_status()["refits"] == before + 3
        assert seen[0] != seen[1] and seen[1] != seen[2]
        # no stale tree is left: a direct query through the hierarchy, and the checker on what it holds
        assert gpu.check_ray_accel() == ""
        direct = casts(gpu, rays_h, True)
        assert direct == casts(other, rays_h, True, brute_force=True)
        hits = gpu.cast_rays(rays_h[:4096], normalize=True)
        assert (hits["object"] >= 0).sum() >= 1000
        info = gpu.refit_ray_accel()  # ... which is still the build's topology
        assert info["rebuilt"] == 0, info
        for k in COUNTS:
            assert info[k] == R.first[k], k
    finally:
        R.close()


def test_fallback_and_healing_inside_replays(other, cube, moving_sphere):
    """The mixed scene with the first sphere replayed: a version with face 7 scaled x40 about its centroid
    (|n|1 >= 4: no provable margin any more) and one with a NaN vertex make that object fall back — the
    queries scan it and still equal brute force — and the next ordinary version heals it."""
    A = moving_sphere
    mesh, rays_h = A["mesh"], A["rays"][:4096]
    far, box = mixed(A, cube)
    good = [displaced(mesh, f)[0] for f in (0.01, 0.03)]
    pos = good[0].astype(np.float64).reshape(-1, 3, 3).copy()
    c = pos[7].mean(0)
    pos[7] = c + (pos[7] - c) * 40.0
    assert np.abs(np.cross(pos[7, 1] - pos[7, 0], pos[7, 2] - pos[7, 0])).sum() >= 4.0
    big = pos.reshape(-1, 9).astype(np.float32)
    nan = good[1].copy()
    nan[1234, 4] = np.nan
    centre = (0.5, 4.0, 1.0)

    def objects(p):
        return [((p, mesh[1], mesh[2]), WIDE), (cube, box), (far, true_box(far))]

    R = Replayed(objects(mesh[0]), 0, 1, rays_h, centre=centre)
    try:
        gpu = R.gpu
        assert R.first["objects"] == 3
        for name, bad, then in (("scaled face", big, good[1]), ("NaN vertex", nan, good[0])):
            got = R.replay(bad)
            st = gpu.refit_status()
            assert st["fell_back"] == 1 and st["kept"] == st["covered"] - 1 == 2, (name, st)
            assert got == brute_answers(other, objects(bad), rays_h, centre), name
            assert gpu.check_ray_accel() != "", name  # (the checker rejects a covered object without a record)
            got = R.replay(then)
            st = gpu.refit_status()
            assert st["fell_back"] == 0 and st["kept"] == 3, (name, st)
            assert got == brute_answers(other, objects(then), rays_h, centre), f"after {name}"
            assert gpu.check_ray_accel() == "", f"after {name}"
            want, _ = sync_arrays(other, objects(mesh[0]), 0, (then, mesh[1], mesh[2]), 1, centre)
            same_arrays(gpu.ray_accel_arrays(), want, f"healed after {name}")
        hits = gpu.cast_rays(rays_h, normalize=True)
        for k in range(3):
            assert (hits["object"] == k).sum() >= 50, k
    finally:
        R.close()


# ------------------------------------------------------------------ 6. refusals
def test_refusals_enqueue_nothing(gpu, moving_sphere):
    A = moving_sphere
    rays = A["rays"][:2048]
    L = capi.lib()

    def refused(what):
        before = casts(gpu, rays)
        st = L.eray_scene_refit_ray_accel_async(gpu.handle)
        assert st == capi.E_INVALID_ARGUMENT, (what, st, capi.last_error(gpu.handle))
        assert capi.last_error(gpu.handle).startswith(PREFIX), (what, capi.last_error(gpu.handle))
        assert casts(gpu, rays) == before, what

    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    gpu.drop_ray_accel()
    refused("no hierarchy")
    gpu.build_ray_accel(device=True)
    gpu.drop_ray_accel()
    refused("after a drop")
    gpu.build_ray_accel()
    refused("a host-built hierarchy")
    assert gpu.check_ray_accel() == ""  # (the host's tree is still valid and in use)
    gpu.build_ray_accel(device=True)
    gpu.refit_ray_accel_async()
    assert gpu.refit_status()["refits"] == 1
    small = soup(np.random.default_rng(12), 40, spread=0.3, size=0.3)
    gpu.add_object(*small, *true_box(small))  # 40 faces < 512: not covered, but the records were sized without it
    refused("an object added since the build")
    gpu.drop_ray_accel()


def test_refusal_inside_a_capture_leaves_it_usable(moving_sphere):
    import torch
    A = moving_sphere
    rays_h = A["rays"][:2048]
    n = rays_h.shape[0]
    st = torch.cuda.Stream()
    gpu = capi.Context(0)
    gpu.set_stream(st.cuda_stream)
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    gpu.build_ray_accel(device=True)
    rays = gpu.to_device(rays_h)
    hit = gpu.empty((n,), capi.HIT_DTYPE)
    try:
        gpu.cast_rays_device(rays.ptr, n, hit.ptr, None, flags=capi.RAYS_NORMALIZE)
        gpu.synchronize()
        want = hit.numpy().tobytes()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            status = capi.lib().eray_scene_refit_ray_accel_async(gpu.handle)  # no workspace yet
            message = capi.last_error(gpu.handle)
            gpu.cast_rays_device(rays.ptr, n, hit.ptr, None, flags=capi.RAYS_NORMALIZE)
        assert status == capi.E_INVALID_ARGUMENT and message.startswith(PREFIX) and "outside a capture" in message, message
        gpu.memset(hit.ptr, 0xFF, hit.nbytes)
        gpu.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert hit.numpy().tobytes() == want
        with pytest.raises(capi.ErayError):  # (and no workspace was made on the way)
            gpu.refit_status()
    finally:
        rays.free()
        hit.free()
        gpu.close()


# ------------------------------------------------------------------ 7. beside the synchronous refit
def test_coexistence_with_the_synchronous_refit(gpu, moving_sphere):
    A = moving_sphere
    rays = A["rays"][:4096]
    pos = A["new"][0].astype(np.float64).reshape(-1, 3, 3).copy()
    c = pos[7].mean(0)
    pos[7] = c + (pos[7] - c) * 40.0
    big = (pos.reshape(-1, 9).astype(np.float32), A["new"][1], A["new"][2])
    scene(gpu, [(A["mesh"], true_box(A["mesh"]))])
    first = gpu.build_ray_accel(device=True)
    update(gpu, 0, A["new"])
    gpu.refit_ray_accel_async()
    gpu.refit_ray_accel_async()
    assert gpu.refit_status()["refits"] == 2
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 0 and info["refitted"] == 1, info
    for k in COUNTS:
        assert info[k] == first[k], (k, info, first)
    assert gpu.refit_status()["refits"] == 2  # (the workspace outlives a kept synchronous refit)
    update(gpu, 0, big)
    brute = answers(gpu, rays, brute_force=True)
    gpu.refit_ray_accel_async()
    st = gpu.refit_status()
    assert st["fell_back"] == 1 and st["kept"] == 0 and st["refits"] == 3, st
    assert answers(gpu, rays) == brute
    info = gpu.refit_ray_accel()
    assert info["rebuilt"] == 1 and info["unculled_faces"] == 1, info
    with pytest.raises(capi.ErayError) as e:  # the rebuild released the workspace with the old layout
        gpu.refit_status()
    assert e.value.status == capi.E_INVALID_ARGUMENT
    gpu.refit_ray_accel_async()  # ... and the next call outside a capture makes a new one
    st = gpu.refit_status()
    assert st["refits"] == 1 and st["kept"] == st["covered"] == 1 and st["fell_back"] == 0, st
    assert gpu.check_ray_accel() == "" and answers(gpu, rays) == brute
    gpu.drop_ray_accel()
