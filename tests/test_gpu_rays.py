"""GPU parity of the ray queries (rays.hip, eray_cast_rays): Object::intersects (object.rs:58-81)
and Engine::cast_ray (engine.rs:112-216) for caller-supplied rays.

Bar: every comparison is bit for bit (integer equality, helpers.assert_bit_equal).  References:
a hand-derived record, the oracle's render for camera rays, and for arbitrary rays the oracle's
Object::intersects per object (oracle.cast_rays(object=k)), with the closest-object len_sq fold
(engine.rs:120-126) restated in np.float32 and the oracle's own selection beside it.
"""
import numpy as np
import pytest

from eray_amd import capi
from tests import ray_refs as R
from tests.helpers import assert_bit_equal, random_mesh

pytestmark = pytest.mark.gpu

MISS_RGB = np.float32([0.1, 0.1, 0.2])  # engine.rs:211-213


# ------------------------------------------------------------------ the reference -----------
def object_records(oracle, mesh, lo, hi, start, raw_dir):
    """Object::intersects (object.rs:58-81) of one object with the box (lo, hi), per ray: the
    oracle's own loop (oracle.cast_rays(object=0)), raw_dir going through Ray::new as a ray passed
    with ERAY_RAYS_NORMALIZE does on the device.  (tests/test_oracle_rays.py holds it to the
    per-face loop over Triangle::intersects that this file used to run itself.)"""
    s = oracle.Scene()
    s.add_object(*mesh, tuple(lo), tuple(hi))
    return oracle.cast_rays(s, oracle.camera(), R.rays_array(start, raw_dir), normalize=True, object=0)


def box_rejects(lo, hi, start, d):
    """The rays BoundingBox::intersects (object.rs:327-379) turns away, restated in f32 numpy."""
    return ~R.bbox_intersects(lo, hi, start, d)


def assert_hits_equal(got, want, what):
    """Every field of every record, bit for bit."""
    assert got.shape == want.shape, what
    assert np.array_equal(got["object"], want["object"]), f"{what}: object"
    assert np.array_equal(got["face"], want["face"]), f"{what}: face"
    for name in ("position", "normal", "uv", "u", "v"):
        assert_bit_equal(got[name], want[name], f"{what}: {name}")


# ------------------------------------------------------------------ inputs, made once --------
def soup(rng, T):
    """T small faces: a centre uniform in [-1, 1]³ plus vertex offsets uniform in ±0.2."""
    centre = rng.uniform(-1, 1, (T, 1, 3))
    pos = (centre + rng.uniform(-0.2, 0.2, (T, 3, 3))).reshape(T, 9).astype(np.float32)
    nrm = rng.normal(size=(T, 9)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (T, 6)).astype(np.float32)
    return pos, nrm, uv


def sphere_rays(rng, n):
    """n rays from the radius-3 sphere toward targets uniform in [-1, 1]³ (dir not normalised)."""
    v = rng.normal(size=(n, 3))
    start = (3.0 * v / np.linalg.norm(v, axis=1, keepdims=True)).astype(np.float32)
    target = rng.uniform(-1, 1, (n, 3)).astype(np.float32)
    return start, (target - start).astype(np.float32)


@pytest.fixture(scope="module")
def arbitrary():
    """Test 3's mesh and rays."""
    rng = np.random.default_rng(7)
    mesh = soup(rng, 300)
    start, raw = sphere_rays(rng, 512)
    # rays with a zero direction component: infinite slabs, and NaN ones where the start lies on
    # the slab's plane (0 * inf)
    extra_s = np.float32([[0.3, -0.2, 3.0], [0.0, 0.0, 3.0], [1.2, 0.1, 3.0], [-3.0, 0.5, 0.5], [0.5, 3.0, 1.2],
                          [0.5, 0.5, 2.0], [1.2, 1.2, -3.0], [0.0, -3.0, 0.0]])
    extra_d = np.float32([[0.0, 0.0, -1.0], [0.0, 0.0, -2.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0],
                          [0.0, -0.5, -1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    start, raw = np.concatenate([start, extra_s]), np.concatenate([raw, extra_d])
    return {"mesh": mesh, "start": start, "raw": raw, "dir": R.normalize_f32(raw)}


def rays_array(start, d):
    return np.ascontiguousarray(np.concatenate([start, d], axis=1), np.float32)


def one_object_scene(gpu, mesh, lo, hi):
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0))
    gpu.add_object(*mesh, tuple(lo), tuple(hi))


# ------------------------------------------------------------------ 1. hand-derived ----------
def test_hand_derived_hit_record(gpu):
    """One face a = (0,0,0), b = (1,0,0), c = (0,1,0), normals (0,0,1), uvs (0,0) (1,0) (0,1), box
    [0,1] x [0,1] x [0,0].  Ray (0.25, 0.25, 1) -> (0,0,-1): n = e1 x e2 = (0,0,1), det = 1, ao =
    (0.25, 0.25, 1), t = 1, u = v = 0.25, so position (0.25, 0.25, 0), normal normalize(0,0,1.5) =
    (0,0,1), uv = (0,0)*0.5 + (1,0)*0.25 + (0,1)*0.25; the box passes through its infinite x / y
    slabs.  The mirrored ray from z = -1 along +z is culled (n . d > 0, primitives.rs:48-51)."""
    pos = np.float32([[0, 0, 0, 1, 0, 0, 0, 1, 0]])
    nrm = np.float32([[0, 0, 1, 0, 0, 1, 0, 0, 1]])
    uv = np.float32([[0, 0, 1, 0, 0, 1]])
    one_object_scene(gpu, (pos, nrm, uv), (0, 0, 0), (1, 1, 0))
    rays = np.float32([[0.25, 0.25, 1, 0, 0, -1], [0.25, 0.25, -1, 0, 0, 1]])
    want = np.zeros(2, capi.HIT_DTYPE)
    want[0] = (0, 0, (0.25, 0.25, 0.0), (0.0, 0.0, 1.0), (0.25, 0.25), 0.25, 0.25)
    want["object"][1] = -1
    for obj in (-1, 0):
        for brute in (False, True):
            got = gpu.cast_rays(rays, object=obj, brute_force=brute)
            assert_hits_equal(got, want, f"object={obj} brute={brute}")
            assert got[1].tobytes() == want[1].tobytes()  # all-zero apart from object == -1


# ------------------------------------------------------------------ 2. camera rays -----------
def test_camera_rays_equal_the_render(gpu, oracle, cube):
    """pixel_to_ray's rays (a Ray's stored dir: no ERAY_RAYS_NORMALIZE) through eray_cast_rays give
    the oracle's render — faces, hit-or-miss and cast_ray sums for bounces 0 and 2 — and
    eray_render's own outputs at that camera."""
    rng = np.random.default_rng(3)
    W, fov, centre = 64, (16.0, 9.0), (0.0, 0.0, 3.0)  # (on the axis: the cube's (0,0,0) box passes)
    s = oracle.Scene()
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera(centre, fov, W, 1.0))
    cam = oracle.camera(centre, fov, W, 1.0)
    Wc, H = oracle.camera_size(cam)
    assert (Wc, H) == (64, 36)
    refl = rng.uniform(0.1, 0.9, (5, 7)).astype(np.float32)
    refl[rng.uniform(size=refl.shape) < 0.3] = 0.0
    color = rng.uniform(0, 1.2, (6, 9, 3)).astype(np.float32)
    keep = [gpu.to_device(refl), gpu.to_device(color)]
    gpu.add_object(*cube, reflection=keep[0].image())
    s.add_object(*cube, reflection=refl)
    pos, nrm, uv = random_mesh(rng, 120, scale=1.0, center=(0.8, 0.2, 0.0))
    lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
    gpu.add_object(pos, nrm, uv, tuple(lo), tuple(hi), color=keep[1].image(), reflection=keep[0].image())
    s.add_object(pos, nrm, uv, tuple(lo), tuple(hi), color=color, reflection=refl)
    for p, var, col, b in (((1.0, 1.0, 2.0), "point", (1.0, 0.9, 0.8), 1.0), ((0.0, 2.0, 0.0), "ambient", (0.9, 0.5, 1.0), 0.3)):
        gpu.add_light(capi.make_light(p, var, col, b))
        s.add_light(p, var, col, b)
    rays = np.empty((H, W, 6), np.float32)
    for y in range(H):
        for x in range(W):  # cast_ray_from_camera(x as f32 / W, y as f32 / H) (engine.rs:100-109)
            st, d = oracle.pixel_to_ray(cam, np.float32(x) / np.float32(W), np.float32(y) / np.float32(H))
            rays[y, x, :3], rays[y, x, 3:] = st, d
    rays = rays.reshape(-1, 6)
    try:
        for bounces in (0, 2):
            ref, ref_face, _ = oracle.render(s, cam, want_faces=True, bounces=bounces)
            assert (ref_face >= 0).sum() > 100 and (ref_face < 0).sum() > 100
            hits, rgb = gpu.cast_rays(rays, bounces=bounces, want_rgb=True)
            assert np.array_equal(hits["object"] != -1, ref_face.reshape(-1) >= 0)
            assert np.array_equal(np.where(hits["object"] != -1, hits["face"], -1), ref_face.reshape(-1))
            assert_bit_equal(rgb.reshape(H, W, 3), ref, f"cast_rays rgb, bounces={bounces}")
            out, face = gpu.empty((H, W, 3), np.float32), gpu.empty((H, W), np.int32)
            gpu.render(W, H, out_rgb=out.ptr, out_face=face.ptr, bounces=bounces)
            r_rgb, r_face = out.numpy(), face.numpy()
            out.free()
            face.free()
            assert_bit_equal(rgb.reshape(H, W, 3), r_rgb, f"eray_render rgb, bounces={bounces}")
            assert np.array_equal(np.where(hits["object"] != -1, hits["face"], -1), r_face.reshape(-1))
        ref2, _ = oracle.render(s, cam, bounces=2)
        ref0, _ = oracle.render(s, cam, bounces=0)
        assert not np.array_equal(ref0, ref2)  # the reflection texture is live
    finally:
        for a in keep:
            a.free()


# ------------------------------------------------------------------ 3. arbitrary rays --------
def test_arbitrary_rays_equal_the_per_face_reference(gpu, oracle, arbitrary):
    """300 small faces, 512 sphere rays passed with ERAY_RAYS_NORMALIZE (plus axis-parallel ones):
    a general box, a tight box that rejects many rays, and the loaded meshes' (0,0,0) point box;
    the tiled search and ERAY_RAYS_BRUTE_FORCE both equal the reference."""
    A = arbitrary
    start, d = A["start"], A["dir"]
    refs = {}
    for name, h in (("wide", 1.2), ("tight", 0.5), ("point", 0.0)):
        refs[name] = (object_records(oracle, A["mesh"], (-h,) * 3, (h,) * 3, start, A["raw"]),
                      box_rejects((-h,) * 3, (h,) * 3, start, d))
        assert not (refs[name][0]["object"][refs[name][1]] >= 0).any()  # the two statements of the box agree
    # conditions of the test, on its own reference, before any GPU call
    wide, wide_rej = refs["wide"]
    tight, tight_rej = refs["tight"]
    assert (wide["object"] >= 0).sum() >= 100
    assert (wide["object"] < 0).sum() >= 100
    assert ((wide["object"] >= 0) & (wide["face"] >= 256)).sum() >= 10  # the second LDS tile
    assert tight_rej.sum() >= 100 and (tight["object"] >= 0).sum() >= 50
    assert wide_rej[:512].sum() == 0  # the ±1.2 box holds every target
    rays = rays_array(start, A["raw"])
    for name, h in (("wide", 1.2), ("tight", 0.5), ("point", 0.0)):
        one_object_scene(gpu, A["mesh"], (-h,) * 3, (h,) * 3)
        want = refs[name][0]
        tiled = gpu.cast_rays(rays, normalize=True)
        brute = gpu.cast_rays(rays, normalize=True, brute_force=True)
        assert_hits_equal(tiled, want, f"{name} box, tiled")
        assert_hits_equal(brute, want, f"{name} box, brute force")
        assert tiled.tobytes() == brute.tobytes()
        assert_hits_equal(gpu.cast_rays(rays, normalize=True, object=0), want, f"{name} box, object 0")
    # the same rays already normalised, passed as stored directions
    one_object_scene(gpu, A["mesh"], (-1.2,) * 3, (1.2,) * 3)
    assert_hits_equal(gpu.cast_rays(rays_array(start, d)), wide, "stored dir")


# ------------------------------------------------------------------ 4. closest object --------
def test_closest_object_is_chosen_by_the_cameras_centre(gpu, oracle, arbitrary):
    """Two overlapping 40-face meshes, camera centre (0,5,0): the object whose hit point is
    strictly closer to the CAMERA (not to the ray's start) wins; object = k gives Object k alone."""
    rng = np.random.default_rng(11)
    centre = (0.0, 5.0, 0.0)
    meshes = [random_mesh(rng, 40, center=(0.0, 0.0, 0.0)), random_mesh(rng, 40, center=(0.3, 0.0, 0.2))]
    start, raw = arbitrary["start"], arbitrary["raw"]  # (every ray: the oracle's loop is fast)
    per, boxes = [], []
    both_objects = oracle.Scene()
    for m in meshes:
        lo, hi = m[0].reshape(-1, 3).min(0), m[0].reshape(-1, 3).max(0)
        boxes.append((lo, hi))
        per.append(object_records(oracle, m, lo, hi, start, raw))
        both_objects.add_object(*m, tuple(lo), tuple(hi))
    want = R.closest_by_centre(per, centre)
    chosen = oracle.cast_rays(both_objects, oracle.camera(centre, (60.0, 60.0), 64, 1.0), R.rays_array(start, raw), normalize=True)
    assert_hits_equal(chosen, want, "the oracle's selection and the numpy one")
    by_start = np.full(start.shape[0], -1)
    both = (per[0]["object"] >= 0) & (per[1]["object"] >= 0)
    t0 = np.linalg.norm(per[0]["position"].astype(np.float64) - start, axis=1)
    t1 = np.linalg.norm(per[1]["position"].astype(np.float64) - start, axis=1)
    by_start[both] = np.where(t1[both] < t0[both], 1, 0)
    assert both.sum() >= 20
    assert (want["object"][both] == 1).sum() >= 20
    assert (want["object"][both] != by_start[both]).sum() >= 20
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera(centre, (60.0, 60.0), 64, 1.0))
    for m, (lo, hi) in zip(meshes, boxes):
        gpu.add_object(*m, tuple(lo), tuple(hi))
    rays = rays_array(start, raw)
    for brute in (False, True):
        assert_hits_equal(gpu.cast_rays(rays, normalize=True, brute_force=brute), want, f"scene, brute={brute}")
        for k in (0, 1):
            own = per[k].copy()
            own["object"][own["object"] >= 0] = k
            assert_hits_equal(gpu.cast_rays(rays, normalize=True, object=k, brute_force=brute), own, f"object {k}")


# ------------------------------------------------------------------ 5. shapes ----------------
@pytest.fixture(scope="module")
def tile_meshes(oracle):
    """Scenes of 257 and 513 faces (one past a tile boundary) whose LAST face is the only one some
    rays hit: a far quad behind a soup that the rays below miss or hit early."""
    rng = np.random.default_rng(5)
    start = np.float32(rng.uniform(-0.9, 0.9, (1000, 3)) * [1, 1, 0] + [0, 0, 3])
    raw = np.tile(np.float32([[0.0, 0.0, -1.0]]), (1000, 1))
    raw[::3] += np.float32(rng.uniform(-0.1, 0.1, (len(raw[::3]), 3)))
    out = {}
    for T in (257, 513):
        pos, nrm, uv = soup(rng, T)
        pos[:, 2::3] *= np.float32(0.5)  # the soup between z = -0.6 and 0.6
        pos[T - 1] = np.float32([-2, -2, -1, 2, -2, -1, 0, 3, -1])  # a big face behind it, facing +z
        mesh = (pos, nrm, uv)
        out[T] = (mesh, object_records(oracle, mesh, (-2, -2, -1), (2, 3, 0.7), start, raw))
    return start, raw, out


@pytest.mark.parametrize("T", [257, 513])
def test_tile_boundaries_and_counts(gpu, tile_meshes, T):
    start, raw, meshes = tile_meshes
    mesh, want = meshes[T]
    assert (want["face"][want["object"] >= 0] == T - 1).sum() >= 100  # the face past the tile boundary
    assert (want["face"][want["object"] >= 0] < T - 1).sum() >= 100
    one_object_scene(gpu, mesh, (-2, -2, -1), (2, 3, 0.7))
    rays = rays_array(start, raw)
    for count in (1, 63, 257, 1000):
        got = gpu.cast_rays(rays[:count], normalize=True)
        assert_hits_equal(got, want[:count], f"T={T} count={count}")
        assert got.tobytes() == gpu.cast_rays(rays[:count], normalize=True, brute_force=True).tobytes()


def test_empty_scene_and_single_outputs(gpu, arbitrary):
    rays = rays_array(arbitrary["start"], arbitrary["raw"])[:300]
    gpu.scene_reset()
    hits, rgb = gpu.cast_rays(rays, normalize=True, want_rgb=True)
    assert (hits["object"] == -1).all() and not hits["face"].any() and not hits["position"].view(np.uint32).any()
    assert_bit_equal(rgb, np.tile(MISS_RGB, (300, 1)), "miss colour")
    only_rgb = gpu.cast_rays(rays, normalize=True, want_hits=False, want_rgb=True)
    assert_bit_equal(only_rgb, rgb, "only out_rgb")
    one_object_scene(gpu, arbitrary["mesh"], (-1.2,) * 3, (1.2,) * 3)
    gpu.add_light(capi.make_light((1.0, 1.0, 2.0), "point"))
    gpu.add_light(capi.make_light((0.0, 2.0, 0.0), "ambient", brightness=0.2))
    hits, rgb = gpu.cast_rays(rays, normalize=True, want_rgb=True)
    assert_hits_equal(gpu.cast_rays(rays, normalize=True), hits, "only out_hit")
    assert_bit_equal(gpu.cast_rays(rays, normalize=True, want_hits=False, want_rgb=True), rgb, "only out_rgb")
    miss = hits["object"] == -1
    assert miss.any() and (~miss).any()
    assert_bit_equal(rgb[miss], np.tile(MISS_RGB, (int(miss.sum()), 1)), "misses")
    assert (rgb[~miss] != MISS_RGB).any()


def test_error_codes(gpu):
    one_object_scene(gpu, (np.float32([[0, 0, 0, 1, 0, 0, 0, 1, 0]]), np.float32([[0, 0, 1] * 3]), np.zeros((1, 6), np.float32)),
                     (0, 0, 0), (1, 1, 0))
    rays = gpu.to_device(np.float32([[0.25, 0.25, 1, 0, 0, -1]] * 4))
    hit = gpu.empty((4,), capi.HIT_DTYPE)
    rgb = gpu.empty((4, 3), np.float32)

    def status(**kw):
        args = dict(rays_ptr=rays.ptr, count=4, out_hit=hit.ptr, out_rgb=None, object=-1, bounces=0, flags=0)
        args.update(kw)
        try:
            gpu.cast_rays_device(**args)
        except capi.ErayError as e:
            assert e.message
            return e.status
        return capi.OK

    try:
        assert status() == capi.OK
        assert status(out_rgb=rgb.ptr, object=0) == capi.E_INVALID_ARGUMENT
        assert status(out_rgb=rgb.ptr, bounces=17) == capi.E_UNSUPPORTED
        assert status(out_rgb=rgb.ptr, bounces=16) == capi.OK
        assert status(count=0) == capi.OK
        assert status(count=0, rays_ptr=None) == capi.OK
        assert status(rays_ptr=None) == capi.E_INVALID_ARGUMENT
        assert status(out_hit=None) == capi.E_INVALID_ARGUMENT
        assert status(object=1) == capi.E_INVALID_ARGUMENT
        assert status(object=-2) == capi.E_INVALID_ARGUMENT
        assert status(flags=4) == capi.E_INVALID_ARGUMENT
        assert status(out_hit=hit.ptr + 4) == capi.E_INVALID_ARGUMENT
        assert capi.lib().eray_cast_rays(gpu.handle, None) == capi.E_INVALID_ARGUMENT
        gpu.synchronize()
    finally:
        for a in (rays, hit, rgb):
            a.free()


# ------------------------------------------------------------------ 6. graph capture ---------
def test_captured_cast_rays_replays(arbitrary):
    """eray_cast_rays on an uploaded scene enqueues one kernel and makes no host round trip: it is
    captured into a graph (torch.cuda.CUDAGraph on the context's stream) and replayed twice."""
    import torch
    st = torch.cuda.Stream()
    gpu = capi.Context(0)  # its own context: the stream below outlives nothing else
    gpu.set_stream(st.cuda_stream)
    rays_h = rays_array(arbitrary["start"], arbitrary["raw"])
    n = rays_h.shape[0]
    one_object_scene(gpu, arbitrary["mesh"], (-1.2,) * 3, (1.2,) * 3)
    gpu.add_light(capi.make_light((1.0, 1.0, 2.0), "point"))
    rays = gpu.to_device(rays_h)
    hit, rgb = gpu.empty((n,), capi.HIT_DTYPE), gpu.empty((n, 3), np.float32)
    try:
        gpu.cast_rays_device(rays.ptr, n, hit.ptr, rgb.ptr, flags=capi.RAYS_NORMALIZE)  # uploads the scene
        gpu.synchronize()
        want_hit, want_rgb = hit.numpy(), rgb.numpy()
        assert (want_hit["object"] >= 0).sum() >= 100
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
