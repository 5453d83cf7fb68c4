"""GPU parity of out_rgb's shadow and reflected rays through the ray-query hierarchy (rays.hip
AccelFaces, cast.hpp's face finder) and of eray_rays_reach_light (rays.hip reach_kernel):

- out_rgb and out_hit with a hierarchy equal the tiles' (before the build) and
  ERAY_RAYS_BRUTE_FORCE's, byte for byte, for bounces 0 and 3, stored and normalised directions,
  both builders and both object orders;
- the reach words are the same with the hierarchy, without it and in brute force, and equal a numpy
  composition of per-object eray_cast_rays calls (Engine::reaches_light, engine.rs:218-228: the
  first object in scene order with a hit decides, by |position - start| > |target - start|).

Every comparison is on bytes.  (Helpers copied from tests/test_gpu_rays_accel.py.)"""
import numpy as np
import pytest

from eray_amd import capi, meshgen

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------ helpers (copied) ---------
def normalize_f32(d):
    """Ray::new's dir.normalize() (raycasting.rs:16-21, vector.rs:150-158) in f32."""
    d = np.asarray(d, np.float32)
    sq = np.float32(0.0) + d[:, 0] * d[:, 0]
    sq = sq + d[:, 1] * d[:, 1]
    sq = sq + d[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (d / np.sqrt(sq)[:, None]).astype(np.float32)


def len_f32(v):
    """Vector::len in f32: the fold from 0, then sqrt."""
    v = np.asarray(v, np.float32)
    with np.errstate(over="ignore", invalid="ignore"):
        sq = np.float32(0.0) + v[:, 0] * v[:, 0]
        sq = sq + v[:, 1] * v[:, 1]
        sq = sq + v[:, 2] * v[:, 2]
        return np.sqrt(sq).astype(np.float32)


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


def moved(mesh, shift):
    pos = (mesh[0].reshape(-1, 3, 3) + np.float32(shift)).reshape(-1, 9).astype(np.float32)
    return pos, mesh[1], mesh[2]


# ------------------------------------------------------------------ scenes A and A' ----------
CENTRE = (0.0, 0.0, 5.0)
POINT_LIGHTS = ((4.0, 3.0, 2.0), (-4.5, 3.5, 0.5))  # on opposite sides, above the floor
FLOOR_Y = -1.05


def floor_mesh():
    """Two faces in the plane y = FLOOR_Y under the sphere, front side up ((b - a) x (c - a) = +y)."""
    y, r = FLOOR_Y, 5.0
    pos = np.float32([[-r, y, -r, -r, y, r, r, y, r], [-r, y, -r, r, y, r, r, y, -r]])
    nrm = np.float32([[0, 1, 0] * 3] * 2)
    uv = np.float32([[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 0]])
    return pos, nrm, uv


def camera_grid(n=64):
    """An n x n grid of camera rays from CENTRE through the plane one unit in front of it (60 degrees
    across), stored directions (not normalised)."""
    c = ((np.arange(n, dtype=np.float64) + 0.5) / n * 2.0 - 1.0) * np.tan(np.radians(30.0))
    x, y = np.meshgrid(c, c)
    d = np.stack([x.ravel(), y.ravel(), -np.ones(n * n)], axis=1).astype(np.float32)
    return np.tile(np.float32(CENTRE), (n * n, 1)), d


@pytest.fixture(scope="module")
def parts(cube):
    rng = np.random.default_rng(77)
    sphere = sphere_mesh(3000)
    box_cube = moved(cube, (-2.3, 0.0, -0.5))  # (unscaled: |n| = 4, no provable margin, every face unculled)
    s0, d0 = camera_grid(64)
    s1, d1 = sphere_rays(rng, 2048)
    return {"cube": (box_cube, true_box(box_cube)), "sphere": (sphere, true_box(sphere)),
            "floor": (floor_mesh(), true_box(floor_mesh())),
            "rays": rays_array(np.concatenate([s0, s1]), np.concatenate([d0, d1]))}


@pytest.fixture(scope="module")
def refl(gpu):
    """The 1 x 1 reflection image of 0.5 (device memory the scenes' materials point at)."""
    a = gpu.to_device(np.full((1, 1), 0.5, np.float32))
    yield a
    gpu.scene_reset()
    a.free()


ORDERS = {"A": ("cube", "sphere", "floor"), "A'": ("floor", "sphere", "cube")}


def scene(gpu, objects, lights=POINT_LIGHTS, ambient=True):
    """objects: (mesh, (lo, hi), reflection image or None)."""
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera(CENTRE, (60.0, 60.0), 64, 1.0))
    for mesh, (lo, hi), image in objects:
        gpu.add_object(*mesh, tuple(lo), tuple(hi), reflection=image)
    for p in lights:
        gpu.add_light(capi.make_light(p, "point"))
    if ambient:
        gpu.add_light(capi.make_light((0.0, 2.0, 0.0), "ambient", brightness=0.2))


def scene_a(gpu, parts, refl, order):
    scene(gpu, [(*parts[name], None if name == "cube" else refl.image()) for name in ORDERS[order]])


def shadow_rays(hits, lights=POINT_LIGHTS):
    """cast_ray's shadow rays of the hits (engine.rs:133-141) in f32: start P + N * 0.1, direction
    normalize(L - P), target L; one per hit and point light."""
    hit = hits["object"] >= 0
    P, N = hits["position"][hit], hits["normal"][hit]
    S = (P + N * np.float32(0.1)).astype(np.float32)
    rays, targets = [], []
    for L in lights:
        L = np.float32(L)
        rays.append(rays_array(S, normalize_f32(L - P)))
        targets.append(np.tile(L, (P.shape[0], 1)))
    return np.concatenate(rays), np.concatenate(targets).astype(np.float32)


def deciders(gpu, rays, nobj, normalize=False, brute_force=True):
    """Per ray the first object in scene order that eray_cast_rays(object=k) hits (-1: none) and
    that hit's position: the calls the reach reference is composed of."""
    first = np.full(rays.shape[0], -1, np.int32)
    pos = np.zeros((rays.shape[0], 3), np.float32)
    for k in range(nobj):
        h = gpu.cast_rays(rays, object=k, normalize=normalize, brute_force=brute_force)
        take = (first < 0) & (h["object"] >= 0)
        first[take] = k
        pos[take] = h["position"][take]
    return first, pos


def reach_reference(gpu, rays, targets, nobj, normalize=False):
    """Engine::reaches_light (engine.rs:218-228) from per-object eray_cast_rays: the first object
    with a hit decides by len(position - start) > len(target - start); no hit: 1."""
    first, pos = deciders(gpu, rays, nobj, normalize)
    start = rays[:, :3]
    with np.errstate(over="ignore", invalid="ignore"):
        far = len_f32(pos - start) > len_f32(targets - start)
    return np.where(first < 0, True, far).astype(np.uint32)


def reach_three_forms(gpu, rays, targets, min_faces, what, normalize=(False, True), device=False, expect=None):
    """The reach words without a hierarchy (tiles), in brute force and with the hierarchy, byte for
    byte; returns the words of each `normalize`."""
    gpu.drop_ray_accel()
    before = {nz: (gpu.rays_reach_light(rays, targets, normalize=nz),
                   gpu.rays_reach_light(rays, targets, normalize=nz, brute_force=True)) for nz in normalize}
    info = gpu.build_ray_accel(min_faces, device=device)
    for k, v in (expect or {}).items():
        assert info[k] == v, (what, k, info)
    out = {}
    for nz in normalize:
        tiles, brute = before[nz]
        tree = gpu.rays_reach_light(rays, targets, normalize=nz)
        brute2 = gpu.rays_reach_light(rays, targets, normalize=nz, brute_force=True)
        assert tree.dtype == np.uint32 and tree.shape == (rays.shape[0],)
        assert np.isin(tree, (0, 1)).all(), what
        for name, other in (("tiles", tiles), ("brute force", brute), ("brute force after the build", brute2)):
            assert tree.tobytes() == other.tobytes(), f"{what} normalize={nz}: hierarchy vs {name}"
        out[nz] = tree
    return out


def rgb_three_forms(gpu, rays, min_faces, what, bounces=(0,), normalize=(False, True), device=False, expect=None):
    """out_hit and out_rgb before the build (tiles), in brute force and with the hierarchy, byte for
    byte; returns the build's info."""
    gpu.drop_ray_accel()
    before = {}
    for b in bounces:
        for nz in normalize:
            before[b, nz] = (gpu.cast_rays(rays, bounces=b, normalize=nz, want_rgb=True),
                             gpu.cast_rays(rays, bounces=b, normalize=nz, want_rgb=True, brute_force=True))
    info = gpu.build_ray_accel(min_faces, device=device)
    for k, v in (expect or {}).items():
        assert info[k] == v, (what, k, info)
    for (b, nz), (tiles, brute) in before.items():
        tree = gpu.cast_rays(rays, bounces=b, normalize=nz, want_rgb=True)
        for name, other in (("tiles", tiles), ("brute force", brute)):
            assert tree[0].tobytes() == other[0].tobytes(), f"{what} bounces={b} normalize={nz}: out_hit vs {name}"
            assert tree[1].tobytes() == other[1].tobytes(), f"{what} bounces={b} normalize={nz}: out_rgb vs {name}"
    return info


# ------------------------------------------------------------------ 1, 2. out_rgb ------------
@pytest.mark.parametrize("device", [False, True], ids=["host-built", "device-built"])
@pytest.mark.parametrize("order", ["A", "A'"])
def test_out_rgb_three_forms(gpu, parts, refl, order, device):
    """Scenes A and A': out_hit and out_rgb with the hierarchy (cube and sphere; the floor keeps the
    scan) equal the tiles' and brute force's, bounces 0 and 3, stored and normalised directions.
    The coverage condition on the test's own input: of the hits' shadow rays at least 5 % are
    blocked, at least 5 % reach, and the sphere decides at least 5 % of the blocked ones."""
    scene_a(gpu, parts, refl, order)
    rays = parts["rays"]
    gpu.drop_ray_accel()
    hits, rgb0 = gpu.cast_rays(rays, bounces=0, normalize=True, want_rgb=True, brute_force=True)
    _, rgb3 = gpu.cast_rays(rays, bounces=3, normalize=True, want_rgb=True, brute_force=True)
    assert rgb0.tobytes() != rgb3.tobytes()  # the reflection image is live
    for k in range(3):
        assert (hits["object"] == k).sum() >= 100, (order, k)
    sh, tg = shadow_rays(hits)
    reach = gpu.rays_reach_light(sh, tg, brute_force=True)
    blocked = reach == 0
    n = reach.shape[0]
    assert n >= 4096 and blocked.sum() >= 0.05 * n and (~blocked).sum() >= 0.05 * n, (n, blocked.sum())
    first, _ = deciders(gpu, sh, 3)
    sphere_k = ORDERS[order].index("sphere")
    assert ((first == sphere_k) & blocked).sum() >= 0.05 * blocked.sum(), (blocked.sum(), np.bincount(first[blocked] + 1))
    rgb_three_forms(gpu, rays, 12, f"scene {order}", bounces=(0, 3), device=device,
                    expect={"objects": 2, "faces": 3012, "unculled_faces": 12})
    gpu.drop_ray_accel()


def test_facing_reflective_spheres(gpu, refl):
    """Two reflective 600-face spheres that face each other, min_faces = 1, bounces = 3: every
    reflected and shadow ray re-enters the walk, whose stack must be empty each time."""
    rng = np.random.default_rng(5)
    ball = sphere_mesh(600)
    left, right = moved(ball, (-1.05, 0.0, 0.0)), moved(ball, (1.05, 0.0, 0.0))
    scene(gpu, [(left, true_box(left), refl.image()), (right, true_box(right), refl.image())])
    s, d = sphere_rays(rng, 2048)
    s2, d2 = camera_grid(32)
    rays = rays_array(np.concatenate([s, s2]), np.concatenate([d, d2]))
    gpu.drop_ray_accel()
    hits, brute = gpu.cast_rays(rays, bounces=3, normalize=True, want_rgb=True, brute_force=True)
    _, brute0 = gpu.cast_rays(rays, bounces=0, normalize=True, want_rgb=True, brute_force=True)
    assert (hits["object"] == 0).sum() >= 200 and (hits["object"] == 1).sum() >= 200
    assert (brute != brute0).any(axis=1).sum() >= 200  # reflected rays that found the other sphere or the miss colour
    info = gpu.build_ray_accel(1)
    assert info["objects"] == 2 and info["faces"] == 1200 and info["max_depth"] >= 8
    got_hits, got = gpu.cast_rays(rays, bounces=3, normalize=True, want_rgb=True)
    assert got_hits.tobytes() == hits.tobytes()
    assert got.tobytes() == brute.tobytes()
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 3. the reach query -------
@pytest.mark.parametrize("order", ["A", "A'"])
def test_reach_three_forms_and_the_composed_reference(gpu, parts, refl, order):
    """8,192 segments, half the scene's own shadow rays and half random, in the three forms and
    against the per-object composition of eray_cast_rays."""
    rng = np.random.default_rng(31)
    scene_a(gpu, parts, refl, order)
    gpu.drop_ray_accel()
    hits = gpu.cast_rays(parts["rays"], normalize=True, brute_force=True)
    sh, tg = shadow_rays(hits)
    pick = rng.choice(sh.shape[0], 4096, replace=False)
    start = rng.uniform(-3, 3, (4096, 3)).astype(np.float32)
    target = rng.uniform(-3, 3, (4096, 3)).astype(np.float32)
    rays = np.concatenate([sh[pick], rays_array(start, (target - start).astype(np.float32))])
    targets = np.concatenate([tg[pick], target])
    words = reach_three_forms(gpu, rays, targets, 12, f"scene {order}",
                              expect={"objects": 2, "faces": 3012, "unculled_faces": 12})
    for nz, got in words.items():
        want = reach_reference(gpu, rays, targets, 3, normalize=nz)
        assert got.tobytes() == want.tobytes(), f"scene {order} normalize={nz}: {int((got != want).sum())} words differ"
        for half in (slice(0, 4096), slice(4096, 8192)):
            assert (got[half] == 0).sum() >= 100 and (got[half] == 1).sum() >= 100, (nz, half)
    # the device-built tree: the same words
    again = reach_three_forms(gpu, rays, targets, 12, f"scene {order}, device-built", device=True)
    assert again[False].tobytes() == words[False].tobytes() and again[True].tobytes() == words[True].tobytes()
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 4. smallest trees --------
def segments(rng, mesh, n=1024):
    """n rays from the radius-3 sphere, half of them aimed at face centroids, with targets that lie
    before, on and beyond the mesh along each ray."""
    T = mesh[0].shape[0]
    s, d = sphere_rays(rng, n)
    aim = mesh[0].reshape(T, 3, 3).mean(1)[rng.integers(T, size=n // 2)]
    d[:n // 2] = (aim + rng.uniform(-0.01, 0.01, (n // 2, 3)) - s[:n // 2]).astype(np.float32)
    targets = (s + d * rng.uniform(0.2, 2.0, (n, 1)).astype(np.float32)).astype(np.float32)
    return rays_array(s, d), targets


@pytest.mark.parametrize("T, depth", [(4, 1), (5, 2), (9, 3)])
def test_smallest_trees(gpu, T, depth):
    """One object of T faces, min_faces = 1: a root that is one leaf, a root over two leaves, three
    levels."""
    rng = np.random.default_rng(200 + T)
    mesh = soup(rng, T, spread=0.8, size=0.08)  # (small faces: every one has a margin and goes under the tree)
    scene(gpu, [(mesh, true_box(mesh), None)], lights=POINT_LIGHTS[:1])
    rays, targets = segments(rng, mesh)
    expect = {"objects": 1, "faces": T, "unculled_faces": 0, "max_depth": depth}
    words = reach_three_forms(gpu, rays, targets, 1, f"T={T}", expect=expect)
    assert (words[True] == 0).sum() >= 20 and (words[True] == 1).sum() >= 20
    rgb_three_forms(gpu, rays, 1, f"T={T}", expect=expect)
    gpu.drop_ray_accel()


def test_unculled_only_empty_scene_and_no_rays(gpu, cube):
    rng = np.random.default_rng(12)
    box = ((-1.0, -1.0, -1.0), (1.0, 1.0, 1.0))
    scene(gpu, [(cube, box, None)], lights=POINT_LIGHTS[:1])
    rays, targets = segments(rng, cube)
    expect = {"objects": 1, "faces": 12, "unculled_faces": 12, "nodes": 0}  # root == kNoNode
    words = reach_three_forms(gpu, rays, targets, 1, "the cube alone", expect=expect)
    assert (words[True] == 0).sum() >= 100 and (words[True] == 1).sum() >= 100
    rgb_three_forms(gpu, rays, 1, "the cube alone", expect=expect)
    # count == 0, with the hierarchy and without
    for drop in (False, True):
        if drop:
            gpu.drop_ray_accel()
        got = gpu.rays_reach_light(rays[:0], targets[:0])
        assert got.shape == (0,) and got.dtype == np.uint32
        gpu.rays_reach_light_device(None, None, 0, None)
    # an empty scene: nothing blocks, every ray shows the miss colour
    gpu.scene_reset()
    gpu.add_light(capi.make_light(POINT_LIGHTS[0], "point"))
    words = reach_three_forms(gpu, rays, targets, 1, "empty scene", expect={"objects": 0, "nodes": 0})
    assert (words[False] == 1).all() and (words[True] == 1).all()
    rgb_three_forms(gpu, rays, 1, "empty scene")
    assert (gpu.cast_rays(rays, want_hits=False, want_rgb=True) == np.float32([0.1, 0.1, 0.2])).all()
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 5. uncovered rays --------
def test_rays_the_proof_does_not_cover(gpu, parts, refl):
    """64 segments whose rays the margin proof does not cover (NaN, infinite, 2^41-long and
    2^-41-short directions, |start|_1 > 2^40): with and without the hierarchy the words, records
    and colours are brute force's."""
    rng = np.random.default_rng(64)
    scene_a(gpu, parts, refl, "A")
    s, d = sphere_rays(rng, 64)
    t = rng.uniform(-3, 3, (64, 3)).astype(np.float32)
    for i in range(64):
        kind, ax = i % 8, (i // 8) % 3
        if kind == 0:
            d[i, ax] = np.nan
        elif kind == 1:
            d[i, ax] = np.inf
        elif kind == 2:
            d[i, ax] = -np.inf
        elif kind == 3:
            d[i] = normalize_f32(d[i:i + 1])[0] * np.float32(2.0 ** 41)
        elif kind == 4:
            d[i] = normalize_f32(d[i:i + 1])[0] * np.float32(2.0 ** -41)
        elif kind == 5:  # a far start whose ray still points at the scene
            s[i] = normalize_f32(s[i:i + 1])[0] * np.float32(2.0 ** 41)
            d[i] = -s[i]
        elif kind == 6:
            s[i, ax] = np.nan
        else:
            t[i, ax] = np.inf if i % 16 < 8 else np.nan
    rays = rays_array(s, d)
    assert (np.abs(s[5::8]).sum(1) > 2.0 ** 40).all()
    for nz in (False, True):
        gpu.drop_ray_accel()
        want = gpu.rays_reach_light(rays, t, normalize=nz, brute_force=True)
        want_hit, want_rgb = gpu.cast_rays(rays, bounces=3, normalize=nz, want_rgb=True, brute_force=True)
        for tree in (False, True):
            if tree:
                assert gpu.build_ray_accel(12)["objects"] == 2
            what = f"normalize={nz} hierarchy={tree}"
            assert gpu.rays_reach_light(rays, t, normalize=nz).tobytes() == want.tobytes(), what
            got_hit, got_rgb = gpu.cast_rays(rays, bounces=3, normalize=nz, want_rgb=True)
            assert got_hit.tobytes() == want_hit.tobytes(), what
            assert got_rgb.tobytes() == want_rgb.tobytes(), what
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ 6. invalidation, capture -
def test_reach_after_a_geometry_change(gpu, parts, refl):
    """add_object drops the hierarchy silently: the query still answers, as brute force does, and
    the new object shows in the words."""
    rng = np.random.default_rng(41)
    scene_a(gpu, parts, refl, "A")
    start = rng.uniform(-3, 3, (4096, 3)).astype(np.float32)
    target = rng.uniform(-3, 3, (4096, 3)).astype(np.float32)
    rays = rays_array(start, (target - start).astype(np.float32))
    assert gpu.build_ray_accel(12)["objects"] == 2
    one = gpu.rays_reach_light(rays, target)
    wall = soup(rng, 600, spread=2.5, size=0.4)
    gpu.add_object(*wall, *true_box(wall))
    stale = gpu.rays_reach_light(rays, target)
    brute = gpu.rays_reach_light(rays, target, brute_force=True)
    assert stale.tobytes() == brute.tobytes()
    assert stale.tobytes() != one.tobytes() and (stale < one).sum() >= 20  # the new object blocks some
    assert gpu.build_ray_accel(12)["objects"] == 3
    assert gpu.rays_reach_light(rays, target).tobytes() == brute.tobytes()
    gpu.drop_ray_accel()


def test_captured_reach_query_with_a_hierarchy_replays(parts):
    """eray_rays_reach_light with a hierarchy enqueues one kernel and makes no host round trip: it
    is captured into a graph on the context's stream and replayed three times."""
    import torch
    rng = np.random.default_rng(43)
    st = torch.cuda.Stream()
    gpu = capi.Context(0)
    gpu.set_stream(st.cuda_stream)
    n = 4096
    start = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    target = rng.uniform(-3, 3, (n, 3)).astype(np.float32)
    scene(gpu, [(*parts[name], None) for name in ORDERS["A"]])
    rays, tgt = gpu.to_device(rays_array(start, (target - start).astype(np.float32))), gpu.to_device(target)
    out = gpu.empty((n,), np.uint32)
    try:
        gpu.rays_reach_light_device(rays.ptr, tgt.ptr, n, out.ptr, flags=capi.RAYS_NORMALIZE)  # tiles
        gpu.synchronize()
        want = out.numpy()
        assert (want == 0).sum() >= 100 and (want == 1).sum() >= 100
        assert gpu.build_ray_accel(12)["objects"] == 2
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=st):
            gpu.rays_reach_light_device(rays.ptr, tgt.ptr, n, out.ptr, flags=capi.RAYS_NORMALIZE)
        for replay in range(3):
            gpu.memset(out.ptr, 0xFF, out.nbytes)
            gpu.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert out.numpy().tobytes() == want.tobytes(), f"replay {replay}"
    finally:
        for a in (rays, tgt, out):
            a.free()
        gpu.close()
