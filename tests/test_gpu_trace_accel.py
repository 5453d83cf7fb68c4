"""GPU parity of the general tracer's shadow and reflected rays through the ray-query hierarchy
(trace.hip: trace_kernel and trace_binned_kernel with a RayAccelView; accel_faces.hpp AccelFaces).

Every frame is rendered in four forms that must agree bit for bit in f32 RGB, PPM bytes and faces:
the default (with the hierarchy), ERAY_RENDER_NO_RAY_ACCEL (the per-lane scan, the behaviour before
the hierarchy reached the tracer), ERAY_RENDER_BRUTE_FORCE, and the CPU oracle.  Every scene object
carries its true bounding box, so its shadow and reflected rays really reach the face search.
trace_ray_accel_objects() tells which form ran: > 0 by default, 0 under either flag and after the
hierarchy is dropped or invalidated.

The scenes' own statistics (hit pixels per object, blocked and reaching shadow rays, which object
decides a blocked one) are asserted on the oracle's output, so that a scene change cannot hollow
the comparison out.  (Helpers copied from tests/test_gpu_rays_secondary.py.)"""
import ctypes

import numpy as np
import pytest

from eray_amd import capi, meshgen
from tests.helpers import assert_bit_equal, random_mesh

pytestmark = pytest.mark.gpu

POINT_LIGHTS = ((4.0, 3.0, 2.0), (-4.5, 3.5, 0.5))
FLOOR_Y = -1.05
SEED = 7
BUILDERS = {"host": {}, "device": {"device": True}, "refittable": {"refittable": True}}


# ------------------------------------------------------------------ helpers (copied) ---------
def normalize_f32(d):
    """Ray::new's dir.normalize() (raycasting.rs:16-21, vector.rs:150-158) in f32."""
    d = np.asarray(d, np.float32)
    sq = np.float32(0.0) + d[:, 0] * d[:, 0]
    sq = sq + d[:, 1] * d[:, 1]
    sq = sq + d[:, 2] * d[:, 2]
    with np.errstate(divide="ignore", invalid="ignore"):
        return (d / np.sqrt(sq)[:, None]).astype(np.float32)


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


def scaled(mesh, s):
    return (mesh[0] * np.float32(s)).astype(np.float32), mesh[1], mesh[2]


def floor_mesh():
    """Two faces in the plane y = FLOOR_Y, front side up ((b - a) x (c - a) = +y)."""
    y, r = FLOOR_Y, 5.0
    pos = np.float32([[-r, y, -r, -r, y, r, r, y, r], [-r, y, -r, r, y, r, r, y, -r]])
    nrm = np.float32([[0, 1, 0] * 3] * 2)
    uv = np.float32([[0, 0, 0, 1, 1, 1], [0, 0, 1, 1, 1, 0]])
    return pos, nrm, uv


def shadow_rays(hits, lights):
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


# ------------------------------------------------------------------ scenes -------------------
class Scene:
    """One scene on the GPU context and in the oracle: objects (mesh, reflection image or None[, colour
    image]), each with its true box; lights (position, variant, colour, brightness)."""

    def __init__(self, gpu, oracle, centre, fov, width, objects, lights):
        self.gpu, self.oracle, self.keep = gpu, oracle, []
        self.centre, self.fov, self.width = centre, fov, width
        self.meshes = [o[0] for o in objects]
        self.point_lights = [p for p, var, _, _ in lights if var == "point"]
        self.s = oracle.Scene()
        self.cam = oracle.camera(centre, fov, width, 1.0)
        self.W, self.H = oracle.camera_size(self.cam)
        gpu.scene_reset()
        gpu.set_camera(capi.make_camera(centre, fov, width, 1.0))
        for mesh, *images in objects:
            lo, hi = true_box(mesh)
            kw, okw = {}, {}
            for name, a in zip(("reflection", "color"), images):
                if a is not None:
                    d = gpu.to_device(np.ascontiguousarray(a, np.float32))
                    self.keep.append(d)
                    kw[name], okw[name] = d.image(), np.ascontiguousarray(a, np.float32)
            gpu.add_object(*mesh, lo, hi, **kw)
            self.s.add_object(*mesh, lo, hi, **okw)
        for p, var, col, b in lights:
            gpu.add_light(capi.make_light(p, var, col, b))
            self.s.add_light(p, var, col, b)

    def close(self):
        self.gpu.drop_ray_accel()
        self.gpu.scene_reset()
        for a in self.keep:
            a.free()

    def camera_rays(self):
        """The corner ray of every pixel (camera.rs:57-76 in f32; Ray::new normalises): (H * W, 6)."""
        f = np.float32
        W, H = self.W, self.H
        C = np.float32(self.centre)
        vw = f(self.fov[0]) / f(self.fov[1]) * f(2.0)
        bl = np.float32([C[0] - vw / f(2.0), C[1] - f(2.0) / f(2.0), C[2] - f(1.0)])
        xf = (np.arange(W, dtype=np.float32) / f(W))[None, :].repeat(H, 0).ravel()
        yf = (np.arange(H, dtype=np.float32) / f(H))[:, None].repeat(W, 1).ravel()
        d = np.stack([bl[0] + vw * xf - C[0], bl[1] + f(2.0) * yf - C[1], np.full(W * H, bl[2] - C[2], np.float32)], 1)
        return rays_array(np.tile(C, (W * H, 1)), d.astype(np.float32))

    def statistics(self):
        """From the oracle alone: hit pixels per object, the primary hits' shadow rays (blocked words
        and the object that decides each), and the shadow rays' start points."""
        o = self.oracle
        hits = o.cast_rays(self.s, self.cam, self.camera_rays(), normalize=True)
        per_object = [int((hits["object"] == k).sum()) for k in range(len(self.meshes))]
        sh, tg = shadow_rays(hits, self.point_lights)
        reach = o.reach_light(self.s, sh, tg)
        first = np.full(sh.shape[0], -1, np.int32)
        for k in range(len(self.meshes)):
            h = o.cast_rays(self.s, self.cam, sh, object=k)
            first[(first < 0) & (h["object"] >= 0)] = k
        return {"hit": per_object, "rays": sh.shape[0], "blocked": reach == 0, "decider": first, "starts": sh[:, :3]}


AMBIENT = ((0.0, 2.0, 0.0), "ambient", (1.0, 1.0, 1.0), 0.2)


def sphere_lights():
    return [(p, "point", (1.0, 1.0, 1.0), 1.0) for p in POINT_LIGHTS] + [AMBIENT]


def spheres_a(gpu, oracle, faces=600, prime=False):
    """Spheres A: two reflective displaced spheres side by side on a reflective two-face floor, two
    point lights on opposite sides.  A' (prime): the floor first and the camera higher, which
    changes the object that decides reaches_light."""
    half = np.full((1, 1), 0.5, np.float32)
    ball = sphere_mesh(faces)
    objs = [(moved(ball, (-1.05, 0.0, 0.0)), half), (moved(ball, (1.05, 0.0, 0.0)), half), (floor_mesh(), half)]
    if prime:
        objs = [objs[2], objs[0], objs[1]]
    return Scene(gpu, oracle, (0.0, 0.6, 2.4) if prime else (0.0, 0.1, 2.2), (60.0, 60.0), 64, objs, sphere_lights())


def soup_scene(gpu, oracle):
    """Soup: two binned random meshes (5000 and 2500 faces; the first has bins of more than
    kTraceHeavyMin entries, the heavy role) and a small one, all reflective."""
    rng = np.random.default_rng(63)
    meshes = [random_mesh(rng, T, scale=s, center=c) for T, s, c in
              ((5000, 0.6, (-1.5, -0.5, 0.2)), (2500, 0.5, (1.0, -0.9, 0.0)), (60, 0.4, (0.4, 0.6, -0.3)))]
    objs = [(m, rng.uniform(0, 0.9, (3, 4)).astype(np.float32)) for m in meshes]
    lights = [((1.0, 1.0, 2.0), "point", (1.0, 1.0, 1.0), 1.0), ((-4.0, 3.0, 1.5), "point", (1.0, 1.0, 1.0), 1.0),
              ((0.0, 2.0, 0.0), "ambient", (0.9, 0.5, 1.0), 0.3)]
    return Scene(gpu, oracle, (0.02, -0.01, 4.0), (3.0, 2.0), 144, objs, lights)


# ------------------------------------------------------------------ the four forms -----------
def trace(gpu, sc, aa, bounces, flags=capi.RENDER_DEFAULT, row0=0, rows=None, band_rows=0, band_stride=0):
    """One eray_render through the general tracer: (rgb, ppm bytes, faces) of the rendered rows."""
    W, H = sc.W, sc.H
    rows = H - row0 if rows is None else rows
    rgb, face = gpu.empty((rows, W, 3), np.float32), gpu.empty((rows, W), np.int32)
    ppm = gpu.empty((rows, W, 3), np.uint8)
    gpu.memset(face.ptr, 0x7F, face.nbytes)
    gpu.memset(ppm.ptr, 0x55, ppm.nbytes)
    try:
        gpu.render(W, H, row0=row0, rows=rows, out_rgb=rgb.ptr, out_ppm=ppm.ptr, out_face=face.ptr, bounces=bounces,
                   anti_aliasing=aa, aa_seed=SEED, flags=flags, band_rows=band_rows, band_stride=band_stride)
        return rgb.numpy(), ppm.numpy(), face.numpy()
    finally:
        for a in (rgb, ppm, face):
            a.free()


def same_frame(a, b, what):
    assert_bit_equal(a[0], b[0], f"{what}: rgb")
    assert a[1].tobytes() == b[1].tobytes(), f"{what}: ppm bytes"
    assert np.array_equal(a[2], b[2]), f"{what}: faces"


def oracle_frame(sc, aa, bounces):
    return sc.oracle.render(sc.s, sc.cam, want_faces=True, bounces=bounces, anti_aliasing=aa, seed=SEED)[:2]


def four_forms(gpu, sc, aa, bounces, what, want=None, **rows):
    """default (hierarchy) = ERAY_RENDER_NO_RAY_ACCEL = ERAY_RENDER_BRUTE_FORCE = oracle (`want`: its rgb
    and faces of the rendered rows), and which form ran each time; returns the default frame."""
    tree = trace(gpu, sc, aa, bounces, **rows)
    assert gpu.trace_ray_accel_objects() > 0, f"{what}: the default form did not take the hierarchy"
    scan = trace(gpu, sc, aa, bounces, flags=capi.RENDER_NO_RAY_ACCEL, **rows)
    assert gpu.trace_ray_accel_objects() == 0, what
    brute = trace(gpu, sc, aa, bounces, flags=capi.RENDER_BRUTE_FORCE, **rows)
    assert gpu.trace_ray_accel_objects() == 0, what
    same_frame(tree, scan, f"{what}: hierarchy vs ERAY_RENDER_NO_RAY_ACCEL")
    same_frame(tree, brute, f"{what}: hierarchy vs brute force")
    if want is not None:
        assert_bit_equal(tree[0], want[0], f"{what}: rgb vs oracle")
        assert np.array_equal(tree[2], want[1]), f"{what}: faces vs oracle"
    return tree


def dropped_form(gpu, sc, aa, bounces, tree, what):
    """After drop_ray_accel the same call scans, and renders the same frame."""
    gpu.drop_ray_accel()
    again = trace(gpu, sc, aa, bounces)
    assert gpu.trace_ray_accel_objects() == 0, what
    same_frame(tree, again, f"{what}: after drop_ray_accel")


# ------------------------------------------------------------------ Spheres A, A' ------------
@pytest.fixture(scope="module")
def scene_a(gpu, oracle):
    sc = spheres_a(gpu, oracle)
    yield sc
    sc.close()


_ORACLE_A = {}


def oracle_a(scene_a, aa, bounces):
    """The oracle's frame of Spheres A, computed once per (aa, bounces) and left unchanged."""
    if (aa, bounces) not in _ORACLE_A:
        _ORACLE_A[aa, bounces] = oracle_frame(scene_a, aa, bounces)
    return _ORACLE_A[aa, bounces]


def sphere_caps(st, spheres, what):
    """The issue's caps on the oracle's statistics: every object >= 400 hit pixels, blocked and
    reaching shadow rays each >= 20 %, each sphere decides >= 10 % of the blocked ones."""
    assert min(st["hit"]) >= 400, (what, st["hit"])
    n, blocked = st["rays"], int(st["blocked"].sum())
    assert blocked >= 0.2 * n and n - blocked >= 0.2 * n, (what, blocked, n)
    for k in spheres:
        assert ((st["decider"] == k) & st["blocked"]).sum() >= 0.1 * blocked, (what, k, np.bincount(st["decider"][st["blocked"]] + 1))


def test_spheres_a_statistics(scene_a):
    """Spheres A as the oracle sees it (the figures in the issue: 760 / 739 / 1,210 hit pixels, 1,938
    of 5,418 shadow rays blocked, decided 1,340 / 598 by the spheres; 1,286 pixels differ between
    bounces 1 and 3)."""
    st = scene_a.statistics()
    sphere_caps(st, (0, 1), "Spheres A")
    b1, b3 = oracle_a(scene_a, 0, 1)[0], oracle_a(scene_a, 0, 3)[0]
    assert not np.isnan(b3).any()
    assert (b1.view(np.uint32) != b3.view(np.uint32)).any(axis=2).sum() >= 500


@pytest.mark.parametrize("builder", list(BUILDERS))
@pytest.mark.parametrize("aa, bounces", [(0, 1), (0, 3), (2, 0), (5, 2)])
def test_spheres_a_four_forms(gpu, scene_a, aa, bounces, builder):
    """Spheres A (trace_kernel: 1,202 faces, nothing binned, no culling records): the spheres through
    the hierarchy (min_faces = 12), the floor by the scan.  AA = 5 is six rays per pixel."""
    info = gpu.build_ray_accel(12, **BUILDERS[builder])
    assert info["objects"] == 2 and info["faces"] == 1200, info
    what = f"Spheres A aa={aa} bounces={bounces} {builder}"
    tree = four_forms(gpu, scene_a, aa, bounces, what, want=oracle_a(scene_a, aa, bounces))
    assert gpu.trace_ray_accel_objects() == 0  # (the last form was brute force)
    dropped_form(gpu, scene_a, aa, bounces, tree, what)


def test_spheres_a_every_object_covered(gpu, scene_a):
    """min_faces = 1: the two-face floor has a hierarchy of its own too."""
    assert gpu.build_ray_accel(1)["objects"] == 3
    tree = four_forms(gpu, scene_a, 0, 3, "Spheres A min_faces=1", want=oracle_a(scene_a, 0, 3))
    dropped_form(gpu, scene_a, 0, 3, tree, "Spheres A min_faces=1")


@pytest.mark.parametrize("aa, bounces", [(0, 3), (5, 2)])
def test_spheres_a_prime_four_forms(gpu, oracle, aa, bounces):
    """Spheres A': the floor first, the camera higher (the issue's figures: 850 / 638 / 652 hit pixels,
    1,608 of 4,280 shadow rays blocked, decided 1,023 / 585 by the spheres)."""
    sc = spheres_a(gpu, oracle, prime=True)
    try:
        if aa == 0:
            sphere_caps(sc.statistics(), (1, 2), "Spheres A'")
        assert gpu.build_ray_accel(12)["objects"] == 2
        what = f"Spheres A' aa={aa} bounces={bounces}"
        tree = four_forms(gpu, sc, aa, bounces, what, want=oracle_frame(sc, aa, bounces))
        dropped_form(gpu, sc, aa, bounces, tree, what)
    finally:
        sc.close()


def test_add_object_invalidates(gpu, oracle):
    """eray_scene_add_object invalidates the hierarchy silently: the next render scans (0 objects) and
    shows the new object; a rebuild takes the hierarchy again."""
    sc = spheres_a(gpu, oracle)
    try:
        assert gpu.build_ray_accel(12)["objects"] == 2
        before = trace(gpu, sc, 1, 1)
        assert gpu.trace_ray_accel_objects() == 2
        ball = moved(sphere_mesh(200), (0.0, 0.3, -1.5))
        gpu.add_object(*ball, *true_box(ball))
        after = trace(gpu, sc, 1, 1)
        assert gpu.trace_ray_accel_objects() == 0
        assert after[0].tobytes() != before[0].tobytes()
        same_frame(after, trace(gpu, sc, 1, 1, flags=capi.RENDER_BRUTE_FORCE), "after add_object vs brute force")
        assert gpu.build_ray_accel(12)["objects"] == 3
        same_frame(after, trace(gpu, sc, 1, 1), "after the rebuild")
        assert gpu.trace_ray_accel_objects() == 3
    finally:
        sc.close()


# ------------------------------------------------------------------ Soup (the heavy role) ----
@pytest.fixture(scope="module")
def soup(gpu, oracle):
    sc = soup_scene(gpu, oracle)
    yield sc
    sc.close()


def heavy_bins(gpu, index=0):
    st = (ctypes.c_uint64 * 14)()
    assert capi.lib().eray_debug_bin_stats(gpu.handle, index, st) == 0
    return int(st[12])  # bins of more than kTraceHeavyMin entries


def test_soup_statistics(soup):
    """The issue's figures: 560 hit pixels (329 / 185 / 46), 894 of 1,120 shadow rays blocked."""
    st = soup.statistics()
    blocked = int(st["blocked"].sum())
    assert blocked >= 100 and st["rays"] - blocked >= 100, (blocked, st["rays"])
    assert min(st["hit"]) >= 20, st["hit"]


@pytest.mark.parametrize("aa, bounces", [(2, 1), (5, 0), (0, 2)])
def test_soup_four_forms(gpu, soup, aa, bounces):
    """trace_binned_kernel: light sub-blocks (the wave's stack in its own BinGroup<1>) and heavy ones
    (wave 0's stack behind BinGroup<4>; AA = 5 makes a second pass over the reused LDS)."""
    info = gpu.build_ray_accel(0)
    assert info["objects"] == 2 and info["faces"] == 7500, info
    what = f"Soup aa={aa} bounces={bounces}"
    tree = four_forms(gpu, soup, aa, bounces, what, want=oracle_frame(soup, aa, bounces))
    assert heavy_bins(gpu) >= 1, "no bin of more than kTraceHeavyMin entries: the heavy role did not run"
    assert 0 < (tree[2] >= 0).sum() < tree[2].size
    dropped_form(gpu, soup, aa, bounces, tree, what)


def test_soup_row_tile_and_bands(gpu, soup):
    """A row tile off the bins' phase and interleaved bands, each in the four forms, against the rows
    of the whole frame."""
    assert gpu.build_ray_accel(0)["objects"] == 2
    aa, bounces = 2, 1
    ref = oracle_frame(soup, aa, bounces)
    whole = four_forms(gpu, soup, aa, bounces, "Soup frame", want=ref)
    tile = four_forms(gpu, soup, aa, bounces, "Soup row tile", want=(ref[0][6:56], ref[1][6:56]), row0=6, rows=50)
    assert_bit_equal(tile[0], whole[0][6:56], "row tile vs frame")
    rows = np.array([4 + (j >> 2) * 8 + (j & 3) for j in range(44)])
    bands = four_forms(gpu, soup, aa, bounces, "Soup bands", want=(ref[0][rows], ref[1][rows]), row0=4, rows=44,
                       band_rows=4, band_stride=8)
    assert_bit_equal(bands[0], whole[0][rows], "bands vs frame")
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ small scenes -------------
@pytest.mark.parametrize("kind", ["live-mask", "no-mask"])
def test_small_scenes(gpu, oracle, kind):
    """trace_kernel's two camera-ray searches with a hierarchy: at most 256 faces in the scene (the
    culling records' live mask stays in use), and more than 256 with nothing binned (no mask: the
    camera rays go through the hierarchy as well).  min_faces = 1, AA = 2, bounces = 2."""
    half = np.full((1, 1), 0.5, np.float32)
    if kind == "live-mask":
        sc = spheres_a(gpu, oracle, faces=100)
    else:
        ball = sphere_mesh(200)
        objs = [(moved(ball, s), half) for s in ((-1.05, 0.0, 0.0), (1.05, 0.0, 0.0), (0.0, 1.3, -0.6))]
        sc = Scene(gpu, oracle, (0.0, 0.1, 2.2), (60.0, 60.0), 64, objs, sphere_lights())
    try:
        total = sum(m[0].shape[0] for m in sc.meshes)
        assert (total <= 256) == (kind == "live-mask"), total
        st = sc.statistics()
        assert min(st["hit"]) >= 100 and st["blocked"].sum() >= 100, (st["hit"], st["blocked"].sum())
        assert gpu.build_ray_accel(1)["objects"] == 3
        tree = four_forms(gpu, sc, 2, 2, kind, want=oracle_frame(sc, 2, 2))
        dropped_form(gpu, sc, 2, 2, tree, kind)
    finally:
        sc.close()


# ------------------------------------------------------------------ uncovered rays -----------
def far_scene(gpu, oracle):
    """Two reflective 600-face spheres that face each other across the camera, the whole scene scaled
    by 2^39 and moved to z = 2^41, the camera centre at z = 2^41 exactly.  Up there Camera::pixel_to_ray
    loses z_dist (2^41 - 1 == 2^41 in f32), so the camera rays fan out in the plane z = 2^41 — through
    the spheres' equators — and every hit point has |P|_1 >= 2^41 - 2^39.  The lights' brightness is
    the scale (falloff is 1 / distance) and the spheres have a colour, so a blocked shadow ray shows."""
    s, z = np.float32(2.0 ** 39), np.float32(2.0 ** 41)
    half = np.full((1, 1), 0.5, np.float32)

    def far(mesh):
        pos = mesh[0].reshape(-1, 3) * s + np.float32([0.0, 0.0, z])
        return pos.reshape(-1, 9).astype(np.float32), mesh[1], mesh[2]

    ball = sphere_mesh(600)
    tint = np.float32([[[0.9, 0.8, 0.7]]])
    objs = [(far(moved(ball, (-1.6, 0.0, 0.0))), half, tint), (far(moved(ball, (1.6, 0.0, 0.0))), half, tint)]
    lights = [(tuple(float(v) for v in np.float32(p) * s + np.float32([0.0, 0.0, z])), "point", (1.0, 1.0, 1.0), float(s))
              for p in POINT_LIGHTS] + [AMBIENT]
    return Scene(gpu, oracle, (0.0, 0.0, float(z)), (60.0, 60.0), 64, objs, lights)


def test_rays_the_proof_does_not_cover(gpu, oracle):
    """A camera centre with a coordinate of 2^41: every shadow and reflected ray starts beyond
    |o|_1 <= 2^40, where the margin proof does not hold, and takes the fallback scan inside the
    hierarchy form.  Hierarchy form = brute force (and the oracle)."""
    sc = far_scene(gpu, oracle)
    try:
        assert np.float32(sc.centre[2]) == np.float32(2.0 ** 41)
        st = sc.statistics()
        assert min(st["hit"]) >= 300, st["hit"]
        assert (np.abs(st["starts"]).sum(1) > 2.0 ** 40).all()
        assert st["blocked"].sum() >= 100 and (~st["blocked"]).sum() >= 100, (st["blocked"].sum(), st["rays"])
        assert gpu.build_ray_accel(12)["objects"] == 2
        tree = four_forms(gpu, sc, 1, 2, "uncovered rays", want=oracle_frame(sc, 1, 2))
        assert (tree[2] >= 0).sum() >= 600
        assert tree[0].tobytes() != trace(gpu, sc, 1, 0)[0].tobytes()  # reflected rays find something
        dropped_form(gpu, sc, 1, 2, tree, "uncovered rays")
    finally:
        sc.close()


# ------------------------------------------------------------------ graphs, invalidation -----
def frames(gpu, sc, n=3, flags=capi.RENDER_DEFAULT, aa=1, bounces=1):
    """eray_render_frames: n replayed frames into the same outputs."""
    W, H = sc.W, sc.H
    rgb, face, ppm = gpu.empty((H, W, 3), np.float32), gpu.empty((H, W), np.int32), gpu.empty((H, W, 3), np.uint8)
    gpu.memset(rgb.ptr, 0xFF, rgb.nbytes)
    try:
        gpu.render_frames(n, W, H, out_rgb=rgb.ptr, out_ppm=ppm.ptr, out_face=face.ptr, flags=flags, bounces=bounces,
                          anti_aliasing=aa, aa_seed=SEED)
        gpu.synchronize()
        return rgb.numpy(), ppm.numpy(), face.numpy()
    finally:
        for a in (rgb, ppm, face):
            a.free()


def test_render_frames_across_builds_drops_and_refits(gpu, oracle):
    """The launch plans hold the hierarchy's addresses: after a drop, a rebuild through another
    builder and refits (in place: the same plan; the async form too) the replayed frames are the
    scene's, never a stale graph's."""
    sc = spheres_a(gpu, oracle)
    fresh = capi.Context(0)
    try:
        assert gpu.build_ray_accel(12, device=True)["objects"] == 2
        one = trace(gpu, sc, 1, 1)
        assert_bit_equal(one[0], oracle_frame(sc, 1, 1)[0], "render vs oracle")
        same_frame(one, frames(gpu, sc), "render_frames(3) vs render")
        assert gpu.trace_ray_accel_objects() == 2
        gpu.drop_ray_accel()
        same_frame(one, frames(gpu, sc), "render_frames after the drop")
        assert gpu.trace_ray_accel_objects() == 0
        assert gpu.build_ray_accel(12, refittable=True)["objects"] == 2
        same_frame(one, frames(gpu, sc), "render_frames after the rebuild")
        assert gpu.trace_ray_accel_objects() == 2
        # the left sphere moves: update_object + refit (synchronous, then on the stream)
        ball = sphere_mesh(600)
        for step, (shift, refit) in enumerate((((-1.3, 0.2, -0.2), gpu.refit_ray_accel),
                                               ((-0.95, -0.1, 0.3), gpu.refit_ray_accel_async))):
            mesh = moved(ball, shift)
            gpu.update_object(0, positions=mesh[0], bbox=true_box(mesh))
            refit()
            got = frames(gpu, sc)
            assert gpu.trace_ray_accel_objects() == 2, step
            # a fresh context given the moved arrays
            other = Scene(fresh, oracle, sc.centre, sc.fov, sc.width,
                          [(mesh, np.full((1, 1), 0.5, np.float32))] + [(m, np.full((1, 1), 0.5, np.float32)) for m in sc.meshes[1:]],
                          sphere_lights())
            try:
                want = trace(fresh, other, 1, 1)
            finally:
                other.close()
            assert got[0].tobytes() != one[0].tobytes()
            same_frame(got, want, f"render_frames after update_object + refit {step}")
    finally:
        fresh.close()
        sc.close()


def test_camera_path_with_a_hierarchy(gpu, oracle):
    """eray_render_camera_path over three cameras equals the three per-camera renders."""
    sc = spheres_a(gpu, oracle)
    W, H = sc.W, sc.H
    centres = ((0.0, 0.1, 2.2), (0.3, 0.4, 2.4), (-0.4, 0.2, 2.0))
    cams = [capi.make_camera(c, (60.0, 60.0), 64, 1.0) for c in centres]
    rgb, face = gpu.empty((H, W, 3), np.float32), gpu.empty((H, W), np.int32)
    try:
        assert gpu.build_ray_accel(12)["objects"] == 2
        want = []
        for cam in cams:
            gpu.set_camera(cam)
            want.append(trace(gpu, sc, 1, 1))
            assert gpu.trace_ray_accel_objects() == 2
        gpu.set_camera(cams[0])
        # one frame per camera into the same outputs: the last camera's frame stays
        gpu.render_camera_path(cams, W, H, out_rgb=rgb.ptr, out_face=face.ptr, bounces=1, anti_aliasing=1, aa_seed=SEED)
        gpu.synchronize()
        assert gpu.trace_ray_accel_objects() == 2
        assert_bit_equal(rgb.numpy(), want[2][0], "camera path, last camera")
        assert np.array_equal(face.numpy(), want[2][2])
        for k in range(3):  # every camera of the path, as a path that ends at it
            gpu.render_camera_path(cams[:k + 1], W, H, out_rgb=rgb.ptr, out_face=face.ptr, bounces=1, anti_aliasing=1,
                                   aa_seed=SEED)
            gpu.synchronize()
            assert_bit_equal(rgb.numpy(), want[k][0], f"camera path, camera {k}")
            assert np.array_equal(face.numpy(), want[k][2])
        assert want[0][0].tobytes() != want[1][0].tobytes() != want[2][0].tobytes()
    finally:
        rgb.free()
        face.free()
        sc.close()


# ------------------------------------------------------------------ interface ----------------
def test_interface(gpu, oracle):
    """ERAY_RENDER_NO_RAY_ACCEL is a known flag (the general tracer and the frame kernel, which
    ignores it); bit 128 is still rejected; the library exports eray_debug_trace_ray_accel."""
    sc = spheres_a(gpu, oracle, faces=100)
    W, H = sc.W, sc.H
    rgb = gpu.empty((H, W, 3), np.float32)
    try:
        plain = gpu.empty((H, W, 3), np.float32)
        gpu.render(W, H, out_rgb=plain.ptr)
        for aa in (0, 2):
            p = capi.RenderParams(W, H, 0, H, 0, aa, rgb.ptr, None, None, capi.RENDER_NO_RAY_ACCEL, SEED, 0, 0)
            assert capi.lib().eray_render(gpu.handle, ctypes.byref(p)) == capi.OK, aa
        gpu.render(W, H, out_rgb=rgb.ptr, flags=capi.RENDER_NO_RAY_ACCEL)
        assert_bit_equal(rgb.numpy(), plain.numpy(), "the frame kernel ignores the flag")
        plain.free()
        p = capi.RenderParams(W, H, 0, H, 0, 2, rgb.ptr, None, None, 128, SEED, 0, 0)
        assert capi.lib().eray_render(gpu.handle, ctypes.byref(p)) == capi.E_INVALID_ARGUMENT
        assert hasattr(capi.lib(), "eray_debug_trace_ray_accel")
        n = ctypes.c_uint32(99)
        assert capi.lib().eray_debug_trace_ray_accel(gpu.handle, ctypes.byref(n)) == capi.OK
        assert capi.lib().eray_debug_trace_ray_accel(gpu.handle, None) == capi.E_INVALID_ARGUMENT
    finally:
        rgb.free()
        sc.close()
