"""GPU parity of the ray queries with the ORACLE, not with themselves: eray_cast_rays' out_hit (the
scene and every single object) and out_rgb (bounces 0, 1 and 3) and eray_rays_reach_light's words
against oracle.cast_rays / oracle.reach_light (thin loops over Engine::cast_ray, Object::intersects
and Engine::reaches_light), for rays that do not start at the camera, every material output
textured, non-integer specular powers, per-texel reflection gates, two point and two ambient
lights.

Each comparison runs in four forms: the LDS tiles (no hierarchy), ERAY_RAYS_BRUTE_FORCE, the
host-built hierarchy and the device-built one (both with min_faces = 1), each with and without
ERAY_RAYS_NORMALIZE.  Everything is compared on bits under ray_refs.assert_words_equal's NaN rule.
The scene, its rays, the conditions it must meet as an input and the hand-derived case are
tests/ray_refs.py's, shared with tests/test_oracle_rays.py, which checks them without a GPU."""
import numpy as np
import pytest

from eray_amd import capi
from tests import ray_refs as R
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

FORMS = ("tiles", "brute force", "host-built", "device-built")
BOUNCES = (0, 1, 3)


def load_scene(gpu, desc, keep):
    """The description on the device; its images go to device memory once and stay in `keep`."""
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera(desc["centre"], (60.0, 60.0), 64, 1.0))
    for i, o in enumerate(desc["objects"]):
        images = {}
        for name in R.IMAGES:
            if o.get(name) is not None:
                if (i, name) not in keep:
                    keep[i, name] = gpu.to_device(np.ascontiguousarray(o[name], np.float32))
                images[name] = keep[i, name].image()
        gpu.add_object(*o["mesh"], tuple(o["box"][0]), tuple(o["box"][1]), **images)
    for position, variant, color, brightness in desc["lights"]:
        gpu.add_light(capi.make_light(position, variant, color, brightness))


def enter_form(gpu, form):
    """Puts the loaded scene into one of the four forms; returns cast_rays' brute_force flag and
    the build's info (None without a hierarchy)."""
    gpu.drop_ray_accel()
    info = None
    if form == "host-built":
        info = gpu.build_ray_accel(1)
    elif form == "device-built":
        info = gpu.build_ray_accel(1, device=True)
    return form == "brute force", info


def as_oracle(hits, dtype):
    """The device's records under the oracle binding's dtype (the same 48 bytes)."""
    assert hits.dtype.itemsize == dtype.itemsize == 48
    return hits.view(dtype)


# ------------------------------------------------------------------ the mixed scene ----------
@pytest.fixture(scope="module")
def mixed(oracle, cube):
    """The scene, its rays and segments, the conditions on them (from the oracle alone) and the
    oracle's answers, computed once."""
    desc = R.mixed_scene(cube)
    rays, sets = R.mixed_rays(oracle, desc)
    R.mixed_conditions(oracle, desc, rays, sets)  # a failure here is the input's, not the kernel's
    seg, targets = R.mixed_segments(oracle, desc, rays, sets)
    scene, cam = R.oracle_scene(oracle, desc), R.oracle_camera(oracle, desc)
    want = {}
    for nz in (False, True):
        want["hit", nz, -1] = oracle.cast_rays(scene, cam, rays, normalize=nz)
        for k in range(len(desc["objects"])):
            want["hit", nz, k] = oracle.cast_rays(scene, cam, rays, normalize=nz, object=k)
        for b in BOUNCES:
            want["rgb", nz, b] = oracle.cast_rays(scene, cam, rays, bounces=b, normalize=nz, want_rgb=True)[1]
        want["reach", nz] = oracle.reach_light(scene, seg, targets, normalize=nz)
        for part in (slice(0, 2048), slice(2048, 4096), slice(4096, 5120)):
            assert (want["reach", nz][part] == 0).sum() >= 100 and (want["reach", nz][part] == 1).sum() >= 100
    return dict(desc=desc, rays=rays, seg=seg, targets=targets, want=want, oracle=oracle)


@pytest.fixture(scope="module")
def images(gpu):
    keep = {}
    yield keep
    gpu.scene_reset()
    for a in keep.values():
        a.free()


@pytest.mark.parametrize("normalize", [False, True], ids=["stored-dir", "normalize"])
@pytest.mark.parametrize("form", FORMS)
def test_hit_records_equal_the_oracle(gpu, mixed, images, form, normalize):
    """out_hit for object = -1 (cast_ray's winner, by the distance to the camera's centre,
    engine.rs:120) and for each object alone."""
    load_scene(gpu, mixed["desc"], images)
    brute, info = enter_form(gpu, form)
    if info is not None:
        assert info["objects"] == 4 and info["faces"] == 12 + 600 + 2 + 40 and info["unculled_faces"] < info["faces"], info
    dtype = mixed["oracle"].HIT_DTYPE
    for obj in (-1, 0, 1, 2, 3):
        got = gpu.cast_rays(mixed["rays"], object=obj, normalize=normalize, brute_force=brute)
        R.assert_records_equal(as_oracle(got, dtype), mixed["want"]["hit", normalize, obj], f"{form}, object={obj}")
    gpu.drop_ray_accel()


@pytest.mark.parametrize("normalize", [False, True], ids=["stored-dir", "normalize"])
@pytest.mark.parametrize("form", FORMS)
def test_out_rgb_equals_the_oracle(gpu, mixed, images, form, normalize):
    """out_rgb = color_sum(cast_ray(ray, 0)) for bounces 0, 1 and 3: every material image through
    Material::get's saturating cast and wrap (material.rs:56-94), the per-texel reflection gate
    (engine.rs:181), powf's NaN for a negative base and a non-integer power, which clamp keeps
    (engine.rs:165-174), and the selection by the camera's centre at every depth."""
    load_scene(gpu, mixed["desc"], images)
    brute, _ = enter_form(gpu, form)
    for b in BOUNCES:
        got = gpu.cast_rays(mixed["rays"], bounces=b, normalize=normalize, brute_force=brute, want_hits=False, want_rgb=True)
        R.assert_words_equal(got, mixed["want"]["rgb", normalize, b], f"{form}, bounces={b}")
    gpu.drop_ray_accel()


@pytest.mark.parametrize("normalize", [False, True], ids=["stored-dir", "normalize"])
@pytest.mark.parametrize("form", FORMS)
def test_reach_words_equal_the_oracle(gpu, mixed, images, form, normalize):
    """eray_rays_reach_light against Engine::reaches_light (engine.rs:218-228): 2,048 of the scene's
    own shadow rays, 2,048 random segments, and 1,024 whose target lies on or one float from the
    deciding hit, where `len > len` and a comparison of squared lengths part."""
    load_scene(gpu, mixed["desc"], images)
    brute, _ = enter_form(gpu, form)
    got = gpu.rays_reach_light(mixed["seg"], mixed["targets"], normalize=normalize, brute_force=brute)
    want = mixed["want"]["reach", normalize]
    assert got.dtype == np.uint32 and got.shape == want.shape
    bad = np.flatnonzero(got != want)
    assert not bad.size, f"{form}: {bad.size} words differ, first {bad[:5].tolist()}"
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ the moved spheres --------
@pytest.mark.parametrize("move", R.MOVES, ids=[f"s{s:g}-t{t:g}-k{k:g}" for s, t, k in R.MOVES])
def test_moved_sphere_records_equal_the_oracle(gpu, oracle, move):
    """displaced_sphere(600, 42) at x * s + t with directions scaled by s * k, and rays on and one
    float to either side of the bounds 2^-40 and 2^40 of |d|inf that the hierarchy's margin proof
    covers: out_hit is the oracle's in all four forms, and the hierarchy holds faces (the CPU walk
    harness, tests/test_accel_host.py, finds the same for these settings)."""
    mesh, rays = R.moved_sphere(*move)
    box = R.true_box(mesh)
    desc = dict(objects=[dict(mesh=mesh, box=box)], lights=[], centre=(0.0, 0.0, 5.0))
    scene, cam = R.oracle_scene(oracle, desc), R.oracle_camera(oracle, desc)
    want = {nz: oracle.cast_rays(scene, cam, rays, normalize=nz) for nz in (False, True)}
    assert (want[False]["object"] >= 0).sum() >= 200 and (want[False]["object"] < 0).sum() >= 200  # (the input's)
    load_scene(gpu, desc, {})
    for form in FORMS:
        brute, info = enter_form(gpu, form)
        if info is not None:
            assert info["objects"] == 1 and info["faces"] == 600 and info["unculled_faces"] < 600 and info["nodes"] > 0, info
        for nz in (False, True):
            got = gpu.cast_rays(rays, normalize=nz, brute_force=brute)
            R.assert_records_equal(as_oracle(got, oracle.HIT_DTYPE), want[nz], f"{form}, normalize={nz}")
    gpu.drop_ray_accel()


# ------------------------------------------------------------------ the hand-derived case ----
def test_hand_derived_case(gpu):
    """ray_refs.hand_case on the device: the record, the colour of engine.rs:143-176 and the reach
    words, worked in scalar f32 from the Rust source with no call into the oracle."""
    case = R.hand_case()
    keep = {}
    try:
        load_scene(gpu, case["scene"], keep)
        want = R.hand_record(capi.HIT_DTYPE, case)
        for form in FORMS:
            brute, _ = enter_form(gpu, form)
            for obj in (-1, 0):
                got = gpu.cast_rays(case["rays"], object=obj, normalize=True, brute_force=brute)
                R.assert_records_equal(got, want, f"{form}, object={obj}")
            rgb = gpu.cast_rays(case["rays"], bounces=2, normalize=True, brute_force=brute, want_hits=False, want_rgb=True)
            assert_bit_equal(rgb, case["rgb"], f"{form}: rgb")
            words = gpu.rays_reach_light(case["segments"], case["targets"], brute_force=brute)
            assert words.tolist() == case["reach"].tolist(), form
        gpu.drop_ray_accel()
    finally:
        gpu.scene_reset()
        for a in keep.values():
            a.free()
