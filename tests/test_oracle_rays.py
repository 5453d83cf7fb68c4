"""The oracle's entry points for caller-supplied rays (oracle_cast_rays, oracle_rays_reach_light:
thin loops over Engine::cast_ray, Object::intersects and Engine::reaches_light), tied on the CPU to
what already pins the oracle: its render (the golden digests' path) for camera rays, the per-face
loop over Triangle::intersects for single-object records, a numpy composition of per-object records
for the reach words, and one case worked by hand from the Rust source.  No GPU."""
import numpy as np
import pytest

from tests import ray_refs as R
from tests.helpers import assert_bit_equal, random_mesh


def camera_rays(oracle, cam):
    """cast_ray_from_camera(x as f32 / W, y as f32 / H) (engine.rs:100-109) of every pixel."""
    W, H = oracle.camera_size(cam)
    rays = np.empty((H, W, 6), np.float32)
    for y in range(H):
        for x in range(W):
            rays[y, x, :3], rays[y, x, 3:] = oracle.pixel_to_ray(cam, np.float32(x) / np.float32(W), np.float32(y) / np.float32(H))
    return rays.reshape(-1, 6), W, H


def cube_scene(oracle, cube):
    s = oracle.Scene()
    s.add_object(*cube)  # default materials, the loader's (0,0,0) box: passes on the axis
    s.add_light((0.0, 2.0, 0.0), "ambient", (1.0, 1.0, 1.0), 0.2)
    s.add_light((1.0, 1.0, 2.0), "point", (1.0, 1.0, 1.0), 1.0)
    return s, (0.0, 0.0, 3.0)


def random_scene(oracle, cube):
    rng = np.random.default_rng(3)
    refl = rng.uniform(0.1, 0.9, (5, 7)).astype(np.float32)
    refl[rng.uniform(size=refl.shape) < 0.3] = 0.0
    s = oracle.Scene()
    s.add_object(*cube, (-1.0, -1.0, -1.0), (1.0, 1.0, 1.0), reflection=refl,
                 specular_power=np.float32([[2.5, 1.0], [7.3, 30.1]]))
    for centre, T in (((0.9, 0.3, 0.2), 120), ((-1.0, -0.2, 0.6), 60)):
        m = random_mesh(rng, T, scale=0.8, center=centre)
        s.add_object(*m, *R.true_box(m), color=rng.uniform(0, 1.2, (6, 9, 3)).astype(np.float32),
                     diffuse=rng.uniform(0.1, 1.0, (2, 3)).astype(np.float32), reflection=refl)
    s.add_light((1.0, 1.0, 2.0), "point", (1.0, 0.9, 0.8), 1.0)
    s.add_light((0.0, 2.0, 0.0), "ambient", (0.9, 0.5, 1.0), 0.3)
    s.add_light((-2.0, 2.5, 1.0), "point", (0.5, 0.7, 1.0), 1.5)
    return s, (0.3, 0.2, 4.0)


@pytest.mark.parametrize("make", [cube_scene, random_scene], ids=["cube", "random"])
def test_camera_rays_equal_the_render(oracle, cube, make):
    """pixel_to_ray's rays (stored directions) through oracle.cast_rays give oracle.render's colours
    and faces, bit for bit, for bounces 0 and 2: the new loop runs the path the goldens pin."""
    s, centre = make(oracle, cube)
    cam = oracle.camera(centre, (60.0, 60.0), 64, 1.0)
    rays, W, H = camera_rays(oracle, cam)
    assert (W, H) == (64, 64)
    frames = {}
    for bounces in (0, 2):
        ref, ref_face, _ = oracle.render(s, cam, want_faces=True, bounces=bounces)
        assert (ref_face >= 0).sum() > 100 and (ref_face < 0).sum() > 100
        hits, rgb = oracle.cast_rays(s, cam, rays, bounces=bounces, want_rgb=True)
        R.assert_words_equal(rgb.reshape(H, W, 3), ref, f"bounces={bounces}: rgb")
        assert np.array_equal(np.where(hits["object"] >= 0, hits["face"], -1), ref_face.reshape(-1))
        assert not hits[hits["object"] < 0].view(np.uint8).reshape(-1, 48)[:, 4:].any()  # a miss: -1, then zeros
        frames[bounces] = ref
    if make is random_scene:
        assert not np.array_equal(frames[0].view(np.uint32), frames[2].view(np.uint32))  # the reflection image is live
        assert len(set(hits["object"].tolist())) == 4  # every object and the miss


@pytest.fixture(scope="module")
def soup300(oracle):
    rng = np.random.default_rng(7)
    mesh = R.soup(rng, 300)
    start, raw = R.sphere_rays(rng, 248)
    # rays with a zero direction component: infinite slabs, and NaN ones where the start lies on
    # the slab's plane (0 * inf)
    extra_s = np.float32([[0.3, -0.2, 3.0], [0.0, 0.0, 3.0], [1.2, 0.1, 3.0], [-3.0, 0.5, 0.5], [0.5, 3.0, 1.2],
                          [0.5, 0.5, 2.0], [1.2, 1.2, -3.0], [0.0, -3.0, 0.0]])
    extra_d = np.float32([[0.0, 0.0, -1.0], [0.0, 0.0, -2.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0], [0.0, -1.0, 0.0],
                          [0.0, -0.5, -1.0], [0.0, 0.0, 1.0], [0.0, 1.0, 0.0]])
    start, raw = np.concatenate([start, extra_s]), np.concatenate([raw, extra_d])
    return {"mesh": mesh, "start": start, "raw": raw, "first": R.first_hits(oracle, mesh, start, raw)}


def test_single_object_records_equal_the_per_face_loop(oracle, soup300):
    """300 faces, 256 rays: oracle.cast_rays(object=k) is the per-face Python loop over
    Triangle::intersects with BoundingBox::intersects in front of it, for a wide, a tight and the
    loader's point box, with Ray::new and with the already normalised direction stored."""
    A = soup300
    d = R.normalize_f32(A["raw"])
    cam = oracle.camera((0.0, 0.0, 5.0), (60.0, 60.0), 64, 1.0)
    assert A["start"].shape[0] == 256
    for h in (1.2, 0.5, 0.0):
        want, rejected = R.with_box(A["first"], (-h,) * 3, (h,) * 3, A["start"], d)
        if h == 1.2:
            assert (want["object"] >= 0).sum() >= 50 and (want["object"] < 0).sum() >= 50 and not rejected[:248].any()
            assert ((want["object"] >= 0) & (want["face"] >= 100)).sum() >= 10
        if h == 0.5:
            assert rejected.sum() >= 50 and (want["object"] >= 0).sum() >= 25
        s = oracle.Scene()
        other = R.soup(np.random.default_rng(1), 5)
        s.add_object(*other, (-9.0,) * 3, (9.0,) * 3)  # object 0 is another mesh: k selects, nothing else
        s.add_object(*A["mesh"], (-h,) * 3, (h,) * 3)
        want["object"][want["object"] >= 0] = 1
        got = oracle.cast_rays(s, cam, R.rays_array(A["start"], A["raw"]), normalize=True, object=1)
        R.assert_records_equal(got, want, f"box {h}, Ray::new")
        got = oracle.cast_rays(s, cam, R.rays_array(A["start"], d), object=1)
        R.assert_records_equal(got, want, f"box {h}, stored dir")


@pytest.fixture(scope="module")
def mixed(oracle, cube):
    desc = R.mixed_scene(cube)
    rays, sets = R.mixed_rays(oracle, desc)
    return desc, rays, sets


def test_mixed_scene_meets_its_conditions(oracle, mixed):
    """The input of tests/test_gpu_rays_oracle.py does what that file needs of it (every object
    wins rays, misses, live reflections, blocked and reaching lights, NaN colours, reflected rays on
    which the two selection rules differ), judged from the oracle's output alone."""
    fig = R.mixed_conditions(oracle, *mixed)
    print(fig)


def test_scene_records_are_the_selection_over_single_object_records(oracle, mixed):
    """object = -1 is cast_ray's own winner: the same records as engine.rs:116-126's rule applied to
    the object = k records in numpy."""
    desc, rays, _ = mixed
    scene, cam = R.oracle_scene(oracle, desc), R.oracle_camera(oracle, desc)
    for nz in (False, True):
        per = [oracle.cast_rays(scene, cam, rays, normalize=nz, object=k) for k in range(4)]
        got = oracle.cast_rays(scene, cam, rays, normalize=nz)
        R.assert_records_equal(got, R.closest_by_centre(per, desc["centre"]), f"normalize={nz}")


def test_reach_equals_the_composition_of_single_object_records(oracle, mixed):
    """oracle.reach_light is engine.rs:218-228 over oracle.cast_rays(object=k): the first object in
    scene order with a hit decides, by len(position - start) > len(target - start)."""
    desc, rays, sets = mixed
    scene, cam = R.oracle_scene(oracle, desc), R.oracle_camera(oracle, desc)
    seg, targets = R.mixed_segments(oracle, desc, rays, sets)
    for nz in (False, True):
        per = [oracle.cast_rays(scene, cam, seg, normalize=nz, object=k) for k in range(4)]
        want = R.reach_from_records(per, seg[:, :3], targets)
        got = oracle.reach_light(scene, seg, targets, normalize=nz)
        assert got.dtype == np.uint32 and np.array_equal(got, want), f"normalize={nz}: {int((got != want).sum())} words differ"
        assert got.shape == (5120,)
        for half in (slice(0, 2048), slice(2048, 4096), slice(4096, 5120)):
            assert (got[half] == 0).sum() >= 100 and (got[half] == 1).sum() >= 100, (nz, half)


def test_hand_derived_case(oracle):
    """ray_refs.hand_case: the record, the colour of engine.rs:143-176 and the reach words, worked
    in scalar f32 from the Rust source."""
    case = R.hand_case()
    scene, cam = R.oracle_scene(oracle, case["scene"]), R.oracle_camera(oracle, case["scene"])
    want = R.hand_record(oracle.HIT_DTYPE, case)
    for obj in (-1, 0):
        R.assert_records_equal(oracle.cast_rays(scene, cam, case["rays"], normalize=True, object=obj), want, f"object={obj}")
    for bounces in (0, 2):  # no reflection image: the bounce never starts
        _, rgb = oracle.cast_rays(scene, cam, case["rays"], bounces=bounces, normalize=True, want_rgb=True)
        assert_bit_equal(rgb, case["rgb"], f"rgb, bounces={bounces}")
    assert oracle.reach_light(scene, case["segments"], case["targets"]).tolist() == case["reach"].tolist()
