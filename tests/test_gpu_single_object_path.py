"""The frame kernel's single-object path (frame_sub.hpp render_sub<kOne>: a small scene of one object
runs a build without the object loops, the closest-object compare and the per-lane object
selection, its ObjGeom read once per sub-block and reused by the shadow test) against the CPU oracle.

Bar: out_rgb, out_ppm and out_face bit for bit the oracle's (as tests/test_gpu_render.py), and the
culled frame bit for bit the brute-force one (which keeps the general code), for every light list
and material form the builds distinguish, at two frame sizes: 70x10 (a width that is no multiple of
16, rows no multiple of 4) and 128x36.
"""
import math

import numpy as np
import pytest

from eray_amd import capi
from eray_amd.dist import band_split
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

SIZES = [(70, 10), (128, 36)]
CAM_Z = 3.0  # the cube's front face (z = 1) spans half the frame's height
CAM_CENTER = (0.0, 0.0, CAM_Z)

AMBIENT = ((0.0, 2.0, 0.0), "ambient", (1.0, 0.9, 0.8), 0.2)
POINT = ((1.0, 1.0, 2.0), "point", (1.0, 1.0, 1.0), 1.0)
POINT2 = ((-1.5, 0.5, 2.5), "point", (0.3, 0.9, 0.5), 0.7)
LIGHT_LISTS = {
    "none": [],
    "ambient_only": [AMBIENT],
    "point_only": [POINT],
    "ambient_then_point": [AMBIENT, POINT],
    "three_two_points": [POINT2, AMBIENT, POINT],
}


def fov(W, H):
    return (float(W), float(H))


def edge_x(W, H):
    """x of the frame's right edge in the plane z = 1 (Camera::pixel_to_ray: the viewport is
    2 * W / H wide at z_dist 1)."""
    return (W / H) * (CAM_Z - 1.0)


def textures(rng):
    """Small random images of different sizes (Material::get's mod_get wraps the uvs)."""
    return dict(color=rng.uniform(0, 1.2, (9, 7, 3)).astype(np.float32),
                diffuse=rng.uniform(0, 1, (5, 11)).astype(np.float32),
                specular=rng.uniform(0, 1, (6, 4)).astype(np.float32),
                specular_power=np.concatenate([np.float32([1.0, 0.5, 2.0]),
                                               rng.uniform(0.0, 40.0, 18).astype(np.float32)]).reshape(3, 7))


class Scene:
    """One scene on the GPU context and in the oracle; frees its device textures on close()."""

    def __init__(self, gpu, oracle, W, H, cam_center=CAM_CENTER):
        self.gpu, self.W, self.H = gpu, W, H
        self.keep = []
        self.o = oracle.Scene()
        self.ocam = oracle.camera(cam_center, fov(W, H), W, 1.0)
        gpu.scene_reset()
        cam = capi.make_camera(cam_center, fov(W, H), W, 1.0)
        assert capi.camera_size(cam) == (W, H)
        gpu.set_camera(cam)

    def add_object(self, mesh, lo=(0.0, 0.0, 0.0), hi=(0.0, 0.0, 0.0), **tex):
        dev = {}
        for name, img in tex.items():
            d = self.gpu.to_device(img)
            self.keep.append(d)
            dev[name] = d.image()
        idx = self.gpu.add_object(*mesh, tuple(lo), tuple(hi), **dev)
        self.o.add_object(*mesh, tuple(lo), tuple(hi), **tex)
        return idx

    def add_lights(self, lights):
        for p, var, col, b in lights:
            self.gpu.add_light(capi.make_light(p, var, col, b))
            self.o.add_light(p, var, col, b)

    def close(self):
        for d in self.keep:
            d.free()


def gpu_frame(gpu, W, H, flags=0, **kw):
    rows = kw.get("rows", H)
    rgb = gpu.empty((rows, W, 3), np.float32)
    ppm = gpu.empty((rows, W, 3), np.uint8)
    face = gpu.empty((rows, W), np.int32)
    try:
        gpu.memset(rgb.ptr, 0, rgb.nbytes)
        gpu.memset(ppm.ptr, 0, ppm.nbytes)
        gpu.memset(face.ptr, 0x7F, face.nbytes)
        gpu.render(W, H, out_rgb=rgb.ptr, out_ppm=ppm.ptr, out_face=face.ptr, flags=flags, **kw)
        gpu.synchronize()
        return rgb.numpy(), face.numpy(), ppm.numpy()
    finally:
        for a in (rgb, ppm, face):
            a.free()


def oracle_frame(oracle, sc):
    ref, ref_face, stats = oracle.render(sc.o, sc.ocam, want_faces=True)
    body = oracle.ppm_bytes(ref)
    ppm = np.frombuffer(body[len(capi.ppm_header(sc.W, sc.H)):], np.uint8).reshape(sc.H, sc.W, 3)
    return (ref, ref_face, ppm), stats


def assert_frame(got, ref, what):
    assert np.array_equal(got[1], ref[1]), f"{what}: faces"
    assert_bit_equal(got[0], ref[0], f"{what}: rgb")
    assert np.array_equal(got[2], ref[2]), f"{what}: ppm"


def check_against_oracle(gpu, oracle, sc, what, min_hits=1):
    """Culled and brute-force frames against the oracle's (so culled = brute force too)."""
    ref, stats = oracle_frame(oracle, sc)
    assert stats["hit_pixels"] >= min_hits, what
    assert_frame(gpu_frame(gpu, sc.W, sc.H), ref, f"{what}, culled")
    assert_frame(gpu_frame(gpu, sc.W, sc.H, flags=capi.RENDER_BRUTE_FORCE), ref, f"{what}, brute force")
    return ref, stats


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("lights", list(LIGHT_LISTS))
def test_light_lists(gpu, oracle, cube, W, H, lights):
    """No light, ambient only, point only, ambient listed before point, and three lights of which
    two are points with the ambient one between them: the lighting fold's order is the reference's
    — point lights in list order, then the ambient ones."""
    rng = np.random.default_rng(3)
    tex = textures(rng)
    sc = Scene(gpu, oracle, W, H)
    try:
        sc.add_object(cube, color=tex["color"], diffuse=tex["diffuse"])
        sc.add_lights(LIGHT_LISTS[lights])
        check_against_oracle(gpu, oracle, sc, f"{W}x{H} lights {lights}")
    finally:
        sc.close()


def wave_rgb_mix_graph():
    """main.rs's graph shape as shaderlib nodes: wave -> rgb, flat colour, mix."""
    return [(capi.TEXEL_WAVE, 16, 12, (1.0, 0.7), ()),
            (capi.TEXEL_FLAT_COLOR, 5, 5, (1.0, 0.2, 0.1), ()),
            (capi.TEXEL_RGB, 8, 6, (), (0, 0, 0)),
            (capi.TEXEL_MIX_COLOR, 16, 12, (0.5,), (2, 1))]


def graph_images(oracle, nodes):
    img = []
    for kind, w, h, param, ins in nodes:
        if kind == capi.TEXEL_WAVE:
            img.append(oracle.node_wave(w, h, param[0], param[1]))
        elif kind == capi.TEXEL_FLAT_COLOR:
            img.append(oracle.node_flat_color(w, h, param[0], param[1], param[2]))
        elif kind == capi.TEXEL_RGB:
            img.append(oracle.node_rgb(w, h, img[ins[0]], img[ins[1]], img[ins[2]]))
        else:
            img.append(oracle.node_mix_color(w, h, img[ins[0]], img[ins[1]], param[0]))
    return img


MATERIALS = ["no_textures", "color_only", "diffuse_only", "specular", "specular_power", "example", "texel_graph"]


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("material", MATERIALS)
def test_material_forms(gpu, oracle, cube, W, H, material):
    """Every material form that selects another build (no specular power / specular power, with or
    without the per-texel graphs) or another branch of Material::get."""
    rng = np.random.default_rng(5)
    tex = textures(rng)
    sc = Scene(gpu, oracle, W, H)
    try:
        gpu_tex = {"no_textures": [], "color_only": ["color"], "diffuse_only": ["diffuse"],
                   "specular": ["color", "diffuse", "specular"],
                   "specular_power": ["color", "specular", "specular_power"]}
        if material in gpu_tex:
            sc.add_object(cube, **{k: tex[k] for k in gpu_tex[material]})
        elif material == "example":
            # the graph evaluated per hit texel on the GPU, Material::update's images in the oracle
            color, diffuse = oracle.example_material(64, 64)
            idx = gpu.add_object(*cube)
            gpu.set_object_example_material(idx, 64, 64, 1.0, 1.0, 1.0, 0.0, 0.0, 0.5)
            sc.o.add_object(*cube, color=color, diffuse=diffuse)
        else:
            nodes = wave_rgb_mix_graph()
            img = graph_images(oracle, nodes)
            idx = gpu.add_object(*cube)
            gpu.set_object_texel_graph(idx, [capi.texel_node(k, w, h, p, ins) for k, w, h, p, ins in nodes],
                                       color=3, diffuse=0)
            sc.o.add_object(*cube, color=img[3], diffuse=img[0])
        sc.add_lights(LIGHT_LISTS["ambient_then_point"])
        check_against_oracle(gpu, oracle, sc, f"{W}x{H} material {material}")
    finally:
        sc.close()


def box_mesh(rng, center, half):
    """A cube's 12 faces (two per side, outward winding) with per-vertex normals and random uvs: a
    mesh built from vertices, which gets a real bounding box."""
    c = np.float32(center)
    corners = np.float32([[x, y, z] for x in (-1, 1) for y in (-1, 1) for z in (-1, 1)]) * np.float32(half) + c
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    pos, nrm = [], []
    for q in quads:
        a, b, cc, d = (corners[i] for i in q)
        for tri in ((a, b, cc), (a, cc, d)):
            n = np.cross(tri[1] - tri[0], tri[2] - tri[0])
            n = (n / np.linalg.norm(n)).astype(np.float32)
            pos.append(np.concatenate(tri))
            nrm.append(np.concatenate([n, n, n]))
    pos, nrm = np.float32(pos), np.float32(nrm)
    uv = rng.uniform(-0.5, 1.5, (len(pos), 6)).astype(np.float32)
    return pos, nrm, uv


def two_step_mesh(rng):
    """A slab below and a small box above it, towards the light: one object whose own faces shadow
    each other, so the shadow scan finds blockers."""
    a = box_mesh(rng, (0.0, -0.6, 0.0), (1.4, 0.2, 1.0))
    b = box_mesh(rng, (0.5, 0.1, 0.6), (0.3, 0.5, 0.3))
    return tuple(np.concatenate([x, y]) for x, y in zip(a, b))


@pytest.mark.parametrize("W,H", SIZES)
@pytest.mark.parametrize("place", ["inside", "partly_outside"])
def test_real_bounding_box_shadow_scan(gpu, oracle, W, H, place):
    """An object with a real bounding box (Object built from vertices): its shadow rays pass the box
    test, so the shadow scan runs — reusing the sub-block's ObjGeom — and some hit points are in
    shadow.  `partly_outside`: the object placed across the frame's edge."""
    rng = np.random.default_rng(8)
    tex = textures(rng)
    pos, nrm, uv = two_step_mesh(rng)
    if place == "partly_outside":
        pos = pos + np.tile(np.float32([edge_x(W, H) - 0.6, 0.3, 0.0]), 3)
    lo, hi = pos.reshape(-1, 3).min(0), pos.reshape(-1, 3).max(0)
    sc = Scene(gpu, oracle, W, H, cam_center=(0.0, 0.4, CAM_Z))
    try:
        sc.add_object((pos, nrm, uv), lo, hi, color=tex["color"], diffuse=tex["diffuse"], specular=tex["specular"])
        sc.add_lights(LIGHT_LISTS["three_two_points"])
        ref, stats = check_against_oracle(gpu, oracle, sc, f"{W}x{H} real box, {place}")
        assert stats["shadow_tests"] > 0
        if place == "partly_outside":  # some of it is in the frame's last column, not all of it in the frame
            assert (ref[1][:, -1] >= 0).any() and not (ref[1][:, 0] >= 0).any()
    finally:
        sc.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_cube_partly_outside_the_frame(gpu, oracle, cube, W, H):
    """The loaded cube (point bounding box) moved across the frame's left edge."""
    rng = np.random.default_rng(9)
    tex = textures(rng)
    pos = cube[0] + np.tile(np.float32([-edge_x(W, H), 0.2, 0.0]), 3)
    sc = Scene(gpu, oracle, W, H)
    try:
        sc.add_object((pos, cube[1], cube[2]), color=tex["color"], diffuse=tex["diffuse"])
        sc.add_lights(LIGHT_LISTS["ambient_then_point"])
        ref, _ = check_against_oracle(gpu, oracle, sc, f"{W}x{H} cube across the left edge")
        assert (ref[1][:, 0] >= 0).any() and not (ref[1][:, -1] >= 0).any()
    finally:
        sc.close()


@pytest.mark.parametrize("W,H", SIZES)
def test_two_overlapping_objects_take_the_general_path(gpu, oracle, cube, W, H):
    """Two objects that overlap on screen: the general code (object loop, closest-object compare),
    still the oracle's frame."""
    rng = np.random.default_rng(10)
    tex = textures(rng)
    near = (cube[0] * np.float32(0.5) + np.tile(np.float32([0.6, 0.2, 1.2]), 3), cube[1], cube[2])
    sc = Scene(gpu, oracle, W, H)
    try:
        sc.add_object(cube, color=tex["color"], diffuse=tex["diffuse"])
        lo, hi = near[0].reshape(-1, 3).min(0), near[0].reshape(-1, 3).max(0)
        sc.add_object(near, lo, hi, color=tex["color"][::-1].copy())
        sc.add_lights(LIGHT_LISTS["three_two_points"])
        ref, _ = check_against_oracle(gpu, oracle, sc, f"{W}x{H} two objects")
        faces = ref[1]
        assert (faces >= 0).sum() > 0
    finally:
        sc.close()


@pytest.fixture(scope="module", params=SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def cube_scene(request, gpu, oracle, cube):
    """The single-object scene of the launch-shape tests and its oracle frame, computed once."""
    W, H = request.param
    rng = np.random.default_rng(12)
    tex = textures(rng)
    sc = Scene(gpu, oracle, W, H)
    sc.add_object(cube, color=tex["color"], diffuse=tex["diffuse"])
    sc.add_lights(LIGHT_LISTS["ambient_then_point"])
    ref, stats = oracle_frame(oracle, sc)
    assert stats["hit_pixels"] > 0
    yield sc, ref
    sc.close()


def reset_scene(gpu, sc, cube):
    """The module's scene back on the shared context (another test may have replaced it)."""
    gpu.scene_reset()
    gpu.set_camera(capi.make_camera(CAM_CENTER, fov(sc.W, sc.H), sc.W, 1.0))
    gpu.add_object(*cube, color=sc.keep[0].image(), diffuse=sc.keep[1].image())
    for p, var, col, b in LIGHT_LISTS["ambient_then_point"]:
        gpu.add_light(capi.make_light(p, var, col, b))


class Ring:
    """`slots` output slots of rows x W (f32 RGB, PPM bytes, faces), each slot's bytes rounded up to
    the 16 the ring's strides must be multiples of (70 x 10 PPM bytes are not)."""

    def __init__(self, ctx, slots, rows, W):
        self.ctx, self.slots, self.rows, self.W = ctx, slots, rows, W
        px = rows * W
        self.nbytes = (12 * px, 3 * px, 4 * px)
        self.stride = tuple((n + 15) // 16 * 16 for n in self.nbytes)
        self.bufs = [ctx.empty((slots * st,), np.uint8) for st in self.stride]
        for a, v in zip(self.bufs, (0, 0, 0x7F)):
            ctx.memset(a.ptr, v, a.nbytes)

    def kw(self):
        return dict(out_rgb=self.bufs[0].ptr, out_ppm=self.bufs[1].ptr, out_face=self.bufs[2].ptr)

    def ring(self, per_launch):
        return capi.FrameRing(self.slots, per_launch, *self.stride)

    def get(self):
        """(rgb, face, ppm), each slots x rows x W (x 3)."""
        self.ctx.synchronize()
        raw = [np.ascontiguousarray(a.numpy().reshape(self.slots, st)[:, :n])
               for a, st, n in zip(self.bufs, self.stride, self.nbytes)]
        shape = (self.slots, self.rows, self.W)
        return (raw[0].view(np.float32).reshape(*shape, 3), raw[2].view(np.int32).reshape(shape),
                raw[1].reshape(*shape, 3))

    def free(self):
        for a in self.bufs:
            a.free()


# frames per launch: the ring takes powers of two, so a launch of 3 frames is the partial launch of
# 3 frames into a ring of 4 per launch
@pytest.mark.parametrize("per_launch,frames", [(1, 8), (4, 3), (8, 8)], ids=["1", "3", "8"])
def test_ring_frames_per_launch(gpu, cube, cube_scene, per_launch, frames):
    sc, ref = cube_scene
    reset_scene(gpu, sc, cube)
    for flags in (capi.RENDER_DEFAULT, capi.RENDER_BRUTE_FORCE):
        ring = Ring(gpu, 8, sc.H, sc.W)
        try:
            gpu.render_frames(frames, sc.W, sc.H, ring=ring.ring(per_launch), flags=flags,
                              **ring.kw())
            got = ring.get()
            for s in range(frames):
                assert_frame(tuple(a[s] for a in got), ref, f"slot {s}, {frames} frames, flags {flags}")
        finally:
            ring.free()


def test_camera_path_device_camera_build(gpu, oracle, cube, cube_scene):
    """render_camera_path: the per-camera setup on the device and the device-camera build; every
    slot is the oracle's frame for its camera."""
    sc, _ = cube_scene
    reset_scene(gpu, sc, cube)
    W, H = sc.W, sc.H
    # (on the view axis: the loaded cube's box is the point at the origin, object.rs:306-315)
    path = [((0.0, 0.0, CAM_Z + 0.8 * math.sin(math.pi * k / 4.0)), 1.0 + 0.3 * math.cos(math.pi * k / 4.0))
            for k in range(8)]
    cams = [capi.make_camera(c, fov(W, H), W, zd) for c, zd in path]
    for flags in (capi.RENDER_DEFAULT, capi.RENDER_BRUTE_FORCE):
        ring = Ring(gpu, 8, H, W)
        try:
            gpu.render_camera_path(cams, W, H, ring=ring.ring(4), flags=flags, **ring.kw())
            got = ring.get()
            for s, (c, zd) in enumerate(path):
                ref, ref_face, stats = oracle.render(sc.o, oracle.camera(c, fov(W, H), W, zd), want_faces=True)
                assert stats["hit_pixels"] > 0
                body = oracle.ppm_bytes(ref)
                ppm = np.frombuffer(body[len(capi.ppm_header(W, H)):], np.uint8).reshape(H, W, 3)
                assert_frame(tuple(a[s] for a in got), (ref, ref_face, ppm), f"camera {s}, flags {flags}")
        finally:
            ring.free()
    gpu.set_camera(capi.make_camera(CAM_CENTER, fov(W, H), W, 1.0))


@pytest.mark.parametrize("rank", [0, 1])
def test_band_rows_of_a_two_way_split(gpu, cube, cube_scene, rank):
    """A rank's interleaved row bands of a 2-way split: its local rows are the oracle frame's
    camera rows of those bands, its PPM rows the same rows bottom-up."""
    sc, ref = cube_scene
    reset_scene(gpu, sc, cube)
    W, H = sc.W, sc.H
    sp = band_split(rank, 2, H)
    kw = dict(row0=sp["row0"], rows=sp["rows"], band_rows=sp["band_rows"], band_stride=sp["band_stride"])
    band = sp["band_rows"] if sp["band_rows"] else sp["rows"]
    stride = sp["band_stride"] if sp["band_rows"] else 0
    cam_rows = np.array([sp["row0"] + (j // band) * stride + (j % band) for j in range(sp["rows"])])
    assert cam_rows.max() < H
    want = (ref[0][cam_rows], ref[1][cam_rows], ref[2][H - 1 - cam_rows][::-1])
    for flags in (capi.RENDER_DEFAULT, capi.RENDER_BRUTE_FORCE):
        assert_frame(gpu_frame(gpu, W, H, flags=flags, **kw), want, f"rank {rank} of 2, flags {flags}")
