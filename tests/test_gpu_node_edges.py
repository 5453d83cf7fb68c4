"""The node kernels (eray_amd/csrc/shaderlib.hip) and pack_ppm_kernel (render.hip) at the shapes and
values where they can go wrong: grid-stride loops that run twice, the 64-bit index path and the
last 32-bit offset, tails and unaligned outputs, empty images, non-finite and subnormal values.

Every comparison is against the CPU oracle, bit for bit.  Every output lies between two guards of
at least 256 sentinel bytes, which must be unchanged afterwards: a kernel writes its own output only.
"""
import contextlib

import numpy as np
import pytest

from eray_amd import capi
from tests import node_refs as R
from tests.helpers import assert_bit_equal

pytestmark = pytest.mark.gpu

GUARD = 256
SENTINEL = 0xA5  # as f32 0xA5A5A5A5 = -2.9e-16: a texel no kernel wrote compares unequal


class Guarded:
    """`nbytes` of device output `offset` bytes past a 16-byte-aligned address, inside one
    allocation filled with SENTINEL: at least GUARD bytes of it before and after the output."""

    def __init__(self, gpu, nbytes, offset=0):
        self.gpu, self.nbytes, self.lead = gpu, int(nbytes), GUARD + offset
        self.total = self.lead + self.nbytes + GUARD
        self.buf = gpu.empty((self.total,), np.uint8)
        assert self.buf.ptr % 256 == 0, "allocations are 256-byte aligned"
        gpu.memset(self.buf.ptr, SENTINEL, self.total)
        self.ptr = self.buf.ptr + self.lead

    def read(self, shape, dtype=np.float32, byte_offset=0, out=None):
        """The output's bytes from `byte_offset` on, as `shape` of `dtype`."""
        if out is None:
            out = np.empty(shape, dtype)
        assert byte_offset + out.nbytes <= self.nbytes
        if out.nbytes:
            self.gpu.copy_to_host(out, self.ptr + byte_offset)
        return out

    def check_guards(self, what=""):
        for name, start, size in (("before", 0, self.lead), ("after", self.lead + self.nbytes, GUARD)):
            g = np.empty(size, np.uint8)
            self.gpu.copy_to_host(g, self.buf.ptr + start)
            bad = np.flatnonzero(g != SENTINEL)
            assert not bad.size, (f"{what}: {bad.size} guard bytes {name} the output were written, the first "
                                  f"{start + int(bad[0]) - self.lead} bytes from its start")


@contextlib.contextmanager
def guarded(gpu, nbytes, offset=0, what=""):
    """A guarded output; the guards are checked when the block ends without an error."""
    g = Guarded(gpu, nbytes, offset)
    try:
        yield g
        g.check_guards(what)
    finally:
        g.buf.free()


@contextlib.contextmanager
def on_device(gpu, *arrays):
    ds = [gpu.to_device(a) for a in arrays]
    try:
        yield ds
    finally:
        for d in ds:
            d.free()


def ppm_body(oracle, img):
    h, w = img.shape[:2]
    return np.frombuffer(oracle.ppm_bytes(img)[len(capi.ppm_header(w, h)):], np.uint8)


def run_rgb(gpu, oracle, w, h, r, g, b, offset=0, compare=assert_bit_equal):
    what = f"rgb {w}x{h}+{offset}"
    with on_device(gpu, r, g, b) as (dr, dg, db), guarded(gpu, 12 * w * h, offset, what) as out:
        gpu.node_rgb(w, h, dr.image(), dg.image(), db.image(), out.ptr)
        compare(out.read((h, w, 3)), oracle.node_rgb(w, h, r, g, b), what)


def run_flat(gpu, oracle, w, h, r, g, b, offset=0, compare=assert_bit_equal):
    what = f"flat {w}x{h}+{offset}"
    with guarded(gpu, 12 * w * h, offset, what) as out:
        gpu.node_flat_color(w, h, r, g, b, out.ptr)
        compare(out.read((h, w, 3)), oracle.node_flat_color(w, h, r, g, b), what)


def run_mix(gpu, oracle, w, h, left, right, factor, offset=0, compare=assert_bit_equal):
    what = f"mix {w}x{h}+{offset} of {left.shape[1]}x{left.shape[0]}, {right.shape[1]}x{right.shape[0]} by {factor}"
    with on_device(gpu, left, right) as (dl, dr), guarded(gpu, 12 * w * h, offset, what) as out:
        gpu.node_mix_color(w, h, dl.image(), dr.image(), factor, out.ptr)
        compare(out.read((h, w, 3)), oracle.node_mix_color(w, h, left, right, factor), what)


def run_pack(gpu, oracle, img, offset=0):
    h, w = img.shape[:2]
    what = f"pack {w}x{h}+{offset}"
    with on_device(gpu, img) as (d,), guarded(gpu, 3 * w * h, offset, what) as out:
        gpu.pack_ppm(d.ptr, w, h, out.ptr)
        got = out.read((3 * w * h,), np.uint8)
        ref = ppm_body(oracle, img)
        bad = np.flatnonzero(got != ref)
        assert not bad.size, f"{what}: {bad.size} bytes differ, first at {int(bad[0])}"


def run_wave(gpu, oracle, w, h, xf, yf, compare=assert_bit_equal):
    what = f"wave {w}x{h} by {xf}, {yf}"
    with guarded(gpu, 4 * w * h, 0, what) as out:
        gpu.node_wave(w, h, xf, yf, out.ptr)
        compare(out.read((h, w)), oracle.node_wave(w, h, xf, yf), what)


def run_material(gpu, w, h, params, refs, want_color=True, want_diffuse=True, compare=assert_bit_equal):
    """params: x_fac, y_fac, r, g, b, factor; refs: the oracle's (colour, diffuse) for them."""
    what = f"material {w}x{h} {params} colour={want_color} diffuse={want_diffuse}"
    with guarded(gpu, 12 * w * h if want_color else 0, 0, what + " (colour)") as c, \
            guarded(gpu, 4 * w * h if want_diffuse else 0, 0, what + " (diffuse)") as d:
        gpu.material_example(w, h, *params, c.ptr if want_color else None, d.ptr if want_diffuse else None)
        if want_color:
            compare(c.read((h, w, 3)), refs[0], what + ": colour")
        if want_diffuse:
            compare(d.read((h, w)), refs[1], what + ": diffuse")


# ------------------------------------------------------------------ 1. strided loops ----------
# The shapes lie between one and two passes of each launch (tests/node_refs.py states the launch
# capacities beside them; tests/test_node_refs.py checks the relation).
WAVE_SHAPE, MATERIAL_SHAPE, VEC_SHAPE, PACK_SHAPE = R.WAVE_SHAPE, R.MATERIAL_SHAPE, R.VEC_SHAPE, R.PACK_SHAPE
MATERIAL_PARAMS = (0.7, -1.3, 0.25, 0.5, 0.75, 0.3)  # x_fac, y_fac, r, g, b, factor


def test_wave_strided(gpu, oracle):
    run_wave(gpu, oracle, *WAVE_SHAPE, 0.7, -1.3)


@pytest.fixture(scope="module")
def material_strided_ref(oracle):
    return oracle.example_material(*MATERIAL_SHAPE, *MATERIAL_PARAMS)


@pytest.mark.parametrize("want_color,want_diffuse", [(True, True), (True, False), (False, True)],
                         ids=["colour+diffuse", "colour", "diffuse"])
def test_material_strided(gpu, material_strided_ref, want_color, want_diffuse):
    run_material(gpu, *MATERIAL_SHAPE, MATERIAL_PARAMS, material_strided_ref, want_color, want_diffuse)


def test_rgb_strided(gpu, oracle):
    w, h = VEC_SHAPE
    rng = np.random.default_rng(11)
    r = rng.random((h, w), np.float32)               # exactly n pixels
    g = rng.random((h + 2, w), np.float32)
    b = rng.random((h, w + 9), np.float32)
    run_rgb(gpu, oracle, w, h, r, g, b)


def test_flat_strided(gpu, oracle):
    run_flat(gpu, oracle, *VEC_SHAPE, 0.25, -1.0, 3.5)


def test_mix_strided(gpu, oracle):
    w, h = VEC_SHAPE
    rng = np.random.default_rng(12)
    left = rng.random((509, 1021, 3), np.float32)    # smaller than the output in both dimensions
    right = rng.random((300, 2100, 3), np.float32)   # wider than the output, shorter than it
    run_mix(gpu, oracle, w, h, left, right, 0.3)


def test_pack_strided(gpu, oracle):
    w, h = PACK_SHAPE
    img = np.random.default_rng(13).uniform(-0.5, 1.5, (h, w, 3)).astype(np.float32)
    run_pack(gpu, oracle, img)


# ------------------------------------------------------------------ 2. tails, alignment, tiny --
TAIL_SHAPES = R.TAIL_SHAPES  # n % 4 = 0, 1, 2, 3
OFFSETS = [0, 4, 8, 12]      # of the output from a 16-byte-aligned address


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("w,h", TAIL_SHAPES)
def test_rgb_tails(gpu, oracle, w, h, offset):
    """Inputs of exactly n pixels, in three shapes."""
    n = w * h
    rng = np.random.default_rng(n)
    run_rgb(gpu, oracle, w, h, rng.random((h, w), np.float32), rng.random((1, n), np.float32),
            rng.random((n, 1), np.float32), offset)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("w,h", TAIL_SHAPES)
def test_flat_tails(gpu, oracle, w, h, offset):
    run_flat(gpu, oracle, w, h, 0.25, -1.0, 3.5, offset)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("w,h", TAIL_SHAPES)
def test_mix_tails(gpu, oracle, w, h, offset):
    rng = np.random.default_rng(w * h)
    run_mix(gpu, oracle, w, h, rng.random((3, 2, 3), np.float32), rng.random((h + 1, w + 2, 3), np.float32), 0.3,
            offset)


@pytest.mark.parametrize("offset", OFFSETS)
@pytest.mark.parametrize("w,h", TAIL_SHAPES)
def test_pack_tails(gpu, oracle, w, h, offset):
    img = np.random.default_rng(w * h).uniform(-0.5, 1.5, (h, w, 3)).astype(np.float32)
    run_pack(gpu, oracle, img, offset)


MIX_INPUTS = [(1, 1), (2, 3), (11, 7)]  # w x h


@pytest.mark.parametrize("li,ri", [(0, 1), (1, 2), (2, 0), (1, 1)])
@pytest.mark.parametrize("h", [1, 7])
@pytest.mark.parametrize("w", [1, 2, 3, 5])
def test_mix_narrow_outputs(gpu, oracle, w, h, li, ri):
    """Several row carries inside one 4-texel group, and the y < h clamp of the last group."""
    rng = np.random.default_rng(100 * w + 10 * h + li)
    (lw, lh), (rw, rh) = MIX_INPUTS[li], MIX_INPUTS[ri]
    run_mix(gpu, oracle, w, h, rng.random((lh, lw, 3), np.float32), rng.random((rh, rw, 3), np.float32), 0.3)


@pytest.mark.parametrize("w,h", [(1, 1), (1, 300), (300, 1)])
def test_wave_and_material_thin(gpu, oracle, w, h):
    run_wave(gpu, oracle, w, h, 0.7, -1.3)
    refs = oracle.example_material(w, h, *MATERIAL_PARAMS)
    for want_color, want_diffuse in ((True, True), (True, False), (False, True)):
        run_material(gpu, w, h, MATERIAL_PARAMS, refs, want_color, want_diffuse)


@pytest.mark.parametrize("w,h", [(0, 5), (5, 0)])
def test_empty_images_write_nothing(gpu, w, h):
    """Every entry point returns OK for an empty image (a failure raises) and writes nothing."""
    one = np.ones((1, 1), np.float32)
    tex = np.ones((1, 1, 3), np.float32)
    with on_device(gpu, one, tex) as (d1, d3):
        calls = {
            "wave": lambda p: gpu.node_wave(w, h, 0.7, -1.3, p),
            "rgb": lambda p: gpu.node_rgb(w, h, d1.image(), d1.image(), d1.image(), p),
            "flat": lambda p: gpu.node_flat_color(w, h, 0.25, -1.0, 3.5, p),
            "mix": lambda p: gpu.node_mix_color(w, h, d3.image(), d3.image(), 0.3, p),
            "material": lambda p: gpu.material_example(w, h, *MATERIAL_PARAMS, p, p + 16),
            "pack": lambda p: gpu.pack_ppm(d3.ptr, w, h, p),
        }
        for name, call in calls.items():
            # the "output" is empty: all of the allocation is guard
            with guarded(gpu, 0, 64, f"{name} {w}x{h}") as out:
                call(out.ptr)
                gpu.synchronize()


# ------------------------------------------------------------------ 3. non-finite, extreme -----
def special_image(h, w, step_x, step_y, c=3):
    """Every value of special_values() in an h x w x c image, at a phase that moves with x, y, c."""
    v = R.special_values()
    y, x, k = np.meshgrid(np.arange(h), np.arange(w), np.arange(c), indexing="ij")
    img = v[(step_x * x + step_y * y + 5 * k) % len(v)]
    return np.ascontiguousarray(img if c > 1 else img[..., 0], np.float32)


@pytest.mark.parametrize("factor", [0.0, 1.0, -0.0, 1e-40, 0.3, -0.2, 1.2, float("inf"), float("nan")])
def test_mix_special_values(gpu, oracle, factor):
    """13 x 13 inputs pair every value with every value (left moves with x, right with y); 0.3 and
    1e-40 scale subnormal texels, so a flushed denormal changes the result."""
    left = special_image(13, 13, 1, 0)
    right = special_image(13, 13, 0, 1)
    run_mix(gpu, oracle, 17, 15, left, right, factor, compare=R.assert_bit_equal_nan)


@pytest.mark.parametrize("rgb", [(float("nan"), float("inf"), float("-inf")),
                                 (R.SUBNORMAL_MIN, -0.0, R.SUBNORMAL_MAX),
                                 (-0.0, R.FLT_MAX, -R.SUBNORMAL_MIN)])
def test_flat_special_values(gpu, oracle, rgb):
    run_flat(gpu, oracle, 7, 5, *rgb, compare=R.assert_bit_equal_nan)


def test_rgb_special_values(gpu, oracle):
    w, h = 17, 15
    run_rgb(gpu, oracle, w, h, special_image(h, w, 1, 3, 1), special_image(h + 1, w, 2, 1, 1),
            special_image(h, w + 3, 3, 5, 1), compare=R.assert_bit_equal_nan)


EXTREME_FACTORS = [0.0, -0.0, 1e-40, 1e30, float("inf"), float("nan")]
MATERIAL_EXTREMES = [(-0.0, float("inf"), 0.5, 0.25), (1.0, 0.0, -0.0, -0.0), (0.3, float("-inf"), 2.0, float("inf")),
                     (R.SUBNORMAL_MAX, 1e-40, -0.0, 0.3)]  # r, g, b, factor


@pytest.mark.parametrize("xf", EXTREME_FACTORS)
def test_wave_extreme_factors(gpu, oracle, xf):
    for yf in EXTREME_FACTORS:
        run_wave(gpu, oracle, 64, 8, xf, yf, compare=R.assert_bit_equal_nan)


@pytest.mark.parametrize("xf", EXTREME_FACTORS)
def test_material_extreme_factors(gpu, oracle, xf):
    for yf in EXTREME_FACTORS:
        for rgbf in MATERIAL_EXTREMES:
            params = (xf, yf, *rgbf)
            run_material(gpu, 64, 8, params, oracle.example_material(64, 8, *params),
                         compare=R.assert_bit_equal_nan)


# ------------------------------------------------------------------ 4. large coordinates -------
WIDE_FACTOR = {"x": 0.37, "y": -1.3}
WIDE_MATERIAL = (0.25, 0.5, 0.75, 0.3)  # r, g, b, factor
CHUNK_BYTES = 1 << 30                    # read back about 1 GB at a time


@pytest.fixture(scope="module")
def wide_refs(oracle):
    """The one-row / one-column references, computed once per (axis, height)."""
    cache = {}

    def get(axis, h):
        key = (axis, h if axis == "y" else 0)       # the row form does not depend on the height
        if key not in cache:
            fac = WIDE_FACTOR[axis]
            wave = R.factored_wave(oracle, axis, R.WIDE_W, h, fac)
            colour, diffuse = R.factored_material(oracle, axis, R.WIDE_W, h, fac, *WIDE_MATERIAL)
            cache[key] = {"wave": wave.line, "colour": colour.line, "diffuse": diffuse.line}
        return {k: R.Factored(axis, R.WIDE_W, h, line) for k, line in cache[key].items()}

    return get


def compare_rows(out, ref, channels, what):
    """Every row of the guarded image against `ref`, read back CHUNK_BYTES at a time."""
    w, h = ref.w, ref.h
    row_shape = (w, 3) if channels == 3 else (w,)
    row_bytes = 4 * w * channels
    step = max(1, CHUNK_BYTES // row_bytes)
    buf = np.empty((step,) + row_shape, np.float32)
    for y0 in range(0, h, step):
        rows = min(step, h - y0)
        got = out.read(None, out=buf[:rows], byte_offset=y0 * row_bytes)
        for k in range(rows):
            assert ref.row_equals(y0 + k, got[k]), f"{what}: row {y0 + k} differs from the oracle"


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("h", [R.NARROW_H, R.WIDE_H], ids=["narrow", "wide"])
def test_wave_large(gpu, wide_refs, h, axis):
    w = R.WIDE_W
    what = f"wave {w}x{h} along {axis}"
    with guarded(gpu, 4 * w * h, 0, what) as out:
        gpu.node_wave(w, h, *R.factored_factors(axis, WIDE_FACTOR[axis]), out.ptr)
        compare_rows(out, wide_refs(axis, h)["wave"], 1, what)


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("h", [R.NARROW_H, R.WIDE_H], ids=["narrow", "wide"])
@pytest.mark.parametrize("output", ["colour", "diffuse"])
def test_material_large(gpu, wide_refs, output, h, axis):
    """Colour and diffuse in separate calls, the other pointer null; the narrow colour image's
    last store ends at byte 2^32 - 4."""
    w = R.WIDE_W
    channels = 3 if output == "colour" else 1
    what = f"material {output} {w}x{h} along {axis}"
    with guarded(gpu, 4 * channels * w * h, 0, what) as out:
        gpu.material_example(w, h, *R.factored_factors(axis, WIDE_FACTOR[axis]), *WIDE_MATERIAL,
                             out.ptr if output == "colour" else None, out.ptr if output == "diffuse" else None)
        compare_rows(out, wide_refs(axis, h)[output], channels, what)


SLAB_TEXELS = 65_536


def compare_slabs(out, ref, what):
    """The first and last two rows and every 97th slab of 65,536 texels of a one-channel image."""
    w, n = ref.w, ref.w * ref.h
    starts = list(range(0, n, 97 * SLAB_TEXELS)) + [0, w, n - 2 * w, n - w]
    sizes = [SLAB_TEXELS] * (len(starts) - 4) + [w] * 4
    for start, size in zip(starts, sizes):
        size = min(size, n - start)
        got = out.read((size,), byte_offset=4 * start)
        want = ref.at(np.arange(start, start + size, dtype=np.int64))
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), \
            f"{what}: texels {start}..{start + size} differ from the oracle"


@pytest.mark.parametrize("axis", ["x", "y"])
@pytest.mark.parametrize("kernel", ["wave", "diffuse"])
def test_texel_index_past_2_32(gpu, wide_refs, kernel, axis):
    """More than 2^32 texels (17 GB of one-channel output): the last row starts at index 2^32 - 4,
    so an x or y derived from a truncated index is wrong there.  Slabs are compared, not the whole
    image."""
    w, h = R.WIDE_W, R.PAST_2_32_H
    what = f"{kernel} {w}x{h} along {axis}"
    factors = R.factored_factors(axis, WIDE_FACTOR[axis])
    with guarded(gpu, 4 * w * h, 0, what) as out:
        if kernel == "wave":
            gpu.node_wave(w, h, *factors, out.ptr)
        else:
            gpu.material_example(w, h, *factors, *WIDE_MATERIAL, None, out.ptr)
        compare_slabs(out, wide_refs(axis, h)[kernel], what)
