"""References and comparisons shared by tests/test_gpu_node_edges.py and its CPU companion
(tests/test_node_refs.py): the NaN-aware bit comparison, the non-finite value set, and images of
the wave node / example material whose value depends on one coordinate only, built from one row or
one column of the CPU oracle."""
from __future__ import annotations

import numpy as np

# Texels one pass of each launch covers, and a shape between one and two passes for each (some
# threads loop twice, some once).  A changed cap must prompt a changed shape.
WAVE_CAPACITY = 8192 * 256          # shaderlib.hip:23 (grid_for1): at most 8192 workgroups of kBlock = 256
MATERIAL_CAPACITY = 2 * 8192 * 256  # the same grid, shaderlib.hip:203: kMatTexels = 2 texels per thread
VEC_CAPACITY = 2048 * 256 * 4       # shaderlib.hip:29 (grid_for): at most 2048 workgroups of kBlock x kVec = 4
PACK_CAPACITY = 2048 * 256          # render.hip launch_pack_ppm: at most 2048 workgroups of 256
WAVE_SHAPE = (1531, 1801)           # w, h
MATERIAL_SHAPE = (2311, 2203)
VEC_SHAPE = (2051, 1031)            # rgb, flat, mix
PACK_SHAPE = (1031, 517)

TAIL_SHAPES = [(4, 4), (5, 5), (6, 5), (7, 5)]  # w * h % 4 = 0, 1, 2, 3

# 17,043,521 > 2^24, so (float)x rounds for the last columns.  21 * w = 357,913,941 texels is the
# largest count whose 12-byte-per-texel image stays below 4 GB (32-bit offsets in the kernels);
# 22 * w takes the 64-bit path; 252 * w = 2^32 - 4, so row 252 crosses texel index 2^32.
WIDE_W = 17_043_521
NARROW_H = 21
WIDE_H = 22
PAST_2_32_H = 253


def f32_from_bits(bits: int) -> float:
    return float(np.array([bits], np.uint32).view(np.float32)[0])


SUBNORMAL_MIN = f32_from_bits(0x00000001)
SUBNORMAL_MAX = f32_from_bits(0x007FFFFF)
FLT_MIN = f32_from_bits(0x00800000)
FLT_MAX = f32_from_bits(0x7F7FFFFF)
QNAN_BITS = 0x7FC00000


def special_values() -> np.ndarray:
    """±0, smallest and largest subnormal, FLT_MIN, FLT_MAX, ±inf, NaN, and ordinary values."""
    bits = [0x00000000, 0x80000000, 0x00000001, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000,
            0xFF800000, QNAN_BITS]
    ordinary = np.float32([0.25, -1.5, 3.0, 0.7])
    return np.concatenate([np.array(bits, np.uint32).view(np.float32), ordinary])


def assert_bit_equal_nan(got, ref, what=""):
    """`got` is NaN exactly where `ref` is (sign and payload of a NaN are not compared: x86 and
    the GPU generate different default NaNs) and bit-identical to it everywhere else."""
    got = np.ascontiguousarray(got, np.float32)
    ref = np.ascontiguousarray(ref, np.float32)
    assert got.shape == ref.shape, f"{what}: shape {got.shape} != {ref.shape}"
    nan_ref, nan_got = np.isnan(ref), np.isnan(got)
    if not np.array_equal(nan_got, nan_ref):
        idx = np.argwhere(nan_got != nan_ref)[:5].tolist()
        raise AssertionError(f"{what}: NaN positions differ ({int((nan_got != nan_ref).sum())} words); "
                             f"first at {idx}")
    g = np.where(nan_ref, np.uint32(0), got.view(np.uint32))
    r = np.where(nan_ref, np.uint32(0), ref.view(np.uint32))
    if not np.array_equal(g, r):
        idx = np.argwhere(g != r)
        first = tuple(idx[0])
        raise AssertionError(f"{what}: {len(idx)} words differ; first at {list(first)}: "
                             f"{int(g[first]):#010x} != {int(r[first]):#010x}")


class Factored:
    """A w x h image (c channels) whose texel (x, y) is line[x] (axis 'x') or line[y] (axis 'y')."""

    def __init__(self, axis: str, w: int, h: int, line: np.ndarray):
        assert axis in ("x", "y") and line.shape[0] == (w if axis == "x" else h)
        self.axis, self.w, self.h = axis, w, h
        self.line = np.ascontiguousarray(line, np.float32)

    def full(self) -> np.ndarray:
        shape = (self.h, self.w) + self.line.shape[1:]
        src = self.line[None] if self.axis == "x" else self.line[:, None]
        return np.ascontiguousarray(np.broadcast_to(src, shape))

    def at(self, index: np.ndarray) -> np.ndarray:
        """The texels of flattened (row-major) indices `index`."""
        index = np.asarray(index, np.int64)
        return self.line[index % self.w if self.axis == "x" else index // self.w]

    def row_equals(self, y: int, got_row: np.ndarray) -> bool:
        """Whether image row y is bit-identical to `got_row` (w[, c] float32)."""
        got = got_row.view(np.uint32)
        if self.axis == "x":
            return np.array_equal(got, self.line.view(np.uint32))
        return bool((got == self.line[y].view(np.uint32)).all())


def factored_factors(axis: str, fac: float) -> tuple[float, float]:
    """(x_fac, y_fac) with the other axis's factor 0: the value depends on `axis` alone."""
    return (fac, 0.0) if axis == "x" else (0.0, fac)


def factored_wave(oracle, axis: str, w: int, h: int, fac: float) -> Factored:
    """oracle.node_wave(w, h, *factored_factors(axis, fac)) from its one-row / one-column call."""
    if axis == "x":
        return Factored(axis, w, h, oracle.node_wave(w, 1, fac, 0.0)[0])
    return Factored(axis, w, h, oracle.node_wave(1, h, 0.0, fac)[:, 0])


def factored_material(oracle, axis: str, w: int, h: int, fac: float, r, g, b, factor):
    """(colour, diffuse) of oracle.example_material(w, h, *factored_factors(axis, fac), r, g, b,
    factor), by the oracle's own arithmetic on the one-row / one-column shape."""
    if axis == "x":
        c, d = oracle.example_material(w, 1, fac, 0.0, r, g, b, factor)
        return Factored(axis, w, h, c[0]), Factored(axis, w, h, d[0])
    c, d = oracle.example_material(1, h, 0.0, fac, r, g, b, factor)
    return Factored(axis, w, h, c[:, 0]), Factored(axis, w, h, d[:, 0])
