"""CPU proof of the reference constructions tests/test_gpu_node_edges.py relies on (tests/node_refs.py):
a wave image / example material with one factor 0 equals the broadcast of the oracle's one-row or
one-column call bit for bit, and the NaN-aware comparison accepts and rejects what it should."""
import os
import re

import numpy as np
import pytest

from tests import node_refs as R
from tests.helpers import assert_bit_equal

W, H = 37, 19
# the factor patterns of the GPU tests: (axis, factor)
PATTERNS = [("x", 0.37), ("y", -1.3), ("x", -123.25), ("y", 1.0e6)]
MATERIAL = (0.25, 0.5, 0.75, 0.3)  # r, g, b, factor


@pytest.mark.parametrize("axis,fac", PATTERNS)
def test_factored_wave_is_the_oracle_image(oracle, axis, fac):
    ref = oracle.node_wave(W, H, *R.factored_factors(axis, fac))
    f = R.factored_wave(oracle, axis, W, H, fac)
    assert_bit_equal(f.full(), ref, f"wave {axis}")
    assert_bit_equal(f.at(np.arange(W * H)).reshape(H, W), ref, f"wave {axis} by index")
    assert all(f.row_equals(y, ref[y]) for y in range(H))


@pytest.mark.parametrize("axis,fac", PATTERNS)
def test_factored_material_is_the_oracle_image(oracle, axis, fac):
    c_ref, d_ref = oracle.example_material(W, H, *R.factored_factors(axis, fac), *MATERIAL)
    c, d = R.factored_material(oracle, axis, W, H, fac, *MATERIAL)
    assert_bit_equal(c.full(), c_ref, f"colour {axis}")
    assert_bit_equal(d.full(), d_ref, f"diffuse {axis}")
    assert_bit_equal(c.at(np.arange(W * H)).reshape(H, W, 3), c_ref, f"colour {axis} by index")
    assert_bit_equal(d.at(np.arange(W * H)).reshape(H, W), d_ref, f"diffuse {axis} by index")
    assert all(c.row_equals(y, c_ref[y]) and d.row_equals(y, d_ref[y]) for y in range(H))


def test_row_equals_sees_one_wrong_word(oracle):
    for axis, fac in PATTERNS[:2]:
        ref = oracle.node_wave(W, H, *R.factored_factors(axis, fac))
        f = R.factored_wave(oracle, axis, W, H, fac)
        bad = ref[H - 1].copy()
        bad.view(np.uint32)[W - 1] ^= 1
        assert not f.row_equals(H - 1, bad)


@pytest.mark.parametrize("shape,capacity", [(R.WAVE_SHAPE, R.WAVE_CAPACITY), (R.MATERIAL_SHAPE, R.MATERIAL_CAPACITY),
                                            (R.VEC_SHAPE, R.VEC_CAPACITY), (R.PACK_SHAPE, R.PACK_CAPACITY)])
def test_strided_shapes_loop_once_and_twice(shape, capacity):
    n = shape[0] * shape[1]
    assert capacity < n < 2 * capacity and n % 4 and n % 256


def test_capacities_are_the_launch_code_s():
    """The caps as the launch code states them: a changed cap fails here first."""
    csrc = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "eray_amd", "csrc")
    with open(os.path.join(csrc, "shaderlib.hip")) as f:
        shader = f.read()
    with open(os.path.join(csrc, "render.hip")) as f:
        render = f.read()

    def number(pattern, text):
        m = re.search(pattern, text, re.DOTALL)
        assert m, pattern
        return int(m.group(1))

    block = number(r"constexpr int kBlock = (\d+);", shader)
    vec = number(r"constexpr int kVec = (\d+);", shader)
    mat = number(r"constexpr int kMatTexels = (\d+);", shader)
    cap1 = number(r"grid_for1\(size_t items\) \{.*?blocks > (\d+)\)", shader)
    cap4 = number(r"grid_for\(size_t items\) \{.*?blocks > (\d+)\)", shader)
    cap_pack = number(r"hipError_t launch_pack_ppm\(.*?blocks > (\d+)\)", render)
    block_pack = number(r"pack_ppm_kernel<<<\(unsigned\)blocks, (\d+),", render)
    assert R.WAVE_CAPACITY == cap1 * block
    assert R.MATERIAL_CAPACITY == mat * cap1 * block
    assert R.VEC_CAPACITY == cap4 * block * vec
    assert R.PACK_CAPACITY == cap_pack * block_pack


def test_tail_shapes_cover_every_remainder():
    assert sorted(w * h % 4 for w, h in R.TAIL_SHAPES) == [0, 1, 2, 3]


def test_reference_keeps_subnormal_products(oracle):
    """0.7 x a subnormal texel stays a non-zero subnormal in the oracle: a kernel that flushed
    denormals would differ from it."""
    left = np.full((1, 1, 3), R.SUBNORMAL_MAX, np.float32)
    out = oracle.node_mix_color(1, 1, left, np.zeros((1, 1, 3), np.float32), 0.3)
    assert 0 < out[0, 0, 0] < R.FLT_MIN


def test_wide_shape_arithmetic():
    """The texel counts the large-coordinate tests are built around."""
    w = R.WIDE_W
    assert w > 2 ** 24 and int(np.float32(w - 2)) != w - 2             # (float)x rounds
    assert 12 * R.NARROW_H * w == 2 ** 32 - 4                         # last colour store ends at 2^32 - 4
    assert 12 * R.WIDE_H * w > 2 ** 32 - 1 > R.WIDE_H * w             # 64-bit path, indices still 32-bit
    assert (R.PAST_2_32_H - 1) * w < 2 ** 32 < R.PAST_2_32_H * w       # the last row crosses index 2^32


def test_special_values_hold_what_the_tests_need():
    v = R.special_values()
    u = v.view(np.uint32)
    for bits in (0, 0x80000000, 1, 0x007FFFFF, 0x00800000, 0x7F7FFFFF, 0x7F800000, 0xFF800000, R.QNAN_BITS):
        assert bits in u
    assert np.isnan(v).sum() == 1 and np.isinf(v).sum() == 2
    assert R.SUBNORMAL_MIN > 0 and R.SUBNORMAL_MAX < R.FLT_MIN and np.isfinite(R.FLT_MAX)


def test_nan_comparison():
    ref = np.array([1.0, np.nan, -0.0, np.inf], np.float32)
    got = ref.copy()
    got.view(np.uint32)[1] = 0xFFC00001                                # another NaN: sign and payload ignored
    R.assert_bit_equal_nan(got, ref)
    for i, bits in ((0, 0x3F800001), (1, 0x3F800000), (2, 0x00000000), (3, 0x7FC00000)):
        bad = got.copy()
        bad.view(np.uint32)[i] = bits                                  # 1 ulp off, NaN lost, -0 -> +0, NaN gained
        with pytest.raises(AssertionError):
            R.assert_bit_equal_nan(bad, ref)
    with pytest.raises(AssertionError):
        R.assert_bit_equal_nan(got[:3], ref)
