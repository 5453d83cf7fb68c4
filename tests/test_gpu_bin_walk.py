"""The screen bins' unit walk, append and sort (bin_walk.hpp walk_units / append_entries,
bin_pairs.hpp, bin_place.hpp bin_sort_kernel) on one hand-made object at 1920x1080 whose faces meet
every case of the walk:

- 16 camera-facing triangles that each cover the whole frame, at staggered depths: in the pair form
  the walk has 16 x 120 x 270 units, more than 256 CUs x 6 workgroups x 256 lanes, so some wave's
  range spans more than one 64-unit slice whatever the resident grid is, and every face spans many
  slices;
- 150 faces without units (back-facing, or behind the camera) between them: the first and last
  faces, pairs between the full-frame ones, a run of 70 (longer than a slice's 64 faces), and one
  after each of the last 40 one-bin faces;
- 120 faces whose rectangle is exactly one bin at row phase 0 (one unit of the pair form's walk,
  w = h = 1: a face inside one pixel row, which face_rect.hpp widens to that bin's four rows), each
  in a bin of its own: 80 in a row, so that whole 64-unit slices are one-unit faces and slice
  boundaries fall between them, then 40 with an empty face after each; the test asserts the pair
  form's unit count, which leaves them one unit each;
- 50 small faces inside one bin each, two pixel rows tall (their widened rectangles are two bins);
- 300 tiny faces stacked over one bin and 100 over another: with the 16 full-frame faces a bin of
  316 entries (sorted by a workgroup), one of 116 (sorted by a wave), and the rest of at most 64
  (unsorted).

Bar: the pair form's bins against the segment form's (the relation of
test_gpu_configs.py test_bin_segments_equal_rectangle_pairs), frames bit-identical to each other
and to the brute-force scan; the sorted bins' order and pad words (the check of
test_c5_sorted_bins_carry_later_chunk_masks); the general tracer (its setup bins every pair with
the jittered masks, bin_pairs_kernel<true>) against its brute-force flag.
"""
import contextlib
import ctypes
import functools

import numpy as np
import pytest

from eray_amd import capi
from tests.helpers import (all_bins, assert_bin_order_and_pads, assert_bit_equal, assert_pair_bins_within_segment_bins,
                           bin_entries)

pytestmark = pytest.mark.gpu

W, H = 1920, 1080
CAM_Z, ASPECT = 5.0, 16.0 / 9.0
STACKS = ((60, 135, 300), (30, 60, 100))  # (bin column, bin row of phase 0, faces)


def _at(px, py, z):
    """The point at depth z that camera pixel coordinates (px, py) look at (camera.rs:57-76: the
    viewport spans [-aspect, aspect] x [-1, 1] at distance 1)."""
    d = CAM_Z - z
    return ((px / W * 2.0 - 1.0) * ASPECT * d, (py / H * 2.0 - 1.0) * d, z)


def _tiny(bx, by, i, z, y=1.5, h=1.0):
    """A camera-facing face inside bin (bx, by)'s pixels, away from its edges: columns 16 bx + 4 ..
    16 bx + 11.6, rows 4 by + y .. 4 by + y + h.  face_rect.hpp widens a face's pixel rectangle to
    floor(min) - 1 .. ceil(max) + 1: rows 1.5 .. 2.5 become rows 0 .. 4 of the bin's, two bin rows
    (two units) at either phase; _one_bin's rows 1.4 .. 1.6 become rows 0 .. 3, the bin itself at
    phase 0 (one unit)."""
    x0, y0 = 16.0 * bx + 4.0 + 0.3 * (i % 5), 4.0 * by + y
    return [_at(x0, y0, z), _at(x0 + 6.0 + 0.2 * (i % 3), y0, z), _at(x0 + 3.0, y0 + h, z)]


ONE_BIN = 120


def _one_bin(j):
    """One-bin face j, in a bin of its own (even columns 2 .. 110 of bin rows 200, 205, 210: none
    of the stacks' or the two-unit faces' bins)."""
    return _tiny(2 * (1 + j % 55), 200 + 5 * (j // 55), j, 0.3, y=1.4, h=0.2)


@functools.lru_cache(maxsize=1)
def _mesh():
    def full(k, facing=True):
        z = -1.0 - 0.25 * k
        d = CAM_Z - z
        v = [(-6.0 * d, -2.0 * d, z), (6.0 * d, -2.0 * d, z), (0.0, 6.0 * d, z)]  # counter-clockwise: towards the camera
        return v if facing else [v[0], v[2], v[1]]

    def empty(i):  # back-facing across the frame, or (a tiny face) behind the camera
        return full(i % 16, facing=False) if i % 2 else _tiny(40 + i % 7, 100, i, CAM_Z + 2.0)

    faces, n_empty = [], 0

    def empties(n):
        nonlocal n_empty
        for _ in range(n):
            faces.append(empty(n_empty))
            n_empty += 1

    empties(3)
    for k in range(16):
        faces.append(full(k))
        empties(2)
    (ax, ay, an), (bx, by, bn) = STACKS
    faces += [_tiny(ax, ay, i, 0.5 + 0.001 * i) for i in range(an // 2)]
    empties(70)
    faces += [_tiny(3 + 2 * j, 10 + 3 * j, j, 0.25) for j in range(50)]
    faces += [_one_bin(j) for j in range(80)]
    for j in range(80, ONE_BIN):
        faces.append(_one_bin(j))
        empties(1)
    faces += [_tiny(ax, ay, i, 0.5 + 0.001 * i) for i in range(an // 2, an)]
    faces += [_tiny(bx, by, i, 0.4 - 0.001 * i) for i in range(bn)]
    empties(5)
    pos = np.asarray(faces, np.float32).reshape(-1, 9)
    assert pos.shape[0] == 16 + 50 + ONE_BIN + an + bn + 150 and n_empty == 150
    rng = np.random.default_rng(33)
    nrm = np.tile(np.float32([0.0, 0.0, 1.0]), (pos.shape[0], 3))
    uv = rng.uniform(0.0, 1.0, (pos.shape[0], 6)).astype(np.float32)
    return pos, nrm, uv


@contextlib.contextmanager
def _scene(gpu):
    """The object with colour and reflection textures, main.rs's camera and lights, and bins that
    hold its entries from the first setup on (16 x 32,520 and the stacks; the default capacity of
    65,536 would overflow into the LDS-tile scan until the host had seen the count)."""
    pos, nrm, uv = _mesh()
    rng = np.random.default_rng(34)
    L = capi.lib()
    before = L.eray_debug_bin_capacity(gpu.handle)
    keep = [gpu.to_device(rng.uniform(0, 1.2, (5, 7, 3)).astype(np.float32)),
            gpu.to_device(rng.uniform(0, 0.9, (3, 4)).astype(np.float32))]
    out = _Out(gpu, H)
    try:
        gpu.scene_reset()
        gpu.set_camera(capi.make_camera((0.0, 0.0, CAM_Z), (16.0, 9.0), W, 1.0))
        gpu.add_light(capi.make_light((0.0, 2.0, 0.0), "ambient", (1.0, 1.0, 1.0), 0.2))
        gpu.add_light(capi.make_light((1.0, 1.0, 2.0), "point", (1.0, 1.0, 1.0), 1.0))
        p = pos.reshape(-1, 3)
        gpu.add_object(pos, nrm, uv, tuple(p.min(0)), tuple(p.max(0)), color=keep[0].image(), reflection=keep[1].image())
        assert L.eray_debug_set_bin_capacity(gpu.handle, 1 << 21) == 0
        yield out
    finally:
        assert L.eray_debug_set_bin_form(gpu.handle, 0) == 0
        if before:
            assert L.eray_debug_set_bin_capacity(gpu.handle, before) == 0
        out.free()
        for a in keep:
            a.free()


class _Out:
    def __init__(self, gpu, rows):
        self.gpu = gpu
        self.rgb = gpu.empty((rows, W, 3), np.float32)
        self.face = gpu.empty((rows, W), np.int32)
        self.ppm = gpu.empty((rows, W, 3), np.uint8)

    def render(self, row0=0, **kw):
        rows = H - row0
        for a, v in ((self.rgb, 0), (self.face, 0x7F), (self.ppm, 0)):
            self.gpu.memset(a.ptr, v, a.nbytes)
        self.gpu.render(W, H, row0=row0, rows=rows, out_rgb=self.rgb.ptr, out_face=self.face.ptr, out_ppm=self.ppm.ptr, **kw)
        n = rows * W
        return (self.rgb.numpy().reshape(-1)[: 3 * n].reshape(rows, W, 3).copy(),
                self.face.numpy().reshape(-1)[:n].reshape(rows, W).copy(),
                self.ppm.numpy().reshape(-1)[: 3 * n].reshape(rows, W, 3).copy())

    def free(self):
        for a in (self.rgb, self.face, self.ppm):
            a.free()


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: faces"
    assert_bit_equal(a[0], b[0], what)
    assert np.array_equal(a[2], b[2]), f"{what}: PPM bytes"


def _counts(gpu):
    st = (ctypes.c_uint64 * 14)()
    assert capi.lib().eray_debug_bin_stats(gpu.handle, 0, st) == 0
    counts = np.zeros(int(st[0]), np.uint32)
    nb = ctypes.c_uint32()
    assert capi.lib().eray_debug_bin_counts(gpu.handle, 0, counts.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                            len(counts), ctypes.byref(nb)) == 0
    return counts


def test_pair_walk_equals_segment_walk_and_brute_force(gpu):
    """The pair form (eray_debug_set_bin_form(1): bin_pairs_kernel<false>) against the segment
    form at row phase 0 and 1: the same mask for every face of the pair form, its bins a subset,
    at most one extra segment entry per twenty; frames bit-identical to each other and to
    RENDER_BRUTE_FORCE.  The pair form walks more units than any resident grid has lanes."""
    L = capi.lib()
    with _scene(gpu) as out:
        for row0 in (0, 1):
            got = []
            for rect in (1, 0):
                assert L.eray_debug_set_bin_form(gpu.handle, rect) == 0
                img = out.render(row0)
                bins, units = all_bins(gpu)
                got.append((img, bins, units))
            (ia, ba, ua), (ib, bb, ub) = got
            print(f"row0 {row0}: pair form {ua} units, {sum(len(v) for v in ba.values())} entries; segment form {ub} units, "
                  f"{sum(len(v) for v in bb.values())} entries")
            assert ua > 393_216, ua  # 256 CUs x 6 workgroups x 256 lanes
            if row0 == 0:
                # the full-frame faces' 120 x 270 bins, two bins per small face, so one per one-bin face
                assert ua - 16 * 120 * 270 - 2 * (50 + STACKS[0][2] + STACKS[1][2]) == ONE_BIN, ua
            assert ub <= ua
            _same(ia, ib, f"segments vs rectangle pairs, row0 {row0}")
            _same(ib, out.render(row0, flags=capi.RENDER_BRUTE_FORCE), f"bins vs brute force, row0 {row0}")
            assert sum(len(v) for v in ba.values()) > 16 * 120 * 269
            assert_pair_bins_within_segment_bins(ba, bb, f"row0 {row0}")


@pytest.mark.parametrize("rect", [0, 1])
def test_sorted_bins_of_both_sorts(gpu, rect):
    """The 316-entry bin (workgroup sort) and the 116-entry bin (wave sort) list their faces in
    increasing index with the later chunks' mask unions in the first two pad words of each chunk
    but the last; every other bin holds at most 64 entries and only zero pad words."""
    L = capi.lib()
    with _scene(gpu) as out:
        assert L.eray_debug_set_bin_form(gpu.handle, rect) == 0
        out.render(0)
        counts = _counts(gpu)
        order = np.argsort(counts)
        print("largest bins:", [(int(b), int(counts[b])) for b in order[-4:]])
        assert [int(counts[b]) for b in order[-2:]] == [STACKS[1][2] + 16, STACKS[0][2] + 16]
        assert counts[order[-3]] <= 64
        rng = np.random.default_rng(35)
        light = rng.choice(order[:-2], 60, replace=False)
        for b in [int(order[-1]), int(order[-2]), *np.nonzero(counts == 17)[0][:50].tolist(), *light.tolist()]:
            n, tri, mask, pad = bin_entries(gpu, b)
            assert n == counts[b]
            assert_bin_order_and_pads(b, n, tri, mask, pad)
        assert (counts == 17).sum() >= 50  # the two-unit faces' bins (and a one-bin face's, where it has an entry)


@pytest.mark.parametrize("aa,bounces", [(2, 0), (0, 1)])
def test_tracer_bins_equal_brute_force(gpu, aa, bounces):
    """The general tracer (its setup keeps every pair with the jittered masks:
    bin_pairs_kernel<true>) equals its brute-force flag, bit for bit."""
    with _scene(gpu) as out:
        a = out.render(0, anti_aliasing=aa, aa_seed=71, bounces=bounces)
        b = out.render(0, anti_aliasing=aa, aa_seed=71, bounces=bounces, flags=capi.RENDER_BRUTE_FORCE)
        assert (a[1] >= 0).all()  # every pixel sees a full-frame face
        _same(a, b, f"tracer aa {aa} bounces {bounces}: bins vs brute force")
