"""Shared helpers for the parity tests."""
from __future__ import annotations

import ctypes

import numpy as np

# RGB tolerance stated by BASELINE.json's north star ("RGB within 1e-5 of CPU .ppm").  The
# kernels are built to be bit-exact; bitwise equality is asserted where the arithmetic is fully
# pinned (every op IEEE f32 in the reference's order, libm restated bit-exactly), and this
# tolerance is the documented fallback where a libm call is not restated (powf with exponent
# != 1).
RGB_TOL = 1e-5


def bit_equal(a: np.ndarray, b: np.ndarray) -> bool:
    a = np.ascontiguousarray(a, np.float32)
    b = np.ascontiguousarray(b, np.float32)
    return a.shape == b.shape and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def mismatch_report(a: np.ndarray, b: np.ndarray) -> str:
    a = np.asarray(a, np.float32)
    b = np.asarray(b, np.float32)
    if a.shape != b.shape:
        return f"shape {a.shape} != {b.shape}"
    bad = a.view(np.uint32) != b.view(np.uint32)
    n = int(bad.sum())
    if not n:
        return "bit-identical"
    idx = np.argwhere(bad)[:5].tolist()
    diff = np.abs(a.astype(np.float64) - b.astype(np.float64))
    return f"{n} words differ; max |diff| {np.nanmax(diff):.3e}; first at {idx}"


def assert_bit_equal(a, b, what=""):
    assert bit_equal(a, b), f"{what}: {mismatch_report(a, b)}"


def random_mesh(rng: np.random.Generator, T: int, scale=1.0, center=(0.0, 0.0, 0.0)):
    """Random triangles around `center` with random per-vertex normals/uvs."""
    pos = (rng.uniform(-1, 1, (T, 9)) * scale + np.tile(center, 3)).astype(np.float32)
    nrm = rng.normal(size=(T, 9)).astype(np.float32)
    uv = rng.uniform(-0.5, 1.5, (T, 6)).astype(np.float32)
    return pos, nrm, uv


# ---- the screen bins of object 0 as the last setup built them (eray_debug_bin_*; GPU tests) ----
def bin_entries(gpu, b, cap=1024):
    """Bin b in bin order: (entry count, faces, pixel masks, pad words), at most cap entries."""
    from eray_amd import capi
    tri, mask, pad = (ctypes.c_uint32 * cap)(), (ctypes.c_uint64 * cap)(), (ctypes.c_uint32 * cap)()
    n = ctypes.c_uint32()
    assert capi.lib().eray_debug_bin_entries(gpu.handle, 0, b, tri, mask, pad, cap, ctypes.byref(n)) == 0
    m = min(n.value, cap)
    return (n.value, np.frombuffer(tri, np.uint32)[:m].copy(), np.frombuffer(mask, np.uint64)[:m].copy(),
            np.frombuffer(pad, np.uint32)[:m].copy())


def all_bins(gpu):
    """Every bin: {bin: sorted [(face, mask)]}, and the units the pair pass walked."""
    from eray_amd import capi
    L = capi.lib()
    st = (ctypes.c_uint64 * 14)()
    assert L.eray_debug_bin_stats(gpu.handle, 0, st) == 0
    cap = 4096
    tri, mask, n = (ctypes.c_uint32 * cap)(), (ctypes.c_uint64 * cap)(), ctypes.c_uint32()
    out = {}
    for b in range(int(st[0])):
        assert L.eray_debug_bin_dump(gpu.handle, 0, b, tri, mask, cap, ctypes.byref(n)) == 0
        assert n.value <= cap
        if n.value:
            out[b] = sorted(zip(tri[: n.value], mask[: n.value]))
    return out, int(st[13])


def assert_bin_order_and_pads(b, n, tri, mask, pad):
    """What frame_first_hit.hpp first_hit_binned_wave relies on (bins.hip bin_sort_kernel): a bin
    of 65..1024 entries lists its faces in increasing index, and the first two entries of each
    chunk but the last hold the low and high half of the union of the later chunks' masks; every
    other pad word, and every pad word of a bin of at most 64 entries, is 0."""
    if n <= 64:
        assert not pad.any(), f"bin {b}: pads in an unsorted bin"
        return
    assert (np.diff(tri.astype(np.int64)) > 0).all(), f"bin {b} ({n} entries) not in face order"
    nch = (n + 63) // 64
    want = np.zeros(n, np.uint32)
    for c in range(nch - 1):
        u = np.bitwise_or.reduce(mask[64 * (c + 1):])
        want[64 * c] = np.uint32(int(u) & 0xFFFFFFFF)
        want[64 * c + 1] = np.uint32(int(u) >> 32)
    assert np.array_equal(pad, want), f"bin {b} ({n} entries): later-chunk mask unions"


def assert_pair_bins_within_segment_bins(ba, bb, what):
    """The rectangle-pair form's bins `ba` against the segment form's `bb` (all_bins): the same
    mask for every face of the pair form, whose bins are a subset; the segment form may add the
    entries the pair form's f32 pre-test drops, at most one per twenty."""
    n_pairs = sum(len(v) for v in ba.values())
    extra = 0
    for b, seg in bb.items():
        pairs = dict(ba.get(b, []))
        seg_d = dict(seg)
        assert len(seg_d) == len(seg), f"bin {b}: a face twice"
        for f, m in pairs.items():
            assert seg_d.get(f) == m, f"bin {b} face {f}: mask {seg_d.get(f)} vs {m} ({what})"
        extra += len(seg_d) - len(pairs)
    assert set(ba) <= set(bb)
    assert extra <= n_pairs // 20, (extra, n_pairs)
