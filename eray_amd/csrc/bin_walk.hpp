// bin_walk.hpp — what the pair passes of the screen bins share (bins.hip includes it; bin_pairs.hpp
// holds the kernels): the walk of the binned faces' units, a wave per contiguous range, and the
// append of the entries found to the sharded entry list.  Device code of bins.hip's one
// translation unit: internal linkage, as when it stood there.
#pragma once

#include "bin_layout.hpp"
#include "internal.hpp"

namespace eray {
namespace gpu {
namespace {

// (kBinWG, the shard constants kShards / kShardStride and kAccStride: bin_layout.hpp.)

// Inclusive prefix max over the wave's lanes (DPP row shifts, then the row broadcasts; an invalid
// source lane reads 0, the identity).  Every lane of the wave calls.
template <int kCtrl, int kRowMask>
__device__ __forceinline__ uint32_t dpp_max_step(uint32_t v) {
    return max(v, (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, kCtrl, kRowMask, 0xf, false));
}
__device__ __forceinline__ uint32_t wave_prefix_max(uint32_t v) {
    v = dpp_max_step<0x111, 0xf>(v);  // row_shr:1
    v = dpp_max_step<0x112, 0xf>(v);  // row_shr:2
    v = dpp_max_step<0x114, 0xf>(v);  // row_shr:4
    v = dpp_max_step<0x118, 0xf>(v);  // row_shr:8: each row's inclusive prefix
    v = dpp_max_step<0x142, 0xa>(v);  // row_bcast:15 (rows 1 and 3)
    return dpp_max_step<0x143, 0xc>(v);  // row_bcast:31 (rows 2 and 3)
}

// The setup enumerates units of every binned face — the (face, bin) pairs of its bin rectangle,
// or the rectangle's bin rows (segments, below) — in face order, with face i's first unit at
// boff[i / chunk] + first_local[i] (its setup chunk's offset + its place in the chunk's own scan)
// and all P units at boff[nparts].  Every wave walks its own contiguous range of units, 64 at a
// time: one search for the face of its first unit, after which each slice starts from the face of
// the previous slice's last unit (the next slice's face ranges loaded ahead).  (A grid-stride
// loop searched anew for every slice — ~12 dependent global loads per 64 units, the pass's
// critical path: C5's four-camera build 1.3-1.8 ms.)  body(j, valid, face) runs once per slice
// with every lane of the wave (lane = unit j; `valid`: j is one of the wave's units).
struct UnitWalk {
    const unsigned long long* s_boff;  // (LDS) boff
    const unsigned long long* first_local;
    uint32_t nparts, chunk, T;
    uint32_t* s_face;  // (LDS) kBinWG words: the faces starting at each lane's unit
};
__device__ __forceinline__ void wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}
template <typename Body>
__device__ __forceinline__ void walk_units(const UnitWalk& u, Body&& body) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long P = u.s_boff[u.nparts];
    auto first = [&](uint32_t i) { return u.s_boff[i / u.chunk] + u.first_local[i]; };
    auto face_of = [&](unsigned long long j) -> uint32_t {
        // the chunk: the last one starting at or before j (in LDS; an empty chunk never is, the next
        // one starts at the same unit) ...
        uint32_t cb = 0, ce = u.nparts;
        while (ce - cb > 1) {
            const uint32_t mid = (cb + ce) >> 1;
            if (u.s_boff[mid] <= j) cb = mid;
            else ce = mid;
        }
        // ... then, inside it, the last face whose first unit is <= j
        const unsigned long long jl = j - u.s_boff[cb];
        uint32_t lo = cb * u.chunk, hi = min(lo + u.chunk, u.T);
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (u.first_local[mid] <= jl) lo = mid + 1;
            else hi = mid;
        }
        return lo - 1;
    };
    const unsigned long long slices = (unsigned long long)gridDim.x * (kBinWG / 64) * 64ull;
    const unsigned long long per = (P + slices - 1) / slices * 64ull;  // units per wave (multiple of 64)
    const unsigned long long w_lo = ((unsigned long long)blockIdx.x * (kBinWG / 64) + wave) * per;
    const unsigned long long w_hi = min(w_lo + per, P);
    uint32_t fb = w_lo < P ? face_of(w_lo) : 0u;
    // face fi's units [a, b) for the 64 faces from fb on (P past the last face)
    auto face_units = [&](uint32_t fb0, unsigned long long& a, unsigned long long& b) {
        const uint32_t fi = fb0 + lane;
        a = P;
        b = P;
        if (fi < u.T) {
            a = first(fi);
            b = fi + 1 < u.T ? first(fi + 1) : P;
        }
    };
    unsigned long long pa, pb;  // the next slice's first 64 faces' units, loaded ahead
    face_units(fb, pa, pb);
    for (unsigned long long j0 = w_lo; j0 < w_hi; j0 += 64) {  // wave-uniform
        const unsigned long long jend = min(j0 + 64ull, w_hi), j = j0 + lane;
        // The wave's 64 consecutive units belong to a run of consecutive faces from fb on: each
        // non-empty face starting inside the slice writes its index at its first unit's slot (no
        // two do: the ranges are contiguous), then a prefix max over the lanes gives every slot
        // the last face starting at or before it — its owner; slot 0's owner may start earlier,
        // and is then fb, the previous slice's last face (a face starting at j0 overrides it).
        u.s_face[threadIdx.x] = lane ? 0u : fb;
        wave_sync();
        bool ahead = true;  // the first 64 faces were loaded ahead
        for (unsigned long long covered = j0; covered < jend; fb += 64, ahead = false) {  // wave-uniform
            unsigned long long a = pa, b = pb;
            if (!ahead) face_units(fb, a, b);
            if (a < b && a >= j0 && a < jend) u.s_face[64 * wave + (uint32_t)(a - j0)] = fb + lane;
            covered = (unsigned long long)__shfl((long long)b, 63);
        }
        wave_sync();
        const uint32_t owner = wave_prefix_max(u.s_face[threadIdx.x]);
        fb = (uint32_t)__builtin_amdgcn_readlane((int)owner, (int)(jend - 1 - j0));  // the next slice starts in this face or later
        if (jend < w_hi) face_units(fb, pa, pb);  // in flight while this slice's units are processed
        body(j, j < jend, owner, j < jend ? j - first(owner) : 0ull);
    }
}

// Entries appended to the shard's region of the entry list (one counter atomic per wave and
// call), each with its rank in its bin from the bin's count atomic (the scatter then needs no
// atomics: a returning atomic per entry there cost as much as this pass).  Every lane calls; m == 0:
// no entry.
struct EntryOut {
    uint32_t *n, *count, *ekey, *eface, *erank;
    unsigned long long* emask;
    uint32_t shard, region;
};
__device__ __forceinline__ void append_entries(const EntryOut& o, unsigned long long m, uint32_t key, uint32_t face) {
    const uint32_t lane = threadIdx.x & 63;
    const unsigned long long bal = __ballot(m != 0);
    if (!bal) return;
    uint32_t base = 0;
    if (lane == 0) base = atomicAdd(o.n + o.shard * kShardStride, (uint32_t)__popcll(bal));
    base = (uint32_t)__shfl((int)base, 0);
    if (m) {
        const uint32_t local = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (local < o.region) {
            const uint32_t slot = o.shard * o.region + local;
            o.erank[slot] = atomicAdd(o.count + key, 1u);
            o.ekey[slot] = key;
            o.eface[slot] = face;
            o.emask[slot] = m;
        }
    }
}

}  // namespace
}  // namespace gpu
}  // namespace eray
