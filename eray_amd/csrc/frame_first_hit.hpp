// frame_first_hit.hpp — the frame kernel's first-hit searches (Object::intersects for a wave's 64
// pixels): the candidate tests in index order (test_step, test_candidates), the scan of an object's
// faces per wave or through workgroup-shared LDS tiles with exact culling (first_hit), and the two
// searches of a binned mesh's screen bins (first_hit_binned: the workgroup's four sub-blocks
// together; first_hit_binned_wave: one wave alone).  Included by render.hip through frame_sub.hpp,
// whose render_sub calls them; their bodies are pinned by frame_kernel's register budget, so they
// are not shared with cast.hpp's per-lane first_face.  Uses render.hip's ERAY_TRACE_* hooks.
#pragma once

#include "frame_scene.hpp"

namespace eray {
namespace gpu {
namespace {

constexpr int kTriTile = 256;

struct Bundle {  // a wave's pixel rectangle in viewport coordinates
    float xlo, xhi, ylo, yhi;
};

// A word of a read-only array through the vector memory path (buffer load; every lane the same
// address): its wait counts with the wave's vector loads (vmcnt, in order), not with its LDS
// operations (lgkmcnt, which an outstanding scalar load would hold up) — for loads issued one
// sub-block ahead and used in the next.
__device__ __forceinline__ uint32_t vload_u32(const uint32_t* base, uint32_t i) {
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<uint32_t*>(base), 0, -1, 0x00020000);
    return __builtin_amdgcn_raw_buffer_load_b32(r, 4u * i, 0, 0);
}

// A bin range [lo, hi) loaded ahead (render_sub's pipelining), or none (ok false).
struct PreRange {
    uint32_t lo, hi;
    bool ok;
};

// Lanes whose Triangle::intersects could pass: the det and t conditions of exact_test, from the
// same expressions (so the same values).  t = dot(ao, n) * (1 / det) is >= 0 exactly when
// dot(ao, n) >= 0, except where the product underflows to -0 or 1 / det is 0 — those lanes are
// kept.  A lane that fails here fails the exact test; a face no lane keeps is skipped.
__device__ __forceinline__ bool plane_may_hit(f3 n, f3 a, f3 o, f3 d) {
    const float det = -dot0(d, n);
    const float dn = dot0(sub(o, a), n);
    return (det >= 1e-6f) & !((dn < -1e-18f) & (det < 1e19f));
}

// Faces [0, n) (n <= 64; lane j holds face j's record) that some searching lane may hit
// (plane_may_hit), as a bit mask.  The planes are broadcast from the lanes that hold them, four
// faces per step.
__device__ __forceinline__ unsigned long long plane_mask(const TriHot& mine, uint32_t n, bool searching, f3 o, f3 d) {
    const float pn[6] = {mine.q1.z, mine.q1.w, mine.q2.x, mine.q2.y, mine.q2.z, mine.q2.w};
    unsigned long long mask = 0;
    for (uint32_t i = 0; i < n; i += 4) {
        bool keep[4];
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k) {
            const uint32_t f = min(i + k, n - 1);
            const f3 nn = mk3(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn[0]), f)),
                              __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn[1]), f)),
                              __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn[2]), f)));
            const f3 a = mk3(__int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn[3]), f)),
                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn[4]), f)),
                             __int_as_float(__builtin_amdgcn_readlane(__float_as_int(pn[5]), f)));
            keep[k] = searching && plane_may_hit(nn, a, o, d);
        }
#pragma unroll
        for (uint32_t k = 0; k < 4; ++k)
            if (i + k < n && __any(keep[k])) mask |= 1ull << (i + k);
    }
    return mask;
}

// --------------------------------------------------------------------- first hit -----------
// Per-ray search state: kUndecided (ray and bounding-box test not evaluated yet), kSearching,
// kDone (hit found, bbox rejected, or not a pixel of the image).
constexpr int kUndecided = 0, kSearching = 1, kDone = 2;

// Objects with at most kDirectMax (internal.hpp) triangles are searched by each wave on its
// own (no LDS tiles, no barrier); larger ones through their screen bins (primary rays, culled)
// or workgroup-shared LDS tiles (shadow rays, brute force).
// Candidate triangles tested together per step (independent, branch-free tests: their long
// dependent chains, division included, overlap).
constexpr int kBatch = 4;
constexpr int kLargeTestBatch = 1;  // the large-mesh builds: one candidate per step (no spills)

// Tests the next kB candidates of `mask` (kB <= its population) in index order.
template <int kB, typename Face, typename Hot>
__device__ __forceinline__ void test_step(unsigned long long& mask, Face&& face, Hot&& hot, int& st, const f3& o,
                                          const f3& d, int& found, float& hu, float& hv, float& ht) {
    uint32_t ids[kB];
    bool has[kB];
    TriHot h[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) {
        has[k] = mask != 0;
        ids[k] = has[k] ? (uint32_t)(__ffsll(mask) - 1) : 0u;
        mask &= mask - 1;
        h[k] = hot(ids[k]);
    }
    bool hit[kB];
    float u[kB], v[kB], t[kB];
#pragma unroll
    for (int k = 0; k < kB; ++k) hit[k] = has[k] && exact_test_flat(h[k], o, d, u[k], v[k], t[k]);
#pragma unroll
    for (int k = 0; k < kB; ++k) {
        if (st == kSearching && hit[k]) {
            found = (int)face(ids[k]);
            hu = u[k];
            hv = v[k];
            ht = t[k];
            st = kDone;
        }
    }
}

// Tests the candidates of `mask` in index order, up to kBatch at a time: bit i stands for face
// face(i) (relative to the object) whose record is hot(i).  Returns false once no lane is
// searching.
template <int kB = kBatch, typename Face, typename Hot>
__device__ __forceinline__ bool test_candidates(unsigned long long mask, Face&& face, Hot&& hot, int& st,
                                                const f3& o, const f3& d, int& found, float& hu, float& hv,
                                                float& ht) {
    while (mask) {
        const int n = __popcll(mask);
        if (kB >= 4 && n >= 4)
            test_step<4>(mask, face, hot, st, o, d, found, hu, hv, ht);
        else if (kB >= 2 && n >= 2)
            test_step<2>(mask, face, hot, st, o, d, found, hu, hv, ht);
        else
            test_step<1>(mask, face, hot, st, o, d, found, hu, hv, ht);
        if (!__any(st == kSearching)) return false;
    }
    return true;
}

// First-hit search over triangles [begin, begin + count) (Object::intersects' face loop,
// object.rs:63-78).  A ray still kUndecided when the wave meets its first candidate triangle is
// resolved by activate(), which must generate its direction (into `d`) and return the
// bounding-box verdict (object.rs:59-61).  `found` receives the face index relative to
// `begin`, or stays -1.  kLds: every thread of the workgroup must call it.
template <bool kCull, bool kLds, bool kPlane = false, int kB = kBatch, typename Scene, typename Activate>
__device__ void first_hit(const FrameParams& p, const Scene& sc, uint32_t begin, uint32_t count, int& st,
                          const f3& o, const f3& d, const Bundle& bd, TriHot* s_hot, TriCull* s_cull,
                          Activate&& activate, int& found, float& hu, float& hv, float& ht) {
    const uint32_t lane = threadIdx.x & 63;
    // false when no ray of the wave can hit anything in this object any more
    auto resolve = [&]() -> bool {
        if (__any(st == kUndecided)) {
            const bool a = activate();
            if (st == kUndecided) st = a ? kSearching : kDone;
        }
        return __any(st == kSearching);
    };
    if (!kLds) {
        for (uint32_t base = 0; base < count; base += 64) {
            if (!__any(st != kDone)) break;
            unsigned long long mask;
            if (kCull) {
                const uint32_t j = base + lane;
                bool keep = false;
                if (j < count) keep = !cull_rejects(sc.cull(begin + j), bd.xlo, bd.xhi, bd.ylo, bd.yhi);
                mask = __ballot(keep);
            } else if (kPlane) {  // rays already resolved (shadow rays): faces some lane may hit
                const uint32_t n = min(64u, count - base);
                mask = plane_mask(sc.hot_lane(begin + base + min(lane, n - 1)), n, st == kSearching, o, d);
            } else {
                const uint32_t n = min(64u, count - base);
                mask = n == 64 ? ~0ull : ((1ull << n) - 1ull);
            }
            if (!mask) continue;
            if (!resolve()) break;
            auto face = [&](uint32_t i) { return base + i; };
            auto hot = [&](uint32_t i) { return sc.hot(begin + base + i); };
            if (!test_candidates<kB>(mask, face, hot, st, o, d, found, hu, hv, ht)) return;
        }
        return;
    }
    for (uint32_t base = 0; base < count; base += kTriTile) {
        if (!__syncthreads_or(st != kDone)) break;  // also orders the LDS reuse below
        const uint32_t n = min((uint32_t)kTriTile, count - base);
        if (threadIdx.x < n) {
            s_hot[threadIdx.x] = p.tris[begin + base + threadIdx.x];
            if (kCull) s_cull[threadIdx.x] = sc.cull_array()[begin + base + threadIdx.x];
        }
        __syncthreads();
        if (!__any(st != kDone)) continue;
        for (uint32_t c = 0; c < n; c += 64) {
            unsigned long long mask;
            if (kCull) {
                const uint32_t j = c + lane;
                mask = __ballot(j < n && !cull_rejects(s_cull[j], bd.xlo, bd.xhi, bd.ylo, bd.yhi));
            } else {
                const uint32_t m = min(64u, n - c);
                mask = m == 64 ? ~0ull : ((1ull << m) - 1ull);
            }
            if (!mask) continue;
            if (!resolve()) break;
            auto face = [&](uint32_t i) { return base + c + i; };
            auto hot = [&](uint32_t i) { return s_hot[c + i]; };
            if (!test_candidates<kB>(mask, face, hot, st, o, d, found, hu, hv, ht)) break;
        }
    }
    __syncthreads();  // the tiles' LDS is reused (aliased by the binned search)
}

constexpr uint32_t kWide = 16;  // candidates that may cover more pixels are tested by the whole wave

// Per-wave LDS of the binned primary search.
struct BinLds {
    float dir[3][64];         // each pixel's camera ray (lane = pixel)
    // each pixel's first hit so far as an order key, 0xffffffff = none: its bin position in a
    // sorted bin (positions grow with the face index), its face index in a longer one
    uint32_t best[64];
    TriHot cand[64];          // the chunk's candidate records (slot = lane that loaded it)
    uint32_t key[64];         // ... and their order keys
    // (candidate slot << 6) | pixel, for every pixel a narrow candidate (<= kWide pixels) may hit
    uint16_t pairs[64 * kWide];
};
constexpr uint32_t kBinLdsBytes = (sizeof(BinLds) + 15) / 16 * 16;

// Primary-ray first hit of a binned object (bins.hip), all four waves of the workgroup together
// (every wave calls it; workgroup-uniform).  The reference's first hit is the smallest face index
// whose Triangle::intersects passes (object.rs:63-78), so each pixel keeps the smallest hitting
// face seen so far (LDS atomicMin of an order key).  A bin of 65 to kBinSortMax entries lists its
// faces in index order (bins.hip sort_bins): the key is the bin position, and a chunk none of
// whose pixels is still without a hit before the chunk's first position is skipped before its
// entries are read.  Other bins are in no particular order (one chunk, or too long to sort): the
// key is the face index, and a chunk is skipped when every pixel's best face is below the
// chunk's smallest.  Each wave's
// sub-block bin is cut into chunks of 64 entries and the workgroup's chunks are dealt round-robin
// over its waves — a bin at a dense spot (thousands of faces) is shared four ways.  A chunk is
// tested as (face, pixel) pairs: each entry carries the pixels where its four culling bounds can
// pass (bin_pixels), restricted to the live pixels; narrow faces' pairs are compacted in LDS and
// tested one per lane, wide ones by the whole wave, and a pair whose key is not below the pixel's
// best so far is skipped.
// Work follows the pixels a face can cover, not 64 lanes per face.  Each wave then re-tests its
// pixels' winners for u, v, t.
template <typename Activate>
__device__ void first_hit_binned(const FrameParams& p, const ObjGeom& ob, uint32_t bin, int& st, const f3& o,
                                 const f3& d, Activate&& activate, int& found, float& hu, float& hv, float& ht,
                                 char* s_bins, PreRange pre) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr uint32_t kWaves = kWG / 64;
    BinLds& L = *reinterpret_cast<BinLds*>(s_bins + wave * kBinLdsBytes);
    uint32_t* s_range = reinterpret_cast<uint32_t*>(s_bins + kWaves * kBinLdsBytes);  // [lo, hi] per wave
    // the bin's entries [lo, hi): loaded one sub-block ahead when the caller has them (pre)
    uint32_t lo = pre.ok ? pre.lo : load_const(ob.bin_start, bin), hi = pre.ok ? pre.hi : load_const(ob.bin_start, bin + 1);
    if (lo != hi && __any(st == kUndecided)) {  // every pixel's ray and bbox verdict, up front
        const bool a = activate();
        if (st == kUndecided) st = a ? kSearching : kDone;
    }
    if (!__any(st == kSearching)) hi = lo;  // nothing to search in this sub-block
    ERAY_TRACE_WAVE0(8);
    L.dir[0][lane] = d.x;
    L.dir[1][lane] = d.y;
    L.dir[2][lane] = d.z;
    L.best[lane] = st == kSearching ? 0xffffffffu : 0u;  // 0: never improved
    if (lane == 0) {
        s_range[2 * wave] = lo;
        s_range[2 * wave + 1] = hi;
    }
    __syncthreads();
    ERAY_TRACE_WAVE0(9);
    uint32_t chunks[kWaves], total = 0;
#pragma unroll
    for (uint32_t w = 0; w < kWaves; ++w) {
        chunks[w] = (s_range[2 * w + 1] - s_range[2 * w] + 63) / 64;
        total += chunks[w];
    }
    for (uint32_t item = wave; item < total; item += kWaves) {  // this wave's chunks
        uint32_t w = 0, c = item;
        while (c >= chunks[w]) c -= chunks[w++];
        BinLds& T = *reinterpret_cast<BinLds*>(s_bins + w * kBinLdsBytes);  // the chunk's sub-block
        const uint32_t lo_w = s_range[2 * w], end = s_range[2 * w + 1];
        const uint32_t base = lo_w + 64 * c;
        const bool sorted = end - lo_w > 64 && end - lo_w <= kBinSortMax;  // workgroup-uniform
        const uint32_t j = base + lane;
        uint32_t fj = 0xffffffffu;  // the entry's order key
        unsigned long long pm = 0;
        unsigned long long live;  // pixels of that sub-block this chunk can still improve
        if (sorted) {
            live = __ballot(T.best[lane] > base);
            if (!live) continue;
            if (j < end) {
                const BinEntry x = as_global_rec(ob.bin_ent + j);  // (one 64-B line per entry)
                fj = j;
                pm = x.mask;
                L.cand[lane] = x.hot;
                L.key[lane] = j;
            }
        } else {
            if (j < end) {
                const BinEntry x = as_global_rec(ob.bin_ent + j);
                fj = x.tri;
                pm = x.mask;
                L.cand[lane] = x.hot;
                L.key[lane] = fj;
            }
            uint32_t cmin = fj;  // the chunk's smallest face
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, off));
            live = __ballot(T.best[lane] > cmin);
            if (!live) continue;
        }
        const unsigned long long pix = pm & live;  // live pixels this face may hit
        const uint32_t cnt = (uint32_t)__popcll(pix);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // L.cand / L.key of this chunk visible to the wave
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        // wide candidates (many pixels): the whole wave tests them, each lane its own pixel
        unsigned long long wide = __ballot(cnt > kWide);
        while (wide) {
            const uint32_t s = (uint32_t)(__ffsll(wide) - 1);
            wide &= wide - 1;
            const unsigned long long ps =
                ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pix >> 32), (int)s) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pix, (int)s);
            const uint32_t fc = (uint32_t)__builtin_amdgcn_readlane((int)fj, (int)s);
            if (((ps >> lane) & 1ull) && fc < T.best[lane]) {
                float u, v, t;
                const f3 dd = mk3(T.dir[0][lane], T.dir[1][lane], T.dir[2][lane]);
                if (exact_test(L.cand[s], o, dd, u, v, t)) atomicMin(&T.best[lane], fc);
            }
        }
        // narrow candidates: (candidate, pixel) pairs compacted in LDS, one test per lane
        const uint32_t ncnt = cnt > kWide ? 0u : cnt;
        uint32_t incl = ncnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off);
            if ((int)lane >= off) incl += y;
        }
        const uint32_t npairs = __shfl(incl, 63);
        uint32_t at = incl - ncnt;
        unsigned long long np = ncnt ? pix : 0ull;
        while (np) {
            const uint32_t bpos = (uint32_t)(__ffsll(np) - 1);
            np &= np - 1;
            L.pairs[at++] = (uint16_t)((lane << 6) | bpos);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t q = 0; q < npairs; q += 64) {
            if (q + lane < npairs) {
                const uint32_t pr = L.pairs[q + lane];
                const uint32_t slot = pr >> 6, px = pr & 63;
                const uint32_t fc = L.key[slot];
                if (fc < T.best[px]) {  // a pixel already hit by an earlier face needs no test
                    float u, v, t;
                    const f3 dd = mk3(T.dir[0][px], T.dir[1][px], T.dir[2][px]);
                    if (exact_test(L.cand[slot], o, dd, u, v, t)) atomicMin(&T.best[px], fc);
                }
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // L.cand / L.key / L.pairs are rewritten by the next chunk
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
    ERAY_TRACE_WAVE0(10);
    __syncthreads();  // every chunk of every sub-block is done
    ERAY_TRACE_WAVE0(11);
    const uint32_t mine = L.best[lane];
    if (st == kSearching && mine != 0xffffffffu) {
        float u, v, t;
        if (hi - lo > 64 && hi - lo <= kBinSortMax) {  // the winner again, for u, v, t
            const BinEntry x = as_global_rec(ob.bin_ent + mine);
            exact_test(x.hot, o, d, u, v, t);
            found = (int)x.tri;
        } else {
            exact_test(as_global_rec(p.tris + ob.tri_begin + mine), o, d, u, v, t);
            found = (int)mine;
        }
        hu = u;
        hv = v;
        ht = t;
        st = kDone;
    }
    ERAY_TRACE_WAVE0(12);
    __syncthreads();  // the LDS is reused by the next object / sub-block
}

// Faces of an object the per-wave binned search takes (its keys pack face << 6 | slot).
constexpr uint32_t kWaveBinMaxTris = (1u << 26) - 1u;

// Primary-ray first hit of a binned object by ONE wave over its own sub-block's bin, with no
// workgroup barrier (the light sub-blocks of a frame's ordered detail list: their bins hold at
// most one 64-entry chunk, so sharing chunks across the workgroup's waves, as first_hit_binned
// does, buys nothing and its barriers tie four sub-blocks' latency chains together).  The same
// (face, pixel) pair tests; each pixel keeps the smallest order key of a hitting pair (LDS
// atomicMin), so the smallest hitting face index wins (object.rs:63-78) and its record is still
// in the wave's LDS: the winner's u, v, t are recomputed from there after each chunk, not re-read
// from memory.  Keys: face << 6 | slot in a bin in no order; in a sorted bin (65..kBinSortMax
// entries, bins.hip bin_sort_kernel) the position, which grows with the face index — a pixel
// whose best position precedes a chunk cannot improve there, and after each chunk the bin ends
// once no pixel that still can is in the later chunks' mask union (BinEntry::pad): a heavy bin's
// wave stops at the chunk that settles its last pixel, not at the bin's end.
template <typename Activate>
__device__ void first_hit_binned_wave(const ObjGeom& ob, uint32_t bin, int& st, const f3& o, const f3& d,
                                      Activate&& activate, int& found, float& hu, float& hv, float& ht, char* s_bins,
                                      PreRange pre) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    BinLds& L = *reinterpret_cast<BinLds*>(s_bins + wave * kBinLdsBytes);
    const uint32_t lo = pre.ok ? pre.lo : load_const(ob.bin_start, bin), hi = pre.ok ? pre.hi : load_const(ob.bin_start, bin + 1);
    if (lo == hi) return;
    if (__any(st == kUndecided)) {  // every pixel's ray and bbox verdict, up front
        const bool a = activate();
        if (st == kUndecided) st = a ? kSearching : kDone;
    }
    ERAY_TRACE_WAVE0(8);
    if (!__any(st == kSearching)) return;
    L.dir[0][lane] = d.x;
    L.dir[1][lane] = d.y;
    L.dir[2][lane] = d.z;
    uint32_t best = st == kSearching ? 0xffffffffu : 0u;  // this lane's pixel: its winning key so far
    L.best[lane] = best;
    const bool sorted = hi - lo > 64 && hi - lo <= kBinSortMax;  // (wave-uniform)
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t j = base + lane;
        uint32_t fj = 0xffffffffu, sfx = 0;
        unsigned long long pm = 0;
        if (j < hi) {
            const BinEntry x = load_rec(ob.bin_ent, j);
            fj = x.tri;
            pm = x.mask;
            sfx = x.pad;
            L.cand[lane] = x.hot;
        }
        unsigned long long live;  // pixels this chunk can still improve
        uint32_t key;
        if (sorted) {
            live = __ballot(best > base - lo);
            if (!live) break;  // (and none in any later chunk)
            key = j - lo;
        } else {
            uint32_t cmin = fj;  // the chunk's smallest face
#pragma unroll
            for (int off = 32; off > 0; off >>= 1) cmin = min(cmin, (uint32_t)__shfl_xor((int)cmin, off));
            live = __ballot((best >> 6) > cmin);
            if (!live) continue;
            key = (fj << 6) | lane;
        }
        ERAY_TRACE_WAVE0(9);
        const unsigned long long pix = pm & live;
        const uint32_t cnt = (uint32_t)__popcll(pix);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // L.cand / L.dir / L.best visible to the wave
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        unsigned long long wide = __ballot(cnt > kWide);
        while (wide) {  // wide candidates: the whole wave tests them, each lane its own pixel
            const uint32_t sl = (uint32_t)(__ffsll(wide) - 1);
            wide &= wide - 1;
            const unsigned long long ps =
                ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(pix >> 32), (int)sl) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)pix, (int)sl);
            const uint32_t kc = (uint32_t)__builtin_amdgcn_readlane((int)key, (int)sl);
            if (((ps >> lane) & 1ull) && kc < L.best[lane]) {
                float u, v, t;
                if (exact_test(L.cand[sl], o, d, u, v, t)) atomicMin(&L.best[lane], kc);
            }
        }
        // narrow candidates: (candidate, pixel) pairs compacted in LDS, one test per lane
        const uint32_t ncnt = cnt > kWide ? 0u : cnt;
        uint32_t incl = ncnt;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off);
            if ((int)lane >= off) incl += y;
        }
        const uint32_t npairs = __shfl(incl, 63);
        uint32_t at = incl - ncnt;
        unsigned long long np = ncnt ? pix : 0ull;
        while (np) {
            const uint32_t bpos = (uint32_t)(__ffsll(np) - 1);
            np &= np - 1;
            L.pairs[at++] = (uint16_t)((lane << 6) | bpos);
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        for (uint32_t q = 0; q < npairs; q += 64) {
            const bool in = q + lane < npairs;
            const uint32_t pr = in ? L.pairs[q + lane] : 0u;
            const uint32_t sl = pr >> 6, px = pr & 63;
            const uint32_t kc = (uint32_t)__shfl((int)key, (int)sl);  // the pair's key, from the lane that loaded it
            if (in && kc < L.best[px]) {  // a pixel already hit by an earlier face needs no test
                float u, v, t;
                const f3 dd = mk3(L.dir[0][px], L.dir[1][px], L.dir[2][px]);
                if (exact_test(L.cand[sl], o, dd, u, v, t)) atomicMin(&L.best[px], kc);
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // every pair of the chunk tested
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        const uint32_t nb = L.best[lane];
        const uint32_t fwin = sorted ? (uint32_t)__shfl((int)fj, (int)(nb & 63u)) : nb >> 6;  // its face
        if (nb != best) {  // improved by this chunk: the winner's record is still L.cand[slot]
            best = nb;
            exact_test(L.cand[nb & 63u], o, d, hu, hv, ht);
            found = (int)fwin;
        }
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // L.cand / L.pairs are rewritten by the next chunk
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        if (sorted) {  // the later chunks' masks (this chunk's first two entries): anything left?
            const unsigned long long later = ((unsigned long long)(uint32_t)__builtin_amdgcn_readlane((int)sfx, 1) << 32) |
                                             (uint32_t)__builtin_amdgcn_readlane((int)sfx, 0);
            if (!(__ballot(best > base + 64 - lo) & later)) break;
        }
    }
    ERAY_TRACE_WAVE0(10);
    ERAY_TRACE_VALUE(15, (hi - lo + 63) / 64);
    if (st == kSearching && found >= 0) st = kDone;
}

}  // namespace
}  // namespace gpu
}  // namespace eray
