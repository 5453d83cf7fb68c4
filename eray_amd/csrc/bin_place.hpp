// bin_place.hpp — the entries of the pair pass into their bins (bins.hip includes it after
// bin_walk.hpp): the scatter, the sort of the bins of more than one chunk by face index, and the
// finaliser (the objects' rectangles narrowed to their non-empty bins, their bin views, the
// counters reset).
#pragma once

#include "bin_walk.hpp"

namespace eray {
namespace gpu {
namespace {

// every stored entry to its bin: start[key] + its rank, as one 64-B line (BinEntry: the face's
// intersection record, its pixel mask and its index in the object); the finaliser zeroes the
// counts for the next camera (coalesced over the keys, not a scattered word per entry).  The
// shards' entries are one index space (each workgroup prefix-sums the 32 shard counts in LDS), so
// every thread of the grid takes a share: a loop over the shards gave each shard's entries to the
// grid's first threads only, which then walked 32 dependent gather-and-store chains one after the
// other (16 cameras at 3840x2160 / 70k: 114 us).
__global__ void __launch_bounds__(kBinWG) bin_scatter_kernel(const uint32_t* __restrict__ n, uint32_t cap,
                                                             const uint32_t* __restrict__ ekey,
                                                             const uint32_t* __restrict__ eface,
                                                             const unsigned long long* __restrict__ emask,
                                                             const uint32_t* __restrict__ erank,
                                                             const uint32_t* __restrict__ start,
                                                             const uint32_t* __restrict__ kbegin, uint32_t nbins,
                                                             const TriHot* __restrict__ hot, uint32_t T1,
                                                             BinEntry* __restrict__ ent) {
    static_assert(kShards <= 64, "one wave scans the shard counts");
    __shared__ uint32_t s_pre[kShards + 1];  // each shard's first index in the joint space, and the total
    const uint32_t region = shard_region(cap);
    if (threadIdx.x < 64) {
        const uint32_t lane = threadIdx.x;
        const uint32_t c = lane < kShards ? min(n[lane * kShardStride], region) : 0u;
        uint32_t incl = c;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = __shfl_up(incl, off);
            if ((int)lane >= off) incl += y;
        }
        if (lane < kShards) s_pre[lane] = incl - c;
        if (lane == kShards - 1) s_pre[kShards] = incl;
    }
    __syncthreads();
    const uint32_t total = s_pre[kShards];
    for (uint32_t g = blockIdx.x * kBinWG + threadIdx.x; g < total; g += gridDim.x * kBinWG) {
        uint32_t lo = 0, hi = kShards;  // the shard holding g: the last one starting at or before it
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) >> 1;
            if (s_pre[mid] <= g) lo = mid;
            else hi = mid;
        }
        const uint32_t e = lo * region + (g - s_pre[lo]);
        const uint32_t key = ekey[e], f = eface[e];
        BinEntry x;
        x.hot = hot[T1 ? f % T1 : f];  // (several cameras: face f is face f % T1 of camera f / T1)
        x.mask = emask[e];
        x.tri = f - kbegin[key / nbins];
        x.pad = 0u;
        ent[start[key] + erank[e]] = x;
    }
}

// The binned objects' non-empty bins -> their pixel rectangles ((~x0, x1 + 1, ~y0, y1 + 1),
// max-reduced); the last workgroup narrows each binned object's rectangle to them, publishes its
// bin views (none on overflow) and resets the counters.  Keys are object-major, so a workgroup's
// 256 keys belong to a run of binned objects [k_first, k_last]: reduced in LDS, then atomically
// max-merged into the objects' accumulators by the workgroups that found a non-empty bin.
constexpr uint32_t kFinSpan = 8;    // binned objects per workgroup reduced in LDS (more: atomics)
constexpr uint32_t kFinTab = 1024;  // binned objects the last workgroup combines in LDS
// (kFinGrid, the workgroups of the per-key pass: bin_layout.hpp.)

__device__ __forceinline__ void max4(uint32_t* dst, const uint32_t (&a)[4]) {
    for (int q = 0; q < 4; ++q) atomicMax(dst + q, a[q]);
}

// The scatter leaves a bin's entries in no particular order.  The frame kernel's result does not
// depend on it (each pixel keeps its smallest hitting face), but its work does: a bin is searched
// in chunks of 64 entries, and a chunk whose faces all come after every live pixel's best hit so
// far is skipped — in face order, the later chunks of a dense bin mostly are.  So each bin with
// more than one chunk (and at most kSortMax entries; longer ones stay as they are) is sorted by
// face index: bins of up to kSortWave entries one wave each, longer ones (the poles of the 1M-face
// stand-in put 300-700 entries into a few bins) one workgroup each.  The frame kernel relies on
// it: in a bin of 65 to kBinSortMax entries the position order is the face order
// (frame_first_hit.hpp first_hit_binned / first_hit_binned_wave), and chunk c's first two entries carry the
// union of the masks of chunks c + 1 .. (BinEntry::pad): pixels outside it cannot be hit by
// anything later in the bin.
constexpr uint32_t kSortMax = kBinSortMax;
constexpr uint32_t kSortWave = 256;            // bins sorted by one wave (whole bin in its LDS slice)
constexpr uint32_t kSortPer = kSortWave / 64;  // entries per lane
constexpr uint32_t kSortChunks = kSortMax / 64;
constexpr uint32_t kSortGrid = 1024;  // workgroups of the sort kernel's grid-stride loops
static_assert(kSortMax == (kBinWG / 64) * kSortWave, "a workgroup's sort LDS holds one longest bin");

// The bins to sort, appended to a work list (one counter atomic per wave and kind), so that the
// sort kernel spreads them over all its waves: the dense bins sit next to each other on the
// screen.  Wave-sorted bins go to the front of sortq (count nsort[0]), workgroup-sorted ones to
// the back (sortq[keys - 1 - i], count nsort[1]); together they are at most `keys`.
__device__ __forceinline__ void queue_sort(const uint32_t* __restrict__ start, uint32_t b, uint32_t keys,
                                           uint32_t* __restrict__ sortq, uint32_t* __restrict__ nsort) {
    const uint32_t lane = threadIdx.x & 63;
    const uint32_t cnt = b < keys ? start[b + 1] - start[b] : 0u;
#pragma unroll
    for (uint32_t big = 0; big < 2; ++big) {
        const bool want = cnt > (big ? kSortWave : 64u) && cnt <= (big ? kSortMax : kSortWave);
        const unsigned long long bal = __ballot(want);
        if (!bal) continue;
        const uint32_t first = (uint32_t)(__ffsll(bal) - 1);
        uint32_t base = 0;
        if (lane == first) base = atomicAdd(nsort + big, (uint32_t)__popcll(bal));
        base = (uint32_t)__shfl((int)base, (int)first);
        const uint32_t at = base + (uint32_t)__popcll(bal & ((1ull << lane) - 1ull));
        if (want) sortq[big ? keys - 1u - at : at] = b;
    }
}

// A sorted entry's pad word: chunk c's first two entries (rank 64 c, 64 c + 1) get the low and
// high halves of sfx[c + 1], the union of the masks of chunks c + 1 .. (sfx[nch] = 0).
__device__ __forceinline__ uint32_t sorted_pad(uint32_t rank, uint32_t nch, const unsigned long long* sfx) {
    const uint32_t c = rank >> 6, k = rank & 63u;
    if (k > 1u || c + 1u >= nch) return 0u;
    const unsigned long long u = sfx[c + 1u];
    return k ? (uint32_t)(u >> 32) : (uint32_t)u;
}

// One queued bin by kThreads threads (a wave: its LDS slice, wave_sync; the workgroup: the whole
// array, __syncthreads): its entries staged in LDS, each entry's rank = the number of the bin's
// faces below its own (a face appears at most once per bin), the chunks' mask unions OR-ed by rank
// and suffix-combined, each entry written back at its rank.  `cu`: one word per chunk of the
// longest bin the threads take (kThreads * kPer entries).
template <uint32_t kThreads, uint32_t kPer>
__device__ __forceinline__ void sort_bin(uint32_t key, const uint32_t* __restrict__ start, BinEntry* __restrict__ ent,
                                         BinEntry* se, unsigned long long* cu, uint32_t t) {
    auto sync = [] {
        if constexpr (kThreads == 64) wave_sync();
        else __syncthreads();
    };
    const uint32_t s0 = start[key], n = start[key + 1] - s0, nch = (n + 63) / 64;
    uint32_t v[kPer], r[kPer];
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
        const uint32_t e = t + kThreads * q;
        v[q] = 0xffffffffu;
        r[q] = 0;
        if (e < n) {
            se[e] = ent[s0 + e];
            v[q] = se[e].tri;
        }
    }
    if (t < kThreads * kPer / 64) cu[t] = 0ull;
    sync();
    for (uint32_t j = 0; j < n; ++j) {
        const uint32_t f = se[j].tri;
#pragma unroll
        for (uint32_t q = 0; q < kPer; ++q) r[q] += f < v[q] ? 1u : 0u;
    }
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q)
        if (t + kThreads * q < n) atomicOr(&cu[r[q] >> 6], se[t + kThreads * q].mask);
    sync();
    if (t == 0)
        for (uint32_t c = nch - 1; c-- > 0;) cu[c] |= cu[c + 1];
    sync();
#pragma unroll
    for (uint32_t q = 0; q < kPer; ++q) {
        const uint32_t e = t + kThreads * q;
        if (e < n) {
            BinEntry x = se[e];
            x.pad = sorted_pad(r[q], nch, cu);
            ent[s0 + r[q]] = x;
        }
    }
    sync();  // the LDS is rewritten by the next bin
}

// The queued bins: those of 65..kSortWave entries one wave each, then those of kSortWave +
// 1..kSortMax entries one workgroup each.
__global__ void __launch_bounds__(kBinWG) bin_sort_kernel(const uint32_t* __restrict__ sortq,
                                                          const uint32_t* __restrict__ nsort,
                                                          const uint32_t* __restrict__ start,
                                                          BinEntry* __restrict__ ent, uint32_t keys) {
    __shared__ BinEntry s_ent[kBinWG / 64][kSortWave];  // a wave's bin; the workgroup's: all of it
    __shared__ unsigned long long s_cu[kBinWG / 64][kSortChunks];
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t items = nsort[0];
    for (uint32_t it = blockIdx.x * (kBinWG / 64) + wave; it < items; it += gridDim.x * (kBinWG / 64))  // wave-uniform
        sort_bin<64, kSortPer>(sortq[it], start, ent, s_ent[wave], s_cu[wave], lane);
    __syncthreads();  // (the workgroup's bins below use every wave's slice)
    const uint32_t nbig = nsort[1];
    for (uint32_t it = blockIdx.x; it < nbig; it += gridDim.x)  // workgroup-uniform
        sort_bin<kBinWG, kSortMax / kBinWG>(sortq[keys - 1u - it], start, ent, &s_ent[0][0], s_cu[0], threadIdx.x);
}

// kFinal false: each workgroup reduces its `per` consecutive keys (a multiple of kBinWG: each
// thread keeps a running union while its keys stay in one object) and publishes; true: one
// workgroup combines.  (One workgroup per 256 keys put ~8k atomics of C5's four-camera build on
// one line: 330 us.)
template <bool kFinal>
__global__ void __launch_bounds__(kBinWG) bins_finalize_kernel(uint32_t per, const uint32_t* __restrict__ start, uint32_t nb,
                                                               uint32_t bins_x, uint32_t nbins, uint32_t W, uint32_t H,
                                                               uint32_t phase, uint32_t* __restrict__ acc,
                                                               uint32_t* __restrict__ part,
                                                               uint32_t* __restrict__ done, uint32_t* __restrict__ n,
                                                               uint32_t cap, const uint32_t* __restrict__ kobj,
                                                               ObjectDesc* __restrict__ objs, const BinEntry* ent,
                                                               uint32_t* __restrict__ count,
                                                               uint32_t* __restrict__ sortq, uint32_t* __restrict__ nsort,
                                                               CamState* __restrict__ st, uint32_t ncam,
                                                               int32_t* __restrict__ path_union, uint32_t union_nobj) {
    __shared__ uint32_t s_acc[kFinSpan][4];
    __shared__ uint32_t s_tab[kFinal ? kFinTab : 1][4];
    const uint32_t keys = nb * nbins;
    const uint32_t b0 = kFinal ? 0u : blockIdx.x * per, b1 = kFinal ? 0u : min(b0 + per, keys);
    const uint32_t k_first = b0 < b1 ? b0 / nbins : 0u, k_last = b0 < b1 ? (b1 - 1) / nbins : 0u;
    if (threadIdx.x < kFinSpan * 4) s_acc[threadIdx.x / 4][threadIdx.x % 4] = 0u;
    __syncthreads();
    if constexpr (!kFinal) {
        uint32_t kc = ~0u, a[4] = {0u, 0u, 0u, 0u};  // this thread's union of object kc's bins so far
        auto flush = [&]() {
            if (kc == ~0u) return;
            if (kc - k_first < kFinSpan) max4(s_acc[kc - k_first], a);
            else max4(acc + kAccStride * kc, a);
        };
        for (uint32_t b = b0 + threadIdx.x; b < b0 + per; b += kBinWG) {  // workgroup-uniform trip count
            if (b < b1) count[b] = 0u;  // (the scatter has read the ranks: zero for the next camera)
            if (b < b1 && start[b + 1] > start[b]) {
                const uint32_t k = b / nbins;
                const uint32_t lb = b - k * nbins;
                const uint32_t bx = lb % bins_x, by = lb / bins_x;
                const int32_t y0 = (int32_t)(by * kBinH + phase) - (int32_t)kBinH;
                const uint32_t x0 = bx * kBinW, x1 = min(x0 + kBinW, W) - 1;
                const uint32_t r0 = (uint32_t)max(y0, 0), r1 = (uint32_t)min(y0 + (int32_t)kBinH, (int32_t)H) - 1;
                const uint32_t w[4] = {~x0, x1 + 1u, ~r0, r1 + 1u};
                if (k != kc) {
                    flush();
                    kc = k;
                    for (int q = 0; q < 4; ++q) a[q] = 0u;
                }
                for (int q = 0; q < 4; ++q) a[q] = max(a[q], w[q]);
            }
            queue_sort(start, b, keys, sortq, nsort);
        }
        flush();
    }
    __syncthreads();
    // this workgroup's objects' unions into the accumulators: only workgroups with a non-empty
    // bin, four atomics per object (a single combining workgroup reading every workgroup's
    // partials took 28 us at 16 cameras x 32k bins)
    const uint32_t span = !kFinal && b0 < b1 ? min(k_last - k_first + 1, kFinSpan) : 0u;
    if (threadIdx.x < span && s_acc[threadIdx.x][1] != 0u) {
        const uint32_t a[4] = {s_acc[threadIdx.x][0], s_acc[threadIdx.x][1], s_acc[threadIdx.x][2], s_acc[threadIdx.x][3]};
        max4(acc + kAccStride * (k_first + threadIdx.x), a);
    }
    if (!kFinal) return;
    const bool in_lds = nb <= kFinTab;
    if (in_lds) {
        for (uint32_t j = threadIdx.x; j < nb; j += kBinWG)
            for (int q = 0; q < 4; ++q) {
                s_tab[j][q] = acc[kAccStride * j + q];
                acc[kAccStride * j + q] = 0u;
            }
        __syncthreads();
    }
    __syncthreads();
    // the shards' counts: an overflow if any shard outgrew its region; the entries needed for the
    // capacity are the fullest shard's times kShards
    uint32_t found = 0, fullest = 0;
    for (uint32_t sh = 0; sh < kShards; ++sh) {
        const uint32_t c = n[sh * kShardStride];
        found += c;
        fullest = max(fullest, c);
    }
    const bool overflow = fullest > shard_region(cap);
    const uint32_t need = max(found, fullest * kShards);
    for (uint32_t j = threadIdx.x; j < nb; j += kBinWG) {
        uint32_t w[4];
        for (int q = 0; q < 4; ++q) w[q] = in_lds ? s_tab[j][q] : atomicExch(acc + kAccStride * j + q, 0u);
        ObjGeom& g = objs[kobj[j]].g;
        if (overflow) {  // keep the face rectangles; the frame kernel scans through LDS tiles
            g.bin_start = nullptr;
            g.bin_ent = nullptr;
            if (path_union) union_rect(path_union, union_nobj, kobj[j] % union_nobj, g.rect);
            continue;
        }
        // a pixel of an empty bin has no face whose culling bounds can pass there (bin_pixels),
        // so no primary ray hits the object: its rectangle narrows to the non-empty bins
        int32_t* r = g.rect;
        if (w[1] == 0) {
            r[0] = r[2] = 1;
            r[1] = r[3] = 0;
        } else {
            r[0] = max(r[0], (int32_t)~w[0]);
            r[1] = min(r[1], (int32_t)w[1] - 1);
            r[2] = max(r[2], (int32_t)~w[2]);
            r[3] = min(r[3], (int32_t)w[3] - 1);
        }
        if (path_union) union_rect(path_union, union_nobj, kobj[j] % union_nobj, r);
        g.bin_start = start + (size_t)j * nbins;
        g.bin_ent = ent;
    }
    __syncthreads();  // (every thread has read the counts)
    if (threadIdx.x < kShards) n[threadIdx.x * kShardStride] = 0u;
    if (threadIdx.x == 0) {
        nsort[0] = nsort[1] = 0u;  // (bin_sort_kernel has run)
        // the most entries any setup needed since the buffers were allocated (the host grows the
        // capacity from it), and whether any overflowed
        for (uint32_t k = 0; k < ncam; ++k) {  // (several cameras: every camera's state)
            st[k].bin_entries = max(st[k].bin_entries, need);
            st[k].bin_overflow |= overflow ? 1u : 0u;
            st[k].nrect = 0u;
            st[k].total_sub = 0u;  // counted by detail_list_kernel
            st[k].heavy_sub = 0u;
            st[k].light_sub = 0u;
        }
    }
}

}  // namespace
}  // namespace gpu
}  // namespace eray
