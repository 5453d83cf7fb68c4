// bin_pairs.hpp — the pair pass of the screen bins (bins.hip includes it after bin_walk.hpp): the
// non-empty (face, bin) pairs of the binned faces with their pixel masks, from the faces' bin
// rectangles pair by pair (bin_pairs_kernel) or row by row (bin_segments_kernel).
#pragma once

#include "bin_walk.hpp"
#include "cull_record.hpp"
#include "face_rect.hpp"

namespace eray {
namespace gpu {
namespace {

// (face, bin) pairs of the binned faces' bin rectangles (face-major, each rectangle row-major):
// the non-empty ones appended to the entry list, counted per bin key.  The general tracer's setup
// (kJitter, SetupParams::keep_all: bin_pixels_jittered's masks) and frames wider than 65535
// pixels; otherwise bin_segments_kernel.
// waves per SIMD the pair pass is built for: 6 (80 VGPRs, a few spills in the mask path) over
// 5 (88 VGPRs): C5's moving-camera frame 491 -> 476 us; 8 (64 VGPRs, 22 spills) 525 us
constexpr int kPairsWaves = 6;
template <bool kJitter>
__global__ void __launch_bounds__(kBinWG, kPairsWaves) bin_pairs_kernel(const TriCull* __restrict__ cull,
                                                           const int4* __restrict__ range,
                                                           const unsigned long long* __restrict__ first_local,
                                                           const unsigned long long* __restrict__ boff,
                                                           uint32_t nparts, uint32_t chunk,
                                                           const uint32_t* __restrict__ fkey, uint32_t T, uint32_t W,
                                                           uint32_t H, uint32_t phase, uint32_t bins_x, uint32_t nbins,
                                                           uint32_t cap, uint32_t* __restrict__ n,
                                                           uint32_t* __restrict__ count, uint32_t* __restrict__ ekey,
                                                           uint32_t* __restrict__ eface,
                                                           unsigned long long* __restrict__ emask,
                                                           uint32_t* __restrict__ erank) {
    __shared__ unsigned long long s_boff[kSetupMaxBlocks + 1];
    __shared__ double s_poly[kJitter ? 16 * kBinWG : 1];  // clip_box's workspace
    __shared__ uint32_t s_face[kBinWG];
    // each wave's queue of pairs that survive the bin-rectangle test: face, bin (tx | ty << 16), key
    __shared__ uint32_t s_qf[kBinWG / 64][128], s_qt[kBinWG / 64][128], s_qk[kBinWG / 64][128];
    for (uint32_t b = threadIdx.x; b <= nparts; b += kBinWG) s_boff[b] = boff[b];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    const EntryOut out{n, count, ekey, eface, erank, emask, (blockIdx.x * (kBinWG / 64) + wave) % kShards, shard_region(cap)};
    const UnitWalk u{s_boff, first_local, nparts, chunk, T, s_face};
    // the queue's first cnt (<= 64) pairs: pixel masks (double precision), the non-empty ones
    // appended to the entry list (wave-uniform; inlined at both calls, as the kernel is built for:
    // left to the inliner, the jittered form called it out of line through 264 B of scratch)
    auto emit = [&](uint32_t cnt) __attribute__((always_inline)) {
        unsigned long long m = 0;
        uint32_t key = 0, i = 0;
        if (lane < cnt) {
            i = s_qf[wave][lane];
            const uint32_t t = s_qt[wave][lane];
            key = s_qk[wave][lane];
            if constexpr (kJitter) m = bin_pixels_jittered(cull[i], W, H, phase, t & 0xffffu, t >> 16, s_poly + threadIdx.x, kBinWG);
            else m = bin_pixels(cull[i], W, H, phase, t & 0xffffu, t >> 16);
        }
        append_entries(out, m, key, i);
    };
    // Most pairs of a face's bin rectangle are empty (C5: 7.1M pairs, 0.47M entries per camera),
    // so each pair of the walk (lane = pair c of face i's rectangle, row-major) is first tested
    // against the bin's whole pixel rectangle with the frame kernel's own f32 culling test
    // (cull_rejects over the rectangle of the bin's corner rays, widened as make_bundle does: a
    // rejected bin has no pixel whose ray can hit the face); the survivors queue in LDS and go
    // through the per-row double-precision masks 64 at a time.
    const float rw = __builtin_amdgcn_rcpf((float)W), rh = __builtin_amdgcn_rcpf((float)H);
    const float wlo = 1.0f - 0x1p-20f, whi = 1.0f + 0x1p-20f;
    uint32_t qn = 0;  // queued pairs (wave-uniform)
    walk_units(u, [&](unsigned long long, bool valid, uint32_t i, unsigned long long cu) {
        bool keep = false;
        uint32_t tx = 0, ty = 0, key = 0;
        if (valid) {
            key = fkey[i];  // (in the same round trip as the face's records)
            const int4 g = range[i];
            const uint32_t w = (uint32_t)(g.y - g.x + 1);
            const uint32_t c = (uint32_t)cu;
            // c / w and c % w (c < 2^24: exact in f32) by a float quotient, corrected by one
            uint32_t qy = (uint32_t)((float)c / (float)w);
            int32_t rx = (int32_t)(c - qy * w);
            if (rx < 0) {
                --qy;
                rx += (int32_t)w;
            } else if (rx >= (int32_t)w) {
                ++qy;
                rx -= (int32_t)w;
            }
            tx = (uint32_t)g.x + (uint32_t)rx;
            ty = (uint32_t)g.z + qy;
            keep = true;
            if constexpr (!kJitter) {
                const int32_t x0 = (int32_t)(tx * kBinW), x1 = min(x0 + (int32_t)kBinW, (int32_t)W) - 1;
                const int32_t yb = (int32_t)(ty * kBinH + phase) - (int32_t)kBinH;
                const int32_t y0 = max(yb, 0), y1 = min(yb + (int32_t)kBinH, (int32_t)H) - 1;
                keep = y0 <= y1 && !cull_rejects(cull[i], ((float)x0 * rw) * wlo, ((float)x1 * rw) * whi,
                                                 ((float)y0 * rh) * wlo, ((float)y1 * rh) * whi);
            }
        }
        const unsigned long long kb = __ballot(keep);
        if (keep) {
            const uint32_t pos = qn + (uint32_t)__popcll(kb & lt);
            s_qf[wave][pos] = i;
            s_qt[wave][pos] = tx | (ty << 16);
            s_qk[wave][pos] = key * nbins + ty * bins_x + tx;
        }
        qn += (uint32_t)__popcll(kb);
        wave_sync();
        if (qn >= 64) {
            emit(64);
            const uint32_t rest = qn - 64;  // the queue's tail to its front
            uint32_t f2 = 0, t2 = 0, k2 = 0;
            if (lane < rest) {
                f2 = s_qf[wave][64 + lane];
                t2 = s_qt[wave][64 + lane];
                k2 = s_qk[wave][64 + lane];
            }
            wave_sync();
            if (lane < rest) {
                s_qf[wave][lane] = f2;
                s_qt[wave][lane] = t2;
                s_qk[wave][lane] = k2;
            }
            wave_sync();
            qn = rest;
        }
    });
    if (qn) emit(qn);
}

// Segments (frame setups): the units are the bin rows of each binned face's bin rectangle.  A
// segment's four camera rows each get the pixel range where all four culling conditions of the
// face can pass — bin_pixels' own double-precision lines (face_rect.hpp row_range), over the
// rectangle's columns instead of one bin's 16: the same values, so a bin's bin_pixels mask is
// exactly those ranges cut to its columns — and only the bins the ranges reach become pairs,
// dealt over the wave's lanes (lane = pair) so that one long segment (a sliver across the frame)
// does not serialise its wave.  Every pair bin_pixels would mark non-empty is appended, with the
// same mask, so the entries are the rectangle form's (which also drops pairs its f32 pre-test
// rejects: the frame kernel's exact tests decide either way).  C5: 7.06M rectangle pairs per
// camera for 0.47M entries — the rectangle form spent its time walking the empty ones.
__global__ void __launch_bounds__(kBinWG, kPairsWaves) bin_segments_kernel(const TriCull* __restrict__ cull,
                                                              const int4* __restrict__ range,
                                                              const unsigned long long* __restrict__ first_local,
                                                              const unsigned long long* __restrict__ boff,
                                                              uint32_t nparts, uint32_t chunk,
                                                              const uint32_t* __restrict__ fkey, uint32_t T, uint32_t W,
                                                              uint32_t H, uint32_t phase, uint32_t bins_x,
                                                              uint32_t nbins, uint32_t cap, uint32_t* __restrict__ n,
                                                              uint32_t* __restrict__ count, uint32_t* __restrict__ ekey,
                                                              uint32_t* __restrict__ eface,
                                                              unsigned long long* __restrict__ emask,
                                                              uint32_t* __restrict__ erank) {
    __shared__ unsigned long long s_boff[kSetupMaxBlocks + 1];
    __shared__ uint32_t s_face[kBinWG];
    __shared__ uint32_t s_own[kBinWG];  // the lanes whose segment's pairs start at each slot
    for (uint32_t b = threadIdx.x; b <= nparts; b += kBinWG) s_boff[b] = boff[b];
    __syncthreads();
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const EntryOut out{n, count, ekey, eface, erank, emask, (blockIdx.x * (kBinWG / 64) + wave) % kShards, shard_region(cap)};
    const UnitWalk u{s_boff, first_local, nparts, chunk, T, s_face};
    walk_units(u, [&](unsigned long long, bool valid, uint32_t i, unsigned long long c) {
        // the lane's segment: face i, bin row ty, its rows' pixel ranges packed lo | hi << 16 (lo >
        // hi: none) and its bins [bx0, bx0 + width)
        uint32_t ty = 0, key = 0, bx0 = 0, width = 0;
        uint32_t rr[kBinH] = {1u, 1u, 1u, 1u};
        if (valid) {
            const int4 g = range[i];
            key = fkey[i];
            ty = (uint32_t)g.z + (uint32_t)c;
            const int32_t xa = g.x * (int32_t)kBinW, xb = min((g.y + 1) * (int32_t)kBinW, (int32_t)W) - 1;
            int32_t lo = INT32_MAX, hi = INT32_MIN;
            row_ranges(cull[i], W, H, phase, ty, xa, xb, rr, lo, hi);
            if (lo <= hi) {
                bx0 = (uint32_t)lo / kBinW;
                width = (uint32_t)hi / kBinW - bx0 + 1;
            }
        }
        // the wave's pairs: lane l's segment owns [start_l, start_l + width_l)
        uint32_t incl = width;
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t y = (uint32_t)__shfl_up((int)incl, off);
            if ((int)lane >= off) incl += y;
        }
        const uint32_t total = (uint32_t)__shfl((int)incl, 63), start = incl - width;
        uint32_t cur = 0;  // the lane owning the pair before the window
        for (uint32_t t0 = 0; t0 < total; t0 += 64) {  // (wave-uniform)
            s_own[threadIdx.x] = lane ? 0u : cur;
            wave_sync();
            if (width && start >= t0 && start < t0 + 64) s_own[64 * wave + (start - t0)] = lane;
            wave_sync();
            const uint32_t o = wave_prefix_max(s_own[threadIdx.x]);  // (lanes in segment order)
            cur = (uint32_t)__builtin_amdgcn_readlane((int)o, 63);
            const uint32_t t = t0 + lane;
            // the owner's segment
            const uint32_t oi = (uint32_t)__shfl((int)i, (int)o), oty = (uint32_t)__shfl((int)ty, (int)o);
            const uint32_t okey = (uint32_t)__shfl((int)key, (int)o), obx0 = (uint32_t)__shfl((int)bx0, (int)o);
            const uint32_t ostart = (uint32_t)__shfl((int)start, (int)o);
            uint32_t orr[kBinH];
#pragma unroll
            for (uint32_t r = 0; r < kBinH; ++r) orr[r] = (uint32_t)__shfl((int)rr[r], (int)o);
            unsigned long long m = 0;
            const uint32_t bx = obx0 + (t - ostart);
            if (t < total) m = bin_mask_of_rows(orr, bx);
            append_entries(out, m, okey * nbins + oty * bins_x + bx, oi);
            wave_sync();  // (s_own is rewritten by the next window)
        }
    });
}

}  // namespace
}  // namespace gpu
}  // namespace eray
