// bin_detail.hpp — the detail sub-block list of the rendered rows from the finished bins (bins.hip
// includes it after bin_walk.hpp): ordered (flags, then compactions in raster order) or appended
// in one launch.
#pragma once

#include "bin_walk.hpp"

namespace eray {
namespace gpu {
namespace {

// Sub-block s = sy * (4 * tiles_x) + sx (padded rows: a 64 x 4 block's four sub-blocks are four
// consecutive threads): listed when some object can be hit there — a binned object's bin is
// non-empty (the frame kernel's bin of the sub-block, first_hit_binned) or another object's pixel
// rectangle reaches it.  Ordered form (one-camera setups): flags, then device-wide compactions in
// raster order — first the heavy sub-blocks (a bin of more than one 64-entry chunk), then the
// others.  The frame kernel deals the list out in rounds of one sub-block per detail wave, so the
// heavy ones go in the first round and the last round holds only one-chunk sub-blocks
// (3840x2160 / 70k: two rounds, and the second one's slowest workgroups set the frame's end,
// profiles/r02/trace/).  Any order gives the same image.
__global__ void __launch_bounds__(kBinWG) detail_flags_kernel(const ObjectDesc* __restrict__ objs, uint32_t nobj,
                                                              uint32_t cam_w, uint32_t row0, uint32_t rows,
                                                              uint32_t band_shift, uint32_t band_mask,
                                                              uint32_t band_stride,
                                                              uint32_t bins_x, uint32_t phase, uint32_t tiles_x,
                                                              uint32_t n, uint32_t heavy_min, uint8_t* __restrict__ flags,
                                                              uint8_t* __restrict__ flags_light,
                                                              uint32_t* __restrict__ packed, uint8_t* __restrict__ occ) {
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t row_subs = 4 * tiles_x;
    const uint32_t sx = s % row_subs, sy = s / row_subs;
    bool hit = false, heavy = false;
    if (s < n && sx * kBinW < cam_w) {
        const int32_t x0 = (int32_t)(sx * kBinW), x1 = x0 + (int32_t)kBinW - 1;
        // the sub-block's camera rows (one band: bands are multiples of kBinH rows)
        const int32_t y0 = (int32_t)band_camera_row(row0, band_shift, band_mask, band_stride, sy * kBinH);
        const int32_t y1 = y0 + (int32_t)min(kBinH, rows - sy * kBinH) - 1;
        for (uint32_t oi = 0; oi < nobj && !hit; ++oi) {
            const ObjGeom& g = objs[oi].g;
            if (!g.tri_count) continue;
            if (g.bin_start) {
                const uint32_t bin = bin_row((uint32_t)y0, phase) * bins_x + sx;
                hit = g.bin_start[bin + 1] > g.bin_start[bin];
                heavy = g.bin_start[bin + 1] - g.bin_start[bin] > heavy_min;
            } else {
                hit = x0 <= g.rect[1] && x1 >= g.rect[0] && y0 <= g.rect[3] && y1 >= g.rect[2];
            }
        }
    }
    if (s < n) {
        flags[s] = (hit && heavy) ? 1 : 0;
        flags_light[s] = (hit && !heavy) ? 1 : 0;
        packed[s] = (sy << 16) | sx;
    }
    // the block's four flags: lanes 4b .. 4b + 3 of the wave (row_subs is a multiple of 4)
    const unsigned long long bal = __ballot(hit);
    if (s < n && (threadIdx.x & 3) == 0) occ[s / 4] = (uint8_t)((bal >> (threadIdx.x & 63)) & 0xfu);
}

// Appended form (camera paths: one launch instead of four): the same flags, the listed sub-blocks
// appended with one counter atomic per workgroup and kind — heavy ones (a bin of more than one
// 64-entry chunk) from the front of the camera's list, light ones from its back — so the frame
// kernel still deals the heavy sub-blocks first and searches the light ones one wave each
// (FrameParams::dlist_split; unordered, every sub-block was shared by a workgroup: the moving
// 3840x2160 / 70k frame kernel ran 40 us against 22.6 static).  The counts land in CamState
// (total_sub, heavy_sub, light_sub; zeroed by the finaliser).  (Carrying the bin range in the
// entry, one scalar load fewer per sub-block, measured slower: C3 +0.3 us, 3840x2160 / 70k +1 us.)
__global__ void __launch_bounds__(kBinWG) detail_list_kernel(const ObjectDesc* __restrict__ objs, uint32_t nobj,
                                                             uint32_t cam_w, uint32_t row0, uint32_t rows,
                                                             uint32_t band_shift, uint32_t band_mask,
                                                             uint32_t band_stride, uint32_t bins_x, uint32_t phase,
                                                             uint32_t tiles_x, uint32_t n,
                                                             uint32_t* __restrict__ list, uint8_t* __restrict__ occ,
                                                             CamState* __restrict__ st) {
    __shared__ uint32_t s_cnt[2][kBinWG / 64];
    __shared__ uint32_t s_base[2];
    // camera blockIdx.y of a multi-camera setup: its descriptors, list, occupancy and counts
    objs += (size_t)blockIdx.y * nobj;
    list += (size_t)blockIdx.y * n;
    occ += (size_t)blockIdx.y * (n / 4);
    CamState& cs = st[blockIdx.y];
    const uint32_t s = blockIdx.x * blockDim.x + threadIdx.x;
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t row_subs = 4 * tiles_x;
    const uint32_t sx = s % row_subs, sy = s / row_subs;
    bool hit = false, heavy = false;
    if (s < n && sx * kBinW < cam_w) {
        const int32_t x0 = (int32_t)(sx * kBinW), x1 = x0 + (int32_t)kBinW - 1;
        // the sub-block's camera rows (one band: bands are multiples of kBinH rows)
        const int32_t y0 = (int32_t)band_camera_row(row0, band_shift, band_mask, band_stride, sy * kBinH);
        const int32_t y1 = y0 + (int32_t)min(kBinH, rows - sy * kBinH) - 1;
        for (uint32_t oi = 0; oi < nobj; ++oi) {
            const ObjGeom& g = objs[oi].g;
            if (!g.tri_count) continue;
            if (g.bin_start) {
                const uint32_t bin = bin_row((uint32_t)y0, phase) * bins_x + sx;
                const uint32_t cnt = g.bin_start[bin + 1] - g.bin_start[bin];
                hit |= cnt != 0;
                heavy |= cnt > 64;
            } else {
                hit |= x0 <= g.rect[1] && x1 >= g.rect[0] && y0 <= g.rect[3] && y1 >= g.rect[2];
            }
        }
    }
    // the block's four flags: lanes 4b .. 4b + 3 of the wave (row_subs is a multiple of 4)
    const unsigned long long bal = __ballot(hit), bh = __ballot(hit && heavy), bl = bal & ~bh;
    if (s < n && (threadIdx.x & 3) == 0) occ[s / 4] = (uint8_t)((bal >> (threadIdx.x & 63)) & 0xfu);
    if (lane == 0) {
        s_cnt[0][wave] = (uint32_t)__popcll(bh);
        s_cnt[1][wave] = (uint32_t)__popcll(bl);
    }
    __syncthreads();
    uint32_t before[2] = {0u, 0u}, all[2] = {0u, 0u};
#pragma unroll
    for (uint32_t w = 0; w < kBinWG / 64; ++w)
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            before[k] += w < wave ? s_cnt[k][w] : 0u;
            all[k] += s_cnt[k][w];
        }
    if (threadIdx.x == 0) {
        s_base[0] = all[0] ? atomicAdd(&cs.heavy_sub, all[0]) : 0u;
        s_base[1] = all[1] ? atomicAdd(&cs.light_sub, all[1]) : 0u;
        if (all[0] + all[1]) atomicAdd(&cs.total_sub, all[0] + all[1]);
    }
    __syncthreads();
    const uint32_t e = (sy << 16) | sx;
    const unsigned long long lt = (1ull << lane) - 1ull;
    if (hit && heavy) list[s_base[0] + before[0] + (uint32_t)__popcll(bh & lt)] = e;
    else if (hit) list[n - 1 - (s_base[1] + before[1] + (uint32_t)__popcll(bl & lt))] = e;
}

// The light sub-blocks after the heavy ones (ordered detail list); the list's length into CamState.
__global__ void __launch_bounds__(kBinWG) detail_append_kernel(const uint32_t* __restrict__ light,
                                                               const uint32_t* __restrict__ counts,
                                                               uint32_t* __restrict__ list, CamState* st) {
    const uint32_t heavy = counts[0], nl = counts[1];
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += gridDim.x * blockDim.x)
        list[heavy + i] = light[i];
    if (blockIdx.x == 0 && threadIdx.x == 0) st->total_sub = heavy + nl;
}

}  // namespace
}  // namespace gpu
}  // namespace eray
