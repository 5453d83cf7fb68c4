// gather_scene.hpp — the scene-camera gather's kernels (comm.cpp includes it, once): a rank's pack
// of its rectangles' rows, a root's assembly of its frames, and the headers that end the transfers.
// The layouts they read are gather_plan.hpp's.
#pragma once

#include "gather_coded.hpp"  // pattern_words
#include "gather_plan.hpp"

namespace {
// Rank `me`'s rows of frame blockIdx.y, rectangle by rectangle (16-B words: rows of W % 16 == 0
// pixels on 16-B aligned buffers, column groups of 48 B), into its slot: own + index * bytes when
// `me` assembles the frame, else send + send_slot * bytes.
__global__ void __launch_bounds__(256) gather_pack_kernel(const uint8_t* __restrict__ local, uint64_t local_stride,
                                                          uint8_t* __restrict__ send, uint8_t* __restrict__ own,
                                                          RankLayout L, uint32_t W, Roots R, uint32_t me) {
    const uint32_t q = blockIdx.x, k = blockIdx.y;
    const uint32_t rk = R.root(k);
    uint8_t* out = rk == me ? own + (size_t)R.index(k) * L.bytes
                            : send + (size_t)R.send_slot(k, me) * L.bytes + kHdr * R.group(rk, me);
    uint32_t i = 0;
    while (i + 1 < L.nrect && q >= L.r[i + 1].first) ++i;
    const GatherRect& g = L.r[i];
    const uint32_t j = (uint32_t)g.l0 + (q - g.first);
    const uint4* src = reinterpret_cast<const uint4*>(local + k * local_stride + (size_t)(L.rows - 1 - j) * W * 3u +
                                                      48u * (uint32_t)g.c0);
    uint4* dst = reinterpret_cast<uint4*>(out + g.off + (size_t)(q - g.first) * g.row_bytes);
    for (uint32_t w = threadIdx.x; w < g.row_bytes / 16u; w += blockDim.x) dst[w] = src[w];
}

// A root: file row blockIdx.x of its frame blockIdx.y (of B) — the miss colour, except inside the
// owning rank's rectangles, whose bytes come from that rank's block of the receive area.
__global__ void __launch_bounds__(256) gather_assemble_kernel(const uint8_t* __restrict__ recv,
                                                              const RankLayout* __restrict__ lay, uint32_t B,
                                                              uint8_t* __restrict__ frames, uint64_t frame_stride,
                                                              uint32_t H, uint32_t W, uint32_t band, uint32_t N,
                                                              uint32_t kind, uint64_t key, int32_t* fault) {
    __shared__ RankLayout s_L;
    // every sender's header (and this root's own): all ERAY_OK and the plan's source, or no frame
    bool bad = false;
    if (threadIdx.x < N) {
        const RankLayout& Lq = lay[threadIdx.x];
        if (Lq.bytes) {
            const XferHeader h = *reinterpret_cast<const XferHeader*>(recv + recv_block(Lq, threadIdx.x, B) +
                                                                      (size_t)B * Lq.bytes);
            bad = !header_ok(h, kind, key);
        }
    }
    if (__syncthreads_or(bad)) {
        if (threadIdx.x == 0 && blockIdx.x == 0 && blockIdx.y == 0) __hip_atomic_store(fault, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
        return;
    }
    const uint32_t F = blockIdx.x, k = blockIdx.y;
    const uint32_t Y = H - 1 - F;  // camera row
    uint32_t r, j;
    if (band) {
        r = (Y / band) % N;
        j = (Y / (N * band)) * band + Y % band;
    } else {
        const uint32_t h = H / N;
        r = (H - 1 - Y) / h;
        j = Y - (H - (r + 1) * h);
    }
    if (threadIdx.x < sizeof(RankLayout) / 4)
        reinterpret_cast<uint32_t*>(&s_L)[threadIdx.x] = reinterpret_cast<const uint32_t*>(lay + r)[threadIdx.x];
    __syncthreads();
    uint32_t bg[3];
    pattern_words(25u | (25u << 8) | (51u << 16), bg);  // sat_u8(0.1 * 255), sat_u8(0.2 * 255)
    const uint8_t* base = recv + recv_block(s_L, r, B) + (size_t)k * s_L.bytes;
    uint4* dst = reinterpret_cast<uint4*>(frames + k * frame_stride + (size_t)F * W * 3u);
    for (uint32_t w = threadIdx.x; w < W * 3u / 16u; w += blockDim.x) {
        const uint32_t c = w / 3u;  // 16-pixel column group (48 B = 3 words)
        uint4 v;
        const uint32_t ph = w % 3u;
        v = make_uint4(bg[ph], bg[(ph + 1) % 3u], bg[(ph + 2) % 3u], bg[ph]);
        for (uint32_t i = 0; i < s_L.nrect; ++i) {
            const GatherRect& g = s_L.r[i];
            if ((int32_t)j >= g.l0 && (int32_t)j <= g.l1 && (int32_t)c >= g.c0 && (int32_t)c <= g.c1) {
                v = reinterpret_cast<const uint4*>(base + g.off + (size_t)((int32_t)j - g.l0) * g.row_bytes)
                    [w - 3u * (uint32_t)g.c0];
                break;
            }
        }
        dst[w] = v;
    }
}

// A rank's header at each of its spots (HeaderSpots: after each send group, after its own packs).
__global__ void gather_header_kernel(uint8_t* __restrict__ buf, HeaderSpots at, XferHeader h) {
    if (threadIdx.x < at.n) *reinterpret_cast<XferHeader*>(buf + at.off[threadIdx.x]) = h;
}
}  // namespace
