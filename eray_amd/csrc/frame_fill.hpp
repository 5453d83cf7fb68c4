// frame_fill.hpp — the frame kernel's outputs and its background: a frame's output arrays
// (FrameOut), the background's 16-byte words, the fill of one block or sub-block (fill_background,
// and fill_block_fast from per-lane constants), the frame's detail rectangles (SubRect) and the
// fill roles' loops over blocks and frames (fill_blocks, fill_frames).  Included by render.hip —
// frame_kernel's fill roles, fill_kernel and ceiling_fill_kernel — and by frame_sub.hpp, whose
// render_sub stores through FrameOut.
#pragma once

#include "frame_scene.hpp"

namespace eray {
namespace gpu {
namespace {

// One frame's output arrays (FrameParams::out_* of the frame: frames in flight write their own).
struct FrameOut {
    float* rgb;
    uint8_t* ppm;
    int32_t* face;
    bool nt;  // stores also non-temporal (FrameParams::store_nt)
};
__device__ __forceinline__ FrameOut frame_out(const FrameParams& p, uint32_t fr) {
    return FrameOut{p.out_rgb ? reinterpret_cast<float*>(reinterpret_cast<char*>(p.out_rgb) + fr * p.rgb_stride) : nullptr,
                    p.out_ppm ? p.out_ppm + fr * p.ppm_stride : nullptr,
                    p.out_face ? reinterpret_cast<int32_t*>(reinterpret_cast<char*>(p.out_face) + fr * p.face_stride)
                               : nullptr,
                    p.store_nt != 0};
}

// background (engine.rs:211-213) and its bytes: sat_u8(0.1*255) = 25, sat_u8(0.2*255) = 51
__device__ __forceinline__ float4 bg_rgb4(uint32_t phase) {  // 16-byte word at float offset 4c
    const float a = 0.1f, b = 0.2f;
    return phase == 0 ? make_float4(a, a, b, a) : phase == 1 ? make_float4(a, b, a, a) : make_float4(b, a, a, b);
}
__device__ __forceinline__ uint4 bg_ppm16(uint32_t phase) {  // 16-byte word at byte offset 16c
    const uint32_t c01 = sat_u8(0.1f * 255.0f), c02 = sat_u8(0.2f * 255.0f);
    const uint32_t w0 = c01 | (c01 << 8) | (c02 << 16) | (c01 << 24);  // 25 25 51 25
    const uint32_t w1 = c01 | (c02 << 8) | (c01 << 16) | (c01 << 24);  // 25 51 25 25
    const uint32_t w2 = c02 | (c01 << 8) | (c01 << 16) | (c02 << 24);  // 51 25 25 51
    return phase == 0 ? make_uint4(w0, w1, w2, w0) : phase == 1 ? make_uint4(w1, w2, w0, w1) : make_uint4(w2, w0, w1, w2);
}

// Background for the pixels [x0, x0 + w) x rows [py0, py0 + kBlkH) (w = 64 or 16), wave-wide.
// (kNt: non-temporal stores, FrameOut::nt — a template argument, not a per-store select)
template <uint32_t kW, bool kNt = false>
__device__ __forceinline__ void fill_background(const FrameParams& p, const FrameOut& o, uint32_t x0, uint32_t py0, bool aligned,
                                                uint32_t lane) {
    if (aligned && x0 + kW <= p.cam_w && py0 + kBlkH <= p.rows) {
        constexpr uint32_t kRow4 = kW * 3 / 4;    // float4 per RGB row
        constexpr uint32_t kRow16 = kW * 3 / 16;  // 16-byte words per PPM row
        constexpr uint32_t kFace4 = kW / 4;       // int4 per face row
        if (o.rgb) {
#pragma unroll
            for (uint32_t i = lane; i < kBlkH * kRow4; i += 64) {
                const uint32_t r = i / kRow4, c = i % kRow4;
                stream16(o.rgb, reinterpret_cast<float4*>(o.rgb + 3 * ((size_t)(py0 + r) * p.img_w + x0)) + c,
                         bg_rgb4(c % 3), kNt);
            }
        }
        if (o.ppm && lane < kBlkH * kRow16) {
            const uint32_t r = lane / kRow16, c = lane % kRow16;
            const size_t row = (size_t)(p.rows - py0 - kBlkH + r);  // file rows, bottom-up
            stream16(o.ppm, reinterpret_cast<uint4*>(o.ppm + 3 * (row * p.img_w + x0)) + c, bg_ppm16(c % 3), kNt);
        }
        if (o.face && lane < kBlkH * kFace4) {
            const uint32_t r = lane / kFace4, c = lane % kFace4;
            stream16(o.face, reinterpret_cast<int4*>(o.face + (size_t)(py0 + r) * p.img_w + x0) + c,
                     make_uint4(~0u, ~0u, ~0u, ~0u), kNt);
        }
    } else {  // image edge or unaligned output: per pixel
        const float4 b = bg_rgb4(0);
        const uint32_t c01 = sat_u8(0.1f * 255.0f), c02 = sat_u8(0.2f * 255.0f);
        for (uint32_t k = lane; k < kW * kBlkH; k += 64) {
            const uint32_t px = x0 + k % kW, py = py0 + k / kW;
            if (px >= p.cam_w || py >= p.rows) continue;
            const size_t idx = (size_t)py * p.img_w + px;
            if (o.rgb) {
                float* q = o.rgb + 3 * idx;
                q[0] = b.x;
                q[1] = b.y;
                q[2] = b.z;
            }
            if (o.ppm) {
                uint8_t* q = o.ppm + 3 * ((size_t)(p.rows - 1 - py) * p.img_w + px);
                q[0] = (uint8_t)c01;
                q[1] = (uint8_t)c01;
                q[2] = (uint8_t)c02;
            }
            if (o.face) o.face[idx] = -1;
        }
    }
}

// A full 64 x 4 background block's stores (fill_background<kBlkW> for aligned blocks inside the
// frame), per lane: the 16-B words it writes and their byte offsets from the block's first byte in
// each output array.  They are the same for every block, so the fill loop adds a wave-uniform
// block base as the buffer store's scalar offset and issues the stores: no per-store address
// arithmetic or pattern selects (the fill waves share their SIMDs' issue slots with the detail
// waves, and a frame's background is ~99 % of its stores).
struct BlockFill {
    uint4 rgb[3];
    uint32_t rgb_off[3];
    uint4 ppm;
    uint32_t ppm_off;
    uint32_t face_off;
};
__device__ __forceinline__ BlockFill block_fill(uint32_t img_w, uint32_t lane) {
    constexpr uint32_t kRow4 = kBlkW * 3 / 4;    // float4 per RGB row (48)
    constexpr uint32_t kRow16 = kBlkW * 3 / 16;  // 16-byte words per PPM row (12)
    constexpr uint32_t kFace4 = kBlkW / 4;       // int4 per face row (16)
    BlockFill b;
#pragma unroll
    for (uint32_t k = 0; k < 3; ++k) {
        const uint32_t i = lane + 64u * k, r = i / kRow4, c = i % kRow4;
        b.rgb_off[k] = r * img_w * 12u + c * 16u;
        const float4 v = bg_rgb4(c % 3u);
        b.rgb[k] = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
    }
    const uint32_t r = lane / kRow16, c = lane % kRow16;  // lanes < kBlkH * kRow16 store
    b.ppm_off = r * img_w * 3u + c * 16u;
    b.ppm = bg_ppm16(c % 3u);
    b.face_off = (lane / kFace4) * img_w * 4u + (lane % kFace4) * 16u;
    return b;
}
template <bool kNt = false, typename B>
__device__ __forceinline__ void stream16_at(B* base, uint32_t voff, uint32_t soff, uint4 v) {
    stream16_pol<kNt>(base, voff, __builtin_amdgcn_readfirstlane(soff), v);
}
// The block (bx, by) (block units, rank-local rows; wave-uniform) from the lane constants.
template <bool kNt>
__device__ __forceinline__ void fill_block_fast(const FrameParams& p, const FrameOut& o, const BlockFill& bf, uint32_t bx,
                                                uint32_t by, uint32_t lane) {
    const uint32_t x0 = bx * kBlkW, py0 = by * kBlkH;
    if (o.rgb) {
        const uint32_t base = (py0 * p.img_w + x0) * 12u;
#pragma unroll
        for (uint32_t k = 0; k < 3; ++k) stream16_at<kNt>(o.rgb, bf.rgb_off[k], base, bf.rgb[k]);
    }
    if (o.ppm && lane < kBlkH * (kBlkW * 3 / 16))
        stream16_at<kNt>(o.ppm, bf.ppm_off, ((p.rows - py0 - kBlkH) * p.img_w + x0) * 3u, bf.ppm);
    if (o.face) stream16_at<kNt>(o.face, bf.face_off, (py0 * p.img_w + x0) * 4u, make_uint4(~0u, ~0u, ~0u, ~0u));
}

// detail rectangle k of the frame (kernel arguments, or the setup's CamState in device-camera
// mode; uniform index: scalar loads)
struct SubRect {  // sub-block coordinates (x in kSubW columns, y in kBlkH local rows), inclusive
    int32_t sx0, sx1, sy0, sy1;
};
template <bool kDev>
__device__ __forceinline__ SubRect frame_rect(const FrameParams& p, const CamState* cs, uint32_t k) {
    if (kDev) return load_const(reinterpret_cast<const SubRect*>(cs->rects), k);
    return SubRect{p.rects[k][0], p.rects[k][1], p.rects[k][2], p.rects[k][3]};
}
template <bool kDev>
__device__ __forceinline__ uint32_t frame_nrect(const FrameParams& p, const CamState* cs) {
    return kDev ? load_const(&cs->nrect, 0) : p.nrect;
}
__device__ __forceinline__ bool inside(const SubRect& r, int32_t sx, int32_t sy) {
    return sx >= r.sx0 && sx <= r.sx1 && sy >= r.sy0 && sy <= r.sy1;
}

// The background of the non-detail sub-blocks: fill workgroup f of nf strides over the 64 x 4
// blocks (shared by the frame kernel's fill roles and fill_kernel).
// s_waitcnt immediate (gfx9 encoding: vmcnt bits 3:0 and 15:14, expcnt 6:4, lgkmcnt 11:8) of the
// fill's per-block pacing: vmcnt(0), expcnt / lgkmcnt not waited for
constexpr int kFillPace = 0x0f70;
// cacheable stores: two operations may stay in flight (vmcnt(2) against (0): ns1 19.5 -> 19.4,
// C3 23.3 -> 22.7, C2 41.5 -> 41.0 us; (5) and (10) lose the pacing, profiles/r05/ab/ab_r05al.txt)
constexpr int kFillPaceCached = 0x0f72;
// ... cacheable stores into a ring beyond the Infinity Cache (the per-lane form): one operation in
// flight (3840x2160 / 70k in 4 slots: vmcnt(1) 23.42, (2) 23.65, (0) 23.75, (3) 24.1 us,
// profiles/r06/ab/ab_r06kk_pace_beyond.txt)
constexpr int kFillPaceBeyond = 0x0f71;
// kSgpr: block coordinates in SGPRs (the store offsets' block part a scalar); without it they are
// per-lane values and every store a full per-lane offset — faster for an unpaced fill into a ring
// beyond the Infinity Cache (3840x2160 in 4 slots 23.0 -> 19.8 us), slower elsewhere (C2's fill
// alone 34.7 -> 35.8 us, 3840x2160 / 70k 19.8 -> 20.1 us), same-box A/B profiles/r05/ab/ab_r05ah.txt
template <bool kDev, bool kNt, bool kPace, bool kSgpr = true>
__device__ __forceinline__ void fill_blocks(const FrameParams& p, const FrameOut& o, const CamState* cs,
                                            const uint8_t* detail_occ, uint32_t f, uint32_t nf, uint32_t wave,
                                            uint32_t lane, bool aligned) {
    constexpr uint32_t nwaves = kWG / 64;
    if constexpr (kSgpr) wave = __builtin_amdgcn_readfirstlane(wave);
    const uint32_t nblk = p.tiles_x * ((p.rows + kBlkH - 1) / kBlkH);
    const uint32_t fstride = nf * nwaves;
    constexpr bool kFast = kPace && !kNt && kSgpr;  // (below)
    BlockFill bf;
    if constexpr (kFast) bf = block_fill(p.img_w, lane);
    // blocks (bx, by) with bx < full_x and by < full_y are whole 64 x 4 blocks inside the frame
    const uint32_t full_x = aligned ? p.cam_w / kBlkW : 0u, full_y = p.rows / kBlkH;
    uint32_t occ = 0;  // detail list: lane i holds the occupancy of this wave's i-th next block
    uint32_t it = 0;
    const uint32_t nrect = detail_occ ? 0u : frame_nrect<kDev>(p, cs);
    // block coordinates advance incrementally (no integer division per block); the workgroup's
    // four waves take four neighbouring blocks, the workgroups consecutive runs of four
    const uint32_t first = f * nwaves + wave, step_y = fstride / p.tiles_x, step_x = fstride - step_y * p.tiles_x;
    uint32_t by = first / p.tiles_x, bx = first - by * p.tiles_x;
    for (uint32_t blk = first; blk < nblk; blk += fstride, ++it) {
        if (it) {
            bx += step_x;
            by += step_y;
            if (bx >= p.tiles_x) {
                bx -= p.tiles_x;
                ++by;
            }
        }
        uint32_t mask = 0;  // detail sub-blocks of this block
        if (detail_occ) {  // one load per 64 blocks, not a dependent load per block
            if ((it & 63u) == 0) {
                const uint32_t b = blk + lane * fstride;
                occ = b < nblk ? detail_occ[b] : 0u;
                asm volatile("" : "+v"(occ));  // (waited for here; the pacing below is explicit)
            }
            mask = (uint32_t)__builtin_amdgcn_readlane((int)occ, (int)(it & 63u));
        }
        for (uint32_t k = 0; k < nrect; ++k) {
            const SubRect r = frame_rect<kDev>(p, cs, k);
            if ((int32_t)by < r.sy0 || (int32_t)by > r.sy1) continue;
#pragma unroll
            for (int32_t i = 0; i < 4; ++i) {
                const int32_t sx = (int32_t)(4 * bx) + i;
                mask |= (sx >= r.sx0 && sx <= r.sx1) ? (1u << i) : 0u;
            }
        }
        // Pacing beside detail work: each block's stores wait until the wave's earlier stores are
        // acknowledged (vmcnt counts them).  Unpaced fill waves flood the memory system and
        // lengthen the detail waves' load chains — 3840x2160 / 70k 19.8 -> 24.6 us per frame, C3
        // 22.2 -> 27.2, C5 128 -> 141; C2 (8 frames) 40.9 -> 43.5 — and a looser bound (vmcnt(5)
        // or (10)) is no better; a fill with the GPU to itself is faster unpaced (3840x2160 18.3
        // vs 21.5 us), same-box A/B profiles/r05/ab/.
        if constexpr (kPace) __builtin_amdgcn_s_waitcnt(kNt ? kFillPace : kSgpr ? kFillPaceCached : kFillPaceBeyond);
        if (!mask) {
            // the hoisted-offset stores where the fill is paced and cached (C2 8 frames 52.8 ->
            // 41.2 us); unpaced or non-temporal, the per-block address form writes faster (fill
            // alone at 3840x2160 in 4 slots 23.3 -> 19.8 us, C5 130 -> 123 us), same-box A/B
            // profiles/r05/ab/
            if (kFast && bx < full_x && by < full_y)
                fill_block_fast<kNt>(p, o, bf, bx, by, lane);
            else
                fill_background<kBlkW, kNt>(p, o, bx * kBlkW, by * kBlkH, aligned, lane);
        } else if (mask != 0xfu) {
            for (uint32_t i = 0; i < 4; ++i)
                if (!((mask >> i) & 1u)) fill_background<kSubW, kNt>(p, o, bx * kBlkW + i * kSubW, by * kBlkH, aligned, lane);
        }
    }
}

// Fill role q of nf over the launch's frames: virtual roles v (more than nf only when nf < F),
// frame v % F, its (v / F)-th fill workgroup.
template <bool kDev>
__device__ __forceinline__ void fill_frames(const FrameParams& p, uint32_t q, uint32_t nf, uint32_t wave, uint32_t lane,
                                            bool aligned, bool pace) {
    const uint32_t F = p.nframes, roles = max(nf, F);
    for (uint32_t v = q; v < roles; v += nf) {
        const uint32_t fr = v % F, slot = p.dev_slots ? fr : 0u;
        const uint8_t* occ = p.detail_occ ? p.detail_occ + (size_t)slot * (p.dlist_stride / 4) : nullptr;
        const FrameOut o = frame_out(p, fr);
        const uint32_t g = v / F, ng = (roles - fr + F - 1) / F;
        const CamState* cs = p.cam_state + slot;
        // (separate loops: the unpaced fill, without the paced one's lane constants in its
        // registers, writes a 4-slot 3840x2160 frame in 19.8 instead of 22.3 us)
        if (o.nt && pace)
            fill_blocks<kDev, true, true>(p, o, cs, occ, g, ng, wave, lane, aligned);
        else if (o.nt)
            fill_blocks<kDev, true, false>(p, o, cs, occ, g, ng, wave, lane, aligned);
        else if (pace && (p.launch_flags & kLaunchRingBeyondCache))
            // paced into a ring beyond the Infinity Cache: per-lane block coordinates and per-block
            // addresses, as the unpaced form there (3840x2160 / 70k in 4 slots 24.06 -> 23.64 us;
            // C2, C3 and the 1-slot frame unchanged: same-box A/B profiles/r06/ab/ab_r06ii_paced_lane.txt)
            fill_blocks<kDev, false, true, false>(p, o, cs, occ, g, ng, wave, lane, aligned);
        else if (pace)
            fill_blocks<kDev, false, true>(p, o, cs, occ, g, ng, wave, lane, aligned);
        else if (p.launch_flags & kLaunchRingBeyondCache)
            fill_blocks<kDev, false, false, false>(p, o, cs, occ, g, ng, wave, lane, aligned);
        else
            fill_blocks<kDev, false, false>(p, o, cs, occ, g, ng, wave, lane, aligned);
    }
}

}  // namespace
}  // namespace gpu
}  // namespace eray
