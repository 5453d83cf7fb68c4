// frame_plan.hpp — what a frame call (capi_frames.cpp) decides before it touches the GPU: the rows
// a call reaches, the render-parameter and ring checks with their messages, the frames per launch,
// which ring slot a launch starts at, how a call's frames split into graph chunks, a remainder and
// plain launches, and when a ring exceeds the Infinity Cache.  Index arithmetic with no HIP header
// or call, so the frame calls and the stand-alone checker (tests/cpp/frame_plan_main.cpp, built with
// the host sanitizers) share it.  The checks return the call's status and write its message into the
// caller's buffer (kWhyLen bytes hold every one of them).
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include "../../include/eray_hip.h"
#include "band_rows.hpp"
#include "bin_layout.hpp"
#include "frame_params.hpp"

namespace eray {
namespace gpu {

constexpr size_t kWhyLen = 256;

// The rendered rows of a call: camera rows [row0, row0 + rows), or rows local rows of
// interleaved bands (eray_render_params::band_rows).
struct RowSpan {
    uint32_t row0, rows, band_shift, band_mask, band_stride;
};
// eray_render_params' band fields as FrameParams encodes them (contiguous: shift 31)
inline RowSpan row_span(const eray_render_params* rp) {
    if (!rp->band_rows) return RowSpan{rp->row0, rp->rows, 31u, 0x7fffffffu, 0u};
    uint32_t shift = 0;
    while ((1u << shift) < rp->band_rows) ++shift;
    return RowSpan{rp->row0, rp->rows, shift, rp->band_rows - 1u, rp->band_stride};
}

constexpr uint32_t kKnownRenderFlags = ERAY_RENDER_BRUTE_FORCE | ERAY_RENDER_DENSE_DETAIL | ERAY_RENDER_NO_DENSE_DETAIL |
                                       ERAY_RENDER_SEPARATE_FILL | ERAY_RENDER_NO_SEPARATE_FILL |
                                       ERAY_RENDER_SHARED_DETAIL | ERAY_RENDER_NO_RAY_ACCEL;

// ERAY_OK when `rp` can be rendered with a camera of W x H pixels (Camera::size) and `bounces`
// reflection levels in effect (rp->bounces where some material reflects, else 0), else the status
// the frame calls return and its message in why[0 .. n).
inline int check_render_params(const eray_render_params* rp, uint32_t W, uint32_t H, uint32_t bounces, char* why, size_t n) {
    if (n) why[0] = 0;
    if (bounces > kMaxBounces)
        return snprintf(why, n, "bounces = %u: at most %u reflection levels", rp->bounces, kMaxBounces), ERAY_E_UNSUPPORTED;
    if (rp->flags & ~kKnownRenderFlags) return snprintf(why, n, "unknown render flags 0x%x", rp->flags), ERAY_E_INVALID_ARGUMENT;
    if (!rp->band_rows && (uint64_t)rp->row0 + rp->rows > H)
        return snprintf(why, n, "rows [%u, %u) exceed the camera height %u", rp->row0, rp->row0 + rp->rows, H),
               ERAY_E_INVALID_ARGUMENT;
    // Image::set indexes y * image.width + x and panics past the end (image.rs:41-43)
    if (W && H && (uint64_t)(H - 1) * rp->image_width + (W - 1) >= (uint64_t)rp->image_width * rp->image_height)
        return snprintf(why, n, "camera size %ux%u does not fit the %ux%u engine image (Image::set panics)", W, H,
                        rp->image_width, rp->image_height),
               ERAY_E_OUT_OF_BOUNDS;
    if (rp->out_ppm && (W != rp->image_width || H != rp->image_height))
        return snprintf(why, n, "fused PPM output needs camera size == image size; use eray_pack_ppm"), ERAY_E_INVALID_ARGUMENT;
    if (rp->band_rows) {  // interleaved bands: aligned to the 4-row sub-blocks, inside the camera
        if (rp->band_rows % 4 || (rp->band_rows & (rp->band_rows - 1)) || rp->band_stride % 4 || rp->row0 % 4 ||
            rp->band_stride < rp->band_rows)
            return snprintf(why, n,
                            "bands: band_rows (%u) must be a power of two >= 4, band_stride (%u) and row0 (%u) "
                            "multiples of 4, band_stride >= band_rows", rp->band_rows, rp->band_stride, rp->row0),
                   ERAY_E_INVALID_ARGUMENT;
        const RowSpan rs = row_span(rp);
        if (rp->rows && (uint64_t)rp->row0 + (uint64_t)((rp->rows - 1) >> rs.band_shift) * rp->band_stride +
                                ((rp->rows - 1) & rs.band_mask) >= H)
            return snprintf(why, n, "bands: %u local rows reach past the camera height %u", rp->rows, H), ERAY_E_INVALID_ARGUMENT;
    }
    return ERAY_OK;
}

// 16-byte row stores: 16-byte aligned rows, and byte offsets of the largest output (f32 RGB)
// within 32 bits (the kernels store through buffer resources, hit.hpp stream16)
inline bool rows_aligned(uint32_t img_w, uint32_t rows, const void* rgb, const void* ppm, const void* face) {
    return (img_w % 16) == 0 && (uint64_t)rows * img_w * 12u < (1ull << 32) &&
           ((reinterpret_cast<uintptr_t>(rgb) | reinterpret_cast<uintptr_t>(ppm) | reinterpret_cast<uintptr_t>(face)) & 15) == 0;
}

// An unculled call of a scene with objects renders every pixel in detail: one rectangle, the frame
// of W pixels x `rows` rows (sub-block units), into p's nrect / rects[0] / total_sub.
inline void whole_frame_rect(uint32_t W, uint32_t rows, uint32_t nobj, FrameParams* p) {
    if (!nobj) return;
    p->nrect = 1;
    p->rects[0][0] = 0;
    p->rects[0][1] = (int32_t)((W - 1) / kBinW);
    p->rects[0][2] = 0;
    p->rects[0][3] = (int32_t)((rows - 1) / kBinH);
    p->total_sub = (uint32_t)(p->rects[0][1] + 1) * (uint32_t)(p->rects[0][3] + 1);
}

// Frames in flight (eray_frame_ring): frames of one call are rendered `per_launch` to a kernel
// launch (FrameParams::nframes), frame k into ring slot k % slots.
struct Ring {
    uint32_t slots = 1, per_launch = 1;
    uint64_t rgb = 0, ppm = 0, face = 0;  // bytes between slots
};
// One launch renders at most this many pixels (frames x rows x width) when the library picks the
// frames per launch, at most kMaxInFlight frames.  Measured (scripts/frames_in_flight.py,
// profiles/r03/frames_in_flight.jsonl, device us per frame by frames per launch): the cube at
// 1920x1080 9.3 / 7.6 / 5.4 / 5.0 for 1 / 2 / 4 / 8, at 3840x2160 22.9 / 19.6 for 1 / 2; the 70k
// stand-in (screen bins, heavier detail work) at 1920x1080 14.2 / 9.2 / 8.2 / 9.2, at 3840x2160
// 29.1 / 34.5 for 1 / 2.  So two frames of 3840x2160 pixels for small scenes, one for scenes with
// binned meshes.
constexpr uint64_t kInFlightPixels = 2ull * 3840ull * 2160ull, kInFlightPixelsBinned = 3840ull * 2160ull;
constexpr uint32_t kMaxInFlight = 8;

// The frames per launch of a call whose frames are cam_w x rows pixels, into a ring of `slots`: 1
// for the general tracer (it renders one frame per launch) and for one slot, else the caller's
// `asked`, else (0) the library's: the largest power of two within the pixel cap — the binned
// scenes' when some object has more than kDirectMax faces.
inline uint32_t frames_per_launch(bool general, uint32_t slots, uint32_t asked, uint64_t cam_w, uint64_t rows,
                                  uint32_t max_object_tris) {
    if (general || slots == 1) return 1;
    if (asked) return asked;
    const uint64_t cap = max_object_tris > kDirectMax ? kInFlightPixelsBinned : kInFlightPixels;
    uint32_t F = 1;
    while (F * 2 <= kMaxInFlight && F * 2 <= slots && (uint64_t)(F * 2) * cam_w * rows <= cap) F *= 2;
    return F;
}

// The ring of a call with frame parameters p (of rp): `r`'s when it is valid (null: one slot), else
// the status and its message in why[0 .. n).
inline int make_ring(const eray_render_params* rp, const FrameParams& p, const eray_frame_ring* r, Ring* out, char* why,
                     size_t n) {
    *out = Ring{};
    if (n) why[0] = 0;
    if (!r) return ERAY_OK;
    if (!r->slots || r->slots > kMaxFramesPerLaunch || (r->slots & (r->slots - 1)))
        return snprintf(why, n, "ring: slots (%u) must be a power of two <= 64", r->slots), ERAY_E_INVALID_ARGUMENT;
    const uint64_t px = (uint64_t)rp->rows * rp->image_width;
    const uint64_t need[3] = {px * 12u, px * 3u, px * 4u};
    const uint64_t stride[3] = {r->rgb_stride, r->ppm_stride, r->face_stride};
    const void* ptr[3] = {rp->out_rgb, rp->out_ppm, rp->out_face};
    for (int k = 0; k < 3; ++k) {
        if (!ptr[k] || r->slots == 1) continue;
        if (stride[k] % 16 || stride[k] < need[k])
            return snprintf(why, n, "ring: output %d's slot stride %llu must be a multiple of 16 of at least %llu bytes", k,
                            (unsigned long long)stride[k], (unsigned long long)need[k]),
                   ERAY_E_INVALID_ARGUMENT;
    }
    if (r->frames_per_launch && (r->frames_per_launch > r->slots || (r->frames_per_launch & (r->frames_per_launch - 1))))
        return snprintf(why, n, "ring: frames_per_launch (%u) must be a power of two <= slots (%u)", r->frames_per_launch,
                        r->slots),
               ERAY_E_INVALID_ARGUMENT;
    out->slots = r->slots;
    out->rgb = r->slots > 1 ? r->rgb_stride : 0;
    out->ppm = r->slots > 1 ? r->ppm_stride : 0;
    out->face = r->slots > 1 ? r->face_stride : 0;
    out->per_launch = frames_per_launch(p.aa || p.bounces, r->slots, r->frames_per_launch, p.cam_w, p.rows, p.max_object_tris);
    return ERAY_OK;
}

// The launch parameters of frames [f, f + count) of a call: ring slot f % slots onwards (slots is
// a multiple of per_launch, so a launch's frames never wrap).
inline FrameParams ring_frames(const FrameParams& p, const Ring& r, uint32_t f, uint32_t count) {
    FrameParams q = p;
    const uint64_t slot = f % r.slots;
    q.nframes = count;
    q.rgb_stride = r.rgb;
    q.ppm_stride = r.ppm;
    q.face_stride = r.face;
    if (q.out_rgb) q.out_rgb = reinterpret_cast<float*>(reinterpret_cast<char*>(q.out_rgb) + slot * r.rgb);
    if (q.out_ppm) q.out_ppm += slot * r.ppm;
    if (q.out_face) q.out_face = reinterpret_cast<int32_t*>(reinterpret_cast<char*>(q.out_face) + slot * r.face);
    const uint64_t ring_bytes = (uint64_t)r.slots * ((q.out_rgb ? r.rgb : 0) + (q.out_ppm ? r.ppm : 0) + (q.out_face ? r.face : 0));
    if (ring_bytes > kInfinityCacheBytes) q.launch_flags |= kLaunchRingBeyondCache;
    return q;
}

// Frame f of a run of n frames rendered per_launch to a launch: the frames its launch renders, f
// onwards, or 0 when the launch of frame f - f % per_launch renders it.
inline uint32_t launch_frames(uint32_t f, uint32_t n, uint32_t per_launch) {
    if (f % per_launch) return 0;
    return per_launch < n - f ? per_launch : n - f;
}
// The frames per launch of runs cut into batches of K frames (the multi-camera setups): per_launch
// (a power of two) halved until it divides K, so that no launch spans two batches.
inline uint32_t fit_per_launch(uint32_t per_launch, uint32_t K) {
    while (K % per_launch) per_launch /= 2;
    return per_launch;
}

// The launch plan of `frames` frames: chunks of `chunk` = min(frames, kGraphFrames) frames,
// frames / chunk of them, and one of the remainder `rest`; what is left is rendered by plain
// launches.  chunk = 0: plain launches only.
constexpr uint32_t kGraphFrames = 64;
struct PlanShape {
    uint32_t chunk = 0, rest = 0;
};
// Captured graphs (capturable: not the null stream), at least two frames: the remainder gets a
// graph of its own when it is more than one frame (no plain launches beyond that one, whose host
// cost can exceed a frame's device time).
inline PlanShape graph_plan_shape(uint32_t frames, bool capturable) {
    PlanShape s;
    if (!capturable || frames < 2) return s;
    s.chunk = frames < kGraphFrames ? frames : kGraphFrames;
    const uint32_t r = frames % s.chunk;
    if (r > 1) s.rest = r;
    return s;
}
// The same chunks enqueued frame by frame, with no graphs (every remainder is a chunk).
inline PlanShape direct_plan_shape(uint32_t frames) {
    PlanShape s;
    if (!frames) return s;
    s.chunk = frames < kGraphFrames ? frames : kGraphFrames;
    s.rest = frames % s.chunk;
    return s;
}
// Walks `frames` frames of a plan in order: chunk(first frame, count, rest) for every chunk (rest:
// the remainder's) and plain(frame) for every frame the plan does not cover; the first status that
// is not 0 ends the walk and is returned.
template <typename Chunk, typename Plain>
int walk_plan(const PlanShape& s, uint32_t frames, Chunk&& chunk, Plain&& plain) {
    uint32_t done = 0;
    for (; s.chunk && done + s.chunk <= frames; done += s.chunk)
        if (int st = chunk(done, s.chunk, false)) return st;
    if (s.rest && done + s.rest == frames) {
        if (int st = chunk(done, s.rest, true)) return st;
        done += s.rest;
    }
    for (; done < frames; ++done)
        if (int st = plain(done)) return st;
    return 0;
}

}  // namespace gpu
}  // namespace eray
