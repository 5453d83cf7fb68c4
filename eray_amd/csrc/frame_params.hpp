// frame_params.hpp — the frame launch's argument record (FrameParams) and the constants it and the
// frame calls need: no HIP header and no HIP call, so the kernels (through internal.hpp), the frame
// calls' planning (frame_plan.hpp) and its stand-alone checker (tests/cpp/frame_plan_main.cpp) share
// it.  The records it only points to are internal.hpp's.
#pragma once

#include <stdint.h>

namespace eray {
namespace gpu {

struct TriHot;
struct TriShade;
struct TriCull;
struct ObjectDesc;
struct LightDesc;
struct CamState;

// Objects with more faces than this are not scanned per wave: screen bins / LDS tiles.
constexpr uint32_t kDirectMax = 256;
// Detail rectangles carried in the kernel arguments (more objects: merged into the last one).
constexpr int kMaxRects = 8;
// Deepest reflection recursion the general tracer keeps frames for (Engine::bounces).
constexpr uint32_t kMaxBounces = 16;
// Frames one launch may render (eray_frame_ring::frames_per_launch <= slots <= 64).
constexpr uint32_t kMaxFramesPerLaunch = 64;
// The MI355X Infinity Cache (the die's last-level cache, MI355X_MICROARCH.md).
constexpr uint64_t kInfinityCacheBytes = 256ull << 20;

constexpr uint32_t kTraceSkipTris = 256;  // general tracer: largest scene with the background skip

struct FrameParams {
    // camera (camera.rs:57-76)
    float cx, cy, cz;
    float ratio;  // fov0 / fov1
    float z_dist;
    uint32_t cam_w, cam_h;
    // output
    uint32_t img_w, img_h;
    uint32_t row0, rows;
    // interleaved row bands (multi-GPU balance): local row j is camera row
    // row0 + (j >> band_shift) * band_stride + (j & band_mask) (band_rows = 1 << band_shift, a
    // power of two); a contiguous block is band_shift = 31, band_mask = 0x7fffffff (row0 + j)
    uint32_t band_shift, band_mask, band_stride;
    float* out_rgb;
    uint8_t* out_ppm;
    int32_t* out_face;
    uint32_t aligned;  // img_w % 16 == 0 and 16-byte aligned outputs: 16-byte row stores
    // scene
    const TriHot* tris;
    const TriShade* shade;
    const TriCull* cull;  // nullptr: brute force
    const ObjectDesc* objects;
    const LightDesc* lights;
    uint32_t nobj, nlights;
    uint32_t max_object_tris;  // selects the kernel variant with LDS triangle tiles
    uint32_t total_tris;
    uint32_t lds_scene;        // the scene is small enough to preload into LDS (kCache*)
    uint32_t nrect;            // detail rectangles (sub-block units: 16 px x 4 rank-local rows,
    uint32_t total_sub;        // inclusive) and the number of sub-blocks they cover, counting
    int32_t rects[kMaxRects][4];  // overlaps once: x0, x1, y0, y1
    uint32_t spec_pow;         // some material has a specular-power output (powf != identity)
    uint32_t example_mat;      // some material evaluates main.rs's graph per hit (example)
    uint32_t tiles_x;    // 64 x 4 pixel blocks per row
    uint32_t bins_x;     // screen bins per row
    uint32_t bin_phase;  // bins start at camera rows bin_phase + k * kBinH (row0 % kBinH)
    // Detail sub-block list (scenes with binned objects, bins.hip detail_list_kernel): the j-th
    // detail sub-block is detail_list[j] = sy << 16 | sx (sub-block units, rank-local rows) and
    // bit i of detail_occ[block] marks sub-block i of 64 x 4 block `block` as listed.  Null: the
    // detail rectangles enumerate the sub-blocks.
    const uint32_t* detail_list;
    const uint8_t* detail_occ;
    // the ordered detail list's heavy sub-blocks (its first detail_heavy[0] entries: a bin of more
    // than one 64-entry chunk), or null (an unordered list: every sub-block treated as heavy)
    const uint32_t* detail_heavy;
    uint32_t detail_wgs;  // most workgroups of the frame kernel's grid doing detail work (0: all)
    uint32_t fill_first;  // the fill workgroups take the grid's first block indices (dispatched first)
    uint32_t separate_fill;  // the frame kernel does detail work only; fill_kernel writes the background
    uint32_t fill_cap;       // at most this many workgroups write the background (0: no cap)
    // device-camera mode: camera, detail rectangles and detail count come from the setup
    // kernels' CamState (the host has not read them back); null: the fields above hold them
    const CamState* cam_state;
    // device-camera mode's fill reservation (launch_frame_kernel computes it on the host in
    // args mode): detail workgroups at the default share and at the small-scene share used
    // when the detail sub-blocks exceed one round (frame_kernel decides from the count)
    uint32_t detail_wgs_alt;
    uint32_t launch_flags;  // ERAY_RENDER_* launch overrides (dense / separate fill), part of the plan key
    // general tracer (trace.hip): anti-aliasing rays per pixel, reflection depth, jitter seed;
    // aa == 0 && bounces == 0 selects the frame kernel
    uint32_t aa, bounces;
    uint32_t seed_lo, seed_hi;
    // trace_kernel's culling records for this camera (scenes of at most kTraceSkipTris faces;
    // null: no background skip), written by trace_cull_kernel when the camera or the scene changes
    TriCull* trace_cull;
    // trace_kernel's camera rays scan the binned objects' screen bins (a setup with
    // SetupParams::keep_all; the descriptors' bin views and rectangles), else every face
    uint32_t trace_bins;
    // ... over the setup's detail list (the sub-blocks some ray of which may hit a face; detail_occ
    // per 64 x 4 block): trace_heavy_kernel's workgroups take the heavy head of the list, a
    // workgroup per sub-block; trace_binned_kernel's first trace_fill_wgs workgroups write the
    // background of the unlisted sub-blocks and the next trace_light_wgs the light list, a wave
    // per sub-block
    uint32_t trace_heavy_wgs, trace_fill_wgs, trace_light_wgs;
    // Frames in flight: one launch renders `nframes` (>= 1) independent frames, its workgroups
    // dealt round-robin over them (frame_kernel).  Frame f writes out_* + f * *_stride (bytes,
    // multiples of 16) and, with dev_slots, reads the batched per-camera setup of slot f
    // (cam_state + f, cull + f * total_tris, objects + f * nobj: launch_camera_setup_batch) and,
    // for scenes with binned objects (the multi-camera setup), its detail list at detail_list +
    // f * dlist_stride and occupancy at detail_occ + f * dlist_stride / 4.
    uint32_t nframes;
    uint32_t dev_slots;
    uint32_t dlist_stride;
    // device-camera mode with a split detail list of this capacity (0: none): list position j of
    // CamState::heavy_sub heavy sub-blocks is j, of a light one dlist_split - 1 - (j - heavy_sub)
    uint32_t dlist_split;
    uint64_t rgb_stride, ppm_stride, face_stride;
    // frame stores also non-temporal (launch_render: a launch whose outputs exceed the 256 MiB
    // Infinity Cache — the frame's lines then do not evict what the detail waves read back)
    uint32_t store_nt;
};

// Launch overrides of eray_render_params::flags (eray_hip.h ERAY_RENDER_*) the frame launcher reads.
constexpr uint32_t kLaunchDense = 2u, kLaunchNoDense = 4u, kLaunchSeparateFill = 8u, kLaunchNoSeparateFill = 16u,
                   kLaunchSharedDetail = 32u;
// (internal, set per launch by the ring plan: the ring's slots together exceed the Infinity Cache)
constexpr uint32_t kLaunchRingBeyondCache = 1u << 16;

}  // namespace gpu
}  // namespace eray
