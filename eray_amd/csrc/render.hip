// render.hip — the per-pixel ray-tracing hot path on gfx950 (CDNA4).
//
// Replaces Engine::render (src/lib/engine.rs:46-81) with the PPM byte pack of
// Image::save_as_ppm (src/lib/image.rs:48-74) fused in.  One thread per pixel; a 256-thread
// workgroup owns a 64x4 pixel tile and each 64-lane wave a 16x4 sub-tile; the tile's f32 RGB
// and PPM rows leave through LDS as 16-byte coalesced stores.
//
// First-hit search (Object::intersects, object.rs:58-81): the workgroup streams the object's
// triangles in index order through LDS in tiles of kTriTile records; each ray keeps the FIRST
// face (by index) whose Triangle::intersects (primitives.rs:41-72) passes — the reference's
// semantics, not the nearest hit.  The loop ends as soon as no ray of the workgroup is still
// searching (__syncthreads_or).
//
// Exact wave culling (primary rays only; disabled by ERAY_RENDER_BRUTE_FORCE).  For a camera
// ray the reference's test quantities are linear in the (unnormalised) ray direction, and the
// camera directions of a 16x4 pixel block span a small convex cone.  Per camera, each triangle
// gets four affine bounds f_k(x', y') of those quantities with float-error margins T_k
// (camera_setup_kernel in setup.hip, see the derivation there).  A wave evaluates them triangle-parallel —
// lane j takes triangle j of a 64-triangle chunk — and __ballot()s the survivors; only the
// survivors are tested ray-parallel, in index order, with the reference's exact arithmetic.
// The margins make the cull conservative: a triangle the exact test could accept for any ray
// of the block is never dropped, so results are identical to the brute-force scan
// (tests/test_render_gpu.py checks this bit-for-bit).
//
// Shadow rays (engine.rs:136-142, 218-228) go through the same LDS tiles without culling; the
// reference's degenerate bounding box rejects almost all of them before the scan.
//
// The device code is cut by concern into headers that only this file includes: frame_scene.hpp
// (scene views), frame_first_hit.hpp (first-hit searches), frame_fill.hpp (outputs and background)
// and frame_sub.hpp (render_sub: one sub-block's cast_ray).  Here: the kernels and every launch_*.
#include <hip/hip_ext.h>

#include <mutex>

// Per-workgroup timestamps for a diagnostics build (scripts/microbench/render_trace.hip defines
// it before including this file); nothing in the product build.
#ifndef ERAY_TRACE_POINT
#define ERAY_TRACE_POINT(k)
#define ERAY_TRACE_WAVE0(k)
#define ERAY_TRACE_VALUE(k, v)
#endif

#include "frame_fill.hpp"
#include "frame_sub.hpp"

namespace eray {
namespace gpu {
namespace {

// --------------------------------------------------------------------- triangle setup ------
// Triangle::intersects recomputes e1 = b - a, e2 = c - a, n = e1 x e2 for every test
// (primitives.rs:44-46); they do not depend on the ray, so they are computed once here with
// the same f32 operations (bit-identical values).
__global__ void __launch_bounds__(256) tri_precompute_kernel(const float* __restrict__ pos,
                                                             const float* __restrict__ nrm,
                                                             const float* __restrict__ uv,
                                                             uint32_t T, TriHot* __restrict__ hot,
                                                             TriShade* __restrict__ shade) {
    uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= T) return;
    const float* P = pos + 9 * (size_t)i;
    f3 a = mk3(P[0], P[1], P[2]), b = mk3(P[3], P[4], P[5]), c = mk3(P[6], P[7], P[8]);
    f3 e1 = sub(b, a), e2 = sub(c, a);
    f3 n = cross(e1, e2);
    hot[i].q0 = make_float4(e1.x, e1.y, e1.z, e2.x);
    hot[i].q1 = make_float4(e2.y, e2.z, n.x, n.y);
    hot[i].q2 = make_float4(n.z, a.x, a.y, a.z);
    const float* N = nrm + 9 * (size_t)i;
    const float* U = uv + 6 * (size_t)i;
    shade[i].s0 = make_float4(N[0], N[1], N[2], N[3]);
    shade[i].s1 = make_float4(N[4], N[5], N[6], N[7]);
    shade[i].s2 = make_float4(N[8], U[0], U[1], U[2]);
    shade[i].s3 = make_float4(U[3], U[4], U[5], 0.0f);
}

// eray_scene_update_object: tri_precompute_kernel for one object's faces whose vertex arrays are
// replaced in place.  pos / nrm / uv: the caller's arrays (T x 9, T x 9, T x 6; null: kept, not
// read); raw_*: the object's slices of the resident raw array; hot / shade: its slices of the
// records.  One face per lane, 256 faces per workgroup.  A workgroup's faces are one contiguous run
// of each input (256 x 36 B, 256 x 24 B), so the run is read with consecutive lanes on consecutive
// words — not 36 B apart per lane — and each word goes, in the same pass, to the resident raw array
// (consecutive again) and to LDS; the lanes then pick their own face's words out of LDS (word
// strides 9 and 6: conflict-free and 2-way) and compute the records with tri_precompute_kernel's
// operations.  Record stores are whole 16-B words; the one word of TriShade that mixes normals and
// uvs (s2) keeps the other array's part from the record when only one of the two is given.
__global__ void __launch_bounds__(256) tri_update_kernel(const float* __restrict__ pos, const float* __restrict__ nrm,
                                                         const float* __restrict__ uv, uint32_t T,
                                                         float* __restrict__ raw_pos, float* __restrict__ raw_nrm,
                                                         float* __restrict__ raw_uv, TriHot* __restrict__ hot,
                                                         TriShade* __restrict__ shade) {
    __shared__ float s_w[256 * 9];
    const uint32_t f0 = blockIdx.x * 256u, tid = threadIdx.x;
    const uint32_t nf = T - f0 < 256u ? T - f0 : 256u;  // (the grid covers T: f0 < T)
    const uint32_t i = f0 + tid;
    const bool live = tid < nf;
    // one array's run through LDS and into the resident copy (workgroup-uniform control flow)
    auto stage = [&](const float* __restrict__ src, float* __restrict__ dst, uint32_t per) {
        const size_t base = (size_t)per * f0;
        const uint32_t words = per * nf;
        __syncthreads();  // (the previous array's words have been picked up)
        for (uint32_t w = tid; w < words; w += 256u) {
            const float v = src[base + w];
            s_w[w] = v;
            dst[base + w] = v;
        }
        __syncthreads();
    };
    if (pos) {
        stage(pos, raw_pos, 9u);
        if (live) {
            const float* P = s_w + 9u * tid;
            f3 a = mk3(P[0], P[1], P[2]), b = mk3(P[3], P[4], P[5]), c = mk3(P[6], P[7], P[8]);
            f3 e1 = sub(b, a), e2 = sub(c, a);
            f3 n = cross(e1, e2);
            hot[i].q0 = make_float4(e1.x, e1.y, e1.z, e2.x);
            hot[i].q1 = make_float4(e2.y, e2.z, n.x, n.y);
            hot[i].q2 = make_float4(n.z, a.x, a.y, a.z);
        }
    }
    if (!nrm && !uv) return;
    float4 s2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (live && (!nrm || !uv)) s2 = shade[i].s2;
    if (nrm) {
        stage(nrm, raw_nrm, 9u);
        if (live) {
            const float* N = s_w + 9u * tid;
            shade[i].s0 = make_float4(N[0], N[1], N[2], N[3]);
            shade[i].s1 = make_float4(N[4], N[5], N[6], N[7]);
            s2.x = N[8];
        }
    }
    if (uv) {
        stage(uv, raw_uv, 6u);
        if (live) {
            const float* U = s_w + 6u * tid;
            s2.y = U[0];
            s2.z = U[1];
            s2.w = U[2];
            shade[i].s3 = make_float4(U[3], U[4], U[5], 0.0f);
        }
    }
    if (live) shade[i].s2 = s2;
}

// ---------------------------------------------------------------------- frame kernel -------
// The image (rank-local rows) is cut into 64 x 4 pixel blocks of four 16 x 4 sub-blocks.  A
// sub-block inside one of the frame's detail rectangles (FrameParams::rects: the objects' pixel
// rectangles, ObjectDesc::rect, in sub-block units) is "detail": one wave runs Engine::cast_ray
// for its 64 pixels, one pixel per lane.  Every other sub-block is background
// (engine.rs:211-213) with no test at all.  One persistent launch does both:
//  * detail: the detail sub-blocks are enumerated rectangle by rectangle (the host makes the
//    rectangles disjoint) and dealt out round-robin over the first
//    workgroups, four consecutive ones per workgroup, so the latency-bound shading is spread
//    over all CUs instead of clustering on the CUs that own the object's screen region;
//  * fill: the remaining workgroups stride over the 64 x 4 blocks and write the background of
//    the non-detail sub-blocks — a whole block as 3 + 1 + 1 wave-contiguous 16-byte stores.
//    This is the frame's HBM-write floor.  Keeping it off the detail workgroups matters: their
//    loads must not wait behind their own stores (a CDNA wave's vmcnt counts both).

// kDense (large meshes only): 4 workgroups per CU instead of 2 (at most 128 VGPRs), for frames
// whose detail sub-blocks exceed one round of the 2-per-CU grid — there the detail waves are
// latency bound and more resident detail waves mean fewer rounds.  Round 5 (profiles/r05/ab/):
// the culled large-mesh path lost its 64-bit per-lane addresses (buffer loads of records and
// bin entries, scalar store offsets) and fits 4 per CU; with the fill at one workgroup per CU
// (launch_frame_kernel) 3840x2160 / 70k 22.2 -> 20.1 us, its moving camera 50.0 -> 46.7 us.
constexpr int kDenseWgs = 4;
// kOne (LDS-scene builds): the scene has one object (render_sub's single-object path).
template <bool kCull, bool kLdsTiles, int kMat, bool kLdsScene, bool kDense = false, bool kDev = false, bool kOne = false>
__global__ void __launch_bounds__(kWG, (kMat & kMatSpecPow) ? 1 : (kLdsTiles && !kDense) ? 1 : (kDense ? kDenseWgs : 3))  // 3 workgroups per CU where that fits
    frame_kernel(const ObjectDesc* h_objects, const LightDesc* h_lights, const TriCull* h_cull, const TriHot* h_tris,
                 const void* h_aux, uint32_t h_counts, uint32_t h_total_tris, uint32_t h_total_sub,
                 uint32_t h_roles, uint32_t h_band, FrameParams p) {
    // h_aux (preloaded): the TriShade array in the LDS-scene builds (the scene preload reads it
    // first), else the detail list (p.detail_list), whose first entry is each detail wave's first
    // load.  (gfx950 preloads 14 argument dwords — 16 user SGPRs less the argument pointer — so
    // h_band and everything after it are loads.)
    // h_roles (a preloaded argument, see frame_roles): the grid size, the detail workgroups and
    // the role flags, so the role decision — and the scene preload behind it — does not wait for
    // a kernel-argument load from memory
    const uint32_t grid = h_roles & 0xfffu;  // == gridDim.x, without the implicit-argument load
    uint32_t detail_wgs = (h_roles >> 12) & 0xfffu;
    bool fill_first = (h_roles >> 30) & 1u;
    const bool separate_fill = (h_roles >> 31) & 1u;
    // large objects: LDS tiles (shadow rays, brute force) and, aliased, the per-wave binned
    // primary search (first_hit ends its tile loop on a barrier, so the two never overlap)
    // (the culled large-mesh builds search bins wave by wave and scan shadow rays per wave: no
    // workgroup tiles)
    constexpr size_t kTileBytes = (kCull && kLdsTiles) ? 0 : kTriTile * sizeof(TriHot);
    constexpr size_t kBinBytes = (kCull && kLdsTiles) ? (kWG / 64) * kBinLdsBytes + 2 * (kWG / 64) * 4 : 0;
    __shared__ __attribute__((aligned(16))) char s_large[kLdsTiles ? (kTileBytes > kBinBytes ? kTileBytes : kBinBytes) : 16];
    TriHot* s_hot = reinterpret_cast<TriHot*>(s_large);
    TriCull* s_cull = nullptr;
    char* s_bins = s_large;
    __shared__ float4 s_rgb[kBlkW * kBlkH * 3 / 4];    // each wave's f32 RGB rows, staged
    __shared__ uint32_t s_ppm[kBlkW * kBlkH * 3 / 4];  // ... and its PPM byte rows
    extern __shared__ __attribute__((aligned(16))) char dyn[];
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t nwaves = kWG / 64;
    const bool aligned = p.aligned != 0;  // (a kernel-argument read where it is used)
    // Frames in flight: the launch renders F independent frames; detail and fill workgroups are
    // dealt round-robin over them (frame v % F), so one frame's latency-bound detail chains
    // overlap the others' fill stores instead of ending the launch alone.
    const uint32_t F = ((h_roles >> 24) & 63u) + 1u;  // == p.nframes (the role decision needs no load)
    auto cam_state = [&](uint32_t fr) { return p.cam_state + (p.dev_slots ? fr : 0u); };
    // detail sub-blocks per frame (device-camera mode: counted by the setup kernels; the most of
    // any frame sizes the detail roles), and the small-scene fill reservation chosen from that
    // count as launch_frame_kernel does from the host's
    uint32_t total_max = h_total_sub;
    if (kDev) {
        total_max = 0;
        for (uint32_t fr = 0; fr < F; ++fr) total_max = max(total_max, load_const(&cam_state(fr)->total_sub, 0));
    }
    if (kDev && p.detail_wgs_alt && F * total_max > detail_wgs * nwaves) {
        detail_wgs = p.detail_wgs_alt;
        fill_first = true;
    }
    // workgroups [0, nd) render the detail sub-blocks (persistent: rounds of nd * 4 sub-blocks),
    // the others write the background at the same time; at most detail_wgs detail workgroups
    // (the launcher keeps a share of the grid for the fill, so a large detail area overlaps the
    // fill's HBM writes instead of preceding them); when every workgroup has detail work, all of
    // them fill afterwards
    const uint32_t nd = min(detail_wgs ? detail_wgs : grid, F * ((total_max + nwaves - 1) / nwaves));
    // the workgroup's role index: detail roles [0, nd), fill roles [nd, grid); with fill_first
    // the fill roles go to the first-dispatched (older, VALU-priority) workgroups
    const uint32_t bid = (fill_first && nd < grid) ? (blockIdx.x + nd) % grid : blockIdx.x;

    ERAY_TRACE_POINT(0);
    // ---- detail sub-blocks -------------------------------------------------------------------
    if (bid < nd) {
        // the ordered detail list's heavy count: the threshold of the cooperative (workgroup-shared)
        // sub-blocks in builds that keep those paths (brute-force large meshes; no count: every
        // iteration shares its work)
        const bool counted = kLdsTiles && !(p.launch_flags & kLaunchSharedDetail);
        const uint32_t heavy0 =
            (!kCull && counted && p.detail_heavy) ? load_const(p.detail_heavy, 0) : 0xffffffffu;
        // the detail list (preloaded in h_aux outside the LDS-scene builds, which have none)
        const uint32_t* list_base = kLdsScene ? p.detail_list : static_cast<const uint32_t*>(h_aux);
        // One camera (args mode): the wave's first list entry (role bid) depends on preloaded
        // arguments only, so it is loaded first, beside the kernel-argument loads that follow
        // (branch-free: without a list it reads a word of the descriptors, unused).
        uint32_t e_first = 0;
        if constexpr (!kDev && !kLdsScene) {
            const uint32_t c = (bid / F) * nwaves + wave;
            e_first = vload_u32(list_base ? list_base : reinterpret_cast<const uint32_t*>(h_objects),
                                list_base && c < h_total_sub ? c : 0u);
        }
        // snake order for the ordered (heavy-first) lists of binned meshes
        constexpr bool kSnake = kLdsTiles;
        const RowMap rm{p.row0, h_band & 31u, h_band >> 5};
        const uint32_t nobj = h_counts & 0xffffu;
        // virtual detail roles v (more than nd only when nd < F): frame v % F, its (v / F)-th
        // detail workgroup of nk
        const uint32_t roles = max(nd, F);
        for (uint32_t v = bid; v < roles; v += nd) {
            const uint32_t fr = v % F, kw = v / F, nk = (roles - fr + F - 1) / F;
            const uint32_t c0 = kw * nwaves;
            const CamState* cs = cam_state(fr);
            const uint32_t total = kDev ? load_const(&cs->total_sub, 0) : h_total_sub;
            // (per-frame setup slots exist only in device-camera mode)
            const uint32_t slot = (kDev && p.dev_slots) ? fr : 0u;
            const uint32_t* dlist = list_base ? (kDev ? list_base + (size_t)slot * p.dlist_stride : list_base) : nullptr;
            const FrameOut fo = frame_out(p, fr);
            const ObjectDesc* objs = h_objects + (size_t)slot * nobj;
            const TriCull* culls = h_cull ? h_cull + (size_t)slot * h_total_tris : nullptr;
            const uint32_t nrect = dlist ? 0u : frame_nrect<kDev>(p, cs);
            const CamDev cam = frame_camera<kDev>(p, cs);
            // a split list (camera paths): the frame's heavy sub-blocks from the front, the light
            // ones from the back (bins.hip detail_list_kernel) — list positions always follow the
            // setup's heavy count; `heavy` is the cooperative threshold (none without a count)
            const bool split = kDev && p.dlist_split && dlist;
            const uint32_t split_heavy = split ? load_const(&cs->heavy_sub, 0) : 0u;
            const uint32_t heavy = split ? (counted ? split_heavy : 0xffffffffu) : heavy0;
            auto lpos = [&](uint32_t j) {
                return split && j >= split_heavy ? p.dlist_split - 1u - (j - split_heavy) : j;
            };
            // detail sub-block j (enumeration order) -> sub-block coordinates
            auto locate = [&](uint32_t j, int32_t& sx, int32_t& sy, bool first = false) {
                if (dlist) {
                    const uint32_t e = __builtin_amdgcn_readfirstlane((!kDev && !kLdsScene && first && v == bid)
                                                                          ? e_first
                                                                          : vload_u32(dlist, lpos(j)));
                    sx = (int32_t)(e & 0xffffu);
                    sy = (int32_t)(e >> 16);
                    return;
                }
                for (uint32_t k = 0; k < nrect; ++k) {  // the rectangles are disjoint (setup): by area
                    const SubRect r = frame_rect<kDev>(p, cs, k);
                    const uint32_t w = (uint32_t)(r.sx1 - r.sx0 + 1);
                    const uint32_t a = w * (uint32_t)(r.sy1 - r.sy0 + 1);
                    if (j < a) {
                        sx = r.sx0 + (int32_t)(j % w);
                        sy = r.sy0 + (int32_t)(j / w);
                        return;
                    }
                    j -= a;
                }
            };
            // the wave's first sub-block and its camera rays, before the scene is in: the kernel
            // arguments' scalar loads and the ray arithmetic overlap the preload's round trip
            int32_t sx0 = 0, sy0 = 0;
            f3 d0;
            constexpr bool kGivenRay = true;
            auto first_rays = [&]() {
                if (c0 + wave < total) locate(c0 + wave, sx0, sy0, true);
                ERAY_TRACE_WAVE0(11);
                d0 = camera_dir(cam, p, (uint32_t)sx0 * kSubW + lane % kSubW, cam_row(rm, (uint32_t)sy0 * kBlkH + lane / kSubW));
                asm volatile("" : "+v"(d0.x), "+v"(d0.y), "+v"(d0.z));  // here, not after the barrier
            };
            auto detail = [&](const auto& sc, const uint32_t pobj, const uint32_t* pstart) {
                // Rounds of nk * 4 sub-blocks, dealt in snake order: in odd rounds the last
                // workgroup takes the first sub-blocks, so the waves whose first sub-block came
                // from the ordered list's heavy head (the longest chains) take the light tail
                // of the second round.  (A device-wide atomic work counter instead measured
                // 2.5x slower at 3840x2160 / 70k: one hot address under the frame's write stream.)
                const uint32_t round = nk * nwaves;
                auto job = [&](uint32_t r, bool& valid, bool& coop) {  // round r's sub-block of this wave
                    const bool odd = (r & 1u) && kSnake;
                    const uint32_t first = r * round + (odd ? round - nwaves - c0 : c0);
                    valid = first < total;
                    coop = first < heavy;
                    return odd ? first + (nwaves - 1 - wave) : first + wave;
                };
                // Binned meshes with a detail list: the wave's next sub-block — its list entry and
                // its bin range in the first binned object pobj (bin starts pstart) — is loaded
                // during the current one (vector loads, used one sub-block later), so a round
                // after the first starts with its search, not with two dependent round trips.
                uint32_t nx_e = 0, nx_lo = 0, nx_hi = 0;  // (VGPRs: the loads' results)
                bool nx_range = false;                    // nx_lo / nx_hi were issued
                for (uint32_t r = 0;; ++r) {  // workgroup-uniform
                    bool valid, coop;
                    const uint32_t j = job(r, valid, coop);
                    if (!valid) break;
                    const bool active = j < total;
                    int32_t sx = sx0, sy = sy0;
                    PreRange pre{0u, 0u, false};
                    const bool have_pre = pstart && r != 0 && nx_range;
                    if (r != 0 && active) {
                        if (pstart) {  // prefetched during the previous sub-block
                            const uint32_t e = __builtin_amdgcn_readfirstlane(nx_e);
                            sx = (int32_t)(e & 0xffffu);
                            sy = (int32_t)(e >> 16);
                        } else {
                            locate(j, sx, sy);
                        }
                    }
                    if (have_pre && active)
                        pre = PreRange{(uint32_t)__builtin_amdgcn_readfirstlane(nx_lo),
                                       (uint32_t)__builtin_amdgcn_readfirstlane(nx_hi), true};
                    // the next round's sub-block of this wave: its list entry now, its bin range
                    // once this sub-block's first hits are known (mid)
                    bool nvalid = false, ncoop = false;
                    const uint32_t jn = job(r + 1, nvalid, ncoop);
                    const bool nactive = nvalid && jn < total && pstart;
                    if (nactive) nx_e = vload_u32(dlist, lpos(jn));
                    nx_range = false;
                    auto mid = [&]() {
                        if (!nactive) return;
                        const uint32_t e = __builtin_amdgcn_readfirstlane(nx_e);
                        const uint32_t bin = ((cam_row(rm, (e >> 16) * kBlkH) + kBinH - p.bin_phase) / kBinH) * p.bins_x +
                                             (e & 0xffffu);
                        nx_lo = vload_u32(pstart, bin);
                        nx_hi = vload_u32(pstart, bin + 1);
                        nx_range = true;
                    };
                    // the ordered detail list's heavy sub-blocks (bins of several chunks) come
                    // first, so the longest chains start in the first round (coop: shared by the
                    // workgroup in builds that keep the cooperative paths, render_sub)
                    // (the first sub-block's rays by value: a pointer would keep them in scratch memory)
                    render_sub<kCull, kLdsTiles, kMat, kDense, kOne>(p, fo, cam, rm, sc, (uint32_t)sx * kSubW,
                                                             (uint32_t)sy * kBlkH, active, s_hot, s_cull, s_bins, s_rgb,
                                                             s_ppm, aligned, kGivenRay && r == 0, d0, coop, pre, pobj,
                                                             mid, h_counts);
                }
            };
            if constexpr (kLdsScene) {
                if (v != bid) __syncthreads();  // the previous frame's reads of the LDS scene are done
                const FrameHot hf{objs, h_lights, culls, h_tris, static_cast<const TriShade*>(h_aux), h_counts, h_total_tris,
                                  h_total_sub, grid};
                const SceneLds sc = preload_scene(hf, dyn, first_rays);
                __syncthreads();
                detail(sc, ~0u, nullptr);
            } else {
                const SceneGlobal sc{p, objs, culls};
                uint32_t pobj = ~0u;  // the first binned object (culled large-mesh builds with a list)
                const uint32_t* pstart = nullptr;
                if constexpr (kLdsTiles && kCull) {
                    // the first object's descriptor is loaded before the list entry is waited for:
                    // the first sub-block's two inputs in one round trip
                    const ObjGeom g0 = nobj ? sc.geom(0) : ObjGeom{};
                    // The scalar cache lines of what the shading reads after the search — the first
                    // object's MaterialDesc (its two 64-B lines) and the lights — touched now, in
                    // the same round trip: their first reads come after the search, each a scalar
                    // cache miss in a dependent chain otherwise
                    uint32_t warm = 0;
                    if (nobj) {
                        const uint32_t* od = reinterpret_cast<const uint32_t*>(objs);
                        warm = load_const(od + 16, 0) ^ load_const(od + 32, 0);
                    }
                    if (h_counts >> 16) warm ^= load_const(reinterpret_cast<const uint32_t*>(h_lights), 0);
                    if ((h_counts >> 16) > 2u) warm ^= load_const(reinterpret_cast<const uint32_t*>(h_lights + 2), 0);
                    first_rays();
                    asm volatile("" ::"s"(warm));
                    if (dlist)
                        for (uint32_t oi = 0; oi < nobj; ++oi) {
                            const ObjGeom g = oi == 0 ? g0 : sc.geom(oi);
                            if (g.bin_start) {
                                pobj = oi;
                                pstart = g.bin_start;
                                break;
                            }
                        }
                } else {
                    first_rays();
                }
                ERAY_TRACE_WAVE0(12);
                detail(sc, pobj, pstart);
            }
        }
        ERAY_TRACE_POINT(1);
        if (nd < grid) {
            return;
        }
    }

    // ---- background of the non-detail sub-blocks ---------------------------------------------
    if (separate_fill) return;  // fill_kernel writes the background beside this launch
    const uint32_t nf = min(nd < grid ? grid - nd : grid, p.fill_cap ? p.fill_cap : grid);  // filling workgroups
    const uint32_t f = nd < grid ? bid - nd : bid;
    if (f >= nf) return;
    ERAY_TRACE_POINT(2);
    // paced beside detail work — except small scenes whose ring of frames exceeds the Infinity Cache
    // (C2 in 16 slots: 55.7 paced, 51.7 us unpaced per 8 frames; the binned north-star frame in
    // 4 slots 25.1 paced, 29.7 unpaced), profiles/r05/ab/
    const bool pace = nd != 0 && (p.detail_occ || !(p.launch_flags & kLaunchRingBeyondCache));
    fill_frames<kDev>(p, f, nf, wave, lane, aligned, pace);
    ERAY_TRACE_POINT(3);
}

// The background alone, beside a detail-only frame kernel on another stream (FrameParams::
// separate_fill): small workgroups that hold few registers, so the fill waves do not take the
// register budget of the large-mesh detail build.  (A flat order — every output array as one
// byte range, one workgroup per CU, 6.9 TB/s alone at 7680x4320 in scripts/microbench/
// fill_pat.hip — wrote C5's background in 263 us beside the detail kernel against 151 us in
// blocks from two workgroups per CU: profiles/r04/ab/ab_flat_fill.txt, launch spans.)
template <bool kDev>
__global__ void __launch_bounds__(kWG) fill_kernel(FrameParams p) {
    fill_frames<kDev>(p, blockIdx.x, gridDim.x, threadIdx.x >> 6, threadIdx.x & 63, p.aligned != 0, true);
}

// Measurement only (eray_time_write_ceiling): the launch's frames' background bytes written by the
// plainest store stream there is — scripts/microbench/fill_pace.hip's `blk` pattern: one
// workgroup per CU, wave w of the grid's W takes 64 x 4 blocks w, w + W, ... over all the
// launch's frames, each block's 16-B write-through stores at per-lane offsets computed per block,
// no pacing, no role logic, no scene.  The same bytes as the frame kernel's background, into the
// same ring slots, so the frame kernel's fill floor can be compared with the chip's own write
// rate for that ring in the same process.  Whole blocks only (aligned frames, rows % 4 == 0).
__global__ void __launch_bounds__(kWG) ceiling_fill_kernel(FrameParams p) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const uint32_t tiles_x = p.img_w / kBlkW, bands = p.rows / kBlkH, nblk = tiles_x * bands;
    const uint32_t nw = gridDim.x * (kWG / 64), w = blockIdx.x * (kWG / 64) + wave;
    for (uint32_t b = w; b < nblk * p.nframes; b += nw) {
        const uint32_t fr = b / nblk, k = b - fr * nblk, bx = k % tiles_x, by = k / tiles_x;
        const FrameOut o = frame_out(p, fr);
        if (o.rgb) {
#pragma unroll
            for (uint32_t i = lane; i < kBlkH * 48u; i += 64) {
                const uint32_t r = i / 48u, c = i % 48u;
                const float4 v = bg_rgb4(c % 3u);
                stream16_pol<false>(o.rgb, 12u * ((by * kBlkH + r) * p.img_w + bx * kBlkW) + 16u * c, 0u,
                                    make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z),
                                               __float_as_uint(v.w)));
            }
        }
        if (o.ppm && lane < 48u) {
            const uint32_t r = lane / 12u, c = lane % 12u;
            stream16_pol<false>(o.ppm, 3u * ((p.rows - kBlkH - by * kBlkH + r) * p.img_w + bx * kBlkW) + 16u * c, 0u,
                                bg_ppm16(c % 3u));
        }
        if (o.face) {
            const uint32_t r = lane / 16u, c = lane % 16u;
            stream16_pol<false>(o.face, 4u * ((by * kBlkH + r) * p.img_w + bx * kBlkW) + 16u * c, 0u,
                                make_uint4(~0u, ~0u, ~0u, ~0u));
        }
    }
}

// Image<Color>::save_as_ppm body: byte row k = image row h-1-k.
__global__ void __launch_bounds__(256) pack_ppm_kernel(const float* __restrict__ rgb, uint32_t w,
                                                       uint32_t h, uint8_t* __restrict__ out) {
    const size_t n = (size_t)w * h;
    const size_t stride = (size_t)gridDim.x * blockDim.x;
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += stride) {
        const uint32_t y = (uint32_t)(i / w), x = (uint32_t)(i - (size_t)y * w);
        const float* c = rgb + 3 * i;
        uint8_t* o = out + 3 * ((size_t)(h - 1 - y) * w + x);
        o[0] = (uint8_t)sat_u8(c[0] * 255.0f);
        o[1] = (uint8_t)sat_u8(c[1] * 255.0f);
        o[2] = (uint8_t)sat_u8(c[2] * 255.0f);
    }
}

}  // namespace

hipError_t launch_tri_precompute(const float* pos, const float* nrm, const float* uv, uint32_t T,
                                 TriHot* hot, TriShade* shade, hipStream_t s) {
    if (!T) return hipSuccess;
    tri_precompute_kernel<<<(T + 255) / 256, 256, 0, s>>>(pos, nrm, uv, T, hot, shade);
    return hipGetLastError();
}

hipError_t launch_tri_update(const float* pos, const float* nrm, const float* uv, uint32_t T, float* raw_pos,
                             float* raw_nrm, float* raw_uv, TriHot* hot, TriShade* shade, hipStream_t s) {
    if (!T || (!pos && !nrm && !uv)) return hipSuccess;
    tri_update_kernel<<<(T + 255) / 256, 256, 0, s>>>(pos, nrm, uv, T, raw_pos, raw_nrm, raw_uv, hot, shade);
    return hipGetLastError();
}

namespace {
// Persistent grid: as many workgroups as are resident at once (occupancy API), capped by the
// work (fill blocks or detail sub-blocks, whichever needs more workgroups).
// frame_kernel's h_roles (a preloaded dword): grid | detail_wgs << 12 | (frames - 1) << 24 |
// fill_first << 30 | separate_fill << 31 (grid <= kMaxFrameGrid, frames <= kMaxFramesPerLaunch)
constexpr uint32_t kMaxFrameGrid = 4095;
uint32_t frame_roles(uint32_t grid, const FrameParams& q) {
    return (grid & 0xfffu) | ((q.detail_wgs & 0xfffu) << 12) | (((q.nframes - 1u) & 63u) << 24) |
           ((q.fill_first ? 1u : 0u) << 30) |
           ((q.separate_fill ? 1u : 0u) << 31);
}

// frame_kernel's h_band: the band shift and stride of the row mapping in one dword
uint32_t band_word(const FrameParams& q) { return (q.band_shift & 31u) | (q.band_stride << 5); }
// frame_kernel's h_aux: TriShade records (LDS-scene builds) or the detail list
template <bool K>
const void* aux_arg(const FrameParams& q) {
    return K ? static_cast<const void*>(q.shade) : static_cast<const void*>(q.detail_list);
}

uint32_t device_cus() {
    static const uint32_t cus = [] {  // (thread-safe initialisation)
        int dev = 0, n = 0;
        return (hipGetDevice(&dev) == hipSuccess &&
                hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
                   ? (uint32_t)n
                   : 256u;
    }();
    return cus;
}

constexpr uint32_t kFillWgsPerCu = 1;

// A kernel launch, with its dispatch's own start / stop timestamps recorded into t[0] / t[1] when
// they are given (LaunchCtx: measurement only).
template <typename... KArgs, typename... Args>
hipError_t launch_k(void (*kernel)(KArgs...), uint32_t grid, size_t dyn, hipStream_t s, const hipEvent_t (&t)[2],
                    Args... args) {
    if (t[0])
        hipExtLaunchKernelGGL(kernel, dim3(grid), dim3(kWG), (uint32_t)dyn, s, t[0], t[1], 0u, (KArgs)args...);
    else
        kernel<<<grid, kWG, dyn, s>>>(args...);
    return hipGetLastError();
}

template <bool C, bool L, int M, bool K, bool D = false, bool V = false, bool O = false>
hipError_t launch_frame_kernel(const FrameParams& p, uint32_t want, size_t dyn, const LaunchCtx& lc, hipStream_t s) {
    static std::mutex mu;  // resident workgroups per CU of this build, per dynamic LDS size
    static int per_cu = -1;
    static size_t per_cu_dyn = 0;
    int wg_cu;
    {
        std::lock_guard<std::mutex> lock(mu);
        if (per_cu < 0 || per_cu_dyn != dyn) {
            if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, frame_kernel<C, L, M, K, D, V, O>, kWG, dyn) !=
                    hipSuccess ||
                per_cu <= 0)
                per_cu = 1;
            per_cu_dyn = dyn;
        }
        wg_cu = per_cu;
    }
    const uint32_t cus = device_cus();
    const uint32_t grid = min(min(want, (uint32_t)wg_cu * cus), kMaxFrameGrid);
    // Workgroups kept for the fill so that it overlaps a large detail area instead of following
    // it: one per 64 background blocks, at most 1/share of the grid.  Measured (graph-replayed
    // frames, profiles/ab/ab_knobs*.log): the fill needs enough store-issuing waves on every CU
    // (3840x2160 / 70k: 128 fill workgroups 52 us, 256 31 us, none 34 us) and the detail waves'
    // VALU issue; share 2 with the detail roles first is best for C2, C3 and 3840x2160 / 70k
    // (27.8 us; share 3 29.4-30.3, share 4 37), while a small-scene frame with more than one
    // round of detail sub-blocks (the cube at 3840x2160) wants one fill workgroup per CU
    // dispatched first (share 3, fill_first: 22.8 -> 20.4 us; at C2 fill_first costs 0.7 us).
    // blocks and detail sub-blocks of all the launch's frames (frames in flight)
    const uint32_t nblk = p.nframes * p.tiles_x * ((p.rows + kBlkH - 1) / kBlkH);
    const uint32_t total_sub = p.nframes * p.total_sub;
    auto detail_wgs = [&](float share) {
        return share >= 1.0f && grid >= 2 ? grid - max(min((uint32_t)((float)grid / share), (nblk + 63) / 64), 1u)
                                          : 0u;
    };
    FrameParams q = p;
    // (the dense large-mesh build, 4 workgroups per CU: one per CU fills, three do detail work —
    // the fill's store stream no longer needs the issue slots it did, round 5)
    q.detail_wgs = detail_wgs((L && D) ? 4.0f : 2.0f);
    q.fill_first = 0;
    q.detail_wgs_alt = 0;
    if (!L) {
        if (p.cam_state) {  // the count is on the device: frame_kernel picks the share
            q.detail_wgs_alt = detail_wgs(3.0f);
        } else if (total_sub > q.detail_wgs * (kWG / 64)) {
            q.detail_wgs = detail_wgs(3.0f);
            q.fill_first = 1;
        }
    }
    // large meshes: the fill roles take the first-dispatched workgroups — the 2-per-CU build (C3):
    // 13.0 -> 12.7-12.9 us; the dense build (3840x2160 / 70k, spill-free since round 3): 23.4 ->
    // 22.4 us (profiles/r03/ab/)
    if (L) q.fill_first = 1;
    q.separate_fill = 0;
    // Fill workgroups: one per CU writes the background where the fill has the GPU (nearly) to
    // itself — fewer concurrent write streams keep the HBM pages open (scripts/microbench/
    // fill_pat.hip: 3840x2160 beyond the cache 23-24 us with 2-4 per CU, 18.6 us with one; the
    // empty-scene floor 24.5 -> 21.3 us, C2's 37.2 -> 34.0 us per 8 frames) — but not beside
    // the binned meshes' detail waves, which take issue slots from fewer fill waves (3840x2160 /
    // 70k: 22.6 -> 28.2 us with one per CU), same-box A/B (profiles/r04/ab/ab_fill_cap.txt).
    q.fill_cap = L ? 0u : kFillWgsPerCu * cus;
    if constexpr (D) {
        // Separate fill: the dense build does detail work only, at most 2 workgroups per CU, and
        // fill_kernel's small workgroups (58 VGPRs) write the background beside it from a second
        // stream (fork / join by events, which a graph capture records as two parallel nodes).
        // Measured (profiles/ab/ab_sepfill.log): with many rounds of detail sub-blocks the detail
        // waves get the register budget the fill roles held (C5's frame 216 -> 190 us); with
        // ~2 rounds the single launch overlaps better (3840x2160 / 70k 27.9 vs 37.8 us).  Used
        // above 16 detail sub-blocks per CU (ERAY_RENDER_SEPARATE_FILL / _NO_SEPARATE_FILL force
        // it on / off).
        const bool separate = (p.launch_flags & kLaunchSeparateFill)     ? true
                              : (p.launch_flags & kLaunchNoSeparateFill) ? false
                                                                         : total_sub > 16u * cus;
        if (separate) {
            if (!lc.side || !lc.fork || !lc.join) return hipErrorInvalidValue;
            q.separate_fill = 1;
            q.detail_wgs = 0;
            q.fill_first = 0;
            const uint32_t dgrid = max(1u, min(min(grid, 2u * cus), (total_sub + kWG / 64 - 1) / (kWG / 64)));
            // (two per CU: beside the detail waves one per CU writes C5's background in 186 us
            // instead of 151, profiles/r04/ab/ab_fill_cap.txt launch spans)
            const uint32_t fgrid = max(1u, min(2u * cus, (nblk + 3) / 4));
            hipError_t e;
            if ((e = hipEventRecord(lc.fork, s)) != hipSuccess || (e = hipStreamWaitEvent(lc.side, lc.fork, 0)) != hipSuccess)
                return e;
            if ((e = launch_k(frame_kernel<C, L, M, K, D, V, O>, dgrid, dyn, s, lc.frame_t, q.objects, q.lights, q.cull,
                              q.tris, aux_arg<K>(q), q.nobj | (q.nlights << 16), q.total_tris, q.total_sub,
                              frame_roles(dgrid, q), band_word(q), q)) != hipSuccess)
                return e;
            if ((e = launch_k(fill_kernel<V>, fgrid, 0, lc.side, lc.fill_t, q)) != hipSuccess) return e;
            if (lc.fill_used) *lc.fill_used = 1u;
            if ((e = hipEventRecord(lc.join, lc.side)) != hipSuccess) return e;
            return hipStreamWaitEvent(s, lc.join, 0);
        }
    }
    return launch_k(frame_kernel<C, L, M, K, D, V, O>, grid, dyn, s, lc.frame_t, q.objects, q.lights, q.cull, q.tris,
                    aux_arg<K>(q), q.nobj | (q.nlights << 16), q.total_tris, q.total_sub, frame_roles(grid, q), band_word(q),
                    q);
}

template <bool C, int M, bool V>
hipError_t launch_frame_cs(const FrameParams& p, uint32_t want, const LaunchCtx& lc, hipStream_t s) {
    // small scenes are preloaded into LDS whole (no object then needs the LDS tiles); otherwise
    // everything is read from the device arrays
    if (p.lds_scene) {
        const size_t dyn = scene_lds_layout(p.nobj, p.nlights, p.total_tris, C).bytes;
        // one object (main.rs's own scene shape): the single-object path (culled builds; the
        // brute-force diagnostic keeps the general code) — C2 8 frames 39.6 -> 37.0 us per launch,
        // one frame alone 9.35 -> 8.62 us; not into a ring beyond the Infinity Cache, where the
        // unpaced fill bounds the launch and the shorter detail chains beside it measured 0.6 us
        // slower (C2 in 16 slots 50.3 -> 50.9 us), same-box A/B profiles/r07/ab/
        if constexpr (C) {
            if (p.nobj == 1 && !(p.launch_flags & kLaunchRingBeyondCache))
                return launch_frame_kernel<C, false, M, true, false, V, true>(p, want, dyn, lc, s);
        }
        return launch_frame_kernel<C, false, M, true, false, V>(p, want, dyn, lc, s);
    }
    if (p.max_object_tris > kDirectMax) {
        if constexpr (!(M & kMatSpecPow)) {
            // more detail sub-blocks than the 2-per-CU grid's detail waves (half the grid, four
            // waves each: launch_frame_kernel) take in one round: the 3-per-CU build
            // (ERAY_RENDER_DENSE_DETAIL / _NO_DENSE_DETAIL force it on / off)
            const bool dense = (p.launch_flags & kLaunchDense)     ? true
                               : (p.launch_flags & kLaunchNoDense) ? false
                                                                   : p.nframes * p.total_sub > device_cus() * (kWG / 64);
            if (dense) return launch_frame_kernel<C, true, M, false, true, V>(p, want, 0, lc, s);
        }
        return launch_frame_kernel<C, true, M, false, false, V>(p, want, 0, lc, s);
    }
    return launch_frame_kernel<C, false, M, false, false, V>(p, want, 0, lc, s);
}

// The build for the scene's material features (kMat*), culled or not (C), with the camera in the
// kernel arguments or in the setup's CamState (V).
template <bool C, bool V>
hipError_t launch_frame_mat(int mat, const FrameParams& p, uint32_t want, const LaunchCtx& lc, hipStream_t s) {
    switch (mat) {
        case 0: return launch_frame_cs<C, 0, V>(p, want, lc, s);
        case kMatSpecPow: return launch_frame_cs<C, kMatSpecPow, V>(p, want, lc, s);
        case kMatExample: return launch_frame_cs<C, kMatExample, V>(p, want, lc, s);
        default: return launch_frame_cs<C, kMatSpecPow | kMatExample, V>(p, want, lc, s);
    }
}
}  // namespace

hipError_t launch_render(const FrameParams& p_in, const LaunchCtx& lc, hipStream_t s) {
    FrameParams p = p_in;
    if (p.nframes < 1 || p.nframes > kMaxFramesPerLaunch || ((p.aa || p.bounces) && p.nframes != 1))
        return hipErrorInvalidValue;
    {  // the launch's output bytes against the Infinity Cache (FrameParams::store_nt)
        const uint64_t px = (uint64_t)p.nframes * p.rows * p.img_w;
        const uint64_t out = px * ((p.out_rgb ? 12u : 0u) + (p.out_ppm ? 3u : 0u) + (p.out_face ? 4u : 0u));
        p.store_nt = out > kInfinityCacheBytes ? 1u : 0u;
    }
    if (p.aa || p.bounces) return launch_trace(p, lc, s);
    const uint32_t by_n = (p.rows + kBlkH - 1) / kBlkH;
    const uint32_t nblk = p.tiles_x * by_n;
    if (!nblk) return hipSuccess;
    // enough workgroups for one fill block or one round of detail sub-blocks per wave (device-
    // camera mode: the detail count is not known here, so as many as fit)
    const uint32_t want = p.nframes * (p.cam_state ? max((nblk + 3) / 4, nblk) : max((nblk + 3) / 4, (p.total_sub + 3) / 4));
    const int mat = (p.spec_pow ? kMatSpecPow : 0) | (p.example_mat ? kMatExample : 0);
    // device-camera mode (the setup's CamState) is a separate build: args-mode frames carry no
    // branch or load for it
    if (p.cull && p.cam_state) return launch_frame_mat<true, true>(mat, p, want, lc, s);
    if (p.cull) return launch_frame_mat<true, false>(mat, p, want, lc, s);
    return launch_frame_mat<false, false>(mat, p, want, lc, s);
}

hipError_t launch_write_ceiling(const FrameParams& p, uint32_t wgs_per_cu, const hipEvent_t (&t)[2], hipStream_t s) {
    if (!p.aligned || p.img_w % kBlkW || p.rows % kBlkH || p.nframes < 1 || !wgs_per_cu || wgs_per_cu > 8)
        return hipErrorInvalidValue;
    return launch_k(ceiling_fill_kernel, wgs_per_cu * device_cus(), 0, s, t, p);
}

hipError_t launch_pack_ppm(const float* rgb, uint32_t w, uint32_t h, uint8_t* out, hipStream_t s) {
    const size_t n = (size_t)w * h;
    if (!n) return hipSuccess;
    size_t blocks = (n + 255) / 256;
    if (blocks > 2048) blocks = 2048;
    pack_ppm_kernel<<<(unsigned)blocks, 256, 0, s>>>(rgb, w, h, out);
    return hipGetLastError();
}

}  // namespace gpu
}  // namespace eray
