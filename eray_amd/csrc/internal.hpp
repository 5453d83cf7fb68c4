// internal.hpp — records, constants and launchers shared by the C-ABI layer (capi*.cpp) and the
// gfx950 kernels.  What the host decides without the GPU lives in HIP-free headers included here:
// the descriptors and their build (scene_build.hpp), the texel programs (texel_prog.hpp), the
// frame launch's arguments (frame_params.hpp), the bins' sizing (bin_layout.hpp).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <array>
#include <vector>

// (these two before accel_walk.hpp: they bring in glibc_cosf.hpp, whose ERAY_HD is for its own
// functions; the headers after this one that use ERAY_HD mean accel_walk.hpp's, as before)
#include "scene_build.hpp"
#include "texel_prog.hpp"

#include "accel_walk.hpp"
#include "band_rows.hpp"
#include "bin_layout.hpp"
#include "frame_params.hpp"

namespace eray {
namespace gpu {

// Hot per-triangle record of the exact test, 48 B (three 16-B loads), computed on the device
// from the face vertices with the reference's own operations (primitives.rs:44-46):
//   q0 = (e1.x, e1.y, e1.z, e2.x)   q1 = (e2.y, e2.z, n.x, n.y)   q2 = (n.z, a.x, a.y, a.z)
struct __align__(16) TriHot {
    float4 q0, q1, q2;
};

// Cold per-triangle shading record, 64 B, read only for the hit face:
//   s0 = (na.x, na.y, na.z, nb.x)  s1 = (nb.y, nb.z, nc.x, nc.y)
//   s2 = (nc.z, uva.u, uva.v, uvb.u)  s3 = (uvb.v, uvc.u, uvc.v, 0)
struct __align__(16) TriShade {
    float4 s0, s1, s2, s3;
};

// Camera-dependent culling record of a triangle for primary rays (see render.hip,
// "exact wave culling").  For each of the four conditions k in {u, v, w, n}:
//   f_k(x', y') = K_k + A_k x' + B_k y'   (a real-valued bound of the reference's test value
//   along the camera ray through viewport coordinate (x', y')), rejected for a whole pixel
//   rectangle when max f_k < -T_k.
struct __align__(16) TriCull {
    float4 A;  // A_u, A_v, A_w, A_n
    float4 B;
    float4 K;
    float4 T;  // thresholds (>= 0; +inf disables the condition)
};

// (TexelInstr and the texel programs' constants: texel_prog.hpp.  TexView, MaterialDesc, ObjGeom,
// ObjectDesc and LightDesc, the descriptors the host builds: scene_build.hpp.)

// Scenes up to these sizes are preloaded whole into each frame workgroup's LDS.
constexpr uint32_t kCacheTris = 256, kCacheObjects = 16, kCacheLights = 16;
// (kDirectMax, the largest object scanned per wave: frame_params.hpp.)
// (Screen bins of large objects' faces, kBinW x kBinH pixels: bin_layout.hpp.)
// Bins of 65 to this many entries are sorted by face index (bins.hip bin_sort_kernel); longer
// ones keep the scatter's order.  In a sorted bin each full 64-entry chunk but the last also
// carries, in the pad words of its first two entries (low, high half), the union of the pixel
// masks of every later chunk: the frame kernel stops the bin once no pixel that can still improve
// is covered by what is left (frame_first_hit.hpp first_hit_binned_wave).
constexpr uint32_t kBinSortMax = 1024;
// The frame kernel reads triangle records (TriHot 48 B, TriShade 64 B) and bin entries (64 B) by
// buffer loads with 32-bit byte offsets (frame_scene.hpp load_rec): a scene holds fewer than 2^26
// triangles (eray_scene_add_object refuses more) and a bin buffer at most 2^26 entries (a setup
// that needs more overflows: its objects are scanned through LDS tiles, still exact).
constexpr uint64_t kMaxSceneTris = (1ull << 26) - 1;
constexpr size_t kMaxBinEntries = (size_t)1 << 26;
// The multi-GPU gathers (comm.cpp) serve at most 64 ranks (gather_plan.hpp), and every buffer a rank
// needs to take part in their status exchanges (status and count words, the plan records, the
// plan's rank table) lives in a scratch block allocated with the context — so no rank can fail to
// enter a collective its peers have entered for want of memory.
constexpr size_t kCollScratchBytes = 32u << 10;

// One entry of a screen bin (bins.hip): a face that may be hit in the bin, its intersection
// record, the bin's pixels it may cover (bit row * kBinW + column) and its index relative to the
// object's first face — one 64-B line, so the scatter that places an entry in its bin writes one
// line and a detail wave reads a 64-entry chunk as 4 KB of consecutive lines.
struct alignas(16) BinEntry {
    TriHot hot;
    unsigned long long mask;
    uint32_t tri;
    uint32_t pad;  // sorted bins: half of the later chunks' mask union (kBinSortMax), else 0
};
static_assert(sizeof(BinEntry) == 64, "one 64-B line per bin entry");

// A camera as the kernels use it (camera.rs:57-76): centre, Fov ratio fov0 / fov1 (computed on
// the host in f32, as Fov::ratio does) and z_dist.  Camera::size is fixed per frame plan.
struct CamDev {
    float cx, cy, cz, ratio, z_dist;
    uint32_t pad[3];
};

// Per-camera frame setup in device memory, written by the setup kernels (setup.hip, bins.hip)
// and read by the frame kernel in device-camera mode (FrameParams::cam_state): no host round
// trip between a camera change and its frame.
struct alignas(16) CamState {
    CamDev cam;                   // the camera of the setup (copied by the setup kernel)
    uint32_t nrect;               // detail rectangles (sub-block units, rank-local rows, disjoint)
    uint32_t total_sub;           // detail sub-blocks (rectangles' area, or the detail list's length)
    uint32_t bin_entries;         // (face, bin) entries the bins needed (host capacity sizing)
    uint32_t bin_overflow;        // the bins did not fit: binned objects fall back to LDS tiles
    // a split detail list (FrameParams::dlist_split, camera paths): heavy sub-blocks appended from
    // the front, light ones from the back (bins.hip detail_list_kernel)
    uint32_t heavy_sub, light_sub;
    int32_t rects[kMaxRects][4];  // x0, x1, y0, y1 (inclusive)
};

// general tracer: a binned sub-block whose bin holds more entries is searched by a whole
// workgroup (trace.hip; the tracer's setup lists those first, bins.hip detail_flags_kernel)
constexpr uint32_t kTraceHeavyMin = 192;

// (FrameParams, the frame launch's argument record: frame_params.hpp.)

// Byte offsets of the LDS scene copy: [ObjectDesc x nobj | LightDesc x nl | TriCull x n (if
// culling) | TriHot x n | TriShade x n]; every section is a whole number of 16-B words.
struct SceneLdsLayout {
    uint32_t objs, lights, cull, hot, shade, bytes;
};
__host__ __device__ inline SceneLdsLayout scene_lds_layout(uint32_t nobj, uint32_t nl, uint32_t n, bool cull) {
    SceneLdsLayout L;
    L.objs = 0;
    L.lights = L.objs + nobj * (uint32_t)sizeof(ObjectDesc);
    L.cull = L.lights + nl * (uint32_t)sizeof(LightDesc);
    L.hot = L.cull + (cull ? n * (uint32_t)sizeof(TriCull) : 0u);
    L.shade = L.hot + n * (uint32_t)sizeof(TriHot);
    L.bytes = L.shade + n * (uint32_t)sizeof(TriShade);
    return L;
}
// (whole 16-B words: scene_build.hpp asserts ObjectDesc's and LightDesc's sizes)

// ------------------------------------------------------------- launchers (.hip files) ------
hipError_t launch_tri_precompute(const float* pos, const float* nrm, const float* uv, uint32_t T,
                                 TriHot* hot, TriShade* shade, hipStream_t s);
// eray_scene_update_object: the same records for one object's T faces from the caller's arrays
// (device; null: kept), written to the object's slices hot / shade, the given arrays stored into the
// object's slices raw_* of the resident raw array in the same pass (render.hip tri_update_kernel).
hipError_t launch_tri_update(const float* pos, const float* nrm, const float* uv, uint32_t T, float* raw_pos,
                             float* raw_nrm, float* raw_uv, TriHot* hot, TriShade* shade, hipStream_t s);
// ------------------------------------------------------------- per-camera setup (setup.hip)
// Everything a camera change needs before its frame, enqueued on the stream with no host round
// trip (so a camera path can be graph-replayed): per triangle the culling record (TriCull) and
// its conservative pixel rectangle, per object the union of those (ObjGeom::rect, written into
// the device descriptors), for binned objects each face's bin rectangle (bins.hip), and, for
// scenes without binned objects, the merged detail rectangles of the rendered rows (CamState).
// camera_setup_kernel's grid: at most this many workgroups, each a contiguous chunk of triangles —
// the workgroups resident at once on MI355X (its chunk pass holds 131 VGPRs and 36.9 KB of LDS:
// 3 per CU x 256 CUs), so a multi-camera setup runs in one round, not 1.33 (1024: a tail round of
// 256 workgroups; same-box A/B profiles/r06/ab/ab_r06q_setup_grid.txt: moving 3840x2160 / 70k
// 46.2 -> 44.7 us, moving 1M faces 268.6 -> 255.5 us per frame)
constexpr uint32_t kSetupMaxBlocks = 768;
// camera_setup_kernel's chunk workgroups for T triangles (each a contiguous chunk of
// ceil(T / blocks) faces)
inline uint32_t setup_blocks(uint32_t T) {
    const uint32_t b = (T + 255u) / 256u;
    return T ? (b < kSetupMaxBlocks ? b : kSetupMaxBlocks) : 1u;
}
// The setup's accumulator words (SetupParams::done / part / acc point into one array): [done
// counter | kSetupMaxBlocks x 10 partials | 4 x nobj rectangle accumulators].  The counter and the
// accumulators are zero between setups whatever the object count (partials are rewritten).
constexpr size_t kSetupAccPart = 1, kSetupAccRects = kSetupAccPart + 10 * (size_t)kSetupMaxBlocks;
inline size_t setup_acc_words(size_t nobj) { return kSetupAccRects + 4 * nobj; }
struct SetupParams {
    const TriHot* hot;
    TriCull* cull;
    uint32_t T;                 // all triangles of the scene
    ObjectDesc* objs;           // device descriptors (rect written)
    uint32_t nobj;
    const uint32_t* obj_begin;  // nobj + 1: first triangle of each object, then T
    const uint32_t* objkey;     // nobj: the object's binned-object index, or ~0u
    const CamDev* cam;          // the camera to set up (device)
    CamState* state;
    uint32_t W, H;              // Camera::size
    uint32_t row0, rows;        // rendered camera rows (the merged rectangles are rank-local)
    uint32_t band_shift, band_mask, band_stride;  // interleaved bands (FrameParams)
    uint32_t* acc;              // 4 x nobj rectangle accumulators, zero between setups
    uint32_t* done;             // workgroup counter (last-workgroup finalisation), zero between setups
    uint32_t* part;             // kSetupMaxBlocks x 10: each workgroup's boundary objects' partials
    uint32_t binned;            // some object is binned: bins.hip narrows rects + builds the detail list
    // binned objects' faces (bins.hip): bin rectangle and its number of units per face (bin_segments:
    // rows of the rectangle, else its bins; zero for other faces), the binned-object index per face
    int4* range;
    unsigned long long* area;
    uint32_t* fkey;
    uint32_t bins_x, phase;
    // the general tracer's setup (trace.hip): culling records and rectangles over the viewport
    // its jittered anti-aliasing rays reach, bin masks of the pixels any of whose rays may pass
    // (face_rect.hpp bin_pixels_jittered)
    uint32_t keep_all;
    uint32_t rect_pairs;  // (diagnostics) the rectangle-pair form where segments apply (bin_segments)
    // Several cameras in one setup (ncam > 1: camera paths of scenes with binned objects): the
    // cameras sp.cam[0 .. ncam), T = ncam * T1 "faces" (face i is face i % T1 of camera i / T1:
    // its culling record, bin rectangle and pairs), nobj = ncam * nobj1 descriptors (camera k's
    // copy of object o at k * nobj1 + o), ncam * nb1 binned objects (camera k's copy of binned
    // object j is k * nb1 + j), ncam CamStates; the bins and their detail lists per camera.
    uint32_t ncam, T1, nobj1, nb1;
    const ObjectDesc* objs_src;  // batched setups: the scene's descriptors, copied into each slot
    // binned faces' first unit: the exclusive scan of `area`, as each chunk workgroup's own scan
    // (first_local) plus its chunk's offset boff[b] (kSetupMaxBlocks + 1 entries; boff[nparts] =
    // all units) — bins.hip bin_segments_kernel / bin_pairs_kernel read them
    unsigned long long* first_local;
    unsigned long long* boff;
    // Camera paths (eray_gather_frames' layout of path frames): every camera's final object
    // rectangles also fold into this union (object o % union_nobj: x0, y0 minimised at
    // path_union[2 o ..], x1, y1 maximised at path_union[2 union_nobj + 2 o ..]), or null
    int32_t* path_union;
    uint32_t union_nobj;
};
hipError_t launch_camera_setup(const SetupParams& sp, hipStream_t s);
// The units the setup enumerates per binned face (`area`, and the scan first_local / boff over
// them): its bin rectangle's rows (bins.hip bin_segments_kernel) for the frame kernel's bins, its
// (face, bin) pairs for the general tracer's (bin_pairs_kernel) and for frames wider than the
// segments' 16-bit columns.
__host__ __device__ inline bool bin_segments(const SetupParams& sp) {
    return !sp.keep_all && !sp.rect_pairs && sp.W <= 65535u;
}
// The setups of `ncam` cameras sp.cam[0 .. ncam) at once, one workgroup each, into per-camera
// slots: culling records sp.cull + k * T, descriptors sp.objs + k * nobj (sp.objs_src with the
// camera's rectangles), state sp.state + k.  Scenes without binned objects and at most
// kSetupBatchMaxObjects objects (every object's union stays in the workgroup's LDS).
constexpr uint32_t kSetupBatchMaxObjects = 256;
hipError_t launch_camera_setup_batch(const SetupParams& sp, uint32_t ncam, hipStream_t s);
// A camera path's rectangle union (SetupParams::path_union, 4 nobj words) copied to `host` (mapped
// pinned memory, read by the host after the stream passes this point) and reset for the next
// path: x0, y0 to INT_MAX, x1, y1 to INT_MIN.  host null: the reset alone.
hipError_t launch_union_flush(int32_t* acc, uint32_t nobj, int32_t* host, hipStream_t s);
// Folds an object's final pixel rectangle r (x0, x1, y0, y1; skipped when empty) into the union.
__device__ __forceinline__ void union_rect(int32_t* u, uint32_t nobj, uint32_t o, const int32_t* r) {
    if (r[0] > r[1] || r[2] > r[3]) return;
    atomicMin(u + 2 * o, r[0]);
    atomicMin(u + 2 * o + 1, r[2]);
    atomicMax(u + 2 * nobj + 2 * o, r[1]);
    atomicMax(u + 2 * nobj + 2 * o + 1, r[3]);
}
// Writes `cam` into the device camera slot (kernel arguments: no host staging buffer to race).
hipError_t launch_set_camera(const CamDev& cam, CamDev* slot, hipStream_t s);
// The ray-query hierarchy of the scene (accel_walk.hpp; built by eray_scene_build_ray_accel): per
// object a record (has == 0: the object keeps the LDS tiles), the nodes, and the leaf-ordered byte
// copies of the face records with their original indices.  objs null: no hierarchy.
struct RayAccelView {
    const accel::Object* objs;
    const accel::Node* nodes;
    const TriHot* hot;
    const uint32_t* index;
};
// Per-context launch resources: the separate fill kernel's stream and its fork / join events.
// Measurement (eray_time_frames_ring): when frame_t[0] is set, the frame kernel is launched with
// hipExtLaunchKernel's start / stop events, which take the dispatch's own begin / end timestamps
// (the figures rocprofv3's kernel trace reports); fill_t likewise for the separate fill kernel.
struct LaunchCtx {
    hipStream_t side;
    hipEvent_t fork, join;
    hipEvent_t frame_t[2] = {nullptr, nullptr};
    hipEvent_t fill_t[2] = {nullptr, nullptr};
    uint32_t* fill_used = nullptr;  // set to 1 when the launch ran the separate fill kernel
    // the general tracer's face finder for shadow and reflected rays (trace.hip): the scene's valid
    // hierarchy when the call's render takes it (capi_frames.cpp prepare_render sets it per call),
    // objs null: the per-lane scan.  Not in FrameParams: the frame kernel's argument layout stays.
    RayAccelView accel{nullptr, nullptr, nullptr, nullptr};
};
// The frame kernel, or the general tracer (trace.hip) when p.aa or p.bounces is set (with
// lc.accel's hierarchy, when it has one).
hipError_t launch_render(const FrameParams& p, const LaunchCtx& lc, hipStream_t s);
hipError_t launch_trace(const FrameParams& p, const LaunchCtx& lc, hipStream_t s);
// Measurement (eray_time_write_ceiling): the frames' background bytes as one plain block-strided
// write stream of wgs_per_cu workgroups per CU (render.hip ceiling_fill_kernel), timed by t.
hipError_t launch_write_ceiling(const FrameParams& p, uint32_t wgs_per_cu, const hipEvent_t (&t)[2], hipStream_t s);
hipError_t launch_trace_cull(const FrameParams& p, hipStream_t s);

// ------------------------------------------------------------- ray queries (rays.hip)
// eray_cast_rays: a batch of caller-supplied rays against the scene.  `f` carries what cast_ray
// reads of a frame (camera centre, triangle records, descriptors, lights, bounces), the rest zero.
struct RayIn {  // eray_ray
    float start[3], dir[3];
};
constexpr uint32_t kRayTile = 256;  // faces per LDS tile of the batch search (TriHot: 12 KB)
struct RayBatch {
    FrameParams f;
    const RayIn* rays;
    uint64_t count;
    int32_t object;      // -1: every object, the closest by the camera's centre; k: object k alone
    uint32_t normalize;  // dir goes through Ray::new
    uint32_t brute;      // per-lane first_face, no tiles (ERAY_RAYS_BRUTE_FORCE)
    uint4* out_hit;      // count x 3 words of 16 B (eray_ray_hit), or null
    float* out_rgb;      // count x 3, or null
};
// (RayAccelView, the hierarchy as the kernels take it: above, before LaunchCtx.)
hipError_t launch_cast_rays(const RayBatch& b, const RayAccelView& a, hipStream_t s);
// eray_rays_reach_light: Engine::reaches_light per caller-supplied shadow ray.  `f` carries the
// triangle records, the descriptors and the object count, the rest zero.
struct ReachBatch {
    FrameParams f;
    const RayIn* rays;
    const float* targets;  // count x 3: the light's position of each ray
    uint64_t count;
    uint32_t normalize;  // dir goes through Ray::new
    uint32_t brute;      // per-lane first_face, no tiles, no hierarchy (ERAY_RAYS_BRUTE_FORCE)
    uint32_t* out;       // count words: 1 reaches, 0 blocked
};
hipError_t launch_reach_light(const ReachBatch& b, const RayAccelView& a, hipStream_t s);

hipError_t launch_pack_ppm(const float* rgb, uint32_t w, uint32_t h, uint8_t* out, hipStream_t s);

// ----------------------------------------------------------------- frame sources (the gather's)
// Where a frame in an output buffer came from (eray_gather_frames' scene-camera transport): the
// context tags every PPM output slot it renders into with the render's kind and key.  kind
// kSrcScene: a frame kernel render of the scene camera, key = a hash of (camera, scene
// generation, Camera::size) — the same on every rank that made the same scene calls, whatever
// internal re-setups (bin capacity growth) a rank did; kSrcPath: a frame of a camera path, key =
// the context's path call counter; kSrcOther: anti-aliasing / bounces / brute force.
constexpr uint32_t kSrcNone = 0, kSrcScene = 1, kSrcPath = 2, kSrcOther = 3;
struct FrameSource {
    uint32_t kind = kSrcNone;
    uint64_t key = 0;
    uint32_t W = 0, H = 0;
    uint32_t row0 = 0, rows = 0, band_shift = 0, band_stride = 0;  // the rendered rows
};
// The pixel rectangles of a source (every object's ObjGeom::rect: x0, x1, y0, y1 inclusive, camera
// rows; empty when x0 > x1; for a camera path the union over its cameras) — outside them every
// frame of the source is the background colour.
struct SceneLayout {
    FrameSource src;
    std::vector<std::array<int32_t, 4>> rects;
};

hipError_t launch_wave(uint32_t w, uint32_t h, float xf, float yf, float* out, hipStream_t s);
hipError_t launch_rgb(uint32_t w, uint32_t h, const float* r, const float* g, const float* b,
                      float* out, hipStream_t s);
hipError_t launch_flat(uint32_t w, uint32_t h, float r, float g, float b, float* out,
                       hipStream_t s);
hipError_t launch_mix(uint32_t w, uint32_t h, TexView left, TexView right, float factor,
                      float* out, hipStream_t s);
hipError_t launch_material_example(uint32_t w, uint32_t h, float xf, float yf, float r, float g,
                                   float b, float factor, float* color, float* diffuse,
                                   hipStream_t s);

}  // namespace gpu
}  // namespace eray
