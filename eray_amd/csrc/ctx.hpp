// ctx.hpp — the context behind include/eray_hip.h's eray_ctx handle and what the C-ABI translation
// units share to work on it: capi.cpp (context, memory, shaderlib nodes), capi_scene.cpp (the scene
// calls and the scene's upload), capi_debug.cpp (the eray_debug_* hooks of the bins and the setup),
// capi_setup.cpp (camera setup, bins, frame tags), capi_frames.cpp (the frame entry points),
// capi_rays.cpp (ray queries and their hierarchy) and comm.cpp (the multi-GPU gather).
// Here: the error policy (set_error, HIP_TRY, use_device), the scene upload, and what the other
// units need of capi_setup.cpp — declared here and nowhere else.  Private to those seven files; the
// HIP-free units report errors without it (objload.cpp through capi.cpp's eray_internal_error).
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <memory>
#include <string>
#include <vector>

#include "../../include/eray_hip.h"
#include "bins.hpp"
#include "frame_plan.hpp"
#include "internal.hpp"
#include "owners.hpp"

namespace eray {
namespace gpu {

constexpr uint32_t kUnionRing = 4;  // camera paths whose rectangle unions the host keeps

// (HostObject, an object of the host scene: scene_build.hpp.)

// eray_gather_frames' plan: comm.cpp defines it, and how it is deleted.
struct GatherPlan;
struct GatherPlanDelete { void operator()(GatherPlan* P) const; };

}  // namespace gpu
}  // namespace eray

using namespace eray::gpu;  // (the C-ABI translation units work in it throughout)

struct eray_ctx {
    int device = 0;
    Stream own_stream;
    hipStream_t stream = nullptr;  // own_stream, or the caller's (eray_set_stream)
    std::string err;

    eray_camera camera{{0.0f, 0.0f, 0.0f}, {60.0f, 60.0f}, 1024u, 1.0f};  // Camera::default()
    std::vector<eray_light> lights;
    std::vector<HostObject> objects;

    bool geom_dirty = true, desc_dirty = true;
    uint64_t scene_gen = 0;  // bumped whenever geometry or descriptors are uploaded
    DeviceBuf<TriHot> d_hot;
    DeviceBuf<TriShade> d_shade;
    DeviceBuf<TriCull> d_cull;
    DeviceBuf<TriCull> d_tcull;  // kTraceSkipTris records: trace.hip's background skip
    DeviceBuf<float> d_raw;
    DeviceBuf<ObjectDesc> d_objs;
    DeviceBuf<LightDesc> d_lights;
    RayAccel ray_accel;  // eray_scene_build_ray_accel's hierarchy; invalid after any geometry change
    // launch plans of eray_render_frames / eray_render_camera_path: HIP graphs of back-to-back
    // frames (chunks of up to kGraphFrames frames and remainders), each cached for the frame
    // parameters + stream + length + kind it was captured with; the least recently used is
    // evicted beyond kGraphCache
    std::vector<FrameGraph> graphs;
    uint64_t graph_clock = 0;
    DeviceBuf<uint32_t> d_prog;  // every object's texel program (MaterialDesc::prog), concatenated
    std::vector<uint32_t> h_prog;
    SceneDescs descs;  // the descriptors as uploaded (scene_build.hpp; kept alive for the async uploads)
    std::vector<float> h_raw;
    uint32_t total_tris = 0;
    // ---- per-camera setup (setup.hip, bins.hip), all on the device
    DeviceBuf<CamDev> d_cam;      // the context camera's device slot
    DeviceBuf<CamState> d_state;  // the last setup's results
    PinnedBuf<CamState> h_state;  // host copy, valid once state_ev has completed
    Event state_ev;
    bool state_pending = false;   // a copy into h_state is in flight
    bool state_known = false;     // h_state holds the results of the setup of setup_key
    std::vector<uint64_t> setup_key;  // camera, size, rows and scene generation of the last setup
    std::vector<uint64_t> tcull_key;  // camera, size, scene generation and stream of d_tcull's records
    FrameSource setup_src;        // the last enqueued scene-camera setup: its source key and rows
    PinnedBuf<ObjectDesc> h_objs_state;  // the descriptors after that setup (pixel rectangles)
    // where the frames in output buffers came from (eray_gather_frames): PPM slot address -> the
    // source of the last render enqueued into it, most recent last (at most kMaxTags)
    struct SlotTag {
        uintptr_t ppm;
        FrameSource src;
    };
    std::vector<SlotTag> slot_tags;
    // camera paths: call counter (kSrcPath keys) and the union of every path camera's object
    // rectangles — accumulated on the device (d_union_acc, captured into path graphs), then copied
    // into ring entry seq % kUnionRing on the device and the host, with an event per entry
    uint64_t path_seq = 0;
    DeviceBuf<int32_t> d_union_acc;
    size_t union_cap() const { return d_union_acc.cap / 4; }  // objects per entry
    PinnedBuf<int32_t> h_union;  // mapped: the flush kernel writes it through h_union.dev
    uint64_t union_seq[kUnionRing] = {};
    FrameSource union_src[kUnionRing];
    uint32_t union_nobj[kUnionRing] = {};  // objects and scene generation the entry's union covers
    uint64_t union_gen[kUnionRing] = {};
    Event union_ev[kUnionRing];
    // eray_gather_frames' plan (comm.cpp makes it on the first scene-camera gather)
    std::unique_ptr<GatherPlan, GatherPlanDelete> gather_plan;
    DeviceBuf<uint32_t> d_acc;    // setup counter, partials and rectangle accumulators (enqueue_setup)
    DeviceBuf<uint32_t> d_begin;  // obj_begin | objkey
    DeviceBuf<int4> d_range;      // binned faces' bin rectangles, areas, binned-object index
    DeviceBuf<unsigned long long> d_area;
    DeviceBuf<uint32_t> d_fkey;
    BinBuffers bins;              // the scene camera's screen bins (bins.hpp; ensure_bins allocates)
    std::vector<uint64_t> bins_layout;
    uint64_t bins_gen = 0;        // bumped whenever bins_alloc (re)allocates the bin buffers
    size_t bin_cap = 0;           // entry capacity to allocate (grown when a setup overflows)
    bool rect_pairs = false;      // (diagnostics) setups walk the bin rectangles' pairs (bins.hip)
    // camera paths (eray_render_camera_path): the cameras of the current graph chunk on the
    // device, the whole path staged in pinned memory
    DeviceBuf<CamDev> d_path;
    DeviceBuf<CamDev> d_path_all;
    // two pinned staging buffers used in turn: a call waits only for the upload two calls back
    // (not for the previous call's frames, which its upload is queued behind)
    PinnedBuf<CamDev> h_path[2];
    Event path_ev[2];  // each buffer's last upload (reusable once complete)
    uint32_t path_buf = 0;
    // batched setups of a path chunk's cameras (scenes without binned objects): per camera slot
    // its culling records, object descriptors and setup state
    DeviceBuf<TriCull> d_bcull;
    DeviceBuf<ObjectDesc> d_bobjs;
    DeviceBuf<CamState> d_bstate;
    // camera paths of scenes with binned objects: the setups of up to mc_k cameras in one
    // multi-camera build (SetupParams::ncam), into per-camera slices of a buffer set; two sets, so
    // that the next cameras' build (on mc_stream) runs beside the current cameras' frames
    struct MultiSet {
        DeviceBuf<TriCull> cull;
        DeviceBuf<ObjectDesc> objs;
        DeviceBuf<CamState> state;
        DeviceBuf<uint32_t> acc;
        DeviceBuf<int4> range;
        DeviceBuf<unsigned long long> area;
        DeviceBuf<uint32_t> fkey;
        BinBuffers bins;
    };
    MultiSet mc[2];
    uint32_t mc_k = 0;
    std::vector<uint64_t> mc_layout;
    uint64_t mc_gen = 0;          // bumped whenever the multi-camera buffers are (re)allocated
    Stream mc_stream;
    Event mc_fork, mc_ready[2], mc_free[2];
    // the latest render of the scene camera or of a camera path (tag_frames): what a scene-camera
    // gather plans for — state every rank holds alike when the ranks make the same render calls
    FrameSource gather_src;
    DeviceBuf<uint8_t> d_coll;     // kCollScratchBytes: the gathers' status exchanges (comm.cpp)
    DeviceBuf<uint8_t> d_staging;  // eray_gather_rows' banded staging (rank 0)
    // the separate fill's stream and events, and the launchers' view of them
    Stream fill_stream;
    Event fill_fork, fill_join;
    LaunchCtx lc{nullptr, nullptr, nullptr};
    // objects the last general-tracer render searched through the hierarchy (prepare_render sets it
    // when it chooses lc.accel; 0: the per-lane scan) — eray_debug_trace_ray_accel
    uint32_t trace_accel_objects = 0;
    Event update_join;  // eray_scene_update_object: the other streams' work so far, waited for by `stream`

    // Waits for the context's streams, then releases what the members do not own themselves.
    // Every member that owns device memory enqueued work may still use is released after this
    // body: the streams are synchronised here first.
    ~eray_ctx() {
        (void)hipSetDevice(device);
        for (hipStream_t s : {stream, (hipStream_t)own_stream, (hipStream_t)mc_stream})
            if (s) (void)hipStreamSynchronize(s);
        gather_plan.reset();  // (while the streams exist)
    }
};

namespace eray {
namespace gpu {

// The ray-query hierarchy as the kernels take it: none unless it is valid (never a stale tree: every
// geometry change clears `valid`).
inline RayAccelView accel_view(const eray_ctx* ctx) {
    const RayAccel& ra = ctx->ray_accel;
    if (!ra.valid) return RayAccelView{nullptr, nullptr, nullptr, nullptr};
    return RayAccelView{ra.objs, ra.nodes, reinterpret_cast<const TriHot*>((const eray::accel::Hot*)ra.hot), ra.index};
}

// Records the message on the context (without one: for this thread, eray_last_error) and returns
// `code`.  Defined in capi.cpp, where the thread's message lives.
int set_error(eray_ctx* ctx, int code, const char* fmt, ...);

#define HIP_TRY(ctx, expr)                                                                   \
    do {                                                                                     \
        hipError_t e_ = (expr);                                                              \
        if (e_ != hipSuccess)                                                                \
            return set_error((ctx), e_ == hipErrorOutOfMemory ? ERAY_E_OUT_OF_MEMORY : ERAY_E_HIP, \
                             "%s: %s (%s:%d)", #expr, hipGetErrorString(e_), __FILE__, __LINE__); \
    } while (0)

inline int use_device(eray_ctx* ctx) {
    if (!ctx) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "null context");
    HIP_TRY(ctx, hipSetDevice(ctx->device));
    return ERAY_OK;
}

// Uploads what changed of the scene (geometry, descriptors) on the context's stream (capi_scene.cpp).
int sync_scene(eray_ctx* ctx);

// ---- the frame path's per-camera state (capi_setup.cpp) ----
// (RowSpan, the rendered rows of a call, and row_span: frame_plan.hpp.)
// Source tags of rendered frames, and which PPM slots hold which (eray_gather_frames).
FrameSource frame_source(uint32_t kind, uint64_t key, uint32_t W, uint32_t H, const RowSpan& rs);
FrameSource scene_source(const eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs);
void untag_range(eray_ctx* ctx, uintptr_t a, size_t bytes);
void tag_frames(eray_ctx* ctx, const uint8_t* ppm, uint64_t stride, uint32_t n, const FrameSource& s);
// Camera setups: one camera's, a path chunk's cameras at once, the scene camera's with its host copy.
// (bins: the buffers the setup's bins are built in, the context's own or a multi-camera set's)
SetupParams setup_params(eray_ctx* ctx, const BinBuffers& bins, const CamDev* d_camera, uint32_t W, uint32_t H,
                         const RowSpan& rs);
// The binned objects before object `index` (its place among the bin keys' objects).
uint32_t binned_before(const eray_ctx* ctx, uint32_t index);
int enqueue_setup(eray_ctx* ctx, const CamDev* d_camera, uint32_t W, uint32_t H, const RowSpan& rs, bool ordered,
                  bool keep_all = false, int32_t* path_union = nullptr);
int ensure_multi(eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs);
int enqueue_multi_setup(eray_ctx* ctx, eray_ctx::MultiSet& m, const CamDev* d_cams, uint32_t ncam, uint32_t W,
                        uint32_t H, const RowSpan& rs, hipStream_t s, int32_t* path_union = nullptr);
bool batch_setup_ok(const eray_ctx* ctx);
CamDev cam_dev(const eray_camera& c);
void state_arrived(eray_ctx* ctx);
int sync_setup(eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs, bool wait, bool* known,
               bool trace_bins = false);

// (owners.hpp)
template <typename T>
int DeviceBuf<T>::ensure(eray_ctx* ctx, size_t need) {
    if (need <= this->cap && this->p_) return ERAY_OK;
    if (this->p_) {
        HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
        HIP_TRY(ctx, this->release());
    }
    HIP_TRY(ctx, alloc(need ? need : 1));
    return ERAY_OK;
}

}  // namespace gpu
}  // namespace eray
