// capi_setup.cpp — the frame path's per-camera state on the context (ctx.hpp): the source tags of
// rendered PPM slots (frame_source, scene_source, tag_frames, untag_range: what eray_gather_frames
// asks about), the screen bins' buffers, and the camera setups of setup.hip / bins.hip — one
// camera's (enqueue_setup), a path chunk's cameras at once (ensure_multi, enqueue_multi_setup) and
// the scene camera's with its host copy (sync_setup, state_arrived).  capi_frames.cpp renders with
// them; capi.cpp's memory calls and comm.cpp's gather use the tags.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"

namespace eray {
namespace gpu {

namespace {
constexpr size_t kMaxTags = 512;

uint64_t fnv1a(const void* data, size_t n, uint64_t h = 1469598103934665603ull) {
    const unsigned char* p = static_cast<const unsigned char*>(data);
    for (size_t i = 0; i < n; ++i) {
        h ^= p[i];
        h *= 1099511628211ull;
    }
    return h;
}

// A tagged slot's PPM bytes: [ppm, ppm + rows * W * 3).
uintptr_t tag_end(const eray_ctx::SlotTag& t) { return t.ppm + (uintptr_t)t.src.rows * t.src.W * 3u; }

// The binned objects' first triangles and object indices (bins_alloc's key tables).
void binned_lists(const eray_ctx* ctx, std::vector<uint32_t>* kbegin, std::vector<uint32_t>* kobj) {
    for (uint32_t i = 0; i < ctx->objects.size(); ++i)
        if (ctx->objects[i].T > kDirectMax) {
            kbegin->push_back(ctx->descs.objs[i].g.tri_begin);
            kobj->push_back(i);
        }
}

// The device buffers of the binned objects' bins for this camera size, row phase and rows
// (reallocated, with a stream synchronisation, only when that layout or the capacity changes).
int ensure_bins(eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs) {
    const uint32_t row0 = rs.row0, rows = rs.rows;
    const uint32_t nb = ctx->descs.binned;
    const uint32_t T = ctx->total_tris;
    int st;
    if ((st = ctx->d_range.ensure(ctx, T)) || (st = ctx->d_area.ensure(ctx, T)) || (st = ctx->d_fkey.ensure(ctx, T)))
        return st;
    size_t binned_tris = 0;
    for (auto& o : ctx->objects)
        if (o.T > kDirectMax) binned_tris += o.T;
    if (!ctx->bin_cap) ctx->bin_cap = std::min(std::max<size_t>(2 * binned_tris, 1u << 16), kMaxBinEntries);
    const uint32_t phase = bin_phase(row0), tiles_x = frame_tiles_x(W);
    std::vector<uint64_t> layout{T, nb, W, H, phase, rows, ctx->bin_cap, ctx->scene_gen};
    if (layout == ctx->bins_layout) return ERAY_OK;
    std::vector<uint32_t> kbegin, kobj;
    binned_lists(ctx, &kbegin, &kobj);
    HIP_TRY(ctx, bins_alloc(ctx->bins, T, nb, kbegin.data(), kobj.data(), W, H, phase, tiles_x, rows, ctx->bin_cap,
                            ctx->stream));
    ctx->bins_layout = std::move(layout);
    ++ctx->bins_gen;         // graphs that captured the old buffers must not be replayed
    ctx->setup_key.clear();  // the bins must be rebuilt
    return ERAY_OK;
}
}  // namespace

uint32_t binned_before(const eray_ctx* ctx, uint32_t index) {
    uint32_t k = 0;
    for (uint32_t i = 0; i < index; ++i) k += ctx->objects[i].T > kDirectMax;
    return k;
}

FrameSource frame_source(uint32_t kind, uint64_t key, uint32_t W, uint32_t H, const RowSpan& rs) {
    FrameSource s;
    s.kind = kind;
    s.key = key;
    s.W = W;
    s.H = H;
    s.row0 = rs.row0;
    s.rows = rs.rows;
    s.band_shift = rs.band_shift;
    s.band_stride = rs.band_stride;
    return s;
}

// The source tag of a render of the scene camera over rows rs: a hash of the camera's value, the
// scene generation (uploads since the context was made) and Camera::size — what every rank that
// made the same scene calls computes alike.
FrameSource scene_source(const eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs) {
    uint64_t h = fnv1a(&ctx->camera, sizeof ctx->camera);
    h = fnv1a(&ctx->scene_gen, sizeof ctx->scene_gen, h);
    const uint32_t wh[2] = {W, H};
    return frame_source(kSrcScene, fnv1a(wh, sizeof wh, h), W, H, rs);
}

// Forgets the source of every tagged slot whose bytes meet [a, a + bytes): memory written (or
// freed) by anything but a render of that source no longer holds its frame.
void untag_range(eray_ctx* ctx, uintptr_t a, size_t bytes) {
    if (!bytes) return;
    auto& v = ctx->slot_tags;
    v.erase(std::remove_if(v.begin(), v.end(),
                           [&](const eray_ctx::SlotTag& t) { return t.ppm < a + bytes && a < std::max(tag_end(t), t.ppm + 1); }),
            v.end());
}
// Records `s` as the source of the n PPM slots ppm + k * stride (k < n); any other tag whose
// bytes the new frames overwrite is dropped.
void tag_frames(eray_ctx* ctx, const uint8_t* ppm, uint64_t stride, uint32_t n, const FrameSource& s) {
    if (!ppm) return;
    if (s.kind == kSrcScene || s.kind == kSrcPath) ctx->gather_src = s;
    auto& v = ctx->slot_tags;
    for (uint32_t k = 0; k < n; ++k) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(ppm) + (uintptr_t)(k * stride);
        untag_range(ctx, a, std::max<size_t>((size_t)s.rows * s.W * 3u, 1));
        if (v.size() >= kMaxTags) v.erase(v.begin());
        v.push_back({a, s});
    }
}

// Enqueues the per-camera setup of `d_camera` (device) for camera rows [row0, row0 + rows): no
// host round trip (setup.hip, bins.hip).
SetupParams setup_params(eray_ctx* ctx, const BinBuffers& bins, const CamDev* d_camera, uint32_t W, uint32_t H,
                         const RowSpan& rs) {
    SetupParams sp{};
    sp.hot = ctx->d_hot;
    sp.cull = ctx->d_cull;
    sp.T = ctx->total_tris;
    sp.objs = ctx->d_objs;
    sp.nobj = (uint32_t)ctx->objects.size();
    sp.obj_begin = ctx->d_begin;
    sp.objkey = ctx->d_begin + sp.nobj + 1;
    sp.cam = d_camera;
    sp.state = ctx->d_state;
    sp.W = W;
    sp.H = H;
    sp.row0 = rs.row0;
    sp.rows = rs.rows;
    sp.band_shift = rs.band_shift;
    sp.band_mask = rs.band_mask;
    sp.band_stride = rs.band_stride;
    sp.done = ctx->d_acc;
    sp.part = ctx->d_acc + kSetupAccPart;
    sp.acc = ctx->d_acc + kSetupAccRects;
    const bool binned = ctx->descs.binned > 0;
    sp.binned = binned ? 1u : 0u;
    sp.rect_pairs = ctx->rect_pairs ? 1u : 0u;
    if (binned) {
        sp.range = ctx->d_range;
        sp.area = ctx->d_area;
        sp.fkey = ctx->d_fkey;
        sp.bins_x = bins.bins_x;
        sp.phase = bins.phase;
        sp.first_local = bins.first;
        sp.boff = bins.boff;
    }
    return sp;
}

// ordered: the detail list in raster order (one-camera setups, whose list serves many frames);
// camera paths append it in one launch instead (bins.hip detail_list_kernel)
// keep_all: the general tracer's bins (SetupParams::keep_all)
int enqueue_setup(eray_ctx* ctx, const CamDev* d_camera, uint32_t W, uint32_t H, const RowSpan& rs, bool ordered,
                  bool keep_all, int32_t* path_union) {
    SetupParams sp = setup_params(ctx, ctx->bins, d_camera, W, H, rs);
    sp.keep_all = keep_all ? 1u : 0u;
    sp.path_union = path_union;
    sp.union_nobj = sp.nobj;
    HIP_TRY(ctx, launch_camera_setup(sp, ctx->stream));
    if (sp.binned) HIP_TRY(ctx, launch_bins_build(sp, ctx->bins, frame_tiles_x(W), ordered, ctx->stream));
    return ERAY_OK;
}

// The multi-camera setup buffers (camera paths of scenes with binned objects) for the current
// bins layout (ensure_bins ran first): two sets of mc_k copies of every per-camera array, camera
// k's descriptors initialised with the scene's; reallocated when the layout or the scene changes
// (mc_gen keys the captured path graphs).
int ensure_multi(eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs) {
    // cameras per build: the chain's kernels are latency bound at tens of thousands of faces (16
    // cameras share one chain), work bound at millions (fewer: the buffers grow with K x faces)
    const uint32_t K = std::max(1u, std::min(16u, (1u << 22) / std::max(ctx->total_tris, 1u)));
    std::vector<uint64_t> layout = ctx->bins_layout;
    layout.push_back(ctx->scene_gen);
    if (layout == ctx->mc_layout) return ERAY_OK;
    if (!ctx->mc_stream) {
        // (a priority of its own: HIP deals its hardware queues to streams round-robin per priority,
        // and on the frames' queue the setup chain serialised with them — moving C5 frame 416 ->
        // 375 us, 3840x2160 / 70k 60.6 -> 55.7 us, profiles/r04/ab/ab_r04m.txt)
        HIP_TRY(ctx, ctx->mc_stream.create(hipStreamNonBlocking, -1));
        for (Event* ev : {&ctx->mc_fork, &ctx->mc_ready[0], &ctx->mc_ready[1], &ctx->mc_free[0], &ctx->mc_free[1]})
            HIP_TRY(ctx, ev->create(hipEventDisableTiming));
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->mc_stream));
    ctx->mc_layout.clear();
    const uint32_t T = ctx->total_tris, nobj = (uint32_t)ctx->objects.size(), nb = ctx->descs.binned;
    const size_t t = (size_t)K * (T ? T : 1);
    const size_t acc_words = setup_acc_words((size_t)K * nobj);
    // camera k's copy of binned object j: key k * nb + j, its faces from k * T + tri_begin
    std::vector<uint32_t> kbegin, kobj, mbegin, mobj;
    binned_lists(ctx, &kbegin, &kobj);
    for (uint32_t k = 0; k < K; ++k)
        for (uint32_t j = 0; j < nb; ++j) {
            mbegin.push_back(k * T + kbegin[j]);
            mobj.push_back(k * nobj + kobj[j]);
        }
    for (auto& m : ctx->mc) {
        int st;
        if ((st = m.cull.ensure(ctx, t)) || (st = m.objs.ensure(ctx, (size_t)K * nobj)) || (st = m.state.ensure(ctx, K)) ||
            (st = m.acc.ensure(ctx, acc_words)) || (st = m.range.ensure(ctx, t)) || (st = m.area.ensure(ctx, t)) ||
            (st = m.fkey.ensure(ctx, t)))
            return st;
        HIP_TRY(ctx, hipMemsetAsync(m.acc, 0, 4 * acc_words, ctx->stream));
        HIP_TRY(ctx, hipMemsetAsync(m.state, 0, sizeof(CamState) * K, ctx->stream));
        for (uint32_t k = 0; k < K && nobj; ++k)  // (each setup rewrites the rectangles and bin views)
            HIP_TRY(ctx, hipMemcpyAsync(m.objs + (size_t)k * nobj, ctx->d_objs, sizeof(ObjectDesc) * nobj,
                                        hipMemcpyDeviceToDevice, ctx->stream));
        HIP_TRY(ctx, bins_alloc(m.bins, K * T, K * nb, mbegin.data(), mobj.data(), W, H, bin_phase(rs.row0), frame_tiles_x(W),
                                rs.rows, std::min((size_t)K * ctx->bin_cap, kMaxBinEntries), ctx->stream, K));
    }
    ctx->mc_layout = std::move(layout);
    ctx->mc_k = K;
    ++ctx->mc_gen;
    return ERAY_OK;
}

// Enqueues on `s` the setups of the `ncam` cameras at d_cams (ncam <= mc_k) into buffer set `m`:
// camera k's culling records at m.cull + k T, descriptors at m.objs + k nobj, state m.state + k,
// detail list m.bins.dlist + k nsub (occupancy m.bins.docc + k nsub / 4).
int enqueue_multi_setup(eray_ctx* ctx, eray_ctx::MultiSet& m, const CamDev* d_cams, uint32_t ncam, uint32_t W,
                        uint32_t H, const RowSpan& rs, hipStream_t s, int32_t* path_union) {
    const uint32_t T = ctx->total_tris, nobj = (uint32_t)ctx->objects.size();
    SetupParams sp = setup_params(ctx, m.bins, d_cams, W, H, rs);
    sp.ncam = ncam;
    sp.T1 = T;
    sp.nobj1 = nobj;
    sp.nb1 = ctx->descs.binned;
    sp.T = ncam * T;
    sp.nobj = ncam * nobj;
    sp.cull = m.cull;
    sp.objs = m.objs;
    sp.state = m.state;
    sp.done = m.acc;
    sp.part = m.acc + kSetupAccPart;
    sp.acc = m.acc + kSetupAccRects;
    sp.range = m.range;
    sp.area = m.area;
    sp.fkey = m.fkey;
    sp.path_union = path_union;
    sp.union_nobj = nobj;
    HIP_TRY(ctx, launch_camera_setup(sp, s));
    HIP_TRY(ctx, launch_bins_build(sp, m.bins, frame_tiles_x(W), false, s));
    return ERAY_OK;
}

// Camera paths of scenes without binned objects set up a whole graph chunk's cameras in one
// launch (one workgroup per camera, into per-camera slots) instead of one setup per frame: the
// setup of a small scene is one workgroup's latency chain (culling records, the double-precision
// clip of face_rect, the rectangle merge), which as its own launch per frame cost about as much
// as the frame.  Up to kBatchTris triangles (the slots hold kGraphFrames x T culling records).
constexpr uint32_t kBatchTris = 16384;
bool batch_setup_ok(const eray_ctx* ctx) {
    return !ctx->descs.binned && ctx->objects.size() <= kSetupBatchMaxObjects && ctx->total_tris <= kBatchTris;
}

CamDev cam_dev(const eray_camera& c) {
    return CamDev{c.center[0], c.center[1], c.center[2], c.fov[0] / c.fov[1], c.z_dist, {0u, 0u, 0u}};
}

// A copy of the setup state has reached the host (h_state): grow the bins' capacity when some
// setup since the last reallocation needed more entries (they then fell back to LDS tiles).
void state_arrived(eray_ctx* ctx) {
    ctx->state_pending = false;
    ctx->state_known = true;
    if (ctx->h_state->bin_entries > ctx->bin_cap && ctx->bin_cap < kMaxBinEntries) {
        // (at most kMaxBinEntries: beyond, the setups keep overflowing into the exact LDS-tile scan)
        ctx->bin_cap = std::min(2 * (size_t)ctx->h_state->bin_entries, kMaxBinEntries);
        ctx->state_known = false;
        ctx->setup_key.clear();  // rebuilt with the larger capacity
    }
}

// Makes the per-camera setup of the context camera current for rows [row0, row0 + rows):
// enqueued when the camera, the rows or the scene changed, its results copied to the host
// asynchronously.  *known: the host has them (args-mode frames); `wait`: block until it does.
// trace_bins: the general tracer's setup (every pair of each face's bin rectangle binned).
int sync_setup(eray_ctx* ctx, uint32_t W, uint32_t H, const RowSpan& rs, bool wait, bool* known,
               bool trace_bins) {
    for (int attempt = 0; attempt < 3; ++attempt) {
        if (ctx->state_pending) {
            const hipError_t q = hipEventQuery(ctx->state_ev);
            if (q == hipSuccess) state_arrived(ctx);
            else if (q != hipErrorNotReady) return set_error(ctx, ERAY_E_HIP, "setup event: %s", hipGetErrorString(q));
        }
        auto bins_ready = [&]() -> int {
            if (!ctx->descs.binned) return ERAY_OK;
            const std::vector<uint64_t> before = ctx->bins_layout;
            if (int st = ensure_bins(ctx, W, H, rs)) return st;
            if (ctx->bins_layout != before)  // new buffers: the bin statistics start over
                HIP_TRY(ctx, hipMemsetAsync(ctx->d_state, 0, sizeof(CamState), ctx->stream));
            return ERAY_OK;
        };
        if (int st = bins_ready()) return st;
        std::vector<uint64_t> key(sizeof(eray_camera) / 4 + 5);
        std::memcpy(key.data(), &ctx->camera, sizeof(eray_camera));
        key[key.size() - 5] = trace_bins ? 1u : 0u;
        key[key.size() - 4] = ((uint64_t)rs.row0 << 32) | rs.band_shift;
        key[key.size() - 3] = ((uint64_t)rs.rows << 32) | rs.band_stride;
        key[key.size() - 2] = ctx->scene_gen;
        key[key.size() - 1] = ((uint64_t)W << 32) | H;
        if (key != ctx->setup_key) {
            if (ctx->state_pending) {  // h_state is about to be rewritten
                HIP_TRY(ctx, hipEventSynchronize(ctx->state_ev));
                state_arrived(ctx);
                if (int st = bins_ready()) return st;  // (a grown capacity)
            }
            HIP_TRY(ctx, launch_set_camera(cam_dev(ctx->camera), ctx->d_cam, ctx->stream));
            if (int st = enqueue_setup(ctx, ctx->d_cam, W, H, rs, true, trace_bins)) return st;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->h_state, ctx->d_state, sizeof(CamState), hipMemcpyDeviceToHost,
                                        ctx->stream));
            // the objects' pixel rectangles of this camera (eray_gather_frames' transfer layout);
            // no copy into the pinned buffer is in flight here (state_pending was drained above)
            const size_t nobj = ctx->objects.size();
            if (ctx->h_objs_state.cap < nobj) HIP_TRY(ctx, ctx->h_objs_state.alloc(nobj));
            if (nobj)
                HIP_TRY(ctx, hipMemcpyAsync(ctx->h_objs_state, ctx->d_objs, sizeof(ObjectDesc) * nobj,
                                            hipMemcpyDeviceToHost, ctx->stream));
            ctx->setup_src = scene_source(ctx, W, H, rs);
            HIP_TRY(ctx, hipEventRecord(ctx->state_ev, ctx->stream));
            ctx->setup_key = std::move(key);
            ctx->state_pending = true;
            ctx->state_known = false;
        }
        if (ctx->state_pending && wait) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->state_ev));
            state_arrived(ctx);  // (may ask for a larger capacity: set up again)
        }
        if (ctx->state_known || !wait) break;
    }
    *known = ctx->state_known;
    return ERAY_OK;
}

}  // namespace gpu
}  // namespace eray
