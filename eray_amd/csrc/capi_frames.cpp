// capi_frames.cpp — the frame entry points of include/eray_hip.h on the context (ctx.hpp): a render
// call's FrameParams (prepare_render), eray_render, the cache of captured frame graphs and launch
// plans, frames in flight into a ring (eray_render_frames*, eray_render_prepare*), the dispatch-timed
// measurements (eray_time_*) and camera paths with their three setup strategies
// (eray_render_camera_path*).  What a call decides before it touches the GPU — the parameter and ring
// checks, frames per launch, ring slots, the split into graph chunks — is frame_plan.hpp's (no HIP;
// tests/cpp/frame_plan_main.cpp checks it on the CPU); here are the HIP calls, the context and the
// strategies.  The camera setups, bins and frame tags they use are capi_setup.cpp's, the kernels'
// launchers render.hip's (internal.hpp).  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <vector>

#include "ctx.hpp"

namespace {
enum class SetupWait { kNo, kYes };

// Does a general-tracer render search through the scene's ray-query hierarchy (trace.hip's kernels
// with a RayAccelView)?  When the hierarchy is valid, covers an object, no flag forbids it, and some
// covered object's bounding box is not a point in x and y.  The last condition: almost every shadow
// and reflected ray fails BoundingBox::intersects on such a box (hit.hpp point_box_rejects; the
// reference's loaded meshes carry a (0,0,0) box), so with nothing but such boxes no walk would ever
// start and the hierarchy kernels' registers and LDS would buy nothing.  The number of covered
// objects, 0 for the scan.
uint32_t trace_accel_objects(const eray_ctx* ctx, uint32_t flags) {
    const RayAccel& ra = ctx->ray_accel;
    if (!ra.valid || !ra.covered || (flags & (ERAY_RENDER_BRUTE_FORCE | ERAY_RENDER_NO_RAY_ACCEL))) return 0u;
    for (const HostObject& o : ctx->objects)
        if (o.T >= ra.min_faces && !(o.lo[0] == o.hi[0] && o.lo[1] == o.hi[1])) return ra.covered;
    return 0u;
}
// The most faces of one object (FrameParams::max_object_tris; from the objects: the scene may not be
// synchronised yet).
uint32_t max_object_tris(const eray_ctx* ctx) {
    uint32_t m = 0;
    for (auto& o : ctx->objects) m = o.T > m ? o.T : m;
    return m;
}
// Frame parameters of a render call.  Culled frames need the camera's setup: when its results
// are on the host (or `wait`), the detail rectangles / count travel in the kernel arguments
// (args mode); otherwise the frame kernel reads them from the setup's CamState (device-camera
// mode) and the call never waits for the setup.
int prepare_render(eray_ctx* ctx, const eray_render_params* rp, FrameParams* out, bool* empty,
                   SetupWait wait = SetupWait::kNo) {
    if (int st = use_device(ctx)) return st;
    ctx->lc.accel = RayAccelView{nullptr, nullptr, nullptr, nullptr};  // (chosen below, per call)
    if (!rp) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "params is null");
    // anti-aliasing and reflection bounces take the general tracer (trace.hip); bounces only
    // matter when some material has a reflection output (engine.rs:181-182)
    const uint32_t bounces = scene_reflective(ctx->objects) ? rp->bounces : 0u;
    const bool general = rp->anti_aliasing > 0 || bounces > 0;
    uint32_t W, H;
    eray_camera_size(&ctx->camera, &W, &H);
    char why[kWhyLen];
    if (int code = check_render_params(rp, W, H, bounces, why, sizeof why)) return set_error(ctx, code, "%s", why);
    const bool cull = !general && !(rp->flags & ERAY_RENDER_BRUTE_FORCE);
    if (int st = sync_scene(ctx)) return st;
    *empty = !rp->rows || !W;
    if (*empty) return ERAY_OK;
    // the general tracer's camera rays scan the binned objects' bins (a setup of its own kind)
    const bool trace_bins = general && !(rp->flags & ERAY_RENDER_BRUTE_FORCE) && ctx->descs.binned > 0;
    bool known = true;
    if (cull || trace_bins)
        if (int st = sync_setup(ctx, W, H, row_span(rp), wait == SetupWait::kYes, &known, trace_bins)) return st;

    FrameParams& p = *out;
    std::memset(&p, 0, sizeof p);  // padding too: the launch-plan cache compares the bytes
    p.nframes = 1;
    const eray_camera& c = ctx->camera;
    p.cx = c.center[0];
    p.cy = c.center[1];
    p.cz = c.center[2];
    p.ratio = c.fov[0] / c.fov[1];
    p.z_dist = c.z_dist;
    p.cam_w = W;
    p.cam_h = H;
    p.img_w = rp->image_width;
    p.img_h = rp->image_height;
    p.row0 = rp->row0;
    p.rows = rp->rows;
    const RowSpan span = row_span(rp);
    p.band_shift = span.band_shift;
    p.band_mask = span.band_mask;
    p.band_stride = span.band_stride;
    p.out_rgb = rp->out_rgb;
    p.out_ppm = rp->out_ppm;
    p.out_face = rp->out_face;
    p.aligned = rows_aligned(p.img_w, p.rows, p.out_rgb, p.out_ppm, p.out_face);
    p.tris = ctx->d_hot;
    p.shade = ctx->d_shade;
    p.cull = cull ? ctx->d_cull : nullptr;
    p.objects = ctx->d_objs;
    p.lights = ctx->d_lights;
    p.nobj = (uint32_t)ctx->objects.size();
    p.nlights = (uint32_t)ctx->lights.size();
    p.max_object_tris = max_object_tris(ctx);
    p.total_tris = ctx->total_tris;
    p.lds_scene = (ctx->total_tris <= kCacheTris && p.nobj <= kCacheObjects && p.nlights <= kCacheLights) ? 1u : 0u;
    p.spec_pow = ctx->descs.spec_pow ? 1u : 0u;
    p.example_mat = ctx->descs.example_mat ? 1u : 0u;
    p.tiles_x = frame_tiles_x(W);
    p.bins_x = bin_cols(W);
    p.bin_phase = bin_phase(rp->row0);
    p.aa = rp->anti_aliasing;
    p.bounces = bounces;
    p.seed_lo = (uint32_t)rp->aa_seed;
    p.seed_hi = (uint32_t)(rp->aa_seed >> 32);
    p.trace_cull = (general && !(rp->flags & ERAY_RENDER_BRUTE_FORCE) && ctx->total_tris <= kTraceSkipTris)
                       ? ctx->d_tcull : nullptr;
    if (p.trace_cull) {  // the tracer's culling records of this camera (enqueued when it or the scene changed)
        std::vector<uint64_t> key(sizeof(eray_camera) / 4 + 3);
        std::memcpy(key.data(), &ctx->camera, sizeof(eray_camera));
        key[key.size() - 3] = ctx->scene_gen;
        key[key.size() - 2] = ((uint64_t)W << 32) | H;
        key[key.size() - 1] = (uint64_t)reinterpret_cast<uintptr_t>(ctx->stream);
        if (key != ctx->tcull_key) {
            ctx->tcull_key.clear();
            HIP_TRY(ctx, launch_trace_cull(p, ctx->stream));
            ctx->tcull_key = std::move(key);
        }
    }
    p.trace_bins = trace_bins ? 1u : 0u;
    if (general) {  // the tracer's shadow and reflected rays through the hierarchy, or the scan
        ctx->trace_accel_objects = trace_accel_objects(ctx, rp->flags);
        if (ctx->trace_accel_objects) ctx->lc.accel = accel_view(ctx);
    }
    // the setup's detail sub-block list (ordered: heavy ones first), the frame kernel's for binned
    // objects or the tracer's (trace.hip trace_binned_kernel, trace_heavy_kernel)
    if (trace_bins || (cull && ctx->descs.binned)) {
        p.detail_list = ctx->bins.dlist;
        p.detail_heavy = ctx->bins.dcount;
        p.detail_occ = ctx->bins.docc;
    }
    p.launch_flags = rp->flags & ~(ERAY_RENDER_BRUTE_FORCE | ERAY_RENDER_NO_RAY_ACCEL | kLaunchRingBeyondCache);
    if (!cull) {  // every pixel in detail
        whole_frame_rect(W, rp->rows, p.nobj, &p);
        return ERAY_OK;
    }
    if (known) {  // args mode
        const CamState& h = *ctx->h_state;
        p.nrect = h.nrect;
        p.total_sub = h.total_sub;
        std::memcpy(p.rects, h.rects, sizeof p.rects);
    } else {  // device-camera mode (the last known count only steers the launch shape)
        p.cam_state = ctx->d_state;
        p.total_sub = ctx->h_state ? ctx->h_state->total_sub : 0u;
    }
    return ERAY_OK;
}

hipError_t launch_frame(eray_ctx* ctx, const FrameParams& p) { return launch_render(p, ctx->lc, ctx->stream); }

// The source tag of frames rendered with p (prepare_render of rp): the scene camera through the
// frame kernel with its culling setup, or another kind.
FrameSource render_source(const eray_ctx* ctx, const FrameParams& p, const eray_render_params* rp) {
    if (p.cull && !p.aa && !p.bounces) return scene_source(ctx, p.cam_w, p.cam_h, row_span(rp));
    FrameSource s;
    s.kind = kSrcOther;
    return s;
}
}  // namespace

extern "C" {

// (diagnostics, eray_hip_debug.h) what prepare_render chose for the last general-tracer render
int eray_debug_trace_ray_accel(eray_ctx* ctx, uint32_t* objects) {
    if (!ctx || !objects) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "eray_debug_trace_ray_accel: null argument");
    *objects = ctx->trace_accel_objects;
    return ERAY_OK;
}

int eray_render(eray_ctx* ctx, const eray_render_params* rp) {
    FrameParams p;
    bool empty = false;
    if (int st = prepare_render(ctx, rp, &p, &empty)) return st;
    if (!empty) {
        HIP_TRY(ctx, launch_frame(ctx, p));
        tag_frames(ctx, p.out_ppm, 0, 1, render_source(ctx, p, rp));
    }
    return ERAY_OK;
}

}  // extern "C"

namespace {
constexpr size_t kGraphCache = 6;

// Appends v's bytes to a graph key.
template <typename V>
void append(std::vector<unsigned char>& key, const V& v) {
    const unsigned char* b = reinterpret_cast<const unsigned char*>(&v);
    key.insert(key.end(), b, b + sizeof v);
}

// The graph of n back-to-back frames, frame f enqueued by body(f), for `key` (+ n and the
// stream), captured unless cached.
template <typename Body>
int ensure_graph(eray_ctx* ctx, std::vector<unsigned char> key, uint32_t n, Body&& body, hipGraphExec_t* out) {
    append(key, n);
    append(key, ctx->stream);
    for (auto& G : ctx->graphs)
        if (G.key == key) {
            G.used = ++ctx->graph_clock;
            *out = G.exec;
            return ERAY_OK;
        }
    if (ctx->graphs.size() >= kGraphCache) {  // evict the least recently used
        size_t lru = 0;
        for (size_t i = 1; i < ctx->graphs.size(); ++i)
            if (ctx->graphs[i].used < ctx->graphs[lru].used) lru = i;
        std::swap(ctx->graphs[lru], ctx->graphs.back());
        ctx->graphs.pop_back();
    }
    HIP_TRY(ctx, hipStreamBeginCapture(ctx->stream, hipStreamCaptureModeThreadLocal));
    int st = ERAY_OK;
    for (uint32_t f = 0; f < n && st == ERAY_OK; ++f) st = body(f, n);
    FrameGraph G;
    hipError_t e = hipStreamEndCapture(ctx->stream, G.graph.put());
    if (st != ERAY_OK) return st;
    if (e == hipSuccess) e = hipGraphInstantiate(G.exec.put(), G.graph, nullptr, nullptr, 0);
    // the executable's packets and arguments go to the device now, not at its first launch (a
    // plan prepared ahead of a timed loop otherwise pays ~20 us at its first replay)
    if (e == hipSuccess) e = hipGraphUpload(G.exec, ctx->stream);
    if (e != hipSuccess) return set_error(ctx, ERAY_E_HIP, "frame graph capture: %s", hipGetErrorString(e));
    G.key = std::move(key);
    G.used = ++ctx->graph_clock;
    *out = G.exec;
    ctx->graphs.push_back(std::move(G));
    return ERAY_OK;
}

std::vector<unsigned char> params_key(const FrameParams& p, uint32_t kind) {
    std::vector<unsigned char> key;
    key.reserve(sizeof p + sizeof kind + 128);  // (room for what the callers append: one allocation)
    append(key, p);
    append(key, kind);
    return key;
}

// The launch plan of `frames` frames (frame_plan.hpp PlanShape) with its graphs: a graph per chunk
// length, replayed; a chunk without a graph (direct_plan) is enqueued frame by frame.
struct Plan : PlanShape {
    hipGraphExec_t chunk_exec = nullptr, rest_exec = nullptr;
};
template <typename Body>
int ensure_plan(eray_ctx* ctx, const std::vector<unsigned char>& key, uint32_t frames, Body&& body, Plan* plan) {
    *plan = Plan{graph_plan_shape(frames, ctx->stream != nullptr)};  // the null stream cannot be captured
    if (plan->chunk)
        if (int st = ensure_graph(ctx, key, plan->chunk, body, &plan->chunk_exec)) return st;
    if (plan->rest)
        if (int st = ensure_graph(ctx, key, plan->rest, body, &plan->rest_exec)) return st;
    return ERAY_OK;
}
Plan direct_plan(uint32_t frames) { return Plan{direct_plan_shape(frames)}; }

// Runs `plan` for `frames` frames of `run`: run.before_chunk(first frame, count) ahead of each
// chunk, the chunk as its graph's launch or, without one, run.body(first, f, count) per frame
// f < count; run.plain(f) renders the frames the plan does not cover.
template <typename Run>
int replay(eray_ctx* ctx, const Plan& plan, uint32_t frames, const Run& run) {
    auto chunk = [&](uint32_t first, uint32_t count, bool rest) -> int {
        if (int st = run.before_chunk(first, count)) return st;
        if (const hipGraphExec_t exec = rest ? plan.rest_exec : plan.chunk_exec) {
            const hipError_t e = hipGraphLaunch(exec, ctx->stream);
            if (e != hipSuccess) return set_error(ctx, ERAY_E_HIP, "render loop: %s", hipGetErrorString(e));
        } else {
            for (uint32_t f = 0; f < count; ++f)
                if (int st = run.body(first, f, count)) return st;
        }
        return ERAY_OK;
    };
    return walk_plan(plan, frames, chunk, [&](uint32_t f) { return run.plain(f); });
}

// The device time of a stretch of work on a stream, between two events of its own.
struct TimedRegion {
    Event ev[2];
    hipStream_t stream = nullptr;
    hipError_t begin(hipStream_t s) {
        stream = s;
        hipError_t e = ev[0].create();
        if (e == hipSuccess) e = ev[1].create();
        return e == hipSuccess ? hipEventRecord(ev[0], stream) : e;
    }
    hipError_t end(float* ms) {  // waits for the work
        hipError_t e = hipEventRecord(ev[1], stream);
        if (e == hipSuccess) e = hipEventSynchronize(ev[1]);
        return e == hipSuccess ? hipEventElapsedTime(ms, ev[0], ev[1]) : e;
    }
};
// work() enqueues `frames` frames on the context's stream; their mean device time when asked.
template <typename Work>
int timed_frames(eray_ctx* ctx, uint32_t frames, float* mean_ms, Work&& work) {
    TimedRegion t;
    if (mean_ms) {
        *mean_ms = 0.0f;
        HIP_TRY(ctx, t.begin(ctx->stream));
    }
    if (int st = work()) return st;
    if (mean_ms) {
        float ms = 0.0f;
        HIP_TRY(ctx, t.end(&ms));
        *mean_ms = ms / (float)frames;
    }
    return ERAY_OK;
}

// The start / end events of `launches` dispatch-timed launches (eray_time_frames_ring,
// eray_time_write_ceiling), `per` events each: the frame kernel's pair first.
struct LaunchTimers {
    std::vector<Event> ev;
    uint32_t launches, per;
    LaunchTimers(uint32_t launches, uint32_t per) : ev((size_t)launches * per), launches(launches), per(per) {}
    hipError_t create() {
        hipError_t e = hipSuccess;
        for (size_t k = 0; k < ev.size() && e == hipSuccess; ++k) e = ev[k].create();
        return e;
    }
    hipEvent_t at(uint32_t l, uint32_t k) const { return ev[(size_t)l * per + k]; }
    // The launches' frame kernel times into out's launches / frames_per_launch / mean / min / max
    // (after the stream has been synchronised).
    hipError_t reduce(uint32_t frames_per_launch, eray_kernel_times* out) const {
        double sum = 0.0;
        float lo = 0.0f, hi = 0.0f;
        for (uint32_t l = 0; l < launches; ++l) {
            float k = 0.0f;
            const hipError_t e = hipEventElapsedTime(&k, at(l, 0), at(l, 1));
            if (e != hipSuccess) return e;
            sum += k;
            lo = l ? std::min(lo, k) : k;
            hi = l ? std::max(hi, k) : k;
        }
        out->launches = launches;
        out->frames_per_launch = frames_per_launch;
        out->frame_kernel_ms = (float)(sum / launches);
        out->frame_kernel_min_ms = lo;
        out->frame_kernel_max_ms = hi;
        return hipSuccess;
    }
};
std::vector<unsigned char> ring_key(std::vector<unsigned char> key, const Ring& r) {
    append(key, r);
    return key;
}

// The hierarchy the call's tracer launches hold (LaunchCtx::accel, not part of FrameParams): its
// four addresses and the hierarchy's generation, which every build, drop, add_object and reset
// advances — so a plan captured with arrays that have since been released is never found again,
// even where an allocation returns an old address.  A refit in place keeps both, and the plan.
// Without a hierarchy in the launches: zeros.
std::vector<unsigned char> accel_key(std::vector<unsigned char> key, const eray_ctx* ctx) {
    const RayAccelView& a = ctx->lc.accel;
    for (const void* ptr : {(const void*)a.objs, (const void*)a.nodes, (const void*)a.hot, (const void*)a.index}) append(key, ptr);
    append(key, a.objs ? ctx->ray_accel.gen : (uint64_t)0);
    return key;
}

// The frames of a call with the scene camera into a ring: frame f is rendered by the launch of
// frame f - f % per_launch.
struct StaticRing {
    eray_ctx* ctx;
    const FrameParams& p;
    const Ring& r;
    uint32_t frames;
    int plan(Plan* out) const {
        auto frame = [this](uint32_t f, uint32_t n) { return body(0, f, n); };
        return ensure_plan(ctx, accel_key(ring_key(params_key(p, 0), r), ctx), frames, frame, out);
    }
    int before_chunk(uint32_t, uint32_t) const { return ERAY_OK; }
    int body(uint32_t, uint32_t f, uint32_t n) const {
        if (const uint32_t nf = launch_frames(f, n, r.per_launch)) HIP_TRY(ctx, launch_frame(ctx, ring_frames(p, r, f, nf)));
        return ERAY_OK;
    }
    int plain(uint32_t f) const { return body(0, f, frames); }
};

// The camera-path rectangle union (eray_gather_frames' layout of path frames): the device
// accumulator for nobj objects (SetupParams::path_union: the path's setup kernels fold every
// camera's rectangles into it) and a ring of kUnionRing finished unions in mapped pinned memory.
int ensure_union(eray_ctx* ctx, uint32_t nobj) {
    if (ctx->d_union_acc && ctx->h_union && ctx->union_cap() >= nobj) return ERAY_OK;
    for (Event& ev : ctx->union_ev) {
        if (!ev) HIP_TRY(ctx, ev.create(hipEventDisableTiming));
        HIP_TRY(ctx, hipEventSynchronize(ev));  // (a flush into the ring still in flight)
    }
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t n = std::max<uint32_t>(nobj, 1u);
    HIP_TRY(ctx, ctx->d_union_acc.alloc(4 * (size_t)n));
    HIP_TRY(ctx, ctx->h_union.alloc(4 * (size_t)n * kUnionRing, hipHostMallocMapped));
    HIP_TRY(ctx, launch_union_flush(ctx->d_union_acc, n, nullptr, ctx->stream));  // the initial reset
    for (auto& s : ctx->union_seq) s = 0;
    return ERAY_OK;
}
// After the frames of path call `src` (key: its sequence number): its union into ring entry
// key % kUnionRing (and the accumulator reset for the next path), one kernel on the stream.
int finish_union(eray_ctx* ctx, const FrameSource& src, uint32_t nobj) {
    const uint32_t e = (uint32_t)(src.key % kUnionRing);
    HIP_TRY(ctx, hipEventSynchronize(ctx->union_ev[e]));  // the entry's flush kUnionRing paths back
    HIP_TRY(ctx, launch_union_flush(ctx->d_union_acc, std::max(nobj, 1u),
                                    ctx->h_union.dev + (size_t)e * 4 * ctx->union_cap(), ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->union_ev[e], ctx->stream));
    ctx->union_seq[e] = src.key;
    ctx->union_src[e] = src;
    ctx->union_nobj[e] = nobj;
    ctx->union_gen[e] = ctx->scene_gen;
    return ERAY_OK;
}

// What the ring entry points start with: the call's frame parameters (prepare_render), then its
// ring (make_ring).  go: there are frames to render; without it the call is done (an empty image, no
// frames) or failed, and returns st.
struct RingCall {
    FrameParams p;
    Ring r;
    bool go = false;
    int st = ERAY_OK;
    RingCall(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring, bool any, SetupWait wait) {
        bool empty = false;
        if ((st = prepare_render(ctx, rp, &p, &empty, wait)) || empty || !any) return;
        char why[kWhyLen];
        if (int code = make_ring(rp, p, ring, &r, why, sizeof why)) st = set_error(ctx, code, "%s", why);
        go = !st;
    }
};

// A dispatch-timed call: max(1, frames / per_launch) full launches of the call's ring frames as plain
// launches, each with start / end events of its own, then the wait, the frame kernel's times and the
// slots' tags.  The measurement `m` says what differs: kWhat (its messages' prefix), kEvents per
// launch, args() — the check of its own arguments, ahead of the call's — accepts(p), enqueue(q, t, l)
// — launch l, with frame parameters q — and finish(p, rp, t, res, src): the result's other fields and
// the source the slots hold now.
template <typename M>
int time_launches(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring, uint32_t frames,
                  eray_kernel_times* out, M m) {
    if (!out) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "%s: out is null", M::kWhat);
    *out = eray_kernel_times{};
    if (int st = m.args(ctx)) return st;
    const RingCall c(ctx, rp, ring, frames != 0, SetupWait::kYes);
    if (!c.go) return c.st;
    if (int st = m.accepts(ctx, c.p)) return st;
    const uint32_t F = c.r.per_launch, L = std::max(1u, frames / F);
    LaunchTimers t(L, M::kEvents);
    HIP_TRY(ctx, t.create());
    for (uint32_t l = 0; l < L; ++l) HIP_TRY(ctx, m.enqueue(ctx, ring_frames(c.p, c.r, l * F, F), t, l));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    eray_kernel_times res{};
    HIP_TRY(ctx, t.reduce(F, &res));
    FrameSource src;
    if (int st = m.finish(ctx, c.p, rp, t, &res, &src)) return st;
    tag_frames(ctx, c.p.out_ppm, c.r.ppm, std::min(L * F, c.r.slots), src);
    *out = res;
    return ERAY_OK;
}

// eray_time_frames_ring: the frame kernel, and the separate fill where the launch shape has one.
struct FrameTiming {
    static constexpr const char* kWhat = "kernel timing";
    static constexpr uint32_t kEvents = 4;  // per launch: the frame kernel's pair, the separate fill's pair
    std::vector<uint32_t> fill_used;
    int args(eray_ctx*) const { return ERAY_OK; }
    int accepts(eray_ctx* ctx, const FrameParams& p) const {
        if (p.aa || p.bounces)
            return set_error(ctx, ERAY_E_UNSUPPORTED, "kernel timing: the frame kernel only (no anti-aliasing or bounces)");
        return ERAY_OK;
    }
    hipError_t enqueue(eray_ctx* ctx, const FrameParams& q, const LaunchTimers& t, uint32_t l) {
        if (fill_used.empty()) fill_used.assign(t.launches, 0u);
        LaunchCtx lc = ctx->lc;
        lc.frame_t[0] = t.at(l, 0);
        lc.frame_t[1] = t.at(l, 1);
        lc.fill_t[0] = t.at(l, 2);
        lc.fill_t[1] = t.at(l, 3);
        lc.fill_used = &fill_used[l];
        return launch_render(q, lc, ctx->stream);
    }
    int finish(eray_ctx* ctx, const FrameParams& p, const eray_render_params* rp, const LaunchTimers& t,
               eray_kernel_times* res, FrameSource* src) const {
        double fill = 0.0, span = 0.0;
        uint32_t nfill = 0;
        for (uint32_t l = 0; l < t.launches; ++l) {
            float s = 0.0f;
            HIP_TRY(ctx, hipEventElapsedTime(&s, t.at(l, 0), t.at(l, 1)));
            if (fill_used[l]) {  // the separate fill beside it: both kernels' span, from the frame kernel's start
                float f0 = 0.0f, f1 = 0.0f, fk = 0.0f;
                HIP_TRY(ctx, hipEventElapsedTime(&fk, t.at(l, 2), t.at(l, 3)));
                HIP_TRY(ctx, hipEventElapsedTime(&f0, t.at(l, 0), t.at(l, 2)));
                HIP_TRY(ctx, hipEventElapsedTime(&f1, t.at(l, 0), t.at(l, 3)));
                fill += fk;
                ++nfill;
                s = std::max(s, f1) - std::min(0.0f, f0);
            }
            span += s;
        }
        res->fill_kernel_ms = nfill ? (float)(fill / nfill) : 0.0f;
        res->launch_span_ms = (float)(span / t.launches);
        *src = render_source(ctx, p, rp);
        return ERAY_OK;
    }
};

// eray_time_write_ceiling: the frames' background bytes as a plain write stream.
struct CeilingTiming {
    static constexpr const char* kWhat = "write ceiling";
    static constexpr uint32_t kEvents = 2;
    uint32_t wgs_per_cu;
    int args(eray_ctx* ctx) const {
        if (wgs_per_cu < 1 || wgs_per_cu > 8)
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "write ceiling: %u workgroups per CU (1..8)", wgs_per_cu);
        return ERAY_OK;
    }
    int accepts(eray_ctx* ctx, const FrameParams& p) const {
        if (!p.aligned || p.img_w % 64u || p.rows % 4u)
            return set_error(ctx, ERAY_E_UNSUPPORTED, "write ceiling: whole 64x4 blocks only (%ux%u, aligned %u)", p.img_w,
                             p.rows, p.aligned);
        return ERAY_OK;
    }
    hipError_t enqueue(eray_ctx* ctx, const FrameParams& q, const LaunchTimers& t, uint32_t l) const {
        const hipEvent_t pair[2] = {t.at(l, 0), t.at(l, 1)};
        return launch_write_ceiling(q, wgs_per_cu, pair, ctx->stream);
    }
    int finish(eray_ctx*, const FrameParams&, const eray_render_params*, const LaunchTimers&, eray_kernel_times* res,
               FrameSource* src) const {
        res->launch_span_ms = res->frame_kernel_ms;
        *src = FrameSource{kSrcOther};  // the slots now hold background frames, not renders of the scene
        return ERAY_OK;
    }
};
}  // namespace

extern "C" {

int eray_render_prepare_ring(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring, uint32_t frames) {
    const RingCall c(ctx, rp, ring, true, SetupWait::kYes);
    if (!c.go) return c.st;
    Plan plan;
    return StaticRing{ctx, c.p, c.r, frames}.plan(&plan);
}

uint32_t eray_frames_per_launch(eray_ctx* ctx, const eray_render_params* rp, uint32_t slots) {
    if (!ctx || !rp || !slots) return 1u;
    uint32_t W, H;
    eray_camera_size(&ctx->camera, &W, &H);
    // (bounces as given: whether a material reflects is not asked here)
    return frames_per_launch(rp->anti_aliasing || rp->bounces, slots, 0, W, rp->rows, max_object_tris(ctx));
}

int eray_render_prepare(eray_ctx* ctx, const eray_render_params* rp, uint32_t frames) {
    return eray_render_prepare_ring(ctx, rp, nullptr, frames);
}

int eray_render_frames_ring(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring, uint32_t frames,
                            float* mean_frame_ms) {
    if (mean_frame_ms) *mean_frame_ms = 0.0f;
    const RingCall c(ctx, rp, ring, frames != 0, SetupWait::kYes);
    if (!c.go) return c.st;
    const StaticRing run{ctx, c.p, c.r, frames};
    Plan plan;
    if (int st = run.plan(&plan)) return st;
    const int st = timed_frames(ctx, frames, mean_frame_ms, [&] { return replay(ctx, plan, frames, run); });
    if (!st) tag_frames(ctx, c.p.out_ppm, c.r.ppm, std::min(frames, c.r.slots), render_source(ctx, c.p, rp));
    return st;
}

int eray_render_frames(eray_ctx* ctx, const eray_render_params* rp, uint32_t frames, float* mean_frame_ms) {
    return eray_render_frames_ring(ctx, rp, nullptr, frames, mean_frame_ms);
}

int eray_time_frames_ring(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring, uint32_t frames,
                          eray_kernel_times* out) {
    return time_launches(ctx, rp, ring, frames, out, FrameTiming{});
}

int eray_time_write_ceiling(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring, uint32_t frames,
                            uint32_t wgs_per_cu, eray_kernel_times* out) {
    return time_launches(ctx, rp, ring, frames, out, CeilingTiming{wgs_per_cu});
}

}  // extern "C"

namespace {
// ---- camera paths (eray_render_camera_path_ring): one frame per camera
//
// Anti-aliasing, bounces, brute force: no per-camera setup — every frame is prepared with its
// camera as the context's (camera in the kernel arguments) and launched plainly.
int general_path(eray_ctx* ctx, const eray_render_params* rp, const FrameParams& p, const Ring& r,
                 const eray_camera* cameras, uint32_t n, float* mean_ms) {
    const eray_camera saved = ctx->camera;
    const int st = timed_frames(ctx, n, mean_ms, [&]() -> int {
        for (uint32_t f = 0; f < n; ++f) {
            ctx->camera = cameras[f];
            FrameParams q;
            bool empty = false;
            if (int st = prepare_render(ctx, rp, &q, &empty)) return st;
            if (!empty) HIP_TRY(ctx, launch_frame(ctx, ring_frames(q, r, f, 1)));
        }
        return ERAY_OK;
    });
    ctx->camera = saved;
    if (!st) tag_frames(ctx, p.out_ppm, r.ppm, std::min(n, r.slots), FrameSource{kSrcOther});
    return st;
}

// The path's cameras to the device: staged in pinned memory and copied once per call, the whole
// path to d_path_all — each graph chunk reads its cameras from d_path (a device-to-device copy of
// its slice before each replay, PathCall::before_chunk) — or, a path of one graph chunk, straight
// into the chunk's camera slots (no per-chunk copy).
int stage_path_cameras(eray_ctx* ctx, const eray_camera* cameras, uint32_t n) {
    const uint32_t hb = ctx->path_buf;
    ctx->path_buf ^= 1u;
    PinnedBuf<CamDev>& h_path = ctx->h_path[hb];
    HIP_TRY(ctx, hipEventSynchronize(ctx->path_ev[hb]));  // the upload two calls back has read this buffer
    if (h_path.cap < n) HIP_TRY(ctx, h_path.alloc(n));
    for (uint32_t f = 0; f < n; ++f) h_path[f] = cam_dev(cameras[f]);
    if (int st = ctx->d_path_all.ensure(ctx, n)) return st;
    if (int st = ctx->d_path.ensure(ctx, kGraphFrames)) return st;
    HIP_TRY(ctx, hipMemcpyAsync(n <= kGraphFrames ? ctx->d_path : ctx->d_path_all, h_path, sizeof(CamDev) * n,
                                hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipEventRecord(ctx->path_ev[hb], ctx->stream));
    return ERAY_OK;
}

// What the culled path strategies share: the call's frame parameters in device-camera mode (every
// frame reads its setup's CamState), its ring, rows and staged cameras.  A strategy adds
// prepare(plan) — its buffers and launch plan — and what replay() asks of a run; in body and
// plain, `f` is the frame's index in the call (its ring slot).
struct PathCall {
    eray_ctx* ctx;
    FrameParams p;
    Ring r;
    uint32_t W, H, n;  // Camera::size, cameras
    RowSpan rs;
    uint32_t T, nobj;

    PathCall(eray_ctx* ctx, const eray_render_params* rp, const FrameParams& scene, const Ring& r, uint32_t n)
        : ctx(ctx), p(scene), r(r), W(scene.cam_w), H(scene.cam_h), n(n), rs(row_span(rp)), T(ctx->total_tris),
          nobj((uint32_t)ctx->objects.size()) {
        // the per-frame detail lists are appended split (heavy sub-blocks from the front, light
        // ones from the back: CamState counts)
        p.cam_state = ctx->d_state;
        p.detail_heavy = nullptr;
        p.dlist_split = p.detail_list ? (uint32_t)ctx->bins.nsub : 0u;
        p.nrect = 0;
        std::memset(p.rects, 0, sizeof p.rects);
    }
    // the call's rectangle union is flushed after the timed stretch, and the context's setup is
    // still the scene camera's afterwards (per-camera slots), unless a strategy says otherwise
    static constexpr bool kUnionTimed = false;
    void finish() const {}
    bool one_chunk() const { return n <= kGraphFrames; }
    // frame f's camera outside a chunk (plain launches)
    const CamDev* camera(uint32_t f) const { return (one_chunk() ? ctx->d_path : ctx->d_path_all) + f; }
    int before_chunk(uint32_t first, uint32_t count) const {
        if (one_chunk()) return ERAY_OK;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_path, ctx->d_path_all + first, sizeof(CamDev) * count,
                                    hipMemcpyDeviceToDevice, ctx->stream));
        return ERAY_OK;
    }
    // The graphs of `run` (kind: batched 2, else 1), keyed with every buffer their kernels hold.
    template <typename Run>
    int graph_plan(const Run& run, uint32_t kind, Plan* plan) const {
        std::vector<unsigned char> key = ring_key(params_key(p, kind), r);
        for (const void* ptr : {(const void*)ctx->d_path, (const void*)ctx->d_bcull, (const void*)ctx->d_bobjs,
                                (const void*)ctx->d_bstate, (const void*)ctx->d_union_acc})
            append(key, ptr);
        // the captured setup and bins kernels hold every bin buffer's address: a reallocation (a grown
        // capacity) must never replay a graph of the old buffers, even if some addresses recur
        append(key, ctx->bins_gen);
        append(key, (uint64_t)0);  // (the multi-camera buffers' generation, when those were captured)
        return ensure_plan(ctx, key, n, [&run](uint32_t f, uint32_t count) { return run.body(0, f, count); }, plan);
    }
};

// Scenes without binned objects, small enough (batch_setup_ok): a chunk's setups in one launch,
// enqueued with the chunk's first frame, into per-camera slots; frames in flight.
struct BatchedPath : PathCall {
    using PathCall::PathCall;
    int prepare(Plan* plan) {
        if (int st = ctx->d_bcull.ensure(ctx, (size_t)kGraphFrames * T)) return st;
        if (int st = ctx->d_bobjs.ensure(ctx, (size_t)kGraphFrames * nobj)) return st;
        if (int st = ctx->d_bstate.ensure(ctx, kGraphFrames)) return st;
        return graph_plan(*this, 2, plan);
    }
    // frame `slot` of a batch whose setups started at camera `cams` (count cameras): the launch of
    // slot s (s % per_launch == 0) renders slots [s, s + per_launch) of the batch, each from its
    // own setup slot
    int frame(const CamDev* cams, uint32_t slot, uint32_t count, uint32_t f, uint32_t per_launch) const {
        if (slot == 0) {
            SetupParams sp = setup_params(ctx, ctx->bins, cams, W, H, rs);
            sp.cull = ctx->d_bcull;
            sp.objs = ctx->d_bobjs;
            sp.objs_src = ctx->d_objs;
            sp.state = ctx->d_bstate;
            sp.path_union = ctx->d_union_acc;
            sp.union_nobj = nobj;
            HIP_TRY(ctx, launch_camera_setup_batch(sp, count, ctx->stream));
        }
        const uint32_t nf = launch_frames(slot, count, per_launch);
        if (!nf) return ERAY_OK;
        FrameParams q = ring_frames(p, r, f, nf);
        q.cam_state = ctx->d_bstate + slot;
        q.cull = ctx->d_bcull + (size_t)slot * T;
        q.objects = ctx->d_bobjs + (size_t)slot * nobj;
        q.dev_slots = 1;
        HIP_TRY(ctx, launch_frame(ctx, q));
        return ERAY_OK;
    }
    int body(uint32_t first, uint32_t f, uint32_t count) const { return frame(ctx->d_path, f, count, first + f, r.per_launch); }
    int plain(uint32_t f) const { return frame(camera(f), 0, 1, f, 1); }  // a batch of one
};

// Scenes with binned objects: the setups of up to mc_k cameras at once (one chain of kernels for
// all of them, ensure_multi), then their frames, each from its camera's slices.
// Multi-camera builds on two streams: enqueued directly, chunk by chunk, not replayed from a
// captured graph (the graph executor left the GPU idle for milliseconds after a path's first
// builds; same-box A/B, scripts/ab_multi.sh: C5's frame 475-485 -> 468 us, 3840x2160 / 70k
// 88-91 -> 57-58 us per moving frame)
struct MultiPath : PathCall {
    static constexpr bool kUnionTimed = true;  // (the union's flush is enqueued inside the timed stretch)
    using PathCall::PathCall;
    int prepare(Plan* plan) {
        if (int st = ensure_multi(ctx, W, H, rs)) return st;
        r.per_launch = fit_per_launch(r.per_launch, ctx->mc_k);  // frames in flight within one build: per_launch divides mc_k
        *plan = direct_plan(n);
        return ERAY_OK;
    }
    // frame `slot` of a run of `count` cameras at `cams`: batch b = slot / K of the run is built
    // into set b % 2; the first batch's build on the main stream, every later one on mc_stream
    // while the previous batch's frames render (it waits for the frames of batch b - 2, the set's
    // previous users), the frames wait for their build; frames in flight: the launch of slot s
    // (s % per_launch == 0) renders slots [s, s + n) of the batch (per_launch divides K, so a
    // launch never spans two builds), each from its slices
    int frame(const CamDev* cams, uint32_t slot, uint32_t count, uint32_t f) const {
        const uint32_t K = ctx->mc_k, k = slot % K, b = slot / K;
        auto& m = ctx->mc[b & 1u];
        if (k == 0) {
            if (b == 0) {
                if (int st = enqueue_multi_setup(ctx, m, cams, std::min(K, count), W, H, rs, ctx->stream, ctx->d_union_acc))
                    return st;
                HIP_TRY(ctx, hipEventRecord(ctx->mc_fork, ctx->stream));
            } else {
                HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->mc_ready[b & 1u], 0));
            }
            if ((b + 1) * K < count) {  // the next batch's build, beside this batch's frames
                auto& m2 = ctx->mc[(b + 1) & 1u];
                HIP_TRY(ctx, hipStreamWaitEvent(ctx->mc_stream, b == 0 ? ctx->mc_fork : ctx->mc_free[(b + 1) & 1u], 0));
                if (int st = enqueue_multi_setup(ctx, m2, cams + (b + 1) * K, std::min(K, count - (b + 1) * K), W, H, rs,
                                                 ctx->mc_stream, ctx->d_union_acc))
                    return st;
                HIP_TRY(ctx, hipEventRecord(ctx->mc_ready[(b + 1) & 1u], ctx->mc_stream));
            }
        }
        const uint32_t nsub = (uint32_t)m.bins.nsub, nf = launch_frames(slot, count, r.per_launch);
        if (!nf) return ERAY_OK;  // rendered by the launch of slot - slot % per_launch
        FrameParams q = ring_frames(p, r, f, nf);
        q.cam_state = m.state + k;
        q.cull = m.cull + (size_t)k * T;
        q.objects = m.objs + (size_t)k * nobj;
        q.detail_list = m.bins.dlist + (size_t)k * nsub;
        q.detail_occ = m.bins.docc + (size_t)k * (nsub / 4);
        q.dev_slots = nf > 1 ? 1u : 0u;
        q.dlist_stride = nf > 1 ? nsub : 0u;
        q.dlist_split = nsub;
        HIP_TRY(ctx, launch_frame(ctx, q));
        if (k + nf >= K || slot + nf >= count) HIP_TRY(ctx, hipEventRecord(ctx->mc_free[b & 1u], ctx->stream));
        return ERAY_OK;
    }
    int body(uint32_t first, uint32_t f, uint32_t count) const { return frame(ctx->d_path, f, count, first + f); }
    int plain(uint32_t f) const { return frame(camera(f), 0, 1, f); }
};

// Any other scene: the context's own setup (screen bins) and one frame per camera.
struct PerFramePath : PathCall {
    using PathCall::PathCall;
    int prepare(Plan* plan) {
        r.per_launch = 1;
        return graph_plan(*this, 1, plan);
    }
    int frame(const CamDev* cam, uint32_t f) const {
        if (int st = enqueue_setup(ctx, cam, W, H, rs, false, false, ctx->d_union_acc)) return st;
        HIP_TRY(ctx, launch_frame(ctx, ring_frames(p, r, f, 1)));
        return ERAY_OK;
    }
    int body(uint32_t first, uint32_t f, uint32_t) const { return frame(ctx->d_path + f, first + f); }
    int plain(uint32_t f) const { return frame(camera(f), f); }
    // the device state now belongs to the path's last camera: the scene camera is set up again at
    // its next render (whose count copy also grows the bins' capacity when a camera needed more;
    // no copy here: waiting for an earlier one would wait for that call's frames)
    void finish() const {
        ctx->setup_key.clear();
        ctx->state_known = false;
    }
};

// Runs a path strategy: its plan, the frames (timed when asked), the call's rectangle union and
// the frames' tags.  This call's frames are camera-path frames (eray_gather_frames): every
// camera's object rectangles fold into the union of the call.
template <typename Strategy>
int run_path(Strategy s, float* mean_ms) {
    eray_ctx* ctx = s.ctx;
    if (int st = ensure_union(ctx, s.nobj)) return st;
    Plan plan;
    if (int st = s.prepare(&plan)) return st;
    const FrameSource src = frame_source(kSrcPath, ++ctx->path_seq, s.W, s.H, s.rs);
    int st = timed_frames(ctx, s.n, mean_ms, [&]() -> int {
        const int st = replay(ctx, plan, s.n, s);
        return st || !Strategy::kUnionTimed ? st : finish_union(ctx, src, s.nobj);
    });
    if (!st && !Strategy::kUnionTimed) st = finish_union(ctx, src, s.nobj);
    if (!st) tag_frames(ctx, s.p.out_ppm, s.r.ppm, std::min(s.n, s.r.slots), src);
    s.finish();
    return st;
}
}  // namespace

extern "C" {

int eray_render_camera_path_ring(eray_ctx* ctx, const eray_render_params* rp, const eray_frame_ring* ring,
                                 const eray_camera* cameras, uint32_t n, float* mean_frame_ms) {
    if (int st = use_device(ctx)) return st;
    if (mean_frame_ms) *mean_frame_ms = 0.0f;
    if (!rp) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "params is null");
    if (n && !cameras) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "cameras is null");
    uint32_t W, H;
    eray_camera_size(&ctx->camera, &W, &H);
    for (uint32_t f = 0; f < n; ++f) {  // one engine image: every camera has the scene camera's size
        uint32_t w, h;
        eray_camera_size(&cameras[f], &w, &h);
        if (w != W || h != H)
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "camera %u: size %ux%u differs from the scene camera's %ux%u",
                             f, w, h, W, H);
    }
    // the scene camera's setup (scene upload, bins layout; the last known detail count steers the
    // launch shape) — enqueued, not waited for: the path's frames read their own cameras' setups
    const RingCall c(ctx, rp, ring, n != 0, SetupWait::kNo);
    if (!c.go) return c.st;
    if (!c.p.cull) return general_path(ctx, rp, c.p, c.r, cameras, n, mean_frame_ms);
    if (int st = stage_path_cameras(ctx, cameras, n)) return st;
    if (batch_setup_ok(ctx)) return run_path(BatchedPath(ctx, rp, c.p, c.r, n), mean_frame_ms);
    if (ctx->descs.binned) return run_path(MultiPath(ctx, rp, c.p, c.r, n), mean_frame_ms);
    return run_path(PerFramePath(ctx, rp, c.p, c.r, n), mean_frame_ms);
}

int eray_render_camera_path(eray_ctx* ctx, const eray_render_params* rp, const eray_camera* cameras, uint32_t n,
                            float* mean_frame_ms) {
    return eray_render_camera_path_ring(ctx, rp, nullptr, cameras, n, mean_frame_ms);
}

}  // extern "C"
