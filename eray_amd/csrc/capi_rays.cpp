// capi_rays.cpp — the ray-query part of include/eray_hip.h on the context of ctx.hpp: the query
// calls (rays.hip), the hierarchy's builds, refits and drop (accel_build.hpp on the host,
// accel_dev.hip on the device) and the hierarchy's debug exports (eray_hip_debug.h).  Host code only;
// capi.cpp's error policy.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <vector>

#include "accel_build.hpp"
#include "accel_check.hpp"
#include "accel_dev.hpp"
#include "ctx.hpp"
#include "rays_args.hpp"

namespace {

using Clock = std::chrono::steady_clock;

// min_faces = 0: objects of at least two of the batch search's tiles get a hierarchy
constexpr uint32_t kDefaultMinFaces = 2 * kRayTile;

float elapsed_ms(Clock::time_point t0) { return std::chrono::duration<float, std::milli>(Clock::now() - t0).count(); }

// What every build call starts with: the device, the clock, the scene uploaded and the stream idle.
int begin_build(eray_ctx* ctx, Clock::time_point* t0) {
    if (int st = use_device(ctx)) return st;
    *t0 = Clock::now();
    if (int st = sync_scene(ctx)) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (earlier queries may still read the old buffers)
    return ERAY_OK;
}

}  // namespace

extern "C" {

// Ray queries (rays.hip): the batch's kernel on the context's stream, nothing else — no setup, no
// copy back, so a call on an uploaded scene can be captured into a graph.
int eray_cast_rays(eray_ctx* ctx, const eray_rays_params* rp) {
    if (int st = use_device(ctx)) return st;
    const char* why = "";
    if (int st = eray::check_rays_params(rp, ctx->objects.size(), &why)) return set_error(ctx, st, "eray_cast_rays: %s", why);
    if (!rp->count) return ERAY_OK;
    if (int st = sync_scene(ctx)) return st;
    RayBatch b;
    std::memset(&b, 0, sizeof b);
    FrameParams& p = b.f;
    p.nframes = 1;
    p.cx = ctx->camera.center[0];
    p.cy = ctx->camera.center[1];
    p.cz = ctx->camera.center[2];
    p.tris = ctx->d_hot;
    p.shade = ctx->d_shade;
    p.objects = ctx->d_objs;
    p.lights = ctx->d_lights;
    p.nobj = (uint32_t)ctx->objects.size();
    p.nlights = (uint32_t)ctx->lights.size();
    p.total_tris = ctx->total_tris;
    p.bounces = scene_reflective(ctx->objects) ? rp->bounces : 0u;
    b.rays = reinterpret_cast<const RayIn*>(rp->rays);
    b.count = rp->count;
    b.object = rp->object;
    b.normalize = (rp->flags & ERAY_RAYS_NORMALIZE) ? 1u : 0u;
    b.brute = (rp->flags & ERAY_RAYS_BRUTE_FORCE) ? 1u : 0u;
    b.out_hit = reinterpret_cast<uint4*>(rp->out_hit);
    b.out_rgb = rp->out_rgb;
    HIP_TRY(ctx, launch_cast_rays(b, accel_view(ctx), ctx->stream));
    return ERAY_OK;
}

// Engine::reaches_light for caller-supplied shadow rays (rays.hip reach_kernel): one kernel on the
// context's stream like eray_cast_rays, so a call on an uploaded scene can be captured.
int eray_rays_reach_light(eray_ctx* ctx, const eray_reach_params* rp) {
    if (int st = use_device(ctx)) return st;
    const char* why = "";
    if (int st = eray::check_reach_params(rp, &why)) return set_error(ctx, st, "eray_rays_reach_light: %s", why);
    if (!rp->count) return ERAY_OK;
    if (int st = sync_scene(ctx)) return st;
    ReachBatch b;
    std::memset(&b, 0, sizeof b);
    FrameParams& p = b.f;
    p.nframes = 1;
    p.tris = ctx->d_hot;
    p.objects = ctx->d_objs;
    p.nobj = (uint32_t)ctx->objects.size();
    p.total_tris = ctx->total_tris;
    b.rays = reinterpret_cast<const RayIn*>(rp->rays);
    b.targets = rp->targets;
    b.count = rp->count;
    b.normalize = (rp->flags & ERAY_RAYS_NORMALIZE) ? 1u : 0u;
    b.brute = (rp->flags & ERAY_RAYS_BRUTE_FORCE) ? 1u : 0u;
    b.out = rp->out;
    HIP_TRY(ctx, launch_reach_light(b, accel_view(ctx), ctx->stream));
    return ERAY_OK;
}

}  // extern "C"

namespace {

// The ray-query hierarchy (accel_build.hpp build_scene) built on the host from the device's own
// TriHot records — the bits the kernels test — and uploaded, once the scene is uploaded and the
// stream idle.  refittable: the layout a refit needs is kept as well (numbering 1: the host
// builder's recursion order); the arrays are the same.
int build_accel_host(eray_ctx* ctx, uint32_t min_faces, Clock::time_point t0, eray_ray_accel_info* info, bool refittable) {
    const char* const fn = refittable ? "eray_scene_build_ray_accel_refittable" : "eray_scene_build_ray_accel";
    RayAccel& ra = ctx->ray_accel;
    ra.drop();
    if (!min_faces) min_faces = kDefaultMinFaces;
    const uint32_t T = ctx->total_tris;
    static_assert(sizeof(eray::accel::Hot) == sizeof(TriHot), "the builder reads the kernels' records");
    std::vector<eray::accel::Hot> hot(T);
    if (T) HIP_TRY(ctx, hipMemcpy(hot.data(), ctx->d_hot, sizeof(TriHot) * (size_t)T, hipMemcpyDeviceToHost));
    std::vector<uint32_t> sizes;
    for (const HostObject& o : ctx->objects) sizes.push_back(o.T);
    eray::accel::SceneBuilt b;
    size_t bad = 0;
    const char* why = "";
    if (!eray::accel::build_scene(hot.data(), sizes.data(), sizes.size(), min_faces, refittable, &b, &bad, &why))
        return set_error(ctx, ERAY_E_UNSUPPORTED, "%s: object %zu: %s", fn, bad, why);
    eray_ray_accel_info out{};
    out.objects = b.objects;
    out.max_depth = b.max_depth;
    out.nodes = b.nodes.size();
    out.faces = b.faces;
    out.unculled_faces = b.unculled;
    if (out.objects) {
        HIP_TRY(ctx, ra.objs.alloc(b.objs.size()));
        HIP_TRY(ctx, ra.nodes.alloc(std::max<size_t>(b.nodes.size(), 1)));
        HIP_TRY(ctx, ra.hot.alloc(std::max<size_t>(b.hot.size(), 1)));
        HIP_TRY(ctx, ra.index.alloc(std::max<size_t>(b.index.size(), 1)));
        HIP_TRY(ctx, hipMemcpy(ra.objs, b.objs.data(), sizeof(eray::accel::Object) * b.objs.size(), hipMemcpyHostToDevice));
        if (!b.nodes.empty())
            HIP_TRY(ctx, hipMemcpy(ra.nodes, b.nodes.data(), sizeof(eray::accel::Node) * b.nodes.size(), hipMemcpyHostToDevice));
        if (!b.hot.empty()) {
            HIP_TRY(ctx, hipMemcpy(ra.hot, b.hot.data(), sizeof(eray::accel::Hot) * b.hot.size(), hipMemcpyHostToDevice));
            HIP_TRY(ctx, hipMemcpy(ra.index, b.index.data(), 4 * b.index.size(), hipMemcpyHostToDevice));
        }
        out.device_bytes = ra.device_bytes();
        ra.min_faces = min_faces;
        ra.node_count = b.nodes.size();
        ra.slot_count = b.hot.size();
        ra.covered = out.objects;
        ra.builder = refittable ? RayAccel::kHostRefittable : RayAccel::kHost;
        if (refittable) {
            ra.layout = std::move(b.layout);
            ra.max_depth = out.max_depth;
        }
        ra.valid = true;
    }
    out.build_ms = elapsed_ms(t0);
    if (info) *info = out;
    return ERAY_OK;
}

// The objects that get a hierarchy: at least min_faces faces.
std::vector<AccelDevObject> covered_objects(const eray_ctx* ctx, uint32_t min_faces) {
    std::vector<AccelDevObject> covered;
    uint32_t begin = 0;
    for (size_t i = 0; i < ctx->objects.size(); ++i) {
        const uint32_t n = ctx->objects[i].T;
        if (n >= min_faces) covered.push_back(AccelDevObject{(uint32_t)i, begin, n});
        begin += n;
    }
    return covered;
}

// eray_scene_build_ray_accel_device once the scene is uploaded and the stream idle.
int build_accel_device(eray_ctx* ctx, uint32_t min_faces, Clock::time_point t0, eray_ray_accel_info* info) {
    RayAccel& ra = ctx->ray_accel;
    ra.drop();
    if (!min_faces) min_faces = kDefaultMinFaces;
    const std::vector<AccelDevObject> covered = covered_objects(ctx, min_faces);
    eray_ray_accel_info out{};
    for (const AccelDevObject& c : covered) {
        ++out.objects;
        out.faces += c.faces;
    }
    if (out.objects) {
        AccelDevInfo dev;
        const char* refuse = nullptr;
        HIP_TRY(ctx, accel_build_device(ctx->d_hot, covered, ctx->objects.size(), ra, ctx->stream, &dev, &refuse));
        if (refuse) return set_error(ctx, ERAY_E_UNSUPPORTED, "eray_scene_build_ray_accel_device: %s", refuse);
        out.nodes = dev.nodes;
        out.max_depth = dev.max_depth;
        out.unculled_faces = dev.unculled;
        out.device_bytes = ra.device_bytes();
        ra.min_faces = min_faces;
        ra.node_count = dev.nodes;
        ra.slot_count = out.faces;
        ra.covered = out.objects;
        ra.builder = RayAccel::kDevice;
        ra.valid = true;
    }
    out.build_ms = elapsed_ms(t0);
    if (info) *info = out;
    return ERAY_OK;
}

// Can a refit keep the topology?  The last build was the device's or the refittable host build and
// covered these objects, at these places, with these face counts, and no object was added and the
// scene not reset since (objs has a record per object of the build's scene: the arrays fit that
// scene only).
bool same_layout(const eray_ctx* ctx) {
    const RayAccel& ra = ctx->ray_accel;
    bool same = ra.refittable() && !ra.scene_changed && ra.objs.cap == ctx->objects.size();
    if (same) {
        const std::vector<AccelDevObject> covered = covered_objects(ctx, ra.min_faces);
        same = covered.size() == ra.layout.size();
        for (size_t i = 0; same && i < covered.size(); ++i)
            same = covered[i].index == ra.layout[i].index && covered[i].hot_begin == ra.layout[i].hot_begin &&
                   covered[i].faces == ra.layout[i].faces;
    }
    return same;
}

}  // namespace

extern "C" {

// The host build (synchronous).  A refit after it rebuilds on the device; the async refit refuses.
int eray_scene_build_ray_accel(eray_ctx* ctx, uint32_t min_faces, eray_ray_accel_info* info) {
    Clock::time_point t0;
    if (int st = begin_build(ctx, &t0)) return st;
    return build_accel_host(ctx, min_faces, t0, info, false);
}

// The same build, the same arrays, with what a refit needs kept beside them: the refit calls then
// keep this tree's topology as they keep a device build's, and rebuild with this builder.
int eray_scene_build_ray_accel_refittable(eray_ctx* ctx, uint32_t min_faces, eray_ray_accel_info* info) {
    Clock::time_point t0;
    if (int st = begin_build(ctx, &t0)) return st;
    return build_accel_host(ctx, min_faces, t0, info, true);
}

// The same hierarchy built on the context's stream from the resident records (accel_dev.hip): one
// round trip of 16 B of counters per covered object, no face record leaves the device.
int eray_scene_build_ray_accel_device(eray_ctx* ctx, uint32_t min_faces, eray_ray_accel_info* info) {
    Clock::time_point t0;
    if (int st = begin_build(ctx, &t0)) return st;
    return build_accel_device(ctx, min_faces, t0, info);
}

// Makes the hierarchy valid for the current records: the device build's topology is kept when only
// eray_scene_update_object happened since (accel_dev.hip accel_refit_device), else a device build.
// A refittable host build is treated alike: its topology is kept, else it is built again.
int eray_scene_refit_ray_accel(eray_ctx* ctx, eray_ray_accel_refit_info* info) {
    if (int st = use_device(ctx)) return st;
    const auto t0 = Clock::now();
    RayAccel& ra = ctx->ray_accel;
    if (ra.builder == RayAccel::kNone)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "eray_scene_refit_ray_accel: the scene has no ray-query hierarchy to refit");
    if (int st = sync_scene(ctx)) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (earlier queries may still read the arrays)
    eray_ray_accel_refit_info out{};
    const bool same = same_layout(ctx), host_refittable = ra.builder == RayAccel::kHostRefittable;
    bool kept = false;
    if (same) {
        AccelDevInfo dev;
        ra.valid = false;  // (until the refit has gone through)
        HIP_TRY(ctx, accel_refit_device(ctx->d_hot, ra, ctx->stream, &dev, &kept));
        if (kept) {
            out.accel.objects = out.refitted = (uint32_t)ra.layout.size();
            out.accel.max_depth = dev.max_depth;
            out.accel.nodes = dev.nodes;
            out.accel.faces = ra.slot_count;
            out.accel.unculled_faces = dev.unculled;
            out.accel.device_bytes = ra.device_bytes();
            out.accel.build_ms = elapsed_ms(t0);
            ra.valid = true;
        }
    }
    if (!kept) {
        // a caller who chose the host split stays on it (and refittable); every other hierarchy
        // is replaced by a device build
        if (int st = host_refittable ? build_accel_host(ctx, ra.min_faces, t0, &out.accel, true)
                                     : build_accel_device(ctx, ra.min_faces, t0, &out.accel))
            return st;
        out.rebuilt = 1;
    }
    if (info) *info = out;
    return ERAY_OK;
}

// The kept-topology refit enqueued on the context's stream (accel_dev.hip accel_refit_enqueue): the
// device takes the verdict per covered object and writes it into the object's `has` word, so the
// host neither waits nor reads; with its workspace in place the call only launches kernels and can
// be captured.  It never rebuilds: where eray_scene_refit_ray_accel would, it refuses.
int eray_scene_refit_ray_accel_async(eray_ctx* ctx) {
    static const char* const fn = "eray_scene_refit_ray_accel_async";
    if (!ctx) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "null context");
    RayAccel& ra = ctx->ray_accel;
    if (ra.builder == RayAccel::kNone)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "%s: the scene has no ray-query hierarchy to refit", fn);
    if (!ra.refittable())
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "%s: the hierarchy was built on the host (only a device build is refitted)", fn);
    if (!same_layout(ctx))
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                         "%s: the scene's objects are not those of the build (eray_scene_refit_ray_accel rebuilds)", fn);
    // first of all HIP calls, so that a refusal leaves a capture as it was (the null stream never
    // captures and is not asked: capi_scene.cpp order_after_side_streams)
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (ctx->stream) HIP_TRY(ctx, hipStreamIsCapturing(ctx->stream, &capturing));
    if (!ra.refit.ready()) {
        if (capturing != hipStreamCaptureStatusNone)
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "%s: no workspace yet: call once outside a capture first", fn);
        if (int st = use_device(ctx)) return st;
        HIP_TRY(ctx, accel_refit_workspace(ra, ctx->stream));
    }
    if (int st = use_device(ctx)) return st;
    HIP_TRY(ctx, accel_refit_enqueue(ctx->d_hot, ra, ctx->stream));
    ra.valid = true;  // (per object the device's `has` word carries the truth)
    return ERAY_OK;
}

int eray_scene_ray_accel_refit_status(eray_ctx* ctx, eray_ray_accel_refit_status* out) {
    if (int st = use_device(ctx)) return st;
    if (!out) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "eray_scene_ray_accel_refit_status: out is null");
    const RayAccel& ra = ctx->ray_accel;
    if (!ra.refit.ready())
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                         "eray_scene_ray_accel_refit_status: no refit workspace (eray_scene_refit_ray_accel_async makes it)");
    eray_ray_accel_refit_status s{};
    HIP_TRY(ctx, accel_refit_status(ra, ctx->stream, &s.refits, &s.kept));
    s.covered = ra.refit.ncov;
    s.fell_back = s.covered - s.kept;
    s.workspace_bytes = ra.refit.bytes;
    *out = s;
    return ERAY_OK;
}

int eray_scene_drop_ray_accel(eray_ctx* ctx) {
    if (int st = use_device(ctx)) return st;
    if (ctx->ray_accel.objs) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));  // (queries in flight read it)
    ctx->ray_accel.drop();
    return ERAY_OK;
}

// ---- diagnostics (eray_hip_debug.h)

// The current hierarchy (of either builder) and the face records copied back and checked on the
// host (accel_check.hpp).
int eray_debug_ray_accel_check(eray_ctx* ctx, char* msg, uint32_t cap) {
    if (int st = use_device(ctx)) return st;
    if (msg && cap) msg[0] = 0;
    auto say = [&](int code, const char* text) {
        if (msg && cap) std::snprintf(msg, cap, "%s", text);
        return set_error(ctx, code, "eray_debug_ray_accel_check: %s", text);
    };
    const RayAccel& ra = ctx->ray_accel;
    if (!ra.valid) return say(ERAY_E_INVALID_ARGUMENT, "the scene has no ray-query hierarchy");
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    const size_t nobj = ctx->objects.size(), T = ctx->total_tris;
    std::vector<uint32_t> sizes(nobj);
    for (size_t i = 0; i < nobj; ++i) sizes[i] = ctx->objects[i].T;
    std::vector<eray::accel::Hot> faces(T), hot(ra.slot_count);
    std::vector<eray::accel::Object> objs(nobj);
    std::vector<eray::accel::Node> nodes(ra.node_count);
    std::vector<uint32_t> index(ra.slot_count);
    if (T) HIP_TRY(ctx, hipMemcpy(faces.data(), ctx->d_hot, sizeof(TriHot) * T, hipMemcpyDeviceToHost));
    if (nobj) HIP_TRY(ctx, hipMemcpy(objs.data(), ra.objs, sizeof(eray::accel::Object) * nobj, hipMemcpyDeviceToHost));
    if (ra.node_count)
        HIP_TRY(ctx, hipMemcpy(nodes.data(), ra.nodes, sizeof(eray::accel::Node) * ra.node_count, hipMemcpyDeviceToHost));
    if (ra.slot_count) {
        HIP_TRY(ctx, hipMemcpy(hot.data(), ra.hot, sizeof(eray::accel::Hot) * ra.slot_count, hipMemcpyDeviceToHost));
        HIP_TRY(ctx, hipMemcpy(index.data(), ra.index, 4 * ra.slot_count, hipMemcpyDeviceToHost));
    }
    const char* bad = eray::accel::check(faces.data(), sizes.data(), nobj, ra.min_faces, objs.data(), nodes.data(), nodes.size(),
                                         hot.data(), index.data(), index.size());
    return bad ? say(ERAY_E_BUILD, bad) : ERAY_OK;
}

// One of the hierarchy's device arrays as it stands (valid or not, once the stream is idle), so
// that tests compare whole arrays: which = 0 the Object records, 1 the nodes, 2 the leaf-ordered
// face records, 3 the index array.  *bytes: its size; copied when out holds that much.
int eray_debug_ray_accel_arrays(eray_ctx* ctx, uint32_t which, void* out, size_t cap, size_t* bytes) {
    if (int st = use_device(ctx)) return st;
    const RayAccel& ra = ctx->ray_accel;
    if (!bytes || which > 3) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "eray_debug_ray_accel_arrays: bad argument");
    if (ra.builder == RayAccel::kNone)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "eray_debug_ray_accel_arrays: the scene has no ray-query hierarchy");
    const void* src[4] = {(const eray::accel::Object*)ra.objs, (const eray::accel::Node*)ra.nodes, (const eray::accel::Hot*)ra.hot,
                          (const uint32_t*)ra.index};
    const size_t size[4] = {sizeof(eray::accel::Object) * ra.objs.cap, sizeof(eray::accel::Node) * ra.node_count,
                            sizeof(eray::accel::Hot) * ra.slot_count, 4 * ra.slot_count};
    *bytes = size[which];
    if (!out) return ERAY_OK;
    if (cap < size[which]) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "eray_debug_ray_accel_arrays: out holds %zu of %zu bytes", cap, size[which]);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (size[which]) HIP_TRY(ctx, hipMemcpy(out, src[which], size[which], hipMemcpyDeviceToHost));
    return ERAY_OK;
}

// Whether eray_scene_refit_ray_accel_async runs the levels of at most 256 nodes in one launch (the
// default) or every level in a launch of its own; the bytes are the same.  Read when the call
// enqueues: a captured graph keeps the form it was captured with.
int eray_debug_set_refit_top_levels(eray_ctx* ctx, int on) {
    if (!ctx) return ERAY_E_INVALID_ARGUMENT;
    ctx->ray_accel.refit_top_levels = on != 0;
    return ERAY_OK;
}

}  // extern "C"
