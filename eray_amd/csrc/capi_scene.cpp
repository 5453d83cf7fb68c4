// capi_scene.cpp — the scene of a context (ctx.hpp): the eray_scene_* entry points of
// include/eray_hip.h, and the scene's upload (sync_scene), which every call that needs the scene
// on the device runs first.  What the upload decides is scene_build.hpp's (the descriptors, the
// raw arrays' layout) and texel_prog.hpp's (the texel graphs' check and their programs); here are
// the allocations, the copies and the launches around them.  Host code only.
#include <hip/hip_runtime.h>

#include <cstring>
#include <vector>

#include "ctx.hpp"
#include "rays_args.hpp"

namespace {

bool image_ok(const eray_image& im) { return !im.data || (im.width > 0 && im.height > 0); }

// ERAY_OK when `index` names an object of the scene.
int check_object_index(eray_ctx* ctx, uint32_t index) {
    if (index >= ctx->objects.size())
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "object %u out of range (%zu objects)", index, ctx->objects.size());
    return ERAY_OK;
}

// The scene's objects changed: the ray-query hierarchy is of another scene.
void invalidate_ray_accel(eray_ctx* ctx) {
    ctx->ray_accel.valid = false;
    ctx->ray_accel.scene_changed = true;
    ++ctx->ray_accel.gen;
}

}  // namespace

int eray::gpu::sync_scene(eray_ctx* ctx) {
    int st;
    // The host staging vectors below feed async copies: drain earlier ones before reuse.
    if (ctx->geom_dirty || ctx->desc_dirty) HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    if (ctx->geom_dirty) {
        uint32_t T = 0;
        for (auto& o : ctx->objects) T += o.T;
        ctx->total_tris = T;
        if ((st = ctx->d_hot.ensure(ctx, T)) || (st = ctx->d_shade.ensure(ctx, T)) || (st = ctx->d_cull.ensure(ctx, T)))
            return st;
        // the general tracer's per-frame culling records (small scenes)
        if ((st = ctx->d_tcull.ensure(ctx, kTraceSkipTris))) return st;

        ctx->h_raw.assign((size_t)T * kRawFloatsPerFace, 0.0f);
        size_t begin = 0;
        for (auto& o : ctx->objects) {
            for (const RawSlice& s : raw_slices(T, begin, o.T))
                std::memcpy(&ctx->h_raw[s.in_scene], o.raw.data() + s.in_object, sizeof(float) * s.count);
            begin += o.T;
        }
        if ((st = ctx->d_raw.ensure(ctx, (size_t)T * kRawFloatsPerFace))) return st;
        if (T) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_raw, ctx->h_raw.data(), sizeof(float) * kRawFloatsPerFace * (size_t)T,
                                        hipMemcpyHostToDevice, ctx->stream));
            const auto all = raw_slices(T, 0, T);
            HIP_TRY(ctx, launch_tri_precompute(ctx->d_raw + all[0].in_scene, ctx->d_raw + all[1].in_scene,
                                               ctx->d_raw + all[2].in_scene, T, ctx->d_hot, ctx->d_shade, ctx->stream));
        }
        ctx->geom_dirty = false;
        ctx->desc_dirty = true;
    }
    if (ctx->desc_dirty) {
        // texel programs: per object a header + its outputs' expression trees (48-B records)
        ctx->h_prog.clear();
        std::vector<size_t> prog_at(ctx->objects.size(), SIZE_MAX);
        for (size_t i = 0; i < ctx->objects.size(); ++i) {
            const HostObject& o = ctx->objects[i];
            if (o.tnodes.empty()) continue;
            const size_t at = ctx->h_prog.size();
            const int out = compile_texel_program(o.tnodes, o.tout, ctx->h_prog);
            if (out >= 0)
                return set_error(ctx, ERAY_E_UNSUPPORTED, "object %zu: output %d expands to more than %u texel nodes",
                                 i, out, kTexelMaxNodes);
            prog_at[i] = at;
        }
        if (!ctx->h_prog.empty()) {
            if ((st = ctx->d_prog.ensure(ctx, ctx->h_prog.size()))) return st;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prog, ctx->h_prog.data(), 4 * ctx->h_prog.size(), hipMemcpyHostToDevice,
                                        ctx->stream));
        }
        SceneDescs& d = ctx->descs;
        build_scene_descs(ctx->objects, ctx->lights, ctx->d_prog, prog_at, d);
        if ((st = ctx->d_objs.ensure(ctx, d.objs.size()))) return st;
        if ((st = ctx->d_lights.ensure(ctx, d.lights.size()))) return st;
        if (!d.objs.empty())
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_objs, d.objs.data(), sizeof(ObjectDesc) * d.objs.size(), hipMemcpyHostToDevice,
                                        ctx->stream));
        if (!d.lights.empty())
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lights, d.lights.data(), sizeof(LightDesc) * d.lights.size(),
                                        hipMemcpyHostToDevice, ctx->stream));
        // setup.hip's object ranges and binned-object indices
        if ((st = ctx->d_begin.ensure(ctx, d.begin.size()))) return st;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_begin, d.begin.data(), 4 * d.begin.size(), hipMemcpyHostToDevice, ctx->stream));
        // rectangle accumulators + the setup's workgroup counter, zero between setups
        const size_t acc_words = setup_acc_words(d.objs.size());
        if (ctx->d_acc.cap < acc_words) {
            if ((st = ctx->d_acc.ensure(ctx, acc_words))) return st;
            HIP_TRY(ctx, hipMemsetAsync(ctx->d_acc, 0, 4 * ctx->d_acc.cap, ctx->stream));
        }
        ctx->desc_dirty = false;
        ++ctx->scene_gen;
    }
    return ERAY_OK;
}

namespace {
// Brings HostObject::raw up to date for the objects whose geometry eray_scene_update_object took
// from device arrays (their slices of the resident raw array; synchronises).  Such an object exists
// only while the geometry is resident: the update uploads the scene first, and every call that
// marks the geometry dirty comes here before it does.
int refresh_raw(eray_ctx* ctx) {
    bool any = false;
    for (auto& o : ctx->objects) any |= o.raw_stale;
    if (!any) return ERAY_OK;
    if (int st = use_device(ctx)) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    size_t begin = 0;
    for (auto& o : ctx->objects) {
        if (o.raw_stale && o.T)
            for (const RawSlice& s : raw_slices(ctx->total_tris, begin, o.T))
                HIP_TRY(ctx, hipMemcpy(o.raw.data() + s.in_object, ctx->d_raw + s.in_scene, sizeof(float) * s.count,
                                       hipMemcpyDeviceToHost));
        o.raw_stale = false;
        begin += o.T;
    }
    return ERAY_OK;
}

// Orders the context's stream after what the library's other streams hold now (enqueue only; not
// during a capture, where an event of a stream outside the capture cannot be waited for).  A
// context on the null stream is never capturing, and asking about the null stream while another
// stream of the process captures would itself be an illegal call: it is not asked.
int order_after_side_streams(eray_ctx* ctx) {
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (ctx->stream) HIP_TRY(ctx, hipStreamIsCapturing(ctx->stream, &capturing));
    if (capturing != hipStreamCaptureStatusNone) return ERAY_OK;
    if (!ctx->update_join) HIP_TRY(ctx, ctx->update_join.create(hipEventDisableTiming));
    for (hipStream_t side : {(hipStream_t)ctx->mc_stream, (hipStream_t)ctx->fill_stream}) {
        if (!side || side == ctx->stream) continue;
        HIP_TRY(ctx, hipEventRecord(ctx->update_join, side));
        HIP_TRY(ctx, hipStreamWaitEvent(ctx->stream, ctx->update_join, 0));
    }
    return ERAY_OK;
}
}  // namespace

extern "C" {

int eray_scene_reset(eray_ctx* ctx) {
    if (!ctx) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "null context");
    ctx->objects.clear();
    ctx->lights.clear();
    ctx->camera = eray_camera{{0.0f, 0.0f, 0.0f}, {60.0f, 60.0f}, 1024u, 1.0f};
    ctx->geom_dirty = ctx->desc_dirty = true;
    invalidate_ray_accel(ctx);
    return ERAY_OK;
}

int eray_scene_set_camera(eray_ctx* ctx, const eray_camera* camera) {
    if (!ctx || !camera) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null argument");
    if (std::memcmp(&ctx->camera, camera, sizeof(eray_camera)) != 0) {
        ctx->camera = *camera;  // (the next culled render sets it up: sync_setup)
    }
    return ERAY_OK;
}

int eray_scene_add_light(eray_ctx* ctx, const eray_light* light) {
    if (!ctx || !light) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null argument");
    if (light->variant != ERAY_LIGHT_POINT && light->variant != ERAY_LIGHT_AMBIENT)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "unknown light variant %d", light->variant);
    ctx->lights.push_back(*light);
    ctx->desc_dirty = true;
    return ERAY_OK;
}

int eray_scene_set_object_example_material(eray_ctx* ctx, uint32_t index, const eray_material_example_params* m) {
    if (!ctx || !m) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null argument");
    if (int st = check_object_index(ctx, index)) return st;
    if (!m->width || !m->height)  // Image::mod_get by 0 panics (image.rs:36-38)
        return set_error(ctx, ERAY_E_OUT_OF_BOUNDS, "example material of zero width or height");
    ctx->objects[index].example = true;
    ctx->objects[index].ex = *m;
    ctx->desc_dirty = true;
    return ERAY_OK;
}

int eray_scene_set_object_texel_graph(eray_ctx* ctx, uint32_t index, const eray_texel_graph* g) {
    if (!ctx) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null context");
    if (int st = check_object_index(ctx, index)) return st;
    char why[kWhyLen];
    if (int st = set_texel_graph(ctx->objects[index], g, why, sizeof why)) return set_error(ctx, st, "%s", why);
    ctx->desc_dirty = true;
    return ERAY_OK;
}

int eray_scene_add_object(eray_ctx* ctx, const eray_object* obj, uint32_t* index) {
    if (!ctx || !obj) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null argument");
    const uint32_t T = obj->triangle_count;
    if (T && (!obj->positions || !obj->normals || !obj->uvs))
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "object arrays are null");
    const eray_material& m = obj->material;
    if (!image_ok(m.color) || !image_ok(m.diffuse) || !image_ok(m.specular) ||
        !image_ok(m.specular_power) || !image_ok(m.reflection))
        return set_error(ctx, ERAY_E_OUT_OF_BOUNDS, "material image with zero width or height (mod_get by 0)");
    uint64_t total = T;
    for (auto& o : ctx->objects) total += o.T;
    if (total > kMaxSceneTris)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "too many triangles: %llu in the scene (at most %llu)",
                         (unsigned long long)total, (unsigned long long)kMaxSceneTris);
    if (int st = refresh_raw(ctx)) return st;  // (the upload below rebuilds every slice from the host copies)
    HostObject h;
    h.T = T;
    h.raw.resize((size_t)T * kRawFloatsPerFace);
    if (T) {
        const float* src[3] = {obj->positions, obj->normals, obj->uvs};
        const auto own = raw_slices(T, 0, T);
        for (int k = 0; k < 3; ++k) std::memcpy(h.raw.data() + own[k].in_object, src[k], sizeof(float) * own[k].count);
    }
    for (int k = 0; k < 3; ++k) {
        h.lo[k] = obj->bbox_min[k];
        h.hi[k] = obj->bbox_max[k];
    }
    h.mat = m;
    ctx->objects.push_back(std::move(h));
    if (index) *index = (uint32_t)(ctx->objects.size() - 1);
    ctx->geom_dirty = ctx->desc_dirty = true;
    invalidate_ray_accel(ctx);
    return ERAY_OK;
}

// The face count of an object of the scene (what eray_object_update::triangle_count must name).
int eray_scene_object_triangle_count(eray_ctx* ctx, uint32_t index, uint32_t* count) {
    if (!ctx || !count) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null argument");
    if (int st = check_object_index(ctx, index)) return st;
    *count = ctx->objects[index].T;
    return ERAY_OK;
}

// New vertex arrays for one object, in place (render.hip tri_update_kernel): the object's slices of
// the records and of the resident raw array are rewritten on the context's stream.  Everything
// derived from the geometry per camera is keyed on scene_gen and redone by its next user.  The work
// of the library's other streams that reads the records (the multi-camera setups on mc_stream, the
// separate fill's fork) is joined back into the context's stream by the call that starts it, so the
// kernel's place in that stream orders it after them; outside a capture the call also waits, on
// the stream, for whatever those streams hold at this point (order_after_side_streams).
int eray_scene_update_object(eray_ctx* ctx, uint32_t index, const eray_object_update* up) {
    if (int st = use_device(ctx)) return st;
    const char* why = "";
    if (int st = eray::check_update_params(up, index, ctx->objects.size(), index < ctx->objects.size() ? ctx->objects[index].T : 0u,
                                           &why))
        return set_error(ctx, st, "eray_scene_update_object: %s", why);
    if (int st = sync_scene(ctx)) return st;  // (a scene not yet on the device is uploaded first)
    HostObject& o = ctx->objects[index];
    const size_t T = o.T;
    size_t begin = 0;
    for (uint32_t i = 0; i < index; ++i) begin += ctx->objects[i].T;
    const auto sl = raw_slices(ctx->total_tris, begin, T);
    const bool device = (up->flags & ERAY_UPDATE_DEVICE) != 0;
    if (T && (up->positions || up->normals || up->uvs)) {
        const float *dp = up->positions, *dn = up->normals, *du = up->uvs;
        DeviceBuf<float> staged;  // host arrays: uploaded here, read by the kernel, released after a wait
        if (!device) {
            const size_t np = dp ? sl[0].count : 0, nn = dn ? sl[1].count : 0, nu = du ? sl[2].count : 0;
            HIP_TRY(ctx, staged.alloc(np + nn + nu));
            if (dp) HIP_TRY(ctx, hipMemcpyAsync(staged, dp, sizeof(float) * np, hipMemcpyHostToDevice, ctx->stream));
            if (dn) HIP_TRY(ctx, hipMemcpyAsync(staged + np, dn, sizeof(float) * nn, hipMemcpyHostToDevice, ctx->stream));
            if (du) HIP_TRY(ctx, hipMemcpyAsync(staged + np + nn, du, sizeof(float) * nu, hipMemcpyHostToDevice, ctx->stream));
            if (dp) dp = staged;
            if (dn) dn = staged + np;
            if (du) du = staged + np + nn;
        }
        if (int st = order_after_side_streams(ctx)) return st;
        HIP_TRY(ctx, launch_tri_update(dp, dn, du, (uint32_t)T, ctx->d_raw + sl[0].in_scene, ctx->d_raw + sl[1].in_scene,
                                       ctx->d_raw + sl[2].in_scene, ctx->d_hot + begin, ctx->d_shade + begin, ctx->stream));
        if (device) {
            o.raw_stale = true;
        } else {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            // the host copy follows the records once they are written (a failure above leaves both as they were)
            const float* src[3] = {up->positions, up->normals, up->uvs};
            for (int k = 0; k < 3; ++k)
                if (src[k]) std::memcpy(o.raw.data() + sl[k].in_object, src[k], sizeof(float) * sl[k].count);
        }
        // positions move the faces: the hierarchy's boxes no longer hold them (its arrays stay for
        // eray_scene_refit_ray_accel); normals and uvs are not in it
        if (up->positions) ctx->ray_accel.valid = false;
        ++ctx->scene_gen;
    }
    if (up->flags & ERAY_UPDATE_BBOX) {
        for (int k = 0; k < 3; ++k) {
            o.lo[k] = up->bbox_min[k];
            o.hi[k] = up->bbox_max[k];
        }
        ctx->desc_dirty = true;  // (the next call uploads the descriptors: sync_scene)
    }
    return ERAY_OK;
}

}  // extern "C"
