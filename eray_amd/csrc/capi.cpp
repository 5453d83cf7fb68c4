// capi.cpp — implementation of include/eray_hip.h: context, device memory, the shaderlib node entry
// points, the scene API with its upload, PPM packing, eray_internal_error and the eray_debug_* hooks.
// The frame path is capi_setup.cpp (camera setup, bins, frame tags) and capi_frames.cpp (the
// eray_render* and eray_time_* entry points); the ray queries and their hierarchy capi_rays.cpp — all
// on the same context, ctx.hpp.  Host code only; the kernels live in render.hip and shaderlib.hip.
//
// Error policy: every HIP call is checked; failures and every case where the reference would
// panic become a status code plus a message (eray_last_error).  Nothing here falls back to a
// CPU path: without a usable GPU the calls fail loudly.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <new>
#include <cstddef>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "rays_args.hpp"

namespace {
thread_local std::string g_thread_error;

// Expands node `idx` of `nodes` (evaluated at a texel derived from instruction `parent` by
// `xform`) into pre-order instructions; indices are relative to `first`.
uint32_t texel_emit(const std::vector<eray_texel_node>& nodes, uint32_t idx, uint32_t parent, uint32_t xform,
                    size_t first, std::vector<TexelInstr>& ins) {
    const eray_texel_node& nd = nodes[idx];
    const uint32_t k = (uint32_t)(ins.size() - first);
    TexelInstr t{};
    t.kind = nd.kind;
    t.w = nd.width;
    t.h = nd.height;
    t.parent = parent;
    t.xform = xform;
    for (int j = 0; j < 3; ++j) t.p[j] = nd.param[j];
    ins.push_back(t);
    if (ins.size() - first > kTexelMaxNodes) return k;  // the caller reports the size
    if (nd.kind == ERAY_TEXEL_RGB) {
        uint32_t c[3];
        for (int j = 0; j < 3; ++j) {
            int same = -1;  // rgb's inputs at the same node read the same pixel index: share
            for (int q = 0; q < j; ++q)
                if (nd.input[q] == nd.input[j]) same = q;
            c[j] = same >= 0 ? c[same] : texel_emit(nodes, (uint32_t)nd.input[j], k, kTexelIndex, first, ins);
        }
        for (int j = 0; j < 3; ++j) ins[first + k].c[j] = c[j];
    } else if (nd.kind == ERAY_TEXEL_MIX_COLOR) {
        const uint32_t l = texel_emit(nodes, (uint32_t)nd.input[0], k, kTexelMod, first, ins);
        const uint32_t r = texel_emit(nodes, (uint32_t)nd.input[1], k, kTexelMod, first, ins);
        ins[first + k].c[0] = l;
        ins[first + k].c[1] = r;
    }
    return k;
}
}  // namespace

int eray::gpu::set_error(eray_ctx* ctx, int code, const char* fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    if (ctx)
        ctx->err = buf;
    else
        g_thread_error = buf;
    return code;
}

namespace {

uint32_t sat_u32_host(float f) {
    if (!(f > 0.0f)) return 0u;
    if (f >= 4294967296.0f) return 0xffffffffu;
    return (uint32_t)f;
}

bool image_ok(const eray_image& im) { return !im.data || (im.width > 0 && im.height > 0); }
TexView tex(const eray_image& im) { return TexView{im.data, im.width, im.height}; }
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

        ctx->h_raw.assign((size_t)T * 24, 0.0f);
        size_t off = 0;
        for (auto& o : ctx->objects) {
            std::memcpy(&ctx->h_raw[off * 9], o.raw.data(), sizeof(float) * 9 * o.T);
            std::memcpy(&ctx->h_raw[(size_t)T * 9 + off * 9], o.raw.data() + 9 * (size_t)o.T,
                        sizeof(float) * 9 * o.T);
            std::memcpy(&ctx->h_raw[(size_t)T * 18 + off * 6], o.raw.data() + 18 * (size_t)o.T,
                        sizeof(float) * 6 * o.T);
            off += o.T;
        }
        if ((st = ctx->d_raw.ensure(ctx, (size_t)T * 24))) return st;
        if (T) {
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_raw, ctx->h_raw.data(), sizeof(float) * 24 * (size_t)T,
                                        hipMemcpyHostToDevice, ctx->stream));
            HIP_TRY(ctx, launch_tri_precompute(ctx->d_raw, ctx->d_raw + 9 * (size_t)T,
                                               ctx->d_raw + 18 * (size_t)T, T, ctx->d_hot,
                                               ctx->d_shade, ctx->stream));
        }
        ctx->geom_dirty = false;
        ctx->desc_dirty = true;
    }
    if (ctx->desc_dirty) {
        ctx->h_objs.clear();
        uint32_t begin = 0;
        ctx->spec_pow = false;
        ctx->example_mat = false;
        // texel programs: per object a header + its outputs' expression trees (48-B records)
        ctx->h_prog.clear();
        std::vector<size_t> prog_at(ctx->objects.size(), SIZE_MAX);
        for (size_t i = 0; i < ctx->objects.size(); ++i) {
            const HostObject& o = ctx->objects[i];
            if (o.tnodes.empty()) continue;
            std::vector<TexelInstr> ins;
            uint32_t head[kTexelHeaderWords] = {};
            for (int out = 0; out < 5; ++out) {
                const int32_t idx = o.tout[out];
                if (idx < 0 || texel_is_color(o.tnodes[idx].kind) != (out == 0)) continue;  // kept / None
                const size_t first = ins.size();
                texel_emit(o.tnodes, (uint32_t)idx, 0, kTexelMod, first, ins);
                if (ins.size() - first > kTexelMaxNodes)
                    return set_error(ctx, ERAY_E_UNSUPPORTED, "object %zu: output %d expands to more than %u texel nodes",
                                     i, out, kTexelMaxNodes);
                head[out] = (uint32_t)first;
                head[5 + out] = (uint32_t)(ins.size() - first);
            }
            prog_at[i] = ctx->h_prog.size();
            ctx->h_prog.insert(ctx->h_prog.end(), head, head + kTexelHeaderWords);
            const uint32_t* w = reinterpret_cast<const uint32_t*>(ins.data());
            ctx->h_prog.insert(ctx->h_prog.end(), w, w + ins.size() * (sizeof(TexelInstr) / 4));
        }
        if (!ctx->h_prog.empty()) {
            if ((st = ctx->d_prog.ensure(ctx, ctx->h_prog.size()))) return st;
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_prog, ctx->h_prog.data(), 4 * ctx->h_prog.size(), hipMemcpyHostToDevice,
                                        ctx->stream));
        }
        for (size_t i = 0; i < ctx->objects.size(); ++i) {
            const HostObject& o = ctx->objects[i];
            ObjectDesc d{};
            d.g.tri_begin = begin;
            d.g.tri_count = o.T;
            d.g.rect[0] = d.g.rect[2] = 0;  // every pixel until the culling pass computes it
            d.g.rect[1] = d.g.rect[3] = INT32_MAX;
            for (int k = 0; k < 3; ++k) {
                d.g.bb_lo[k] = o.lo[k];
                d.g.bb_hi[k] = o.hi[k];
            }
            d.mat = MaterialDesc{tex(o.mat.color), tex(o.mat.diffuse), tex(o.mat.specular),
                                 tex(o.mat.specular_power), tex(o.mat.reflection)};
            if (o.example) {
                d.mat.color = TexView{nullptr, 0, 0};
                d.mat.diffuse = TexView{nullptr, 0, 0};
                d.mat.example = 1;
                d.mat.ex_w = o.ex.width;
                d.mat.ex_h = o.ex.height;
                d.mat.ex_xf = o.ex.x_fac;
                d.mat.ex_yf = o.ex.y_fac;
                d.mat.ex_r = o.ex.r;
                d.mat.ex_g = o.ex.g;
                d.mat.ex_b = o.ex.b;
                d.mat.ex_factor = o.ex.factor;
            }
            if (prog_at[i] != SIZE_MAX) {  // graph outputs replace the textures (None: defaults)
                d.mat.prog = ctx->d_prog + prog_at[i];
                TexView* tv[5] = {&d.mat.color, &d.mat.diffuse, &d.mat.specular, &d.mat.specular_power,
                                  &d.mat.reflection};
                for (int out = 0; out < 5; ++out)
                    if (o.tout[out] >= 0) *tv[out] = TexView{nullptr, 0, 0};
                ctx->example_mat = true;
                if (o.tout[3] >= 0 && !texel_is_color(o.tnodes[o.tout[3]].kind)) ctx->spec_pow = true;
            }
            ctx->h_objs.push_back(d);
            ctx->spec_pow |= d.mat.specular_power.data != nullptr;
            ctx->example_mat |= d.mat.example != 0;
            begin += o.T;
        }
        ctx->h_lights.clear();
        for (auto& l : ctx->lights) {
            LightDesc d{};
            for (int k = 0; k < 3; ++k) {
                d.pos[k] = l.position[k];
                d.color[k] = l.color[k];
            }
            d.variant = l.variant;
            d.brightness = l.brightness;
            ctx->h_lights.push_back(d);
        }
        if ((st = ctx->d_objs.ensure(ctx, ctx->h_objs.size()))) return st;
        if ((st = ctx->d_lights.ensure(ctx, ctx->h_lights.size()))) return st;
        if (!ctx->h_objs.empty())
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_objs, ctx->h_objs.data(), sizeof(ObjectDesc) * ctx->h_objs.size(),
                                        hipMemcpyHostToDevice, ctx->stream));
        if (!ctx->h_lights.empty())
            HIP_TRY(ctx, hipMemcpyAsync(ctx->d_lights, ctx->h_lights.data(),
                                        sizeof(LightDesc) * ctx->h_lights.size(), hipMemcpyHostToDevice,
                                        ctx->stream));
        // setup.hip's object ranges and binned-object indices
        const uint32_t nobj = (uint32_t)ctx->objects.size();
        ctx->h_begin.assign(2 * (size_t)nobj + 1, 0u);
        uint32_t nb = 0;
        for (uint32_t i = 0; i < nobj; ++i) {
            ctx->h_begin[i] = ctx->h_objs[i].g.tri_begin;
            ctx->h_begin[nobj + 1 + i] = ctx->objects[i].T > kDirectMax ? nb++ : ~0u;
        }
        ctx->binned = nb;
        ctx->h_begin[nobj] = ctx->total_tris;
        if ((st = ctx->d_begin.ensure(ctx, ctx->h_begin.size()))) return st;
        HIP_TRY(ctx, hipMemcpyAsync(ctx->d_begin, ctx->h_begin.data(), 4 * ctx->h_begin.size(), hipMemcpyHostToDevice,
                                    ctx->stream));
        // rectangle accumulators + the setup's workgroup counter, zero between setups
        const size_t acc_words = 4 * (size_t)nobj + 1 + 10 * (size_t)kSetupMaxBlocks;
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
    const size_t T = ctx->total_tris;
    size_t begin = 0;
    for (auto& o : ctx->objects) {
        if (o.raw_stale && o.T) {
            const size_t n = o.T;
            HIP_TRY(ctx, hipMemcpy(o.raw.data(), ctx->d_raw + 9 * begin, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(o.raw.data() + 9 * n, ctx->d_raw + 9 * T + 9 * begin, sizeof(float) * 9 * n, hipMemcpyDeviceToHost));
            HIP_TRY(ctx, hipMemcpy(o.raw.data() + 18 * n, ctx->d_raw + 18 * T + 6 * begin, sizeof(float) * 6 * n, hipMemcpyDeviceToHost));
        }
        o.raw_stale = false;
        begin += o.T;
    }
    return ERAY_OK;
}

}  // namespace

extern "C" {

int eray_abi_version(void) { return ERAY_ABI_VERSION; }

int eray_ctx_create(int device, eray_ctx** out) {
    if (!out) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "out is null");
    *out = nullptr;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return set_error(nullptr, ERAY_E_HIP, "no HIP device available (%s)",
                         e == hipSuccess ? "0 devices" : hipGetErrorString(e));
    if (device < 0 || device >= count)
        return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "device %d out of range (%d devices)", device, count);
    eray_ctx* ctx = new (std::nothrow) eray_ctx();
    if (!ctx) return set_error(nullptr, ERAY_E_OUT_OF_MEMORY, "context allocation failed");
    ctx->device = device;
    e = hipSetDevice(device);
    if (e == hipSuccess) e = ctx->own_stream.create(hipStreamNonBlocking);
    ctx->stream = ctx->own_stream;
    // the separate fill kernel's stream and fork / join events (render.hip launch_frame_kernel);
    // low priority, so that it never shares a hardware queue with a caller's normal-priority
    // stream (the fill would then wait for the frame kernel it runs beside)
    if (e == hipSuccess) e = ctx->fill_stream.create(hipStreamNonBlocking, 1);
    if (e == hipSuccess) e = ctx->fill_fork.create(hipEventDisableTiming);
    if (e == hipSuccess) e = ctx->fill_join.create(hipEventDisableTiming);
    ctx->lc = LaunchCtx{ctx->fill_stream, ctx->fill_fork, ctx->fill_join};
    // the per-camera setup's device state and its pinned host copy
    if (e == hipSuccess) e = ctx->d_cam.alloc(1);
    if (e == hipSuccess) e = ctx->d_state.alloc(1);
    if (e == hipSuccess) e = hipMemset(ctx->d_state, 0, sizeof(CamState));
    if (e == hipSuccess) e = ctx->d_coll.alloc(kCollScratchBytes);

    if (e == hipSuccess) e = ctx->h_state.alloc(1);
    if (e == hipSuccess) std::memset(ctx->h_state, 0, sizeof(CamState));
    for (Event* ev : {&ctx->state_ev, &ctx->path_ev[0], &ctx->path_ev[1]})
        if (e == hipSuccess) e = ev->create(hipEventDisableTiming);
    if (e != hipSuccess) {
        delete ctx;
        return set_error(nullptr, ERAY_E_HIP, "context init: %s", hipGetErrorString(e));
    }
    *out = ctx;
    return ERAY_OK;
}

int eray_ctx_destroy(eray_ctx* ctx) {
    delete ctx;  // (~eray_ctx waits for its streams)
    return ERAY_OK;
}

const char* eray_last_error(const eray_ctx* ctx) {
    return ctx ? ctx->err.c_str() : g_thread_error.c_str();
}

int eray_set_stream(eray_ctx* ctx, void* stream) {
    if (int st = use_device(ctx)) return st;
    ctx->stream = (hipStream_t)stream;
    return ERAY_OK;
}

void* eray_get_stream(eray_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }

int eray_synchronize(eray_ctx* ctx) {
    if (int st = use_device(ctx)) return st;
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ERAY_OK;
}

int eray_device_alloc(eray_ctx* ctx, size_t bytes, void** dev_ptr) {
    if (int st = use_device(ctx)) return st;
    if (!dev_ptr) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "dev_ptr is null");
    HIP_TRY(ctx, hipMalloc(dev_ptr, bytes ? bytes : 1));
    return ERAY_OK;
}

int eray_device_free(eray_ctx* ctx, void* dev_ptr) {
    if (int st = use_device(ctx)) return st;
    if (!dev_ptr) return ERAY_OK;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, dev_ptr) == hipSuccess)  // (frames in it lose their source)
        untag_range(ctx, reinterpret_cast<uintptr_t>(base), size);
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    HIP_TRY(ctx, hipFree(dev_ptr));
    return ERAY_OK;
}

int eray_memset(eray_ctx* ctx, void* dev_ptr, int value, size_t bytes) {
    if (int st = use_device(ctx)) return st;
    if (!bytes) return ERAY_OK;
    if (!dev_ptr) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "dev_ptr is null");
    untag_range(ctx, reinterpret_cast<uintptr_t>(dev_ptr), bytes);
    HIP_TRY(ctx, hipMemsetAsync(dev_ptr, value, bytes, ctx->stream));
    return ERAY_OK;
}

int eray_copy_to_device(eray_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (int st = use_device(ctx)) return st;
    if (!bytes) return ERAY_OK;
    if (!dst || !src) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null pointer");
    untag_range(ctx, reinterpret_cast<uintptr_t>(dst), bytes);
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ERAY_OK;
}

int eray_copy_to_host(eray_ctx* ctx, void* dst, const void* src, size_t bytes) {
    if (int st = use_device(ctx)) return st;
    if (!bytes) return ERAY_OK;
    if (!dst || !src) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null pointer");
    HIP_TRY(ctx, hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, ctx->stream));
    HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
    return ERAY_OK;
}

// ------------------------------------------------------------------------ shaderlib ---------
int eray_node_wave(eray_ctx* ctx, uint32_t w, uint32_t h, float x_fac, float y_fac, float* out) {
    if (int st = use_device(ctx)) return st;
    if ((size_t)w * h && !out) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "wave: out is null");
    HIP_TRY(ctx, launch_wave(w, h, x_fac, y_fac, out, ctx->stream));
    return ERAY_OK;
}

int eray_node_rgb(eray_ctx* ctx, uint32_t w, uint32_t h, eray_image r, eray_image g, eray_image b,
                  float* out) {
    if (int st = use_device(ctx)) return st;
    const size_t n = (size_t)w * h;
    const eray_image* in[3] = {&r, &g, &b};
    const char* names[3] = {"red", "green", "blue"};
    for (int k = 0; k < 3; ++k) {
        if (!in[k]->data)
            return set_error(ctx, ERAY_E_MISSING, "rgb: missing input `%s`", names[k]);
        if ((size_t)in[k]->width * in[k]->height < n)
            return set_error(ctx, ERAY_E_OUT_OF_BOUNDS,
                             "rgb: input `%s` has %zu pixels, the %ux%u output indexes %zu",
                             names[k], (size_t)in[k]->width * in[k]->height, w, h, n);
    }
    if (n && !out) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "rgb: out is null");
    HIP_TRY(ctx, launch_rgb(w, h, r.data, g.data, b.data, out, ctx->stream));
    return ERAY_OK;
}

int eray_node_flat_color(eray_ctx* ctx, uint32_t w, uint32_t h, float r, float g, float b,
                         float* out) {
    if (int st = use_device(ctx)) return st;
    if ((size_t)w * h && !out) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "flat_color: out is null");
    HIP_TRY(ctx, launch_flat(w, h, r, g, b, out, ctx->stream));
    return ERAY_OK;
}

int eray_node_mix_color(eray_ctx* ctx, uint32_t w, uint32_t h, eray_image left, eray_image right,
                        float factor, float* out) {
    if (int st = use_device(ctx)) return st;
    if (!left.data) return set_error(ctx, ERAY_E_MISSING, "mix_color: missing input `left`");
    if (!right.data) return set_error(ctx, ERAY_E_MISSING, "mix_color: missing input `right`");
    const size_t n = (size_t)w * h;
    if (n && (!left.width || !left.height || !right.width || !right.height))
        return set_error(ctx, ERAY_E_OUT_OF_BOUNDS, "mix_color: empty input image (mod_get by 0)");
    if (n && !out) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "mix_color: out is null");
    HIP_TRY(ctx, launch_mix(w, h, tex(left), tex(right), factor, out, ctx->stream));
    return ERAY_OK;
}

int eray_material_example(eray_ctx* ctx, uint32_t w, uint32_t h, float x_fac, float y_fac, float r,
                          float g, float b, float factor, float* out_color, float* out_diffuse) {
    if (int st = use_device(ctx)) return st;
    HIP_TRY(ctx, launch_material_example(w, h, x_fac, y_fac, r, g, b, factor, out_color, out_diffuse,
                                         ctx->stream));
    return ERAY_OK;
}

// ------------------------------------------------------------------------ scene -------------
int eray_scene_reset(eray_ctx* ctx) {
    if (!ctx) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "null context");
    ctx->objects.clear();
    ctx->lights.clear();
    ctx->camera = eray_camera{{0.0f, 0.0f, 0.0f}, {60.0f, 60.0f}, 1024u, 1.0f};
    ctx->geom_dirty = ctx->desc_dirty = true;
    ctx->ray_accel.valid = false;
    ctx->ray_accel.scene_changed = true;
    ++ctx->ray_accel.gen;
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
    if (index >= ctx->objects.size())
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "object %u out of range (%zu objects)", index,
                         ctx->objects.size());
    if (!m->width || !m->height)  // Image::mod_get by 0 panics (image.rs:36-38)
        return set_error(ctx, ERAY_E_OUT_OF_BOUNDS, "example material of zero width or height");
    ctx->objects[index].example = true;
    ctx->objects[index].ex = *m;
    ctx->desc_dirty = true;
    return ERAY_OK;
}

int eray_scene_set_object_texel_graph(eray_ctx* ctx, uint32_t index, const eray_texel_graph* g) {
    if (!ctx) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null context");
    if (index >= ctx->objects.size())
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "object %u out of range (%zu objects)", index,
                         ctx->objects.size());
    HostObject& o = ctx->objects[index];
    if (!g) {
        o.tnodes.clear();
        std::fill(o.tout, o.tout + 5, -1);
        ctx->desc_dirty = true;
        return ERAY_OK;
    }
    if (g->count && !g->nodes) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "nodes is null");
    for (uint32_t i = 0; i < g->count; ++i) {
        const eray_texel_node& n = g->nodes[i];
        if (n.kind > ERAY_TEXEL_MIX_COLOR) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "node %u: kind %u", i, n.kind);
        // every image a Material::get lookup can reach is indexed by mod_get or by pixel index:
        // a zero-sized one panics there (image.rs:36-38)
        if (!n.width || !n.height)
            return set_error(ctx, ERAY_E_OUT_OF_BOUNDS, "node %u: zero width or height", i);
        const int inputs = n.kind == ERAY_TEXEL_RGB ? 3 : n.kind == ERAY_TEXEL_MIX_COLOR ? 2 : 0;
        for (int j = 0; j < inputs; ++j) {
            const int32_t in = n.input[j];
            if (in < 0 || (uint32_t)in >= i)  // unconnected (MissingMany) or not an earlier node
                return set_error(ctx, ERAY_E_MISSING_MANY, "node %u: input %d is not an earlier node", i, j);
            const eray_texel_node& src = g->nodes[in];
            // rgb takes IValue images, mix_color IColor ones (get_sv!, shader.rs:140-178)
            if (texel_is_color(src.kind) != (n.kind == ERAY_TEXEL_MIX_COLOR))
                return set_error(ctx, ERAY_E_INVALID_TYPE, "node %u: input %d has the wrong image type", i, j);
            // rgb reads pixels[y * width + x] of each input (rgb.rs:89-95): it panics past the end
            if (n.kind == ERAY_TEXEL_RGB && (uint64_t)src.width * src.height < (uint64_t)n.width * n.height)
                return set_error(ctx, ERAY_E_OUT_OF_BOUNDS, "node %u: input %d has fewer pixels than the node", i, j);
        }
    }
    const int32_t outs[5] = {g->color, g->diffuse, g->specular, g->specular_power, g->reflection};
    for (int k = 0; k < 5; ++k)
        if (outs[k] < -1 || outs[k] >= (int32_t)g->count)
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "output %d: node %d out of range", k, outs[k]);
    o.tnodes.assign(g->nodes, g->nodes + g->count);
    std::copy(outs, outs + 5, o.tout);
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
    h.raw.resize((size_t)T * 24);
    if (T) {
        std::memcpy(h.raw.data(), obj->positions, sizeof(float) * 9 * (size_t)T);
        std::memcpy(h.raw.data() + 9 * (size_t)T, obj->normals, sizeof(float) * 9 * (size_t)T);
        std::memcpy(h.raw.data() + 18 * (size_t)T, obj->uvs, sizeof(float) * 6 * (size_t)T);
    }
    for (int k = 0; k < 3; ++k) {
        h.lo[k] = obj->bbox_min[k];
        h.hi[k] = obj->bbox_max[k];
    }
    h.mat = m;
    ctx->objects.push_back(std::move(h));
    if (index) *index = (uint32_t)(ctx->objects.size() - 1);
    ctx->geom_dirty = ctx->desc_dirty = true;
    ctx->ray_accel.valid = false;
    ctx->ray_accel.scene_changed = true;
    ++ctx->ray_accel.gen;
    return ERAY_OK;
}

// The face count of an object of the scene (what eray_object_update::triangle_count must name).
int eray_scene_object_triangle_count(eray_ctx* ctx, uint32_t index, uint32_t* count) {
    if (!ctx || !count) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null argument");
    if (index >= ctx->objects.size())
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "object %u out of range (%zu objects)", index, ctx->objects.size());
    *count = ctx->objects[index].T;
    return ERAY_OK;
}

}  // extern "C"

namespace {
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
    const size_t T = o.T, total = ctx->total_tris;
    size_t begin = 0;
    for (uint32_t i = 0; i < index; ++i) begin += ctx->objects[i].T;
    const bool device = (up->flags & ERAY_UPDATE_DEVICE) != 0;
    if (T && (up->positions || up->normals || up->uvs)) {
        const float *dp = up->positions, *dn = up->normals, *du = up->uvs;
        DeviceBuf<float> staged;  // host arrays: uploaded here, read by the kernel, released after a wait
        if (!device) {
            const size_t np = dp ? 9 * T : 0, nn = dn ? 9 * T : 0, nu = du ? 6 * T : 0;
            HIP_TRY(ctx, staged.alloc(np + nn + nu));
            if (dp) HIP_TRY(ctx, hipMemcpyAsync(staged, dp, sizeof(float) * np, hipMemcpyHostToDevice, ctx->stream));
            if (dn) HIP_TRY(ctx, hipMemcpyAsync(staged + np, dn, sizeof(float) * nn, hipMemcpyHostToDevice, ctx->stream));
            if (du) HIP_TRY(ctx, hipMemcpyAsync(staged + np + nn, du, sizeof(float) * nu, hipMemcpyHostToDevice, ctx->stream));
            if (dp) dp = staged;
            if (dn) dn = staged + np;
            if (du) du = staged + np + nn;
        }
        if (int st = order_after_side_streams(ctx)) return st;
        HIP_TRY(ctx, launch_tri_update(dp, dn, du, (uint32_t)T, ctx->d_raw + 9 * begin, ctx->d_raw + 9 * total + 9 * begin,
                                       ctx->d_raw + 18 * total + 6 * begin, ctx->d_hot + begin, ctx->d_shade + begin,
                                       ctx->stream));
        if (device) {
            o.raw_stale = true;
        } else {
            HIP_TRY(ctx, hipStreamSynchronize(ctx->stream));
            // the host copy follows the records once they are written (a failure above leaves both as they were)
            if (up->positions) std::memcpy(o.raw.data(), up->positions, sizeof(float) * 9 * T);
            if (up->normals) std::memcpy(o.raw.data() + 9 * T, up->normals, sizeof(float) * 9 * T);
            if (up->uvs) std::memcpy(o.raw.data() + 18 * T, up->uvs, sizeof(float) * 6 * T);
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

int eray_camera_size(const eray_camera* c, uint32_t* w, uint32_t* h) {
    if (!c || !w || !h) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "null argument");
    *w = c->width;
    *h = sat_u32_host((float)c->width / (c->fov[0] / c->fov[1]));
    return ERAY_OK;
}

int eray_pack_ppm(eray_ctx* ctx, const float* rgb, uint32_t w, uint32_t h, uint8_t* out) {
    if (int st = use_device(ctx)) return st;
    if ((size_t)w * h && (!rgb || !out)) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "null pointer");
    untag_range(ctx, reinterpret_cast<uintptr_t>(out), (size_t)w * h * 3u);
    HIP_TRY(ctx, launch_pack_ppm(rgb, w, h, out, ctx->stream));
    return ERAY_OK;
}

int eray_ppm_header(uint32_t w, uint32_t h, char* buf, size_t cap, size_t* len) {
    char tmp[64];
    int n = std::snprintf(tmp, sizeof tmp, "P6 %u %u %u\n", w, h, 255u);
    if (n < 0) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "format failed");
    if (len) *len = (size_t)n;
    if (buf) {
        if (cap < (size_t)n + 1) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "buffer too small");
        std::memcpy(buf, tmp, (size_t)n + 1);
    }
    return ERAY_OK;
}

}  // extern "C"

// Error reporting for objload.cpp, which is HIP-free and cannot see ctx.hpp.
int eray_internal_error(eray_ctx* ctx, int code, const char* msg) { return set_error(ctx, code, "%s", msg); }

// Diagnostics (not part of include/eray_hip.h): the screen bins of object `index` as built for
// the last setup — out[0] bins, out[1] entries, out[2] (face, pixel) pairs (mask bits),
// out[3] most entries in one bin, out[4] non-empty bins, out[5] most pairs in one bin,
// out[6..9] the object's pixel rectangle (x0, x1, y0, y1; int32 as uint64), out[10] the bin with
// the most entries, out[11] / out[12] the bins of more than 64 / kTraceHeavyMin entries, out[13]
// the units the pair pass walked: the faces' bin-rectangle rows (segments) or their (face, bin)
// pairs (the tracer's setups, eray_debug_set_bin_form) (out: 14 words).  Synchronises.
extern "C" int eray_debug_bin_stats(eray_ctx* ctx, uint32_t index, uint64_t* out) {
    if (!ctx || !out || index >= ctx->objects.size() || ctx->objects[index].T <= kDirectMax || !ctx->bins.start)
        return ERAY_E_INVALID_ARGUMENT;
    const BinBuffers& b = ctx->bins;
    const uint32_t k = binned_before(ctx, index);
    std::vector<uint32_t> start(b.nbins + 1);
    ObjectDesc d{};
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(start.data(), b.start + (size_t)k * b.nbins, start.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&d, ctx->d_objs + index, sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin stats copy failed");
    const size_t n = start[b.nbins] - start[0];
    std::vector<unsigned long long> mask(n);  // the entries' masks (a strided copy out of the 64-B entries)
    if (n && hipMemcpy2D(mask.data(), 8, reinterpret_cast<const char*>(b.ent + start[0]) + offsetof(BinEntry, mask),
                         sizeof(BinEntry), 8, n, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin stats copy failed");
    uint64_t pairs = 0, most = 0, nonempty = 0, most_pairs = 0, most_at = 0, over64 = 0, over192 = 0;
    for (size_t i = 0; i < b.nbins; ++i) {
        const uint64_t e = start[i + 1] - start[i];
        over64 += e > 64;
        over192 += e > kTraceHeavyMin;
        if (e > most) most_at = i;
        most = e > most ? e : most;
        nonempty += e != 0;
        uint64_t pb = 0;
        for (uint32_t j = start[i]; j < start[i + 1]; ++j) pb += (uint64_t)__builtin_popcountll(mask[j - start[0]]);
        pairs += pb;
        most_pairs = pb > most_pairs ? pb : most_pairs;
    }
    out[0] = b.nbins;
    out[1] = n;
    out[2] = pairs;
    out[3] = most;
    out[4] = nonempty;
    out[5] = most_pairs;
    for (int q = 0; q < 4; ++q) out[6 + q] = (uint64_t)(int64_t)d.g.rect[q];
    out[10] = most_at;
    out[11] = over64;
    out[12] = over192;
    // out[13]: the units of the faces' bin rectangles (every object)
    unsigned long long pairs_all = 0;
    if (hipMemcpy(&pairs_all, b.boff + setup_blocks(ctx->total_tris), sizeof pairs_all, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin stats copy failed");
    out[13] = pairs_all;
    return ERAY_OK;
}

// Diagnostics: the entries of bin `bin` of object `index` in bin order (faces relative to the
// object, pixel masks, pad words: a sorted bin's later-chunk mask unions, BinEntry), at most
// `cap`; *n = the bin's entry count; `pad` may be null.  Synchronises.
extern "C" int eray_debug_bin_entries(eray_ctx* ctx, uint32_t index, uint32_t bin, uint32_t* tri, uint64_t* mask,
                                      uint32_t* pad, uint32_t cap, uint32_t* n) {
    if (!ctx || !n || index >= ctx->objects.size() || ctx->objects[index].T <= kDirectMax || !ctx->bins.start ||
        bin >= ctx->bins.nbins)
        return ERAY_E_INVALID_ARGUMENT;
    const BinBuffers& b = ctx->bins;
    const uint32_t k = binned_before(ctx, index);
    uint32_t se[2];
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(se, b.start + (size_t)k * b.nbins + bin, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin dump copy failed");
    *n = se[1] - se[0];
    const uint32_t m = std::min(*n, cap);
    std::vector<BinEntry> ent(m);
    if (m && hipMemcpy(ent.data(), b.ent + se[0], sizeof(BinEntry) * (size_t)m, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin dump copy failed");
    for (uint32_t i = 0; i < m; ++i) {
        tri[i] = ent[i].tri;
        mask[i] = ent[i].mask;
        if (pad) pad[i] = ent[i].pad;
    }
    return ERAY_OK;
}

// Diagnostics: eray_debug_bin_entries without the pad words.
extern "C" int eray_debug_bin_dump(eray_ctx* ctx, uint32_t index, uint32_t bin, uint32_t* tri, uint64_t* mask,
                                   uint32_t cap, uint32_t* n) {
    return eray_debug_bin_entries(ctx, index, bin, tri, mask, nullptr, cap, n);
}

// Diagnostics: the entry count of every bin of object `index` (bins.nbins of them, row-major over
// the camera's bin rows, at most `cap`); *nbins = the object's bin count.  Synchronises.
extern "C" int eray_debug_bin_counts(eray_ctx* ctx, uint32_t index, uint32_t* counts, uint32_t cap, uint32_t* nbins) {
    if (!ctx || !nbins || index >= ctx->objects.size() || ctx->objects[index].T <= kDirectMax || !ctx->bins.start)
        return ERAY_E_INVALID_ARGUMENT;
    const BinBuffers& b = ctx->bins;
    const uint32_t k = binned_before(ctx, index);
    *nbins = b.nbins;
    const uint32_t m = std::min(b.nbins, cap);
    std::vector<uint32_t> st((size_t)m + 1);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        (m && hipMemcpy(st.data(), b.start + (size_t)k * b.nbins, sizeof(uint32_t) * ((size_t)m + 1),
                        hipMemcpyDeviceToHost) != hipSuccess))
        return set_error(ctx, ERAY_E_HIP, "bin counts copy failed");
    for (uint32_t i = 0; i < m; ++i) counts[i] = st[i + 1] - st[i];
    return ERAY_OK;
}

// Diagnostics (not part of include/eray_hip.h): the screen bins' entry capacity.  Setting it
// reallocates the bins at the next setup; a setup whose entries exceed it renders its binned
// objects through LDS tiles and the capacity grows once the host sees the count (tests).
extern "C" int eray_debug_set_bin_capacity(eray_ctx* ctx, uint64_t entries) {
    if (!ctx || !entries) return ERAY_E_INVALID_ARGUMENT;
    ctx->bin_cap = std::min((size_t)entries, kMaxBinEntries);
    ctx->setup_key.clear();
    return ERAY_OK;
}

extern "C" uint64_t eray_debug_bin_capacity(const eray_ctx* ctx) { return ctx ? (uint64_t)ctx->bins.cap : 0u; }
// Diagnostics: the frame setups' pair pass walks every (face, bin) pair of the faces' bin
// rectangles (rect_pairs != 0) instead of the rectangles' rows (bins.hip bin_segments_kernel);
// the next setup rebuilds the bins (tests compare the two forms' entries).
extern "C" int eray_debug_set_bin_form(eray_ctx* ctx, int rect_pairs) {
    if (!ctx) return ERAY_E_INVALID_ARGUMENT;
    ctx->rect_pairs = rect_pairs != 0;
    ctx->setup_key.clear();
    ctx->mc_layout.clear();
    return ERAY_OK;
}
// Diagnostics: the last setup's device state (CamState, 192 B) and object `index`'s pixel
// rectangle as the frame kernel reads them (synchronises).
extern "C" int eray_debug_setup_state(eray_ctx* ctx, uint32_t index, void* state_out, int32_t* rect_out) {
    if (!ctx || !state_out || !rect_out || index >= ctx->objects.size()) return ERAY_E_INVALID_ARGUMENT;
    ObjectDesc d{};
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(state_out, ctx->d_state, sizeof(CamState), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&d, ctx->d_objs + index, sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "setup state copy failed");
    std::memcpy(rect_out, d.g.rect, sizeof d.g.rect);
    return ERAY_OK;
}
