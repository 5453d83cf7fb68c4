// capi.cpp — implementation of include/eray_hip.h: context, error text, stream and device memory,
// the shaderlib node entry points, Camera::size, PPM packing and eray_internal_error.  The scene
// calls and the scene's upload are capi_scene.cpp; the frame path capi_setup.cpp (camera setup, bins,
// frame tags) and capi_frames.cpp (the eray_render* and eray_time_* entry points); the ray queries
// and their hierarchy capi_rays.cpp; the eray_debug_* hooks of the setup capi_debug.cpp — all on
// the same context, ctx.hpp.  Host code only; the kernels live in render.hip and shaderlib.hip.
//
// Error policy: every HIP call is checked; failures and every case where the reference would
// panic become a status code plus a message (eray_last_error).  Nothing here falls back to a
// CPU path: without a usable GPU the calls fail loudly.
#include <hip/hip_runtime.h>

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <new>
#include <string>

#include "ctx.hpp"
#include "device_math.hpp"

namespace {
thread_local std::string g_thread_error;
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
TexView tex(const eray_image& im) { return TexView{im.data, im.width, im.height}; }
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

int eray_camera_size(const eray_camera* c, uint32_t* w, uint32_t* h) {
    if (!c || !w || !h) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "null argument");
    *w = c->width;
    *h = eray::dev::sat_u32((float)c->width / (c->fov[0] / c->fov[1]));
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
