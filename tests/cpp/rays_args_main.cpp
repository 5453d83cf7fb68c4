// Stand-alone checker of eray_cast_rays' argument validation (eray_amd/csrc/rays_args.hpp, the
// function capi_rays.cpp calls), meant for the host sanitizers and a machine without a GPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude tests/cpp/rays_args_main.cpp -Leray_amd/lib -leray_hip \
//       -Wl,-rpath,$PWD/eray_amd/lib -Wl,-rpath,/opt/rocm/lib -o /tmp/rays_args && /tmp/rays_args
//
// NULL pointers, count == 0, object indices, flags, bounces, alignment — none of which may read
// through a pointer — then the entry itself with no context (an error, not a crash) and, where no
// GPU is present, eray_ctx_create's ERAY_E_HIP.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../../eray_amd/csrc/rays_args.hpp"

static int g_failed = 0;
#define CHECK(cond)                                                                       \
    do {                                                                                  \
        if (!(cond)) {                                                                    \
            std::fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                                   \
        }                                                                                 \
    } while (0)

int main() {
    using eray::check_rays_params;
    const char* why = nullptr;
    // pointers that must never be dereferenced by the validation: one past nothing
    const eray_ray* rays = reinterpret_cast<const eray_ray*>(uintptr_t(0x1000));
    eray_ray_hit* hit = reinterpret_cast<eray_ray_hit*>(uintptr_t(0x2000));
    float* rgb = reinterpret_cast<float*>(uintptr_t(0x3000));
    auto params = [&] {
        eray_rays_params p;
        std::memset(&p, 0, sizeof p);
        p.rays = rays;
        p.count = 4;
        p.object = -1;
        p.out_hit = hit;
        return p;
    };
    CHECK(check_rays_params(nullptr, 1, &why) == ERAY_E_INVALID_ARGUMENT && why && *why);
    CHECK(check_rays_params(nullptr, 1, nullptr) == ERAY_E_INVALID_ARGUMENT);
    eray_rays_params p = params();
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK && why && !*why);
    CHECK(check_rays_params(&p, 0, &why) == ERAY_OK);  // an empty scene: every ray a miss
    p.count = 0;
    p.rays = nullptr;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK);  // nothing to launch
    p.count = 1;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_INVALID_ARGUMENT);  // NULL rays
    p = params();
    p.out_hit = nullptr;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_INVALID_ARGUMENT);  // both outputs NULL
    p.out_rgb = rgb;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK);  // only out_rgb
    p.object = 0;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_INVALID_ARGUMENT);  // out_rgb with one object
    p = params();
    for (int32_t object : {1, 2, 0x7fffffff, -2, (int32_t)0x80000000}) {
        p.object = object;
        CHECK(check_rays_params(&p, 1, &why) == ERAY_E_INVALID_ARGUMENT);
    }
    p.object = 0;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK);
    CHECK(check_rays_params(&p, 0, &why) == ERAY_E_INVALID_ARGUMENT);
    p = params();
    p.bounces = 16;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK);
    p.bounces = 17;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_UNSUPPORTED);
    p.bounces = 0xffffffffu;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_UNSUPPORTED);
    p = params();
    p.flags = ERAY_RAYS_NORMALIZE | ERAY_RAYS_BRUTE_FORCE;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK);
    p.flags = 4u;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_INVALID_ARGUMENT);
    p = params();
    p.out_hit = reinterpret_cast<eray_ray_hit*>(uintptr_t(0x2004));
    CHECK(check_rays_params(&p, 1, &why) == ERAY_E_INVALID_ARGUMENT);  // 16-byte stores
    p.count = ~0ull;
    p.out_hit = hit;
    CHECK(check_rays_params(&p, 1, &why) == ERAY_OK);

    // the entry point itself: no context is an error with a message, whatever the parameters
    p = params();
    CHECK(eray_cast_rays(nullptr, &p) == ERAY_E_INVALID_ARGUMENT);
    CHECK(eray_cast_rays(nullptr, nullptr) == ERAY_E_INVALID_ARGUMENT);
    CHECK(std::strlen(eray_last_error(nullptr)) > 0);
    eray_ctx* ctx = nullptr;
    const int st = eray_ctx_create(0, &ctx);
    if (st == ERAY_OK) {  // a GPU is present: the same validation through the context
        p = params();
        p.object = 5;
        CHECK(eray_cast_rays(ctx, &p) == ERAY_E_INVALID_ARGUMENT);
        p = params();
        p.count = 0;
        CHECK(eray_cast_rays(ctx, &p) == ERAY_OK);
        eray_ctx_destroy(ctx);
    } else {
        CHECK(st == ERAY_E_HIP && ctx == nullptr);  // no GPU: loudly, never a CPU path
    }
    std::printf("rays_args: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
