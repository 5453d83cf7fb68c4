// Stand-alone checker of eray_rays_reach_light's argument validation (check_reach_params in
// eray_amd/csrc/rays_args.hpp, the function capi_rays.cpp calls), meant for the host sanitizers and a
// machine without a GPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       -Iinclude tests/cpp/reach_args_main.cpp -Leray_amd/lib -leray_hip \
//       -Wl,-rpath,$PWD/eray_amd/lib -Wl,-rpath,/opt/rocm/lib -o /tmp/reach_args && /tmp/reach_args
//
// Every refusal (NULL params, unknown flags, reserved != 0, NULL rays / targets / out with
// count > 0) and the accepted cases (both flags, count == 0 with NULL pointers, a huge count) —
// none of which may read through a pointer — then the entry itself with no context (an error, not
// a crash) and, where no GPU is present, eray_ctx_create's ERAY_E_HIP.
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
    using eray::check_reach_params;
    static_assert(sizeof(eray_reach_params) == 40, "eray_reach_params is 40 B");
    const char* why = nullptr;
    // pointers that must never be dereferenced by the validation: one past nothing
    const eray_ray* rays = reinterpret_cast<const eray_ray*>(uintptr_t(0x1000));
    const float* targets = reinterpret_cast<const float*>(uintptr_t(0x2000));
    uint32_t* out = reinterpret_cast<uint32_t*>(uintptr_t(0x3000));
    auto params = [&] {
        eray_reach_params p;
        std::memset(&p, 0, sizeof p);
        p.rays = rays;
        p.targets = targets;
        p.count = 4;
        p.out = out;
        return p;
    };
    CHECK(check_reach_params(nullptr, &why) == ERAY_E_INVALID_ARGUMENT && why && *why);
    CHECK(check_reach_params(nullptr, nullptr) == ERAY_E_INVALID_ARGUMENT);
    eray_reach_params p = params();
    CHECK(check_reach_params(&p, &why) == ERAY_OK && why && !*why);
    CHECK(check_reach_params(&p, nullptr) == ERAY_OK);
    for (uint32_t flags : {ERAY_RAYS_NORMALIZE, ERAY_RAYS_BRUTE_FORCE, ERAY_RAYS_NORMALIZE | ERAY_RAYS_BRUTE_FORCE}) {
        p.flags = flags;
        CHECK(check_reach_params(&p, &why) == ERAY_OK);
    }
    for (uint32_t flags : {4u, 7u, 0x80000000u, 0xffffffffu}) {
        p.flags = flags;
        CHECK(check_reach_params(&p, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // unknown flags
    }
    p = params();
    for (uint32_t reserved : {1u, 0xffffffffu}) {
        p.reserved = reserved;
        CHECK(check_reach_params(&p, &why) == ERAY_E_INVALID_ARGUMENT && *why);
    }
    p = params();
    p.rays = nullptr;
    CHECK(check_reach_params(&p, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // NULL rays
    p = params();
    p.targets = nullptr;
    CHECK(check_reach_params(&p, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // NULL targets
    p = params();
    p.out = nullptr;
    CHECK(check_reach_params(&p, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // NULL out
    std::memset(&p, 0, sizeof p);
    CHECK(check_reach_params(&p, &why) == ERAY_OK);  // count == 0: nothing to launch, NULLs are fine
    p.reserved = 1;
    CHECK(check_reach_params(&p, &why) == ERAY_E_INVALID_ARGUMENT);  // (still checked with count == 0)
    p = params();
    p.count = ~0ull;
    CHECK(check_reach_params(&p, &why) == ERAY_OK);

    // the entry point itself: no context is an error with a message, whatever the parameters
    p = params();
    CHECK(eray_rays_reach_light(nullptr, &p) == ERAY_E_INVALID_ARGUMENT);
    CHECK(eray_rays_reach_light(nullptr, nullptr) == ERAY_E_INVALID_ARGUMENT);
    CHECK(std::strlen(eray_last_error(nullptr)) > 0);
    eray_ctx* ctx = nullptr;
    const int st = eray_ctx_create(0, &ctx);
    if (st == ERAY_OK) {  // a GPU is present: the same validation through the context
        p = params();
        p.reserved = 1;
        CHECK(eray_rays_reach_light(ctx, &p) == ERAY_E_INVALID_ARGUMENT);
        CHECK(eray_rays_reach_light(ctx, nullptr) == ERAY_E_INVALID_ARGUMENT);
        std::memset(&p, 0, sizeof p);
        CHECK(eray_rays_reach_light(ctx, &p) == ERAY_OK);
        eray_ctx_destroy(ctx);
    } else {
        CHECK(st == ERAY_E_HIP && ctx == nullptr);  // no GPU: loudly, never a CPU path
    }
    std::printf("reach_args: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
