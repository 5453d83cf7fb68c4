// Stand-alone checker of eray_scene_update_object's argument validation (check_update_params in
// eray_amd/csrc/rays_args.hpp, the function capi_scene.cpp calls): plain host code, no library to link,
// meant for the host sanitizers and a machine without a GPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined \
//       tests/cpp/update_args_main.cpp -o /tmp/update_args && /tmp/update_args
//
// Every refusal (NULL update, an index that is not an object, a triangle_count that is not the
// object's, unknown flags, nothing to update) and the accepted forms (each array alone, all three,
// host and device pointers, the box alone, the box with arrays, an object of no faces) — none of
// which may read through an array pointer — and the struct's documented offsets.
#include <cstddef>
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
    using eray::check_update_params;
    static_assert(sizeof(eray_object_update) == 56, "eray_object_update is 56 B");
    static_assert(offsetof(eray_object_update, positions) == 0 && offsetof(eray_object_update, normals) == 8 &&
                      offsetof(eray_object_update, uvs) == 16 && offsetof(eray_object_update, triangle_count) == 24 &&
                      offsetof(eray_object_update, flags) == 28 && offsetof(eray_object_update, bbox_min) == 32 &&
                      offsetof(eray_object_update, bbox_max) == 44,
                  "the offsets include/eray_hip.h documents");
    static_assert(sizeof(eray_ray_accel_refit_info) == 56 && offsetof(eray_ray_accel_refit_info, refitted) == 48 &&
                      offsetof(eray_ray_accel_refit_info, rebuilt) == 52,
                  "eray_ray_accel_refit_info as documented");
    const char* why = nullptr;
    // pointers that must never be dereferenced by the validation
    const float* pos = reinterpret_cast<const float*>(uintptr_t(0x1000));
    const float* nrm = reinterpret_cast<const float*>(uintptr_t(0x2000));
    const float* uv = reinterpret_cast<const float*>(uintptr_t(0x3000));
    const size_t nobj = 3;
    const uint32_t T = 300;  // the faces of object 1
    auto update = [&] {
        eray_object_update u;
        std::memset(&u, 0, sizeof u);
        u.positions = pos;
        u.normals = nrm;
        u.uvs = uv;
        u.triangle_count = T;
        return u;
    };
    // refusals
    CHECK(check_update_params(nullptr, 1, nobj, T, &why) == ERAY_E_INVALID_ARGUMENT && why && *why);
    CHECK(check_update_params(nullptr, 1, nobj, T, nullptr) == ERAY_E_INVALID_ARGUMENT);
    eray_object_update u = update();
    for (uint32_t index : {3u, 4u, 0x7fffffffu, 0xffffffffu})
        CHECK(check_update_params(&u, index, nobj, T, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // not an object
    CHECK(check_update_params(&u, 0, 0, 0, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // an empty scene
    for (uint32_t count : {0u, T - 1, T + 1, 0xffffffffu}) {
        u.triangle_count = count;
        CHECK(check_update_params(&u, 1, nobj, T, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // not the object's count
    }
    u = update();
    for (uint32_t flags : {4u, 5u, 7u, 0x80000000u, 0xffffffffu}) {
        u.flags = flags;
        CHECK(check_update_params(&u, 1, nobj, T, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // unknown flags
    }
    u = update();
    u.positions = u.normals = u.uvs = nullptr;
    for (uint32_t flags : {0u, ERAY_UPDATE_DEVICE}) {
        u.flags = flags;
        CHECK(check_update_params(&u, 1, nobj, T, &why) == ERAY_E_INVALID_ARGUMENT && *why);  // nothing to update
    }
    // accepted forms
    u = update();
    CHECK(check_update_params(&u, 1, nobj, T, &why) == ERAY_OK && why && !*why);
    CHECK(check_update_params(&u, 1, nobj, T, nullptr) == ERAY_OK);
    for (uint32_t flags : {0u, ERAY_UPDATE_DEVICE, ERAY_UPDATE_BBOX, ERAY_UPDATE_DEVICE | ERAY_UPDATE_BBOX}) {
        for (int keep = 0; keep < 7; ++keep) {  // every subset of the arrays but the empty one
            u = update();
            u.flags = flags;
            if (keep & 1) u.positions = nullptr;
            if (keep & 2) u.normals = nullptr;
            if (keep & 4) u.uvs = nullptr;
            CHECK(check_update_params(&u, 1, nobj, T, &why) == ERAY_OK && !*why);
        }
    }
    u = update();
    u.positions = u.normals = u.uvs = nullptr;
    for (uint32_t flags : {ERAY_UPDATE_BBOX, ERAY_UPDATE_BBOX | ERAY_UPDATE_DEVICE}) {
        u.flags = flags;
        CHECK(check_update_params(&u, 1, nobj, T, &why) == ERAY_OK);  // the box alone
    }
    u = update();
    u.triangle_count = 0;
    CHECK(check_update_params(&u, 2, nobj, 0, &why) == ERAY_OK);  // an object of no faces
    u.triangle_count = 0xffffffffu;
    CHECK(check_update_params(&u, 0, 1, 0xffffffffu, &why) == ERAY_OK);
    std::printf("update_args: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
