// rays_args.hpp — eray_cast_rays', eray_rays_reach_light's and eray_scene_update_object's argument
// validation (include/eray_hip.h states the rules): plain host code with no HIP call, so the C-ABI
// layer (capi_rays.cpp; the update: capi_scene.cpp) and the stand-alone checkers (tests/cpp/rays_args_main.cpp, tests/cpp/reach_args_main.cpp,
// tests/cpp/update_args_main.cpp, built with the host sanitizers) share it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "../../include/eray_hip.h"

namespace eray {

constexpr uint32_t kRaysMaxBounces = 16;  // (= gpu::kMaxBounces: the walk's frames)

// ERAY_OK when `rp` can be enqueued against a scene of `nobj` objects (count == 0 included: the
// caller then launches nothing), else the status eray_cast_rays returns and *why (a literal).
inline int check_rays_params(const eray_rays_params* rp, size_t nobj, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!rp) return *why = "params is null", ERAY_E_INVALID_ARGUMENT;
    if (rp->flags & ~(ERAY_RAYS_NORMALIZE | ERAY_RAYS_BRUTE_FORCE)) return *why = "unknown ray flags", ERAY_E_INVALID_ARGUMENT;
    if (rp->bounces > kRaysMaxBounces) return *why = "bounces: at most 16 reflection levels", ERAY_E_UNSUPPORTED;
    if (!rp->out_hit && !rp->out_rgb) return *why = "out_hit and out_rgb are both null", ERAY_E_INVALID_ARGUMENT;
    if (rp->out_rgb && rp->object >= 0)
        return *why = "out_rgb needs object == -1 (cast_ray has no single-object form)", ERAY_E_INVALID_ARGUMENT;
    if (rp->object < -1 || (rp->object >= 0 && (size_t)rp->object >= nobj))
        return *why = "object is neither -1 nor an object of the scene", ERAY_E_INVALID_ARGUMENT;
    if (rp->count && !rp->rays) return *why = "rays is null", ERAY_E_INVALID_ARGUMENT;
    if (reinterpret_cast<uintptr_t>(rp->out_hit) & 15u) return *why = "out_hit is not 16-byte aligned", ERAY_E_INVALID_ARGUMENT;
    return ERAY_OK;
}

// The same for eray_rays_reach_light: ERAY_OK when `rp` can be enqueued (count == 0 included).
inline int check_reach_params(const eray_reach_params* rp, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!rp) return *why = "params is null", ERAY_E_INVALID_ARGUMENT;
    if (rp->flags & ~(ERAY_RAYS_NORMALIZE | ERAY_RAYS_BRUTE_FORCE)) return *why = "unknown ray flags", ERAY_E_INVALID_ARGUMENT;
    if (rp->reserved) return *why = "reserved is not 0", ERAY_E_INVALID_ARGUMENT;
    if (rp->count && !rp->rays) return *why = "rays is null", ERAY_E_INVALID_ARGUMENT;
    if (rp->count && !rp->targets) return *why = "targets is null", ERAY_E_INVALID_ARGUMENT;
    if (rp->count && !rp->out) return *why = "out is null", ERAY_E_INVALID_ARGUMENT;
    return ERAY_OK;
}

// The same for eray_scene_update_object against a scene of `nobj` objects whose object `index` (when
// it is one) has `faces` faces: ERAY_OK when the update can be applied.
inline int check_update_params(const eray_object_update* up, uint32_t index, size_t nobj, uint32_t faces, const char** why) {
    const char* dummy;
    if (!why) why = &dummy;
    *why = "";
    if (!up) return *why = "update is null", ERAY_E_INVALID_ARGUMENT;
    if (index >= nobj) return *why = "object_index is not an object of the scene", ERAY_E_INVALID_ARGUMENT;
    if (up->flags & ~(ERAY_UPDATE_DEVICE | ERAY_UPDATE_BBOX)) return *why = "unknown update flags", ERAY_E_INVALID_ARGUMENT;
    if (up->triangle_count != faces)
        return *why = "triangle_count is not the object's (an update keeps the face count and order)", ERAY_E_INVALID_ARGUMENT;
    if (!up->positions && !up->normals && !up->uvs && !(up->flags & ERAY_UPDATE_BBOX))
        return *why = "positions, normals and uvs are all null without ERAY_UPDATE_BBOX", ERAY_E_INVALID_ARGUMENT;
    return ERAY_OK;
}

}  // namespace eray
