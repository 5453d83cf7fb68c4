// accel_faces.hpp — the face finder (cast.hpp) that goes through the ray-query hierarchy
// (accel_walk.hpp), shared by the ray queries (rays.hip: rays_accel_kernel, reach_kernel) and the
// general tracer (trace.hip: the kAccel kernels).  One lane is one ray; the walk's stack is the
// lane's column of an LDS array laid out [level][lane], accel::kStackDepth levels of kStride lanes
// (a wave's lanes touch consecutive dwords: no bank conflict, no scratch).  kStride is the array's
// row length in dwords: 256 for a workgroup-wide array, 64 for one wave's own.
#pragma once

#include "cast.hpp"
#include "device_math.hpp"
#include "hit.hpp"
#include "internal.hpp"

namespace eray {
namespace gpu {
namespace {

using namespace eray::dev;

// The walk's stack of one lane: level k at base[kStride * k].
template <uint32_t kStride>
struct LaneStack {
    uint32_t* base;
    uint32_t n;
    __device__ __forceinline__ void push(uint32_t x) { base[kStride * n++] = x; }
    __device__ __forceinline__ uint32_t pop() { return base[kStride * --n]; }
    __device__ __forceinline__ bool empty() const { return n == 0; }
};

// An object's first passing face through its hierarchy (accel_walk.hpp) for a ray that passed its
// box; rays the margin proof does not cover scan per lane.
template <uint32_t kStride>
__device__ __forceinline__ int accel_object_face(const TriHot* tris, const RayAccelView& a, const accel::Object& ao,
                                                 const ObjGeom& ob, f3 o, f3 d, float& u, float& v, float& t,
                                                 uint32_t* stack) {
    const float of[3] = {o.x, o.y, o.z}, df[3] = {d.x, d.y, d.z};
    LaneStack<kStride> st{stack, 0u};
    const int f = accel::accel_first_face(ao, a.nodes, a.index, of, df, st, [&](uint32_t slot) {
        const TriHot r = a.hot[slot];
        float uu, vv, tt;
        if (!exact_test(r, o, d, uu, vv, tt)) return false;
        u = uu;
        v = vv;
        t = tt;
        return true;
    });
    return f == accel::kAccelFallback ? first_face(tris, ob, o, d, u, v, t, nullptr) : f;
}

// The face finder (cast.hpp) of shadow and reflected rays in a scene with a hierarchy: an object
// that has one is searched as a primary ray of the ray queries searches it (the box, the unculled
// faces, the walk; fallback rays scan), any other by the per-lane scan — these rays run inside the
// divergent walk of cast.hpp, where no workgroup barrier can be reached by the whole workgroup.
// `stack` is the lane's column of the stack array: empty at every call, and every search leaves it
// empty again.
template <uint32_t kStride>
struct AccelFaces {
    const TriHot* tris;
    const RayAccelView& a;
    uint32_t* stack;
    __device__ __forceinline__ int operator()(uint32_t oi, const ObjGeom& ob, f3 o, f3 d, float& u, float& v, float& t) const {
        const accel::Object ao = load_const(&a.objs[oi], 0);
        if (!ao.has) return first_face(tris, ob, o, d, u, v, t, nullptr);
        if (!bbox_hit(ob, o, d)) return -1;
        return accel_object_face<kStride>(tris, a, ao, ob, o, d, u, v, t, stack);
    }
};

}  // namespace
}  // namespace gpu
}  // namespace eray
