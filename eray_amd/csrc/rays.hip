// rays.hip — ray queries on gfx950: Object<Built>::intersects (object.rs:58-81) and
// Engine::cast_ray (engine.rs:112-216) for a batch of caller-supplied rays (eray_cast_rays), and
// Engine::reaches_light (engine.rs:218-228) for caller-supplied shadow rays (eray_rays_reach_light).
//
// The frame kernel and the general tracer make their own rays from the camera; here the rays
// come from the caller and go anywhere, so nothing camera-shaped (culling records, pixel
// rectangles, screen bins) applies.  One lane is one ray; a 256-thread workgroup takes 256
// consecutive rays at a time and strides over the batch.
//
// The search.  Per object (scene order): the bounding box (object.rs:59), then the first face by
// index whose Triangle::intersects passes (object.rs:63-78).  The object's TriHot records stream
// through an LDS tile of kRayTile faces, loaded by the whole workgroup with coalesced 16-B loads
// and read back at a wave-uniform address (an LDS broadcast: three ds_read_b128 per face and
// wave, no per-lane global loads).  A lane stops at its first passing face; a wave leaves the
// tile once none of its lanes is still searching; the workgroup stops loading tiles once no wave
// needs them — so an object whose box every ray of the workgroup fails (the loaded meshes'
// (0,0,0) box for almost every ray) costs no face load at all.  With object == -1 the closest
// object is the one whose hit point is strictly closer to the scene camera's centre than every
// earlier object's (engine.rs:120-126: the camera's centre, not the ray's start).
//
// The winner's TriShade record and textures are read once per hit, after the object loop; a hit
// record leaves as three 16-B stores.  out_rgb is cast_ray(ray, 0).sum() from that primary hit:
// cast.hpp's fill_level and walk, whose shadow and reflected rays scan per lane as in trace.hip.
//
// With a ray-query hierarchy (eray_scene_build_ray_accel; accel_walk.hpp, accel_build.hpp) the
// objects that have one are searched by rays_accel_kernel instead: the box as before, then the
// object's unculled faces in index order, then the tree, one lane one ray, with a per-lane stack of
// kStackDepth node indices in LDS (laid out [level][thread]: a wave's lanes touch consecutive dwords, no bank conflict)
// — no scratch, no spill.  A lane reads nodes and leaf faces through its own 16-B loads (three per
// node, three per face): incoherent rays share nothing, and the nodes of a 70k-face mesh are well
// under 1 MB, resident in L2.  The result is the smallest passing index with exact_test's u, v, t on
// a byte copy of the same record, i.e. the scan's bits.  Rays the margin proof does not cover scan
// per lane (first_face); objects without a hierarchy keep the tiles, and since the choice is per
// object (wave- and workgroup-uniform) the tiles' barriers stay uniform.  out_rgb's shadow and
// reflected rays search the objects that have a hierarchy through it as well: cast.hpp's walk takes
// a face finder, and rays_accel_kernel passes AccelFaces (accel_faces.hpp, shared with the general
// tracer), which holds the RayAccelView and the lane's stack column (empty again once the primary walk has returned, so the secondary walks
// reuse it: no more LDS, no scratch).  Objects without a hierarchy are scanned per lane by those
// rays — they run inside the walk's divergent loop, where no workgroup barrier can stand.  Same
// faces, same u, v, t, same colours.
//
// eray_rays_reach_light (reach_kernel) is Engine::reaches_light (engine.rs:218-228) for shadow
// rays the caller supplies, one lane per ray and one dword out, in the same three forms: the
// hierarchy, the tiles (a lane that an earlier object has decided passes inbox == false and keeps
// the barriers uniform), and the per-lane scan.
//
// ERAY_RAYS_BRUTE_FORCE is the plain form: every lane walks every face through its own loads
// (cast.hpp first_face), no tiles, no workgroup-level skips — the same exact_test on the same
// records, so the same u, v, t bit for bit (tests/test_gpu_rays.py compares the two).
#include "accel_faces.hpp"
#include "cast.hpp"
#include "device_math.hpp"
#include "hit.hpp"
#include "internal.hpp"

namespace eray {
namespace gpu {
namespace {

using namespace eray::dev;

// An object's first passing face for the workgroup's 256 rays, through LDS tiles.  Every thread
// of the workgroup must call (barriers); `inbox`: this lane's ray passed the object's box.
// s_need[2][4]: each wave's "some lane still searches" flag, double-buffered by `phase` so that
// a wave that has left a tile round cannot overwrite a flag another wave has yet to read.
__device__ __forceinline__ int tile_first_face(const TriHot* tris, const ObjGeom& ob, bool inbox, f3 o, f3 d, float& u,
                                               float& v, float& t, TriHot* s_tile, uint32_t (*s_need)[4],
                                               uint32_t& phase) {
    const uint32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const float4* src = reinterpret_cast<const float4*>(tris + ob.tri_begin);
    float4* dst = reinterpret_cast<float4*>(s_tile);
    bool search = inbox;
    int f = -1;
    for (uint32_t t0 = 0; t0 < ob.tri_count; t0 += kRayTile) {  // (workgroup-uniform)
        const bool wave_need = __any(search) != 0;
        uint32_t* need = s_need[phase & 1u];
        ++phase;
        if (lane == 0) need[wave] = wave_need ? 1u : 0u;
        __syncthreads();  // the flags are in; every wave has left the previous tile
        if (!(need[0] | need[1] | need[2] | need[3])) break;  // (workgroup-uniform)
        const uint32_t n = min(kRayTile, ob.tri_count - t0);
        for (uint32_t q = threadIdx.x; q < 3 * n; q += 256) dst[q] = src[3 * (size_t)t0 + q];
        __syncthreads();
        if (!wave_need) continue;
        for (uint32_t k = 0; k < n; ++k) {  // (wave-uniform: one LDS address per read)
            const TriHot r = s_tile[k];
            float uu, vv, tt;
            if (search && exact_test(r, o, d, uu, vv, tt)) {
                u = uu;
                v = vv;
                t = tt;
                f = (int)(t0 + k);
                search = false;
            }
            if (!__any(search)) break;
        }
    }
    return f;
}

// Triangle::intersects' position and normal (primitives.rs:66-67) and RaycastHit's uv
// (object.rs:70-72) of hit h, as the words of an eray_ray_hit; a miss: object -1, the rest 0.
__device__ __forceinline__ void hit_record(const FrameParams& p, f3 o, f3 d, const Hit& h, uint4 (&q)[3]) {
    q[0] = make_uint4(~0u, 0u, 0u, 0u);
    q[1] = make_uint4(0u, 0u, 0u, 0u);
    q[2] = make_uint4(0u, 0u, 0u, 0u);
    if (h.f < 0) return;
    const TriShade sh = p.shade[p.objects[h.o].g.tri_begin + (uint32_t)h.f];
    const f3 P = add(o, mul(d, h.t));
    const f3 na = mk3(sh.s0.x, sh.s0.y, sh.s0.z), nb = mk3(sh.s0.w, sh.s1.x, sh.s1.y);
    const f3 nc = mk3(sh.s1.z, sh.s1.w, sh.s2.x);
    const f3 N = normalize(add(add(mul(na, h.u), mul(nb, h.v)), mul(nc, h.t)));  // (t, not w: primitives.rs:67)
    const float w = 1.0f - h.u - h.v;
    const float uv0 = ((sh.s2.y * w) + (sh.s2.w * h.u)) + (sh.s3.y * h.v);
    const float uv1 = ((sh.s2.z * w) + (sh.s3.x * h.u)) + (sh.s3.z * h.v);
    q[0] = make_uint4(h.o, (uint32_t)h.f, __float_as_uint(P.x), __float_as_uint(P.y));
    q[1] = make_uint4(__float_as_uint(P.z), __float_as_uint(N.x), __float_as_uint(N.y), __float_as_uint(N.z));
    q[2] = make_uint4(__float_as_uint(uv0), __float_as_uint(uv1), __float_as_uint(h.u), __float_as_uint(h.v));
}

// A finished ray's outputs: its hit record and, with kRgb, cast_ray(ray, 0).sum() from that hit.
// `find`: the face finder of the shadow and reflected rays (cast.hpp).
template <bool kRgb, bool kBounce, class Find>
__device__ __forceinline__ void store_ray(const RayBatch& b, uint64_t i, f3 o, f3 d, const Hit& h, const Find& find) {
    const FrameParams& p = b.f;
    if (b.out_hit) {
        uint4 q[3];
        hit_record(p, o, d, h, q);
        uint4* dst = b.out_hit + 3 * i;
        dst[0] = q[0];
        dst[1] = q[1];
        dst[2] = q[2];
    }
    if constexpr (kRgb) {
        rgb c = miss_color();
        if (h.f >= 0) {
            Level L;
            fill_level(p, o, d, h, L);
            c = walk<kBounce>(p, L, find);
        }
        float* dst = b.out_rgb + 3 * i;
        dst[0] = c.r;
        dst[1] = c.g;
        dst[2] = c.b;
    }
}

// This lane's ray from the batch (dead lanes: a harmless ray), as rays_kernel loads its own.
__device__ __forceinline__ void load_ray(const RayIn* rays, uint32_t norm, uint64_t i, bool live, f3& o, f3& d) {
    o = mk3(0.0f, 0.0f, 0.0f);
    d = mk3(0.0f, 0.0f, -1.0f);
    if (live) {
        const RayIn r = rays[i];
        o = mk3(r.start[0], r.start[1], r.start[2]);
        d = mk3(r.dir[0], r.dir[1], r.dir[2]);
        if (norm) d = normalize(d);  // Ray::new (raycasting.rs:16-21, vector.rs:150-158)
    }
}

// kRgb: out_rgb is wanted (cast_ray's lights, shadows and, with kBounce, reflection levels).
template <bool kRgb, bool kBounce>
__global__ void __launch_bounds__(256) rays_kernel(RayBatch b) {
    __shared__ TriHot s_tile[kRayTile];
    __shared__ uint32_t s_need[2][4];
    const FrameParams& p = b.f;
    const f3 C = mk3(p.cx, p.cy, p.cz);
    const uint32_t o0 = b.object >= 0 ? (uint32_t)b.object : 0u, o1 = b.object >= 0 ? o0 + 1u : p.nobj;
    uint32_t phase = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < b.count; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < b.count;
        f3 o = mk3(0.0f, 0.0f, 0.0f), d = mk3(0.0f, 0.0f, -1.0f);
        if (live) {
            const RayIn r = b.rays[i];
            o = mk3(r.start[0], r.start[1], r.start[2]);
            d = mk3(r.dir[0], r.dir[1], r.dir[2]);
            if (b.normalize) d = normalize(d);  // Ray::new (raycasting.rs:16-21, vector.rs:150-158)
        }
        Hit h;
        h.f = -1;
        for (uint32_t oi = o0; oi < o1; ++oi) {  // scene order (engine.rs:116)
            const ObjGeom ob = load_const(&p.objects[oi].g, 0);
            float u, v, t;
            int f = -1;
            if (b.brute) {
                if (live) f = first_face(p.tris, ob, o, d, u, v, t, nullptr);
            } else {
                f = tile_first_face(p.tris, ob, live && bbox_hit(ob, o, d), o, d, u, v, t, s_tile, s_need, phase);
            }
            closer(h, oi, f, u, v, t, o, d, C);
        }
        if (live) store_ray<kRgb, kBounce>(b, i, o, d, h, ScanFaces{p.tris, nullptr});
    }
}

// (LaneStack, accel_object_face and AccelFaces, the finder through the hierarchy: accel_faces.hpp,
// here with the workgroup-wide stack array's stride of 256.)
constexpr uint32_t kStackStride = 256;

// rays_kernel's tiled form for a scene with a ray-query hierarchy: objects that have one go
// through it, the others through the tiles (the choice is per object, so every barrier of
// tile_first_face is reached by the whole workgroup).
template <bool kRgb, bool kBounce>
__global__ void __launch_bounds__(256) rays_accel_kernel(RayBatch b, RayAccelView a) {
    __shared__ TriHot s_tile[kRayTile];
    __shared__ uint32_t s_need[2][4];
    __shared__ uint32_t s_stack[accel::kStackDepth][256];
    const FrameParams& p = b.f;
    const f3 C = mk3(p.cx, p.cy, p.cz);
    const uint32_t o0 = b.object >= 0 ? (uint32_t)b.object : 0u, o1 = b.object >= 0 ? o0 + 1u : p.nobj;
    uint32_t phase = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < b.count; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < b.count;
        f3 o, d;
        load_ray(b.rays, b.normalize, i, live, o, d);
        Hit h;
        h.f = -1;
        for (uint32_t oi = o0; oi < o1; ++oi) {  // scene order (engine.rs:116)
            const ObjGeom ob = load_const(&p.objects[oi].g, 0);
            const accel::Object ao = load_const(&a.objs[oi], 0);
            float u, v, t;
            int f = -1;
            if (ao.has) {  // (workgroup-uniform)
                if (live && bbox_hit(ob, o, d))
                    f = accel_object_face<kStackStride>(p.tris, a, ao, ob, o, d, u, v, t, &s_stack[0][threadIdx.x]);
            } else {
                f = tile_first_face(p.tris, ob, live && bbox_hit(ob, o, d), o, d, u, v, t, s_tile, s_need, phase);
            }
            closer(h, oi, f, u, v, t, o, d, C);
        }
        if (live) store_ray<kRgb, kBounce>(b, i, o, d, h, AccelFaces<kStackStride>{p.tris, a, &s_stack[0][threadIdx.x]});
    }
}

// eray_rays_reach_light: Engine::reaches_light (engine.rs:218-228) per caller-supplied shadow ray,
// one lane per ray, one dword out.  The objects go in scene order and the first one with a hit
// decides; a lane that an earlier object has decided stays in the loop with inbox == false, so the
// tiles' barriers stay workgroup-uniform.  kAccel: objects that have a hierarchy go through it
// (the lane's stack column in LDS); without it the kernel carries no stack and keeps the tiled
// kernel's occupancy.  b.brute is cast.hpp's reaches_light with the per-lane scan.
template <bool kAccel>
__global__ void __launch_bounds__(256) reach_kernel(ReachBatch b, RayAccelView a) {
    __shared__ TriHot s_tile[kRayTile];
    __shared__ uint32_t s_need[2][4];
    __shared__ uint32_t s_stack[kAccel ? accel::kStackDepth : 1][256];
    const FrameParams& p = b.f;
    uint32_t phase = 0;
    for (uint64_t base = (uint64_t)blockIdx.x * 256u; base < b.count; base += (uint64_t)gridDim.x * 256u) {
        const uint64_t i = base + threadIdx.x;
        const bool live = i < b.count;
        f3 o, d;
        load_ray(b.rays, b.normalize, i, live, o, d);
        f3 Lp = o;
        if (live) Lp = mk3(b.targets[3 * i], b.targets[3 * i + 1], b.targets[3 * i + 2]);
        if (b.brute) {  // (workgroup-uniform)
            if (live) b.out[i] = reaches_light(p, o, d, Lp, ScanFaces{p.tris, nullptr}) ? 1u : 0u;
            continue;
        }
        const float dist = len(sub(Lp, o));
        bool decided = false, reach = true;
        for (uint32_t oi = 0; oi < p.nobj; ++oi) {  // scene order (engine.rs:220)
            const ObjGeom ob = load_const(&p.objects[oi].g, 0);
            const bool inbox = live && !decided && bbox_hit(ob, o, d);
            float u, v, t;
            int f = -1;
            bool tiles = true;
            if constexpr (kAccel) {
                const accel::Object ao = load_const(&a.objs[oi], 0);
                if (ao.has) {  // (workgroup-uniform)
                    tiles = false;
                    if (inbox) f = accel_object_face<kStackStride>(p.tris, a, ao, ob, o, d, u, v, t, &s_stack[0][threadIdx.x]);
                }
            }
            if (tiles) f = tile_first_face(p.tris, ob, inbox, o, d, u, v, t, s_tile, s_need, phase);
            if (f >= 0) {
                decided = true;
                reach = len(sub(add(o, mul(d, t)), o)) > dist;
            }
        }
        if (live) b.out[i] = reach ? 1u : 0u;
    }
}

}  // namespace

namespace {
// a workgroup per 256 rays, at most the 8 per CU the registers and the 12-KB tile allow at once
dim3 ray_grid(uint64_t count) {
    static const uint32_t cus = [] {
        int dev = 0, n = 0;
        return (hipGetDevice(&dev) == hipSuccess &&
                hipDeviceGetAttribute(&n, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && n > 0)
                   ? (uint32_t)n
                   : 256u;
    }();
    const uint64_t blocks = (count + 255u) / 256u, cap = 8ull * cus;
    return dim3((uint32_t)(blocks < cap ? blocks : cap));
}
}  // namespace

hipError_t launch_reach_light(const ReachBatch& b, const RayAccelView& a, hipStream_t s) {
    if (!b.count) return hipSuccess;
    if (!b.rays || !b.targets || !b.out) return hipErrorInvalidValue;
    const dim3 grid = ray_grid(b.count);
    if (a.objs && !b.brute) hipLaunchKernelGGL((reach_kernel<true>), grid, dim3(256), 0, s, b, a);
    else hipLaunchKernelGGL((reach_kernel<false>), grid, dim3(256), 0, s, b, a);
    return hipGetLastError();
}

hipError_t launch_cast_rays(const RayBatch& b, const RayAccelView& a, hipStream_t s) {
    if (!b.count) return hipSuccess;
    if (!b.rays || (!b.out_hit && !b.out_rgb)) return hipErrorInvalidValue;
    const dim3 grid = ray_grid(b.count);
    if (a.objs && !b.brute) {  // (the hierarchy's stack: 32 KB of LDS more, 3 workgroups per CU resident)
        if (!b.out_rgb) hipLaunchKernelGGL((rays_accel_kernel<false, false>), grid, dim3(256), 0, s, b, a);
        else if (b.f.bounces) hipLaunchKernelGGL((rays_accel_kernel<true, true>), grid, dim3(256), 0, s, b, a);
        else hipLaunchKernelGGL((rays_accel_kernel<true, false>), grid, dim3(256), 0, s, b, a);
        return hipGetLastError();
    }
    if (!b.out_rgb) hipLaunchKernelGGL((rays_kernel<false, false>), grid, dim3(256), 0, s, b);
    else if (b.f.bounces) hipLaunchKernelGGL((rays_kernel<true, true>), grid, dim3(256), 0, s, b);
    else hipLaunchKernelGGL((rays_kernel<true, false>), grid, dim3(256), 0, s, b);
    return hipGetLastError();
}

}  // namespace gpu
}  // namespace eray
