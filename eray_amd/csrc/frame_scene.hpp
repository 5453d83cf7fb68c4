// frame_scene.hpp — how the frame kernel reads its scene: the frame's pixel-block geometry, the
// record loads (global, buffer and LDS-uniform), the kernel's preloaded leading arguments
// (FrameHot) and the two scene views a frame_kernel build is instantiated over — SceneGlobal (the
// device arrays) and SceneLds (a small scene preloaded into LDS by preload_scene).  Included by
// render.hip, the translation unit that defines frame_kernel, through frame_first_hit.hpp,
// frame_fill.hpp and frame_sub.hpp; nothing else includes it.
#pragma once

// (in this order: glibc_cosf.hpp and internal.hpp each define ERAY_HD for their own functions)
#include "cull_record.hpp"
#include "device_math.hpp"
#include "glibc_cosf.hpp"
#include "internal.hpp"
#include "hit.hpp"

namespace eray {
namespace gpu {
namespace {

using namespace eray::dev;

constexpr int kWG = 256;

constexpr uint32_t kBlkW = 64, kBlkH = 4;  // pixel block
constexpr uint32_t kSubW = 16;             // sub-block width (x kBlkH rows): one wave's pixels
static_assert(kSubW == kBinW && kBlkH == kBinH, "a screen bin is one wave's sub-block");

// Scene descriptors and triangle records are read-only for the whole frame: reading them
// through the constant address space lets wave-uniform reads become scalar (s_load) loads.
// Texture pointers come out of the descriptors: say they are global (no flat loads).
__device__ __forceinline__ const __attribute__((address_space(1))) float* as_global(const float* ptr) {
    return (const __attribute__((address_space(1))) float*)ptr;
}
template <typename T>
__device__ __forceinline__ T as_global_rec(const T* ptr) {  // per-lane record read, global
    static_assert(sizeof(T) % 16 == 0, "16-byte records only");
    using v4 = unsigned int __attribute__((ext_vector_type(4)));
    using gv4 = const __attribute__((address_space(1))) v4;
    gv4* src = (gv4*)ptr;
    T out;
    v4* dst = reinterpret_cast<v4*>(&out);
#pragma unroll
    for (size_t k = 0; k < sizeof(T) / 16; ++k) dst[k] = src[k];
    return out;
}

// Record `index` of a wave-uniform array by buffer loads: the array base lives in SGPRs (the
// buffer resource) and each lane only carries a 32-bit byte offset — no 64-bit per-lane address
// arithmetic or registers (arrays below 4 GB: triangle records, bin entries).
template <typename T>
__device__ __forceinline__ T load_rec(const T* base, uint32_t index) {
    static_assert(sizeof(T) % 16 == 0, "16-byte records only");
    using v4 = unsigned int __attribute__((ext_vector_type(4)));
    const __amdgpu_buffer_rsrc_t r = __builtin_amdgcn_make_buffer_rsrc(const_cast<T*>(base), 0, -1, 0x00020000);
    T out;
    v4* dst = reinterpret_cast<v4*>(&out);
#pragma unroll
    for (uint32_t k = 0; k < sizeof(T) / 16; ++k)
        dst[k] = __builtin_amdgcn_raw_buffer_load_b128(r, index * (uint32_t)sizeof(T) + 16u * k, 0, 0);
    return out;
}

// --------------------------------------------------------------------- scene views ---------
// Read paths of the frame's scene data (descriptors, lights, triangle records).
//  * SceneGlobal reads the device arrays; uniform reads go through the constant address
//    space and become scalar loads.
//  * SceneLds reads a copy of the whole scene that each workgroup preloads into LDS in one
//    round trip (small scenes: kCacheTris triangles, kCacheObjects objects, kCacheLights
//    lights).  Uniform reads are LDS broadcasts moved to SGPRs with readfirstlane.
// Either way one instantiation touches one address space (no generic "flat" loads).
template <typename T>
__device__ __forceinline__ T lds_uniform(const T* ptr) {
    static_assert(sizeof(T) % 4 == 0, "dword-sized records only");
    T out;
    const uint32_t* src = reinterpret_cast<const uint32_t*>(ptr);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&out);
#pragma unroll
    for (size_t k = 0; k < sizeof(T) / 4; ++k) dst[k] = __builtin_amdgcn_readfirstlane(src[k]);
    return out;
}

// The frame kernel's first reads, passed as leading scalar kernel arguments: the compiler
// preloads them into SGPRs (-amdgpu-kernarg-preload-count, build.py), so the scene preload's
// loads issue without a kernel-argument round trip first.
struct FrameHot {
    const ObjectDesc* objects;
    const LightDesc* lights;
    const TriCull* cull;
    const TriHot* tris;
    const TriShade* shade;
    uint32_t counts;      // nobj | nlights << 16
    uint32_t total_tris;
    uint32_t total_sub;   // detail sub-blocks
    uint32_t grid;        // workgroups launched
};

struct SceneGlobal {
    const FrameParams& p;
    const ObjectDesc* objects;  // the frame's descriptors and culling records (a batched camera
    const TriCull* culls;       // setup's slot: FrameParams::dev_slots)
    __device__ ObjGeom geom(uint32_t i) const { return load_const(&objects[i].g, 0); }
    __device__ const ObjGeom* geom_ptr(uint32_t i) const { return &objects[i].g; }
    __device__ MaterialDesc mat(uint32_t i) const { return load_const(&objects[i].mat, 0); }
    __device__ LightDesc light(uint32_t i) const { return load_const(p.lights, i); }
    __device__ TriCull cull(uint32_t g) const { return culls[g]; }          // per lane
    __device__ const TriCull* cull_array() const { return culls; }
    __device__ TriHot hot(uint32_t g) const { return load_const(p.tris, g); }  // uniform
    __device__ TriHot hot_lane(uint32_t g) const { return load_rec(p.tris, g); }  // per lane
    __device__ TriShade shade(uint32_t g) const { return load_rec(p.shade, g); }  // per lane
};

struct SceneLds {
    const ObjectDesc* objs;
    const LightDesc* lights;
    const TriCull* culls;
    const TriHot* hots;
    const TriShade* shades;
    const ObjectDesc* g_objs;  // the device arrays (scalar loads of uniform records)
    const LightDesc* g_lights;
    const TriHot* g_tris;
    const TriCull* g_cull;
    // Wave-uniform records (objects, materials, lights) by scalar loads from the device arrays,
    // not LDS reads + readfirstlane: C2 8.67 -> 8.40 us per frame (profiles/ab/ab_c2chain.log),
    // though one wave's chain alone is 0.2 us longer (7.26 -> 7.44 us, a 4-row frame).
    __device__ ObjGeom geom(uint32_t i) const { return load_const(&g_objs[i].g, 0); }
    __device__ const ObjGeom* geom_ptr(uint32_t i) const { return &g_objs[i].g; }
    __device__ MaterialDesc mat(uint32_t i) const { return load_const(&g_objs[i].mat, 0); }
    __device__ LightDesc light(uint32_t i) const { return load_const(g_lights, i); }
    __device__ TriCull cull(uint32_t g) const { return culls[g]; }
    __device__ const TriCull* cull_array() const { return g_cull; }
    __device__ TriHot hot(uint32_t g) const { return hots[g]; }  // broadcast read (VGPRs)
    __device__ TriHot hot_lane(uint32_t g) const { return hots[g]; }
    __device__ TriShade shade(uint32_t g) const { return shades[g]; }
};

// Copies the scene into LDS (layout: scene_lds_layout, internal.hpp): every 16-byte word is
// loaded before any is stored, four per thread per pass, so a small scene costs one round trip.
// `meanwhile()` runs once while the first pass's loads are in flight.
template <typename Meanwhile>
__device__ SceneLds preload_scene(const FrameHot& p, char* dyn, Meanwhile&& meanwhile) {
    const SceneLdsLayout L = scene_lds_layout(p.counts & 0xffffu, p.counts >> 16, p.total_tris, p.cull != nullptr);
    const uint32_t n_obj = L.lights / 16, n_light = (L.cull - L.lights) / 16;
    const uint32_t n_cull = (L.hot - L.cull) / 16, n_hot = (L.shade - L.hot) / 16;
    const uint32_t total = L.bytes / 16;
    using v4 = unsigned int __attribute__((ext_vector_type(4)));
    using gv4 = const __attribute__((address_space(1))) v4;
    gv4* src_obj = (gv4*)p.objects;
    gv4* src_light = (gv4*)p.lights;
    gv4* src_cull = (gv4*)p.cull;
    gv4* src_hot = (gv4*)p.tris;
    gv4* src_shade = (gv4*)p.shade;
    v4* dst = reinterpret_cast<v4*>(dyn);
    for (uint32_t base = 0; base < total; base += 4 * kWG) {
        v4 v[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {  // branch-free (clamped index): the loads issue back to back
            const uint32_t i = min(base + k * kWG + threadIdx.x, total - 1);
            const uint32_t i1 = i - n_obj, i2 = i1 - n_light, i3 = i2 - n_cull, i4 = i3 - n_hot;
            gv4* src = i < n_obj ? src_obj + i
                     : i1 < n_light ? src_light + i1
                     : i2 < n_cull ? src_cull + i2
                     : i3 < n_hot ? src_hot + i3
                     : src_shade + i4;
            v[k] = *src;
        }
        if (base == 0) {
            meanwhile();
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const uint32_t i = base + k * kWG + threadIdx.x;
            if (i < total) dst[i] = v[k];
        }
    }
    return SceneLds{reinterpret_cast<const ObjectDesc*>(dyn + L.objs), reinterpret_cast<const LightDesc*>(dyn + L.lights),
                    reinterpret_cast<const TriCull*>(dyn + L.cull), reinterpret_cast<const TriHot*>(dyn + L.hot),
                    reinterpret_cast<const TriShade*>(dyn + L.shade), p.objects, p.lights, p.tris, p.cull};
}

}  // namespace
}  // namespace gpu
}  // namespace eray
