// scene_build.hpp — what the scene upload (capi_scene.cpp sync_scene) decides before it touches
// the GPU: the host scene's objects (HostObject), the descriptor records the kernels read
// (ObjectDesc, LightDesc) and how they are built from the objects, the lights and the texel
// programs (build_scene_descs), the layout of the raw vertex arrays (raw_slices), and which
// scenes reflect (scene_reflective).  No HIP header and no HIP call, so the upload, the kernels
// (through internal.hpp) and the stand-alone checker (tests/cpp/scene_build_main.cpp, built with the
// host sanitizers) share it.  The bin entries it only points to are internal.hpp's.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/eray_hip.h"
#include "frame_params.hpp"
#include "texel_prog.hpp"

namespace eray {
namespace gpu {

struct BinEntry;

struct TexView {
    const float* data;  // nullptr: the output is absent (Option::None)
    uint32_t w, h;
};

struct MaterialDesc {
    TexView color;  // IColor, 3 floats per texel
    TexView diffuse, specular, specular_power, reflection;  // IValue
    // example: 1 = color and diffuse are main.rs's graph evaluated at the hit texel
    uint32_t example, ex_w, ex_h;
    float ex_xf, ex_yf, ex_r, ex_g, ex_b, ex_factor;
    // a shader graph per hit texel (eray_scene_set_object_texel_graph), or null
    const uint32_t* prog;
};

struct ObjGeom {  // what the triangle scans need of an object, 64 B
    uint32_t tri_begin, tri_count;
    // Camera pixels whose primary ray can hit the object: x0..x1 x y0..y1 (inclusive, camera
    // rows), from the culling records (tri_rect_kernel); empty when x0 > x1.
    int32_t rect[4];
    float bb_lo[3], bb_hi[3];
    // Screen bins of a large object's faces (bins.hip), or null: bin b's entries are
    // bin_ent[bin_start[b] .. bin_start[b + 1]) (bins of 65..kBinSortMax entries in increasing
    // face index, with the later chunks' mask unions, BinEntry).
    const uint32_t* bin_start;
    const BinEntry* bin_ent;
};

struct alignas(16) ObjectDesc {  // 192 B: the LDS scene copy moves whole 16-B words
    ObjGeom g;
    MaterialDesc mat;
};

struct LightDesc {
    float pos[3];
    int32_t variant;  // 0 point, 1 ambient
    float color[3];
    float brightness;
};
static_assert(sizeof(ObjGeom) == 64, "ObjGeom is 64 B");
static_assert(sizeof(ObjectDesc) == 192, "ObjectDesc is 192 B");
static_assert(sizeof(LightDesc) % 16 == 0, "16-B words");

struct HostObject {
    std::vector<float> raw;  // T*9 positions | T*9 normals | T*6 uvs (raw_slices)
    uint32_t T = 0;
    // eray_scene_update_object replaced (part of) the geometry from device arrays: the resident raw
    // array holds it, `raw` does not (refresh_raw reads it back before the scene is uploaded again)
    bool raw_stale = false;
    float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
    eray_material mat{};
    bool example = false;  // color + diffuse from main.rs's graph at the hit texel
    eray_material_example_params ex{};
    std::vector<eray_texel_node> tnodes;  // a shader graph per hit texel (texel_graph)
    int32_t tout[5] = {-1, -1, -1, -1, -1};
};

// The raw vertex arrays: a scene of `total` faces keeps total*9 positions | total*9 normals |
// total*6 uvs (floats), an object of T faces the same of its own in HostObject::raw.  The three
// slices of an object of T faces whose first face is face `begin` of the scene: where each starts
// in the scene's array and in the object's, and its length.  (A whole scene's: raw_slices(T, 0, T).)
struct RawSlice {
    size_t in_scene, in_object, count;
};
inline std::array<RawSlice, 3> raw_slices(size_t total, size_t begin, size_t T) {
    return {{{9 * begin, 0, 9 * T}, {9 * total + 9 * begin, 9 * T, 9 * T}, {18 * total + 6 * begin, 18 * T, 6 * T}}};
}
constexpr size_t kRawFloatsPerFace = 24;

// eray_scene_set_object_texel_graph on the host object: `g` checked and kept, or (null) the
// object's graph removed.  The call's status, its message in why[0 .. n).
inline int set_texel_graph(HostObject& o, const eray_texel_graph* g, char* why, size_t n) {
    if (n) why[0] = 0;
    if (!g) {
        o.tnodes.clear();
        std::fill(o.tout, o.tout + 5, -1);
        return ERAY_OK;
    }
    if (int st = check_texel_graph(g, why, n)) return st;
    const int32_t outs[5] = {g->color, g->diffuse, g->specular, g->specular_power, g->reflection};
    o.tnodes.assign(g->nodes, g->nodes + g->count);
    std::copy(outs, outs + 5, o.tout);
    return ERAY_OK;
}

// Does some material reflect?  Bounces only matter then (engine.rs:181-182).  A graph output
// replaces the texture (None if mistyped).
inline bool scene_reflective(const std::vector<HostObject>& objects) {
    bool reflective = false;
    for (auto& o : objects) {
        const int32_t r = o.tout[4];
        reflective |= r >= 0 ? !texel_is_color(o.tnodes[r].kind) : o.mat.reflection.data != nullptr;
    }
    return reflective;
}

// What the kernels and the camera setups read of the scene beside the face records.
struct SceneDescs {
    std::vector<ObjectDesc> objs;
    std::vector<LightDesc> lights;
    std::vector<uint32_t> begin;  // obj_begin (nobj + 1: each object's first face, then all faces) | objkey (nobj:
                                  // the object's place among those of more than kDirectMax faces, or ~0u)
    uint32_t binned = 0;          // objects of more than kDirectMax faces
    bool spec_pow = false;        // some material has a specular-power output
    bool example_mat = false;     // some material is evaluated per hit (main.rs's graph, a texel program)
};

// The descriptors of `objects` and `lights`.  prog_at[i]: the first word of object i's texel
// program in the programs' array at `prog_base` (device), SIZE_MAX without one.
inline void build_scene_descs(const std::vector<HostObject>& objects, const std::vector<eray_light>& lights,
                              const uint32_t* prog_base, const std::vector<size_t>& prog_at, SceneDescs& out) {
    const auto tex = [](const eray_image& im) { return TexView{im.data, im.width, im.height}; };
    const uint32_t nobj = (uint32_t)objects.size();
    out.objs.clear();
    out.begin.assign(2 * (size_t)nobj + 1, 0u);
    out.binned = 0;
    out.spec_pow = false;
    out.example_mat = false;
    uint32_t begin = 0;
    for (uint32_t i = 0; i < nobj; ++i) {
        const HostObject& o = objects[i];
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
            d.mat.prog = prog_base + prog_at[i];
            TexView* tv[5] = {&d.mat.color, &d.mat.diffuse, &d.mat.specular, &d.mat.specular_power,
                              &d.mat.reflection};
            for (int out_k = 0; out_k < 5; ++out_k)
                if (o.tout[out_k] >= 0) *tv[out_k] = TexView{nullptr, 0, 0};
            out.example_mat = true;
            if (o.tout[3] >= 0 && !texel_is_color(o.tnodes[o.tout[3]].kind)) out.spec_pow = true;
        }
        out.objs.push_back(d);
        out.spec_pow |= d.mat.specular_power.data != nullptr;
        out.example_mat |= d.mat.example != 0;
        // setup.hip's object ranges and binned-object indices
        out.begin[i] = begin;
        out.begin[nobj + 1 + i] = o.T > kDirectMax ? out.binned++ : ~0u;
        begin += o.T;
    }
    out.begin[nobj] = begin;
    out.lights.clear();
    for (auto& l : lights) {
        LightDesc d{};
        for (int k = 0; k < 3; ++k) {
            d.pos[k] = l.position[k];
            d.color[k] = l.color[k];
        }
        d.variant = l.variant;
        d.brightness = l.brightness;
        out.lights.push_back(d);
    }
}

}  // namespace gpu
}  // namespace eray
