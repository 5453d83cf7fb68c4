// texel_prog.hpp — per-texel shader graphs (eray_scene_set_object_texel_graph) from the caller's
// graph to the value at a hit texel: the graph's validation with its statuses and messages
// (check_texel_graph), its expansion into the pre-order instruction trees the kernels run
// (compile_texel_program), and the evaluator of those trees (texel_program), which the frame kernel
// and the general tracer call per hit (frame_sub.hpp, cast.hpp).  No HIP header and no HIP call
// outside a HIP compile (ERAY_HD, as glibc_cosf.hpp), so the scene upload (capi_scene.cpp), the
// kernels (through internal.hpp and hit.hpp) and the stand-alone checker
// (tests/cpp/scene_build_main.cpp, built with the host sanitizers) share one statement of each.
// The check writes its message into the caller's buffer, as frame_plan.hpp's checks do.
#pragma once

#include <stddef.h>
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "../../include/eray_hip.h"
#include "device_math.hpp"  // sat_u32, ERAY_HD_FORCEINLINE
#include "glibc_cosf.hpp"

#if defined(__HIPCC__) || defined(__HIP__)
#define ERAY_HD_NOINLINE __host__ __device__ __noinline__  // (the kernels call texel_program from several sites)
#else
#define ERAY_HD_NOINLINE inline
#endif

namespace eray {
namespace gpu {

// One node of a material output's expression tree, evaluated per hit texel (texel_program): the
// host expands the shader graph (eray_texel_graph) per output into a tree in pre-order — a node
// shared along different paths is evaluated at each path's texel — where every node's texel
// derives from its parent's.
struct TexelInstr {  // 48 B
    uint32_t kind;    // eray_texel_node_kind
    uint32_t w, h;    // the node's image size
    uint32_t parent;  // instruction index of the parent (0: the root itself)
    uint32_t xform;   // kTexelMod: parent texel mod (w, h) (mix's mod_get); kTexelIndex: the
                      // parent's pixel index y * w_parent + x as (i % w, i / w) (rgb's pixels[i])
    float p[3];
    uint32_t c[3];    // children (later instructions; rgb's identical inputs share one)
    uint32_t pad;
};
static_assert(sizeof(TexelInstr) == 48, "the program's instruction records are 12 words");
constexpr uint32_t kTexelMod = 0, kTexelIndex = 1;
constexpr uint32_t kTexelMaxNodes = 32;  // per output tree
// Program header (uint32 words): first instruction and count per Material output (color,
// diffuse, specular, specular_power, reflection), count 0 = not a program output; then the
// instructions from word kTexelHeaderWords (48-B records).
constexpr uint32_t kTexelHeaderWords = 12;

// Node types of the shaderlib outputs: wave's is IValue, rgb / flat_color / mix_color's IColor.
inline bool texel_is_color(uint32_t kind) { return kind != ERAY_TEXEL_WAVE; }

// ERAY_OK when `g` (not null) is a graph eray_scene_set_object_texel_graph takes, else the status
// the call returns and its message in why[0 .. n).
inline int check_texel_graph(const eray_texel_graph* g, char* why, size_t n) {
    if (n) why[0] = 0;
    if (g->count && !g->nodes) return snprintf(why, n, "nodes is null"), ERAY_E_INVALID_ARGUMENT;
    for (uint32_t i = 0; i < g->count; ++i) {
        const eray_texel_node& nd = g->nodes[i];
        if (nd.kind > ERAY_TEXEL_MIX_COLOR) return snprintf(why, n, "node %u: kind %u", i, nd.kind), ERAY_E_INVALID_ARGUMENT;
        // every image a Material::get lookup can reach is indexed by mod_get or by pixel index:
        // a zero-sized one panics there (image.rs:36-38)
        if (!nd.width || !nd.height) return snprintf(why, n, "node %u: zero width or height", i), ERAY_E_OUT_OF_BOUNDS;
        const int inputs = nd.kind == ERAY_TEXEL_RGB ? 3 : nd.kind == ERAY_TEXEL_MIX_COLOR ? 2 : 0;
        for (int j = 0; j < inputs; ++j) {
            const int32_t in = nd.input[j];
            if (in < 0 || (uint32_t)in >= i)  // unconnected (MissingMany) or not an earlier node
                return snprintf(why, n, "node %u: input %d is not an earlier node", i, j), ERAY_E_MISSING_MANY;
            const eray_texel_node& src = g->nodes[in];
            // rgb takes IValue images, mix_color IColor ones (get_sv!, shader.rs:140-178)
            if (texel_is_color(src.kind) != (nd.kind == ERAY_TEXEL_MIX_COLOR))
                return snprintf(why, n, "node %u: input %d has the wrong image type", i, j), ERAY_E_INVALID_TYPE;
            // rgb reads pixels[y * width + x] of each input (rgb.rs:89-95): it panics past the end
            if (nd.kind == ERAY_TEXEL_RGB && (uint64_t)src.width * src.height < (uint64_t)nd.width * nd.height)
                return snprintf(why, n, "node %u: input %d has fewer pixels than the node", i, j), ERAY_E_OUT_OF_BOUNDS;
        }
    }
    const int32_t outs[5] = {g->color, g->diffuse, g->specular, g->specular_power, g->reflection};
    for (int k = 0; k < 5; ++k)
        if (outs[k] < -1 || outs[k] >= (int32_t)g->count)
            return snprintf(why, n, "output %d: node %d out of range", k, outs[k]), ERAY_E_INVALID_ARGUMENT;
    return ERAY_OK;
}

// Expands node `idx` of `nodes` (evaluated at a texel derived from instruction `parent` by
// `xform`) into pre-order instructions; indices are relative to `first`.
inline uint32_t texel_emit(const std::vector<eray_texel_node>& nodes, uint32_t idx, uint32_t parent, uint32_t xform,
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

// The texel program of one object's graph (checked nodes, Material outputs tout: node index or
// -1), appended to `words`: the header, then every output's expression tree.  An output whose node
// has the wrong type (Material::get reads it as None) or that is kept gets count 0.  Returns -1,
// or the first output whose tree expands to more than kTexelMaxNodes instructions (`words` is
// then unchanged).
inline int compile_texel_program(const std::vector<eray_texel_node>& nodes, const int32_t (&tout)[5],
                                 std::vector<uint32_t>& words) {
    std::vector<TexelInstr> ins;
    uint32_t head[kTexelHeaderWords] = {};
    for (int out = 0; out < 5; ++out) {
        const int32_t idx = tout[out];
        if (idx < 0 || texel_is_color(nodes[idx].kind) != (out == 0)) continue;  // kept / None
        const size_t first = ins.size();
        texel_emit(nodes, (uint32_t)idx, 0, kTexelMod, first, ins);
        if (ins.size() - first > kTexelMaxNodes) return out;
        head[out] = (uint32_t)first;
        head[5 + out] = (uint32_t)(ins.size() - first);
    }
    words.insert(words.end(), head, head + kTexelHeaderWords);
    const uint32_t* w = reinterpret_cast<const uint32_t*>(ins.data());
    words.insert(words.end(), w, w + ins.size() * (sizeof(TexelInstr) / 4));
    return -1;
}

namespace {

// i % n for the texture sizes of Image::mod_get (image.rs:36-38); n is wave-uniform and a power
// of two in practice, where the modulo is a mask
ERAY_HD_FORCEINLINE uint32_t mod_size(uint32_t i, uint32_t n) {
    return (n & (n - 1)) == 0 ? (i & (n - 1)) : i % n;
}

// Material output `out` (0 color .. 4 reflection) of a texel program (MaterialDesc::prog) at uv:
// the value Material::get would read from the texture Graph::run makes (material.rs:56-94).
// Returns false when the output is not a program output.  First the texel of every tree node,
// top-down (the root's is Material::get's mod_get texel), then the values, bottom-up:
//   wave  |cos((x as f32 * x_fac + y as f32 * y_fac) / 10)|     (wave.rs:127)
//   rgb   (red[i], green[i], blue[i]) at the node's own index  (rgb.rs:89-95)
//   flat  (r, g, b)                                            (flat_color.rs:88)
//   mix   l * (1 - factor) + r * factor per channel            (mix_color.rs:85-91)
ERAY_HD_NOINLINE bool texel_program(const uint32_t* prog, uint32_t out, float u, float v, float (&val)[3]) {
    using eray::dev::sat_u32;
    const uint32_t first = prog[out], n = prog[5 + out];
    if (!n) return false;
    const TexelInstr* ins = reinterpret_cast<const TexelInstr*>(prog + kTexelHeaderWords) + first;
    uint32_t cx[kTexelMaxNodes], cy[kTexelMaxNodes];
    float vr[kTexelMaxNodes], vg[kTexelMaxNodes], vb[kTexelMaxNodes];
    cx[0] = mod_size(sat_u32(u * (float)ins[0].w), ins[0].w);
    cy[0] = mod_size(sat_u32(v * (float)ins[0].h), ins[0].h);
    for (uint32_t k = 1; k < n; ++k) {
        const TexelInstr& t = ins[k];
        const uint32_t q = t.parent;
        if (t.xform == kTexelMod) {
            cx[k] = cx[q] % t.w;
            cy[k] = cy[q] % t.h;
        } else {
            const uint64_t i = (uint64_t)cy[q] * ins[q].w + cx[q];
            cx[k] = (uint32_t)(i % t.w);
            cy[k] = (uint32_t)(i / t.w);
        }
    }
    for (uint32_t k = n; k-- > 0;) {
        const TexelInstr& t = ins[k];
        if (t.kind == 0) {  // wave
            vr[k] = __builtin_fabsf(libm::cosf_glibc(libm::div10_f32((float)cx[k] * t.p[0] + (float)cy[k] * t.p[1])));
        } else if (t.kind == 1) {  // rgb
            vr[k] = vr[t.c[0]];
            vg[k] = vr[t.c[1]];
            vb[k] = vr[t.c[2]];
        } else if (t.kind == 2) {  // flat_color
            vr[k] = t.p[0];
            vg[k] = t.p[1];
            vb[k] = t.p[2];
        } else {  // mix_color
            const float f = t.p[0];
            const uint32_t l = t.c[0], r = t.c[1];
            vr[k] = vr[l] * (1.0f - f) + vr[r] * f;
            vg[k] = vg[l] * (1.0f - f) + vg[r] * f;
            vb[k] = vb[l] * (1.0f - f) + vb[r] * f;
        }
    }
    val[0] = vr[0];
    val[1] = vg[0];
    val[2] = vb[0];
    return true;
}

}  // namespace
}  // namespace gpu
}  // namespace eray
