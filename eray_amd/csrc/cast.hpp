// cast.hpp — Engine::cast_ray's pieces for rays that start anywhere (engine.rs:112-228), shared by
// the general tracer (trace.hip: jittered camera rays, reflected and shadow rays) and the ray
// queries (rays.hip: caller-supplied rays): an object's first face, the closest object by the
// camera's centre, the hit's Level (Material::get), reaches_light, a light's shading and the
// depth-first walk that is cast_ray(ray, 0).sum().  Same f32 operations, in the same order, as the
// Rust source each function cites (compile with -ffp-contract=off).
//
// How an object's first face is found is the caller's: surface, reaches_light and walk take a
// face finder, a callable (oi, ob, o, d, u, v, t) -> int that returns Object::intersects' face of
// object oi (geometry ob) for Ray(o, d), -1 for none, with that face's u, v, t.  ScanFaces is the
// per-lane scan (first_face) that trace.hip's kernels without a hierarchy and rays.hip's rays_kernel
// use through the overloads without a finder; rays_accel_kernel, reach_kernel and trace.hip's
// kernels with a hierarchy pass one that goes through the ray-query hierarchy (accel_faces.hpp).
// Every finder returns the same face and the same bits.
#pragma once

#include "device_math.hpp"
#include "glibc_cosf.hpp"
#include "hit.hpp"
#include "internal.hpp"

namespace eray {
namespace gpu {
namespace {

using namespace eray::dev;

// Object<Built>::intersects up to the face (object.rs:58-78): bbox, then the first face in
// index order; u, v, t of that face.
// `live` (camera rays of a scene of at most kSkipTris faces, else null): bit f of the
// wave-uniform mask is clear when face f's culling record rejects every camera ray of the wave —
// its exact test cannot pass, so skipping it leaves the first passing face unchanged.
__device__ __forceinline__ int first_face(const TriHot* tris, const ObjGeom& ob, f3 o, f3 d, float& u, float& v,
                                          float& t, const uint64_t* live) {
    if (!bbox_hit(ob, o, d)) return -1;
    const TriHot* r = tris + ob.tri_begin;
    if (live) {
        if (!ob.tri_count) return -1;
        const uint32_t b = ob.tri_begin, e = ob.tri_begin + ob.tri_count;
        for (uint32_t w = b >> 6; w <= (e - 1) >> 6; ++w) {
            uint64_t m = live[w];
            if (w == (b >> 6)) m &= ~0ull << (b & 63);
            if (w == ((e - 1) >> 6) && (e & 63)) m &= ~(~0ull << (e & 63));
            while (m) {
                const uint32_t f = w * 64 + (uint32_t)__builtin_ctzll(m) - b;
                m &= m - 1;
                if (exact_test(r[f], o, d, u, v, t)) return (int)f;
            }
        }
        return -1;
    }
    for (uint32_t f = 0; f < ob.tri_count; ++f)
        if (exact_test(r[f], o, d, u, v, t)) return (int)f;
    return -1;
}

// The default face finder: every face of the object in index order, through the lane's own loads.
struct ScanFaces {
    const TriHot* tris;
    const uint64_t* live;
    __device__ __forceinline__ int operator()(uint32_t, const ObjGeom& ob, f3 o, f3 d, float& u, float& v, float& t) const {
        return first_face(tris, ob, o, d, u, v, t, live);
    }
};

// One level of cast_ray: the closest object's hit and the Material::get values at it.
struct Level {
    f3 P, N, d;  // hit point, interpolated normal, the (normalised) ray direction
    rgb color;
    float kd, ks, sp, refl;
    uint32_t li;  // next light of the per-light loop (engine.rs:130-192)
};

// A ray's closest object so far (engine.rs:116-126): the first object whose hit point is strictly
// closer to the camera (|P - C|²) than every earlier object's replaces it.
struct Hit {
    float dsq, u, v, t;
    int32_t f;    // face relative to the object's first, -1: no hit yet
    uint32_t o;
};
__device__ __forceinline__ void closer(Hit& h, uint32_t oi, int f, float u, float v, float t, f3 o, f3 d, f3 C) {
    if (f < 0) return;
    const float dsq = len_sq(sub(add(o, mul(d, t)), C));
    if (h.f < 0 || dsq < h.dsq) h = Hit{dsq, u, v, t, f, oi};
}

// The hit's Level: Triangle::intersects' P and N (primitives.rs:60-69), RaycastHit's UV and
// Material::get (object.rs:70-74, material.rs:56-94).
// (frame_sub.hpp's render_sub holds this, shade and walk's ambient term once more, for camera rays.  Apart on purpose:
// as functions shared with it they changed frame_kernel's code, registers and spills included)
__device__ void fill_level(const FrameParams& p, f3 o, f3 d, const Hit& h, Level& L) {
    const float bu = h.u, bv = h.v, bt = h.t;
    const ObjectDesc& od = p.objects[h.o];
    const TriShade sh = p.shade[od.g.tri_begin + (uint32_t)h.f];
    L.P = add(o, mul(d, bt));
    const f3 na = mk3(sh.s0.x, sh.s0.y, sh.s0.z), nb = mk3(sh.s0.w, sh.s1.x, sh.s1.y);
    const f3 nc = mk3(sh.s1.z, sh.s1.w, sh.s2.x);
    L.N = normalize(add(add(mul(na, bu), mul(nb, bv)), mul(nc, bt)));  // (t, not w: primitives.rs:63)
    L.d = d;
    const float w = 1.0f - bu - bv;
    const float uv0 = ((sh.s2.y * w) + (sh.s2.w * bu)) + (sh.s3.y * bv);
    const float uv1 = ((sh.s2.z * w) + (sh.s3.x * bu)) + (sh.s3.z * bv);
    const MaterialDesc& mat = od.mat;
    // defaults at use (engine.rs:128,155,160,164,181)
    L.color = rgb{0.0f, 0.0f, 0.0f};
    L.kd = 0.5f;
    L.ks = 0.5f;
    L.sp = 1.0f;
    L.refl = 0.0f;
    if (mat.example) {  // main.rs's graph at the texel Material::get reads
        const uint32_t ix = mod_size(sat_u32(uv0 * (float)mat.ex_w), mat.ex_w);
        const uint32_t iy = mod_size(sat_u32(uv1 * (float)mat.ex_h), mat.ex_h);
        const float wv = __builtin_fabsf(libm::cosf_glibc(libm::div10_f32((float)ix * mat.ex_xf + (float)iy * mat.ex_yf)));
        const float omf = 1.0f - mat.ex_factor;
        L.color = rgb{wv * omf + mat.ex_r * mat.ex_factor, wv * omf + mat.ex_g * mat.ex_factor,
                      wv * omf + mat.ex_b * mat.ex_factor};
        L.kd = wv;
    }
    if (mat.prog) {  // a shader graph at the texel (its outputs have no texture)
        float t3[3];
        if (texel_program(mat.prog, 0, uv0, uv1, t3)) L.color = rgb{t3[0], t3[1], t3[2]};
        if (texel_program(mat.prog, 1, uv0, uv1, t3)) L.kd = t3[0];
        if (texel_program(mat.prog, 2, uv0, uv1, t3)) L.ks = t3[0];
        if (texel_program(mat.prog, 3, uv0, uv1, t3)) L.sp = t3[0];
        if (texel_program(mat.prog, 4, uv0, uv1, t3)) L.refl = t3[0];
    }
    if (const float* c = texel(mat.color, uv0, uv1, 3)) L.color = rgb{c[0], c[1], c[2]};
    if (const float* c = texel(mat.diffuse, uv0, uv1, 1)) L.kd = *c;
    if (const float* c = texel(mat.specular, uv0, uv1, 1)) L.ks = *c;
    if (const float* c = texel(mat.specular_power, uv0, uv1, 1)) L.sp = *c;
    if (const float* c = texel(mat.reflection, uv0, uv1, 1)) L.refl = *c;
    L.li = 0;
}

// The closest object's first hit along Ray(o, d) (engine.rs:116-126) and its Level; false on a
// miss.  `find` gives each object's face (reflected rays; camera rays of small scenes via `live`).
template <class Find>
__device__ bool surface(const FrameParams& p, f3 o, f3 d, Level& L, int32_t* face_out, const Find& find) {
    const f3 C = mk3(p.cx, p.cy, p.cz);
    Hit h;
    h.f = -1;
    for (uint32_t oi = 0; oi < p.nobj; ++oi) {
        const ObjGeom ob = p.objects[oi].g;
        float u, v, t;
        const int f = find(oi, ob, o, d, u, v, t);
        closer(h, oi, f, u, v, t, o, d, C);
    }
    if (h.f < 0) return false;
    if (face_out) *face_out = h.f;
    fill_level(p, o, d, h, L);
    return true;
}
__device__ bool surface(const FrameParams& p, f3 o, f3 d, Level& L, int32_t* face_out, const uint64_t* live) {
    return surface(p, o, d, L, face_out, ScanFaces{p.tris, live});
}

// Engine::reaches_light (engine.rs:218-228): the FIRST object with any hit decides.
template <class Find>
__device__ bool reaches_light(const FrameParams& p, f3 S, f3 sd, f3 Lp, const Find& find) {
    const float dist = len(sub(Lp, S));
    for (uint32_t oi = 0; oi < p.nobj; ++oi) {
        const ObjGeom ob = p.objects[oi].g;
        float u, v, t;
        if (find(oi, ob, S, sd, u, v, t) >= 0) return len(sub(add(S, mul(sd, t)), S)) > dist;
    }
    return true;
}

// diffuse + specular of one point light that reaches the hit (engine.rs:143-176)
__device__ __forceinline__ rgb shade(const Level& L, const LightDesc& Ld) {
    const f3 Lp = mk3(Ld.pos[0], Ld.pos[1], Ld.pos[2]);
    const f3 LmP = sub(Lp, L.P);
    float prod = rust_clamp(dot0(L.N, LmP), 0.0f, 1.0f);
    if (prod != prod) prod = 0.0f;
    const float falloff = 1.0f / len(LmP);
    const rgb lc{Ld.color[0], Ld.color[1], Ld.color[2]};
    const rgb diffusion = cmul(cmul(cmul(cmul(cmulc(L.color, lc), L.kd), prod), Ld.brightness), falloff);
    const f3 reflected = sub(L.d, mul(mul(L.N, 2.0f), dot0(L.d, L.N)));
    const float res =
        rust_clamp(L.ks * Ld.brightness * powf_ref(dot0(normalize(reflected), normalize(LmP)), L.sp), 0.0f, 1.0f);
    const float sf = rust_clamp(powf_ref(falloff, L.sp), 0.0f, 1.0f);
    return cadd(diffusion, rgb{res * sf, res * sf, res * sf});
}

// Engine::cast_ray(ray, 0).sum() (engine.rs:112-216, color.rs:82-87) as a depth-first walk from
// the first level's hit `first`.  kBounce false: no reflection levels (bounces == 0), so the walk
// needs no per-depth frames.
template <bool kBounce, class Find>
__device__ rgb walk(const FrameParams& p, const Level& first, const Find& find) {
    Level st[kBounce ? kMaxBounces + 1 : 1];
    st[0] = first;
    bool any = false;
    rgb acc{0.0f, 0.0f, 0.0f};
    auto emit = [&](rgb c, int depth) {  // c * refl[depth-1] * ... * refl[0], then the fold
        if (kBounce)
            for (int j = depth - 1; j >= 0; --j) c = cmul(c, st[j].refl);
        acc = any ? cadd(acc, c) : c;
        any = true;
    };
    const rgb miss{0.1f, 0.1f, 0.2f};  // engine.rs:211-213
    int depth = 0;
    while (depth >= 0) {
        Level& L = st[kBounce ? depth : 0];
        if (L.li < p.nlights) {
            const LightDesc Ld = p.lights[L.li++];
            if (Ld.variant == 1) continue;  // ambient lights come after the loop
            const f3 Lp = mk3(Ld.pos[0], Ld.pos[1], Ld.pos[2]);
            const f3 S = add(L.P, mul(L.N, 0.1f));
            if (reaches_light(p, S, normalize(sub(Lp, L.P)), Lp, find)) emit(shade(L, Ld), depth);
            if (kBounce && (uint32_t)depth < p.bounces && L.refl != 0.0f) {  // engine.rs:181-191
                const f3 rd = normalize(sub(L.d, mul(mul(L.N, 2.0f), dot0(L.d, L.N))));
                if (surface(p, S, rd, st[depth + 1], nullptr, find))
                    ++depth;
                else
                    emit(miss, depth + 1);
            }
        } else {
            for (uint32_t li = 0; li < p.nlights; ++li) {  // ambient lights (engine.rs:197-208)
                const LightDesc A = p.lights[li];
                if (A.variant != 1) continue;
                const rgb m{rust_min(A.color[0], L.color.r), rust_min(A.color[1], L.color.g),
                            rust_min(A.color[2], L.color.b)};
                emit(cmul(cmul(m, L.kd), A.brightness), depth);
            }
            --depth;
        }
    }
    return acc;
}
template <bool kBounce>
__device__ rgb walk(const FrameParams& p, const Level& first) {
    return walk<kBounce>(p, first, ScanFaces{p.tris, nullptr});
}

// The miss colour (engine.rs:211-213): a ray that hits nothing returns vec![it].
__device__ __forceinline__ rgb miss_color() { return rgb{0.1f, 0.1f, 0.2f}; }

}  // namespace
}  // namespace gpu
}  // namespace eray
