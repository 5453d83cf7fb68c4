// frame_sub.hpp — Engine::cast_ray for one wave's 16 x 4 pixel sub-block (render_sub): the camera
// ray and the sub-block's viewport rectangle (frame_camera, camera_dir, RowMap, make_bundle), the
// closest object among the first hits (frame_first_hit.hpp), Material::get, shadow rays, shading
// and the stores of the sub-block's pixels (store_slice).  Included by render.hip alone, whose
// frame_kernel calls render_sub once per detail sub-block.  Uses render.hip's ERAY_TRACE_* hooks.
#pragma once

#include "frame_fill.hpp"
#include "frame_first_hit.hpp"

namespace eray {
namespace gpu {
namespace {

__device__ const float g_texel_dummy[4] = {0.0f, 0.0f, 0.0f, 0.0f};

// The frame's camera: the kernel arguments, or the setup kernel's copy in device-camera mode
// (FrameParams::cam_state; wave-uniform, scalar loads).
template <bool kDev>
__device__ __forceinline__ CamDev frame_camera(const FrameParams& p, const CamState* cs) {
    if (kDev) return load_const(&cs->cam, 0);
    return CamDev{p.cx, p.cy, p.cz, p.ratio, p.z_dist, {0u, 0u, 0u}};
}

// Camera::pixel_to_ray(x / W, y / H).dir (engine.rs:100-109, camera.rs:57-76, Ray::new)
__device__ __forceinline__ f3 camera_dir(const CamDev& cam, const FrameParams& p, uint32_t px, uint32_t y) {
    const f3 C = mk3(cam.cx, cam.cy, cam.cz);
    const float xf = (float)px / (float)p.cam_w;
    const float yf = (float)y / (float)p.cam_h;
    const float vw = cam.ratio * 2.0f;
    const f3 horizontal = mk3(vw, 0.0f, 0.0f), vertical = mk3(0.0f, 2.0f, 0.0f);
    const f3 botleft = sub(sub(sub(C, divs(horizontal, 2.0f)), divs(vertical, 2.0f)),
                           mk3(0.0f, 0.0f, cam.z_dist));
    return normalize(sub(add(add(botleft, mul(horizontal, xf)), mul(vertical, yf)), C));
}

// Rank-local row -> camera row (interleaved bands or a contiguous block), from the frame kernel's
// band word (h_band: shift | stride << 5) and row0.
struct RowMap {
    uint32_t row0, shift, stride;
};
__device__ __forceinline__ uint32_t cam_row(const RowMap& m, uint32_t j) {
    return band_camera_row(m.row0, m.shift, 0xffffffffu >> (32u - m.shift), m.stride, j);
}

__device__ __forceinline__ Bundle make_bundle(const FrameParams& p, const RowMap& rm, uint32_t x0, uint32_t xe,
                                              uint32_t py0, uint32_t pye) {
    // the pixel rectangle in viewport coordinates, widened to contain every pixel's x' = x/W and
    // y' = y/H (approximate reciprocal, then 2^-20 outward; x', y' >= 0)
    const float rw = __builtin_amdgcn_rcpf((float)p.cam_w), rh = __builtin_amdgcn_rcpf((float)p.cam_h);
    const float lo = 1.0f - 0x1p-20f, hi = 1.0f + 0x1p-20f;
    const uint32_t y0 = cam_row(rm, py0);  // (a sub-block's rows lie in one band)
    return Bundle{((float)x0 * rw) * lo, ((float)xe * rw) * hi, ((float)y0 * rh) * lo,
                  ((float)(y0 + (pye - py0)) * rh) * hi};
}

// the pixel rectangle of `ob` (camera rows) meets the sub-block's pixels
__device__ __forceinline__ bool rect_meets(const ObjGeom& ob, const RowMap& rm, uint32_t wx0, uint32_t py0) {
    const int32_t x0 = (int32_t)wx0, y0 = (int32_t)cam_row(rm, py0);
    return ob.rect[0] <= x0 + (int32_t)kSubW - 1 && ob.rect[1] >= x0 && ob.rect[2] <= y0 + (int32_t)kBlkH - 1 &&
           ob.rect[3] >= y0;
}

// Engine::cast_ray for the 16 x 4 pixels at (wx0, py0) (rank-local rows), one pixel per lane;
// `active` false: the wave only takes part in the workgroup's LDS-tile barriers.
// kMat: material features some object of the scene uses — kMatSpecPow (a specular-power output:
// powf is not the identity), kMatExample (main.rs's graph evaluated per hit texel); a kernel
// without them carries none of their code or registers.
constexpr int kMatSpecPow = 1, kMatExample = 2;
// Pipelining across a wave's sub-blocks (binned meshes): `pre` (or null) holds the bin range of
// this sub-block for object `pre_obj`, loaded during the wave's previous sub-block; `mid()` runs
// once the first hits are known (the next sub-block's range loads are issued there).
struct NoMid {
    __device__ void operator()() const {}
};

// Staged outputs of a wave's sub-block: its 16 x 4 pixels' f32 RGB rows (768 B) and PPM byte rows
// (192 B, file order) in an LDS slice.
constexpr uint32_t kWavePix = kSubW * kBlkH;
constexpr uint32_t kSliceRgbBytes = 3 * 4 * kWavePix, kSlicePpmBytes = 3 * kWavePix;
// The 16-B row stores of a staged slice (sub-block at (wx0, py0), rank-local rows).
// (wave-uniform sub-block: 32-bit lane offsets, the sub-block's base as the scalar offset)
__device__ __forceinline__ void store_slice(const FrameParams& p, const FrameOut& fo, uint32_t wx0, uint32_t py0,
                                            const float* wrgb, const uint8_t* wppm, uint32_t lane) {
    constexpr uint32_t kRgbRow4 = kSubW * 3 / 4;    // float4 per wave row (12)
    constexpr uint32_t kPpmRow16 = kSubW * 3 / 16;  // 16-byte words per wave row (3)
    // (the lane offsets are recomputed here, a few instructions, rather than kept live across the
    // detail rounds, where the 4-per-CU build would spill them)
    asm volatile("" : "+v"(lane));
    if (fo.rgb && lane < kBlkH * kRgbRow4) {
        const uint32_t r = lane / kRgbRow4, c = lane % kRgbRow4;
        const float4 v = reinterpret_cast<const float4*>(wrgb)[lane];
        const uint4 w = make_uint4(__float_as_uint(v.x), __float_as_uint(v.y), __float_as_uint(v.z), __float_as_uint(v.w));
        if (fo.nt)
            stream16_at<true>(fo.rgb, r * p.img_w * 12u + c * 16u, (py0 * p.img_w + wx0) * 12u, w);
        else
            stream16_at<false>(fo.rgb, r * p.img_w * 12u + c * 16u, (py0 * p.img_w + wx0) * 12u, w);
    }
    if (fo.ppm && lane < kBlkH * kPpmRow16) {
        const uint32_t r = lane / kPpmRow16, c = lane % kPpmRow16;  // r-th byte row of the block
        const uint4 w = reinterpret_cast<const uint4*>(wppm)[lane];
        if (fo.nt)
            stream16_at<true>(fo.ppm, r * p.img_w * 3u + c * 16u, ((p.rows - py0 - kBlkH) * p.img_w + wx0) * 3u, w);
        else
            stream16_at<false>(fo.ppm, r * p.img_w * 3u + c * 16u, ((p.rows - py0 - kBlkH) * p.img_w + wx0) * 3u, w);
    }
}

// kStaging: the build keeps the LDS-staged output path (only the dense large-mesh builds, whose
// 4-slot north-star frames use it; the others store per lane only and carry none of its registers)
//
// kOne (LDS-scene builds, the launcher's choice for a scene of one object — main.rs's own shape):
// the object loops are gone, and with them the closest-object compare, the per-lane object
// selection and the second tri_begin read; the object's ObjGeom is read once per sub-block and
// reused by the shadow test, and the light count comes from `counts` (the preloaded nobj |
// nlights << 16), not from a kernel-argument read per loop.  The MaterialDesc and the lights are
// still read where they are used: reading them ahead of the search as well, to wait for them once,
// measured slower — the records held across the search cost more SGPR spills than their round
// trips.
template <bool kCull, bool kLdsTiles, int kMat, bool kStaging = true, bool kOne = false, typename Scene,
          typename Mid = NoMid>
__device__ __forceinline__ void render_sub(const FrameParams& p, const FrameOut& fo, const CamDev& cam, const RowMap& rm,
                                           const Scene& sc, uint32_t wx0, uint32_t py0,
                                           bool active, TriHot* s_hot, TriCull* s_cull, char* s_bins, float4* s_rgb,
                                           uint32_t* s_ppm, bool aligned, bool has_given = false,
                                           f3 given_d = f3{0.0f, 0.0f, 0.0f}, bool coop = true,
                                           PreRange pre = PreRange{0u, 0u, false}, uint32_t pre_obj = ~0u,
                                           Mid&& mid = Mid{}, uint32_t counts = 0) {
    static_assert(!kOne || !kLdsTiles, "the single-object path is a small-scene (LDS-scene) build's");
    // coop (workgroup-uniform): the workgroup's four sub-blocks share their large objects' work —
    // binned chunks dealt over the waves, shadow rays through shared LDS tiles — with barriers;
    // otherwise (light sub-blocks) every wave searches its own bins and shadow rays alone
    // Culled large-mesh builds (screen bins): every sub-block is searched by its own wave
    // (first_hit_binned_wave handles bins of any length), the cooperative paths are compiled out —
    // 139 instead of 161 VGPRs and 1.5-2.7 % faster frames at 3840x2160 / 70k, C3, C5 and moving
    // cameras, where switching them off at run time gained nothing (profiles/r04/ab/ab_r04am.txt,
    // ab_r04an.txt).  A large object without bins (a bin-capacity overflow's fallback frame) is
    // then scanned by each wave alone; brute-force builds (!kCull) keep the LDS tiles.
    if constexpr (kCull && kLdsTiles) coop = false;
    wx0 = __builtin_amdgcn_readfirstlane(wx0);  // (wave-uniform: scalar registers)
    py0 = __builtin_amdgcn_readfirstlane(py0);
    constexpr bool kSpecPow = (kMat & kMatSpecPow) != 0, kExample = (kMat & kMatExample) != 0;
    // candidates tested together by the per-wave scans (small objects, shadow rays): four for ILP,
    // one in the large-mesh builds, whose registers bound their resident waves
    constexpr int kTestB = kLdsTiles ? kLargeTestBatch : kBatch;
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const f3 C = mk3(cam.cx, cam.cy, cam.cz);
    const uint32_t px = wx0 + (lane % kSubW), ly = lane / kSubW;
    const uint32_t py = py0 + ly;
    const bool valid = active && px < p.cam_w && py < p.rows;
    const uint32_t y = cam_row(rm, py);
    const Bundle bd = make_bundle(p, rm, wx0, min(wx0 + kSubW - 1, p.cam_w - 1), py0, min(py0 + kBlkH - 1, p.rows - 1));

    // ---- cast_ray (engine.rs:112-216): closest object among first hits -----------
    ERAY_TRACE_WAVE0(4);
    f3 d = given_d;  // the camera ray, when the caller has it (has_given)
    bool ray_ready = has_given;
    bool have = false;
    float closest = 0.0f, bu = 0.0f, bv = 0.0f, bt = 0.0f;
    uint32_t best_obj = 0;
    int best_face = -1;
    // object and light counts; the single-object path's ObjGeom, read once
    const uint32_t nobj = kOne ? 1u : p.nobj;
    const uint32_t nlights = kOne ? counts >> 16 : p.nlights;
    ObjGeom one_ob{};
    if constexpr (kOne) one_ob = sc.geom(0);
    auto geom = [&](uint32_t oi) {
        if constexpr (kOne)
            return one_ob;
        else
            return sc.geom(oi);
    };
    for (uint32_t oi = 0; oi < nobj; ++oi) {
        const ObjGeom ob = geom(oi);  // uniform
        ERAY_TRACE_WAVE0(16);
        const bool direct = !kLdsTiles || ob.tri_count <= kDirectMax;
        const bool wave_bins = kCull && !direct && !coop && ob.bin_start && ob.tri_count <= kWaveBinMaxTris;
        // outside the object's pixel rectangle no primary ray can hit it (only where skipping
        // keeps the workgroup's barriers uniform: without coop nothing here has a barrier)
        if (kCull && (direct || !coop) && !rect_meets(ob, rm, wx0, py0)) continue;
        auto activate = [&]() {
            if (!ray_ready) {
                uint32_t pxo = px, yo = y;  // opaque: keep ray generation on this path
                asm volatile("" : "+v"(pxo), "+v"(yo));
                d = camera_dir(cam, p, pxo, yo);
                ray_ready = true;
            }
            const bool bb = bbox_hit(ob, C, d);
            return bb;
        };
        int st = valid ? kUndecided : kDone, f = -1;
        float u, v, t;
        if (direct) {
            first_hit<kCull, false, false, kTestB>(p, sc, ob.tri_begin, ob.tri_count, st, C, d, bd, s_hot, s_cull, activate, f, u,
                                    v, t);
        } else if (wave_bins) {  // this wave's own bin, no barrier
            const uint32_t bin = ((cam_row(rm, py0) + kBinH - p.bin_phase) / kBinH) * p.bins_x + wx0 / kBinW;
            first_hit_binned_wave(ob, bin, st, C, d, activate, f, u, v, t, s_bins,
                                  oi == pre_obj ? pre : PreRange{0u, 0u, false});
        } else if (kCull && ob.bin_start && coop) {  // the workgroup's four sub-blocks together
            const uint32_t bin = ((cam_row(rm, py0) + kBinH - p.bin_phase) / kBinH) * p.bins_x + wx0 / kBinW;
            first_hit_binned(p, ob, bin, st, C, d, activate, f, u, v, t, s_bins,
                             oi == pre_obj ? pre : PreRange{0u, 0u, false});
        } else if (!coop) {  // no bins (or too many faces for the wave's keys): this wave scans alone
            first_hit<kCull, false, false, kTestB>(p, sc, ob.tri_begin, ob.tri_count, st, C, d, bd, s_hot, s_cull,
                                                   activate, f, u, v, t);
        } else {
            first_hit<kCull, kLdsTiles, false, kTestB>(p, sc, ob.tri_begin, ob.tri_count, st, C, d, bd, s_hot, s_cull, activate,
                                        f, u, v, t);
        }
        if (f >= 0) {
            const f3 P = add(C, mul(d, t));
            const float dsq = len_sq(sub(P, C));
            if (!have || dsq < closest) {  // strict `<`: the first object wins ties
                have = true;
                closest = dsq;
                best_obj = oi;
                best_face = f;
                bu = u;
                bv = v;
                bt = t;
            }
        }
    }

    mid();
    ERAY_TRACE_WAVE0(5);
    // ---- hit data and Material::get (material.rs:56-94) --------------------------
    // (cast.hpp holds this shading too — fill_level, shade, walk's ambient term — for rays that start anywhere.  Apart
    // on purpose: as shared functions they changed frame_kernel's code, registers and spills included)
    // The object loop only finds each lane's texel addresses; the loads are issued once after
    // it and first used by the shading, so their latency overlaps the shadow rays.
    f3 P = mk3(0.0f, 0.0f, 0.0f), N = mk3(0.0f, 0.0f, 0.0f);
    rgb color{0.0f, 0.0f, 0.0f};
    float kd = 0.5f, ks = 0.5f, sp = 1.0f;
    const float *tc = nullptr, *tkd = nullptr, *tks = nullptr, *tsp = nullptr;  // texels, if any
    // every hit lane's shading record in one load from a wave-uniform point (a lane without a
    // hit reads record 0)
    TriShade sh = TriShade{};
    if (__any(have)) {
        uint32_t g = 0;
        for (uint32_t oi = 0; oi < nobj; ++oi) {
            if (!__any(have && best_obj == oi)) continue;
            const uint32_t tb = kOne ? one_ob.tri_begin : load_const(&sc.geom_ptr(oi)->tri_begin, 0);
            if (have && best_obj == oi) g = tb + (uint32_t)best_face;
        }
        sh = sc.shade(g);
    }
    for (uint32_t oi = 0; oi < nobj; ++oi) {  // per-lane object, read from uniform copies
        if (!__any(have && best_obj == oi)) continue;
        const MaterialDesc mat = sc.mat(oi);
        ERAY_TRACE_WAVE0(17);
        if (!(have && best_obj == oi)) continue;
        P = add(C, mul(d, bt));
        const f3 na = mk3(sh.s0.x, sh.s0.y, sh.s0.z), nb = mk3(sh.s0.w, sh.s1.x, sh.s1.y);
        const f3 nc = mk3(sh.s1.z, sh.s1.w, sh.s2.x);
        N = normalize(add(add(mul(na, bu), mul(nb, bv)), mul(nc, bt)));
        const float w = 1.0f - bu - bv;
        const float uv0 = ((sh.s2.y * w) + (sh.s2.w * bu)) + (sh.s3.y * bv);
        const float uv1 = ((sh.s2.z * w) + (sh.s3.x * bu)) + (sh.s3.z * bv);
        if (kExample && mat.example) {  // main.rs's graph at the texel Material::get would read
            const uint32_t ix = mod_size(sat_u32(uv0 * (float)mat.ex_w), mat.ex_w);
            const uint32_t iy = mod_size(sat_u32(uv1 * (float)mat.ex_h), mat.ex_h);
            const float wv = __builtin_fabsf(libm::cosf_glibc(libm::div10_f32((float)ix * mat.ex_xf + (float)iy * mat.ex_yf)));
            const float omf = 1.0f - mat.ex_factor;  // mix_color.rs:89 (material_example_kernel)
            color = rgb{wv * omf + mat.ex_r * mat.ex_factor, wv * omf + mat.ex_g * mat.ex_factor,
                        wv * omf + mat.ex_b * mat.ex_factor};
            kd = wv;
        }
        if (kExample && mat.prog) {  // a shader graph at the texel (its outputs have no texture)
            float t3[3];
            if (texel_program(mat.prog, 0, uv0, uv1, t3)) color = rgb{t3[0], t3[1], t3[2]};
            if (texel_program(mat.prog, 1, uv0, uv1, t3)) kd = t3[0];
            if (texel_program(mat.prog, 2, uv0, uv1, t3)) ks = t3[0];
            if (kSpecPow && texel_program(mat.prog, 3, uv0, uv1, t3)) sp = t3[0];
        }
        tc = texel(mat.color, uv0, uv1, 3);
        tkd = texel(mat.diffuse, uv0, uv1, 1);
        tks = texel(mat.specular, uv0, uv1, 1);
        if (kSpecPow) tsp = texel(mat.specular_power, uv0, uv1, 1);
    }
    // every lane loads (a lane without the texture reads a dummy word); Material::get's values
    // are selected where the shading first needs them
    const bool has_c = tc, has_kd = tkd, has_ks = tks, has_sp = kSpecPow && tsp;
    const auto* tcg = as_global(tc ? tc : g_texel_dummy);
    const float vc0 = tcg[0], vc1 = tcg[1], vc2 = tcg[2];
    const float vkd = *as_global(tkd ? tkd : g_texel_dummy);
    const float vks = *as_global(tks ? tks : g_texel_dummy);
    const float vsp = kSpecPow ? *as_global(tsp ? tsp : g_texel_dummy) : 1.0f;
    bool resolved = false;
    auto material = [&]() {
        if (resolved) return;
        resolved = true;
        if (has_c) color = rgb{vc0, vc1, vc2};
        if (has_kd) kd = vkd;
        if (has_ks) ks = vks;
        if (has_sp) sp = vsp;
    };

    bool any = false;  // the lighting list as a running left fold (color.rs:82-87)
    rgb acc{0.0f, 0.0f, 0.0f};
    auto push = [&](rgb c) {
        if (any) {
            acc = cadd(acc, c);
        } else {
            acc = c;
            any = true;
        }
    };
    ERAY_TRACE_WAVE0(13);
    const HitBox hb = hit_box(have, P, N);  // (wave-uniform; shadow-ray face bounds)
    // Point lights first (engine.rs:130-135), 32 at a time: every light's shadow ray, then the
    // shading of the lights that reach the hit, in list order.  The texture loads above are
    // still in flight during the first shadow scan; the shading is their first use.
    for (uint32_t li0 = 0; li0 < nlights; li0 += 32) {
        const uint32_t li1 = min(nlights, li0 + 32);
        uint32_t lit = 0;  // bit li - li0: point light li reaches the lane's hit
        for (uint32_t li = li0; li < li1; ++li) {
            const LightDesc L = sc.light(li);
            ERAY_TRACE_WAVE0(18);
            if (L.variant == 1 || (!(kLdsTiles && coop) && !__any(have))) continue;  // (LDS tiles: barriers)
            const f3 Lp = mk3(L.pos[0], L.pos[1], L.pos[2]);
            // reaches_light(Ray::new(P + N * 0.1, Lp - P)) (engine.rs:136-142, 218-228)
            f3 S = mk3(0.0f, 0.0f, 0.0f);
            f3 sd = mk3(0.0f, 0.0f, 1.0f);
            float dist = 0.0f;
            bool reached = true, decided = false;
            bool ray = false;  // S, sd, dist computed
            auto shadow_ray = [&]() {
                if (ray) return;
                ray = true;
                if (have) {
                    S = add(P, mul(N, 0.1f));
                    sd = normalize(sub(Lp, P));
                    dist = len(sub(Lp, S));
                }
            };
            for (uint32_t oj = 0; oj < nobj; ++oj) {
                const ObjGeom ob = geom(oj);
                ERAY_TRACE_WAVE0(19);
                // A point box (the loaded meshes'): when it certainly rejects every lane's shadow
                // ray (point_box_rejects), bbox_hit is false for all of them — no ray, no face
                // load (not where the LDS tiles' barriers need every wave)
                if (!(kLdsTiles && coop && ob.tri_count > kDirectMax) && point_box_xy(ob) &&
                    !__any(have && !decided && !point_box_rejects(ob, add(P, mul(N, 0.1f)), sub(Lp, P)))) {
                    ERAY_TRACE_VALUE(20, 1u + oj);  // (diagnostics: the skip fired for object oj)
                    continue;
                }
                ERAY_TRACE_VALUE(21, 1u + oj);  // (... the shadow scan of object oj ran)
                int f = -1;
                float u, v, t;
                if (!kLdsTiles || ob.tri_count <= kDirectMax) {
                    // faces some hit point's shadow ray may pass (box bounds, lane-parallel),
                    // then the exact tests in index order; the ray itself only when needed
                    int st = kDone;
                    bool opened = false;
                    for (uint32_t base = 0; base < ob.tri_count; base += 64) {
                        const uint32_t n = min(64u, ob.tri_count - base);
                        bool keep = lane < n;
                        if (keep && hb.ok) keep = shadow_box_may_hit(sc.hot_lane(ob.tri_begin + base + lane), Lp, hb);
                        const unsigned long long mask = __ballot(keep);
                        if (!mask) continue;
                        if (!opened) {
                            opened = true;
                            shadow_ray();
                            st = (have && !decided && bbox_hit(ob, S, sd)) ? kSearching : kDone;
                        }
                        if (!__any(st == kSearching)) break;
                        auto face = [&](uint32_t i) { return base + i; };
                        auto hot = [&](uint32_t i) { return sc.hot(ob.tri_begin + base + i); };
                        if (!test_candidates<kTestB>(mask, face, hot, st, S, sd, f, u, v, t)) break;
                    }
                } else if (!coop) {  // this wave alone (no barrier): faces its searching lanes may hit
                    shadow_ray();
                    int st = (have && !decided && bbox_hit(ob, S, sd)) ? kSearching : kDone;
                    auto never = []() { return false; };
                    first_hit<false, false, true, kTestB>(p, sc, ob.tri_begin, ob.tri_count, st, S, sd, bd, s_hot, s_cull,
                                                  never, f, u, v, t);
                } else {
                    shadow_ray();
                    int st = (have && !decided && bbox_hit(ob, S, sd)) ? kSearching : kDone;
                    auto never = []() { return false; };
                    first_hit<false, kLdsTiles, false, kTestB>(p, sc, ob.tri_begin, ob.tri_count, st, S, sd, bd, s_hot, s_cull,
                                                never, f, u, v, t);
                }
                if (f >= 0) {
                    const f3 hp = add(S, mul(sd, t));
                    reached = len(sub(hp, S)) > dist;
                    decided = true;
                }
            }
            if (have && reached) lit |= 1u << (li - li0);
        }
        ERAY_TRACE_WAVE0(14);
        if (!__any(lit != 0)) continue;
        material();
        for (uint32_t li = li0; li < li1; ++li) {
            const LightDesc L = sc.light(li);
            if (L.variant == 1 || !((lit >> (li - li0)) & 1u)) continue;  // engine.rs:143-178
            const f3 Lp = mk3(L.pos[0], L.pos[1], L.pos[2]);
            const f3 LmP = sub(Lp, P);
            float prod = rust_clamp(dot0(N, LmP), 0.0f, 1.0f);
            if (prod != prod) prod = 0.0f;
            const float falloff = 1.0f / len(LmP);
            const rgb lc{L.color[0], L.color[1], L.color[2]};
            const rgb diffusion =
                cmul(cmul(cmul(cmul(cmulc(color, lc), kd), prod), L.brightness), falloff);
            const f3 reflected = sub(d, mul(mul(N, 2.0f), dot0(d, N)));
            const float dotr = dot0(normalize(reflected), normalize(LmP));
            // specular_power defaults to 1 and powf(x, 1) == x; pow only when a
            // material has a specular-power output (kSpecPow)
            const float res =
                rust_clamp(ks * L.brightness * (kSpecPow ? powf_ref(dotr, sp) : dotr), 0.0f, 1.0f);
            const float sf = rust_clamp(kSpecPow ? powf_ref(falloff, sp) : falloff, 0.0f, 1.0f);
            const rgb specular{res * sf, res * sf, res * sf};
            push(cadd(diffusion, specular));
        }
    }
    if (have) {
        material();
        for (uint32_t li = 0; li < nlights; ++li) {  // ambient lights (engine.rs:197-209)
            const LightDesc L = sc.light(li);
            if (L.variant != 1) continue;
            const rgb m{rust_min(L.color[0], color.r), rust_min(L.color[1], color.g),
                        rust_min(L.color[2], color.b)};
            push(cmul(cmul(m, kd), L.brightness));
        }
    } else {
        push(rgb{0.1f, 0.1f, 0.2f});  // engine.rs:211-213
    }

    ERAY_TRACE_WAVE0(6);
    // ---- outputs: Image::set + Color::as_bytes, rows bottom-up (image.rs:41-74) ---
    const uint32_t b0 = sat_u8(acc.r * 255.0f), b1 = sat_u8(acc.g * 255.0f), b2 = sat_u8(acc.b * 255.0f);
    if (valid && fo.face) fo.face[(size_t)py * p.img_w + px] = have ? best_face : -1;
    // Frames into a ring beyond the Infinity Cache (non-temporal launches aside; dense builds
    // only: C2 in 16 slots is no faster staged) leave through the wave's LDS slice as
    // write-through 16-B row stores (3840x2160 / 70k in 4 slots 25.6 -> 24.8 us); elsewhere each lane stores its own pixel with plain (write-back) stores: C5 123.5 ->
    // 116, C2 40.6 -> 40.3 us (no LDS round trip and wave barriers in the chain).  Write-through
    // partial stores lose badly (C5 154 us).  Same-box A/B profiles/r05/ab/ab_r05ao.txt ..
    // ab_r05aq.txt
    const bool staged = kStaging && (p.launch_flags & kLaunchRingBeyondCache) && !fo.nt;
    if (staged && active && aligned && wx0 + kSubW <= p.cam_w && py0 + kBlkH <= p.rows) {
        // the wave's 16 x 4 pixels leave through its own LDS slice as 16-B row stores
        float* wrgb = reinterpret_cast<float*>(reinterpret_cast<char*>(s_rgb) + kSliceRgbBytes * wave);
        uint8_t* wppm = reinterpret_cast<uint8_t*>(s_ppm) + kSlicePpmBytes * wave;
        const uint32_t wl = lane % kSubW;
        float* srgb = wrgb + 3 * (ly * kSubW + wl);
        srgb[0] = acc.r;
        srgb[1] = acc.g;
        srgb[2] = acc.b;
        uint8_t* sppm = wppm + 3 * ((kBlkH - 1 - ly) * kSubW + wl);
        sppm[0] = (uint8_t)b0;
        sppm[1] = (uint8_t)b1;
        sppm[2] = (uint8_t)b2;
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
        store_slice(p, fo, wx0, py0, wrgb, wppm, lane);
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();  // the slice is rewritten by the next block
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    } else if (valid) {
        const size_t idx = (size_t)py * p.img_w + px;
        if (fo.rgb) {
            float* o = fo.rgb + 3 * idx;
            o[0] = acc.r;
            o[1] = acc.g;
            o[2] = acc.b;
        }
        if (fo.ppm) {
            uint8_t* o = fo.ppm + 3 * ((size_t)(p.rows - 1 - py) * p.img_w + px);
            o[0] = (uint8_t)b0;
            o[1] = (uint8_t)b1;
            o[2] = (uint8_t)b2;
        }
    }
    ERAY_TRACE_WAVE0(7);
}

}  // namespace
}  // namespace gpu
}  // namespace eray
