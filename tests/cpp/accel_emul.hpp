// accel_emul.hpp — what the CPU programs of the ray-query hierarchy share (accel_walk_main.cpp,
// accel_dev_main.cpp, accel_refit_main.cpp, accel_refit_async_main.cpp), stated once: the f32
// predicate and the linear scan, the seeded generator with its ray sets and meshes, the device
// build and the synchronous refit emulated step for step with the headers the kernels share
// (accel_margin.hpp, accel_layout.hpp), the checker's named corruptions, the walk of one tree
// against the scan, and the dealing of rays over threads.  No GPU, no HIP.  Compile with
// -ffp-contract=off.
//
// Everything is inline: a program that calls none of the emulations (accel_walk_main) links without
// accel_check.cpp.  The order of draws from the one generator g_rng decides every figure the
// programs print: a program's sequence of ray-set and mesh calls is part of its statement.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <thread>
#include <vector>

#include "../../eray_amd/csrc/accel_build.hpp"
#include "../../eray_amd/csrc/accel_check.hpp"
#include "../../eray_amd/csrc/accel_layout.hpp"

namespace accel_emul {

using namespace eray::accel;

// ---- geometry ---------------------------------------------------------------------------------
struct F3 {
    float x, y, z;
};
inline F3 sub(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline F3 cross(F3 s, F3 o) { return {s.y * o.z - s.z * o.y, s.z * o.x - s.x * o.z, s.x * o.y - s.y * o.x}; }
inline float dot0(F3 a, F3 b) {
    float acc = 0.0f;
    acc = acc + a.x * b.x;
    acc = acc + a.y * b.y;
    acc = acc + a.z * b.z;
    return acc;
}

// The record of face (a, b, c): e1 = b - a, e2 = c - a, n = e1 x e2 (primitives.rs:44-46).
inline Hot make_hot(const float* p) {
    const F3 a{p[0], p[1], p[2]}, b{p[3], p[4], p[5]}, c{p[6], p[7], p[8]};
    const F3 e1 = sub(b, a), e2 = sub(c, a), n = cross(e1, e2);
    return Hot{{e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, n.x, n.y, n.z, a.x, a.y, a.z}};
}

inline std::vector<Hot> records(const std::vector<float>& pos) {
    std::vector<Hot> hot(pos.size() / 9);
    for (size_t f = 0; f < hot.size(); ++f) hot[f] = make_hot(&pos[9 * f]);
    return hot;
}

// Triangle::intersects with the precomputed record (hit.hpp exact_test), plain f32.
inline bool exact_test(const Hot& r, F3 o, F3 d) {
    const F3 e1{r.q[0], r.q[1], r.q[2]}, e2{r.q[3], r.q[4], r.q[5]}, n{r.q[6], r.q[7], r.q[8]}, a{r.q[9], r.q[10], r.q[11]};
    if (dot0(n, d) > 0.0f) return false;
    const float det = -dot0(d, n);
    if (!(det >= 1e-6f)) return false;
    const float invdet = 1.0f / det;
    const F3 ao = sub(o, a), dao = cross(ao, d);
    const float u = dot0(e2, dao) * invdet, v = -dot0(e1, dao) * invdet, t = dot0(ao, n) * invdet;
    return t >= 0.0f && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f;
}

inline int scan(const std::vector<Hot>& hot, F3 o, F3 d) {
    for (size_t f = 0; f < hot.size(); ++f)
        if (exact_test(hot[f], o, d)) return (int)f;
    return -1;
}

// ---- rays -------------------------------------------------------------------------------------
struct Ray {
    float o[3], d[3];
    bool in_range;  // finite, |d|2 in [1e-3, 1e3]: must not be a fallback ray
};

struct HostStack {
    uint32_t v[kStackDepth];
    uint32_t n = 0, high = 0;
    void push(uint32_t x) {
        if (n >= kStackDepth) {
            std::fprintf(stderr, "stack overflow\n");
            std::abort();
        }
        v[n++] = x;
        high = n > high ? n : high;
    }
    uint32_t pop() { return v[--n]; }
    bool empty() const { return n == 0; }
};

inline std::mt19937_64 g_rng(12345);
inline double uni(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(g_rng); }
inline double gauss() { return std::normal_distribution<double>(0.0, 1.0)(g_rng); }

inline Ray mk(const double* o, const double* d) {
    Ray r;
    for (int k = 0; k < 3; ++k) {
        r.o[k] = (float)o[k];
        r.d[k] = (float)d[k];
    }
    bool fin = true;
    for (int k = 0; k < 3; ++k) fin = fin && std::isfinite(r.o[k]) && std::isfinite(r.d[k]);
    const double len = std::sqrt((double)r.d[0] * r.d[0] + (double)r.d[1] * r.d[1] + (double)r.d[2] * r.d[2]);
    r.in_range = fin && len >= 1e-3 && len <= 1e3;
    return r;
}

// n rays from the radius-3 sphere (times `far`) toward targets uniform in [-1, 1]^3, dir scaled
inline void sphere_rays(std::vector<Ray>& out, size_t n, double far, double scale) {
    for (size_t i = 0; i < n; ++i) {
        double v[3] = {gauss(), gauss(), gauss()};
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        double o[3], d[3];
        for (int k = 0; k < 3; ++k) {
            o[k] = 3.0 * far * v[k] / l;
            d[k] = (uni(-1, 1) - o[k]) * scale;
        }
        out.push_back(mk(o, d));
    }
}

// rays built from the mesh's own faces: grazing, along edges, through vertices, axis-parallel,
// starts on box planes, scaled directions, far starts, non-finite components
inline void adversarial_rays(std::vector<Ray>& out, const std::vector<float>& pos, size_t n) {
    const size_t T = pos.size() / 9;
    const double angles[5] = {1e-7, 1e-6, 1e-5, 1e-4, 1e-3};
    const double scales[3] = {1.0, 1e-3, 1e3};
    for (size_t i = 0; i < n; ++i) {
        const float* p = &pos[9 * (g_rng() % T)];
        double a[3], e1[3], e2[3], nn[3];
        for (int k = 0; k < 3; ++k) {
            a[k] = p[k];
            e1[k] = (double)p[3 + k] - p[k];
            e2[k] = (double)p[6 + k] - p[k];
        }
        nn[0] = e1[1] * e2[2] - e1[2] * e2[1];
        nn[1] = e1[2] * e2[0] - e1[0] * e2[2];
        nn[2] = e1[0] * e2[1] - e1[1] * e2[0];
        const double nl = std::sqrt(nn[0] * nn[0] + nn[1] * nn[1] + nn[2] * nn[2]);
        const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
        if (!(nl > 0.0) || !(l1 > 0.0)) continue;
        double bu = uni(0, 1), bv = uni(0, 1);
        if (bu + bv > 1) {
            bu = 1 - bu;
            bv = 1 - bv;
        }
        double P[3], o[3], d[3];
        for (int k = 0; k < 3; ++k) P[k] = a[k] + bu * e1[k] + bv * e2[k];
        const int kind = (int)(i % 8);
        const double sc = scales[(i / 8) % 3];
        if (kind <= 2) {  // within `ang` of the face's plane, through P, from the front
            const double ang = angles[(i / 24) % 5] * (kind == 2 ? -1.0 : 1.0), mix = uni(0, 1);
            double t[3];
            for (int k = 0; k < 3; ++k) t[k] = mix * e1[k] / l1 + (1 - mix) * (e2[k] - e1[k]);
            const double tl = std::sqrt(t[0] * t[0] + t[1] * t[1] + t[2] * t[2]);
            for (int k = 0; k < 3; ++k) d[k] = (std::cos(ang) * t[k] / tl - std::sin(ang) * nn[k] / nl);
            const double back = uni(0.5, 3.0);
            for (int k = 0; k < 3; ++k) o[k] = P[k] - back * d[k], d[k] *= sc;
        } else if (kind == 3) {  // along an edge
            const double back = uni(0.5, 3.0);
            for (int k = 0; k < 3; ++k) d[k] = e1[k] / l1, o[k] = a[k] - back * d[k], d[k] *= sc;
        } else if (kind == 4) {  // through a vertex
            double v[3] = {gauss(), gauss(), gauss()};
            const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int k = 0; k < 3; ++k) o[k] = 3.0 * v[k] / l, d[k] = (a[k] + e1[k] - o[k]) * sc;
        } else if (kind == 5) {  // one or two zero direction components, through P
            const int ax = (int)(g_rng() % 3), two = (int)(g_rng() % 2);
            for (int k = 0; k < 3; ++k) d[k] = (k == ax || (two && k == (ax + 1) % 3)) ? 0.0 : (g_rng() % 2 ? 1.0 : -1.0);
            for (int k = 0; k < 3; ++k) o[k] = P[k] - 2.5 * d[k], d[k] *= sc;
        } else if (kind == 6) {  // a zero component with the start on a vertex's coordinate plane
            const int ax = (int)(g_rng() % 3);
            for (int k = 0; k < 3; ++k) d[k] = k == ax ? 0.0 : uni(-1, 1);
            for (int k = 0; k < 3; ++k) o[k] = k == ax ? a[k] : P[k] - 3.0 * d[k];
            for (int k = 0; k < 3; ++k) d[k] *= sc;
        } else {  // a start at distance 1e3 toward P
            double v[3] = {gauss(), gauss(), gauss()};
            const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
            for (int k = 0; k < 3; ++k) o[k] = 1e3 * v[k] / l, d[k] = (P[k] - o[k]) / 1e3 * sc;
        }
        out.push_back(mk(o, d));
    }
    const double bad[4] = {NAN, INFINITY, -INFINITY, 0.0};
    for (int i = 0; i < 64; ++i) {  // non-finite components and the zero direction
        double o[3] = {uni(-3, 3), uni(-3, 3), 3.0}, d[3] = {uni(-1, 1), uni(-1, 1), -1.0};
        double* const od = i & 1 ? o : d;
        if (i < 48) od[(i >> 1) % 3] = bad[(i >> 3) % 3];
        else d[0] = d[1] = d[2] = 0.0;
        out.push_back(mk(o, d));
    }
}

// one set of at least 2 * nrays rays: the sphere distribution, its scaled forms (|d|2 <= 1e3: the
// unscaled dir is at most 3 + sqrt(3) long), the adversarial and the non-finite rays of `pos`
inline std::vector<Ray> make_rays(const std::vector<float>& pos, size_t nrays) {
    std::vector<Ray> rays;
    sphere_rays(rays, nrays, 1.0, 1.0);
    sphere_rays(rays, nrays / 8, 1.0, 1e-3);
    sphere_rays(rays, nrays / 8, 1.0, 1e3 / 4.5);
    sphere_rays(rays, nrays / 8, 1e3 / 3.0, 1.0 / 1e3);
    adversarial_rays(rays, pos, nrays);
    return rays;
}

// ---- meshes: T x 9 floats, (a, b, c) per face ---------------------------------------------------
inline bool load(const char* path, std::vector<float>& pos) {
    FILE* f = std::fopen(path, "rb");
    if (!f) return false;
    std::fseek(f, 0, SEEK_END);
    const long n = std::ftell(f);
    std::fseek(f, 0, SEEK_SET);
    pos.resize((size_t)n / 4);
    const size_t got = std::fread(pos.data(), 4, pos.size(), f);
    std::fclose(f);
    return got == pos.size() && n > 0 && pos.size() % 9 == 0;
}

inline std::vector<float> soup(uint32_t T, double spread, double size) {
    std::vector<float> pos(9 * (size_t)T);
    for (uint32_t f = 0; f < T; ++f) {
        const double c[3] = {uni(-spread, spread), uni(-spread, spread), uni(-spread, spread)};
        for (int k = 0; k < 9; ++k) pos[9 * (size_t)f + k] = (float)(c[k % 3] + uni(-size, size));
    }
    return pos;
}

// slivers (one edge 1e-4 .. 1e-7 of the others), zero-area faces and a few huge ones among a soup
inline std::vector<float> slivers(uint32_t T) {
    std::vector<float> pos = soup(T, 1.0, 0.2);
    for (uint32_t f = 0; f < T; f += 3) {
        float* p = &pos[9 * (size_t)f];
        const double s = std::pow(10.0, -4.0 - (f / 3) % 4);
        for (int k = 0; k < 3; ++k) p[6 + k] = (float)(p[k] + s * (p[3 + k] - p[k]) + s * uni(-1, 1) * 0.1);
        if (f % 15 == 0)
            for (int k = 0; k < 3; ++k) p[6 + k] = p[3 + k];  // b == c
        if (f % 33 == 0 && f + 1 < T)
            for (int k = 0; k < 9; ++k) p[9 + k] *= 40.0f;  // the next face: |n|1 large, unculled
    }
    return pos;
}

inline std::vector<float> cube() {
    static const float v[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}};
    static const int q[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {2, 3, 7, 6}, {1, 2, 6, 5}, {0, 4, 7, 3}};
    std::vector<float> pos;
    for (auto& f : q)
        for (int t = 0; t < 2; ++t)
            for (int k : {0, 1 + t, 2 + t})
                for (int j = 0; j < 3; ++j) pos.push_back(v[f[k]][j]);
    return pos;
}

// A smooth displacement of `amp` per vertex position (shared vertices stay shared).
inline std::vector<float> displaced(const std::vector<float>& pos, double amp) {
    std::vector<float> out(pos.size());
    for (size_t v = 0; v < pos.size(); v += 3)
        for (int j = 0; j < 3; ++j) out[v + j] = (float)(pos[v + j] + amp * std::sin(2.5 * pos[v + (j + 1) % 3] + 0.3));
    return out;
}

// The sliver mesh's plain faces moved rigidly, each by a smooth function of its centroid; the
// slivers, the zero-area faces and the huge ones stay where they are, among faces that moved.
inline std::vector<float> slivers_moved(const std::vector<float>& pos, double amp) {
    std::vector<float> out = pos;
    const uint32_t T = (uint32_t)(pos.size() / 9);
    for (uint32_t f = 0; f < T; ++f) {
        if (f % 3 == 0 || (f >= 1 && (f - 1) % 33 == 0)) continue;
        float* p = &out[9 * (size_t)f];
        double c[3], d[3];
        for (int j = 0; j < 3; ++j) c[j] = ((double)p[j] + p[3 + j] + p[6 + j]) / 3.0;
        for (int j = 0; j < 3; ++j) d[j] = amp * std::sin(2.5 * c[(j + 1) % 3] + 0.3);
        for (int k = 0; k < 9; ++k) p[k] = (float)(p[k] + d[k % 3]);
    }
    return out;
}

inline void scale_face(float* p, double s) {  // about its centroid
    double c[3];
    for (int j = 0; j < 3; ++j) c[j] = ((double)p[j] + p[3 + j] + p[6 + j]) / 3.0;
    for (int k = 0; k < 9; ++k) p[k] = (float)(c[k % 3] + (p[k] - c[k % 3]) * s);
}

// ---- the emulations ---------------------------------------------------------------------------
// The device build of one object (accel_dev.hip), step for step on the host.
inline Built emulate_device_build(const std::vector<Hot>& faces, uint32_t node_base, uint32_t slot_base) {
    const uint32_t T = (uint32_t)faces.size();
    Built out;
    std::memset(&out.obj, 0, sizeof out.obj);
    // margin pass: flags, (alpha, beta), centroid bounds and max gamma of the culled faces
    std::vector<double> ab(2 * (size_t)T);
    std::vector<char> unculled(T);
    double lo[3] = {INFINITY, INFINITY, INFINITY}, hi[3] = {-INFINITY, -INFINITY, -INFINITY}, gamma = 0.0;
    for (uint32_t f = 0; f < T; ++f) {
        const FaceMargin m = face_margin_of(faces[f]);
        unculled[f] = !m.culled;
        ab[2 * (size_t)f] = m.alpha;
        ab[2 * (size_t)f + 1] = m.beta;
        if (!m.culled) continue;
        double c[3];
        centroid_of(faces[f], c);
        for (int j = 0; j < 3; ++j) {
            lo[j] = std::fmin(lo[j], c[j]);
            hi[j] = std::fmax(hi[j], c[j]);
        }
        gamma = std::fmax(gamma, m.gamma);
    }
    // key pass: unculled faces to the head in ascending index, (key, index) of the others
    out.hot.resize(T);
    out.index.resize(T);
    std::vector<uint64_t> keys;
    std::vector<uint32_t> ids;
    uint32_t U = 0;
    for (uint32_t f = 0; f < T; ++f) {
        if (unculled[f]) {
            out.hot[U] = faces[f];
            out.index[U++] = f;
            continue;
        }
        double c[3];
        centroid_of(faces[f], c);
        keys.push_back(morton_key(c, lo, hi));
        ids.push_back(f);
    }
    const uint32_t C = T - U;
    std::vector<uint32_t> order(C);
    for (uint32_t p = 0; p < C; ++p) order[p] = p;
    std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return keys[x] < keys[y]; });
    std::vector<uint32_t> sorted(C);
    for (uint32_t p = 0; p < C; ++p) sorted[p] = ids[order[p]] + slot_base;  // (the kernels' g = gbegin + index)
    // levels, deepest first
    const TreeLayout t = tree_layout(C);
    std::vector<Node> nodes((size_t)node_base + t.nodes);  // (global ids, as on the device)
    std::vector<NodeBounds> bounds(nodes.size());
    std::vector<Hot> hot((size_t)slot_base + T);
    std::vector<uint32_t> index((size_t)slot_base + T);
    for (uint32_t level = t.depth; level-- > 0;)
        for (uint32_t j = 0; j < (1u << level); ++j)
            level_node(t, level, j, sorted.data(), slot_base, faces.data(), ab.data(), node_base, slot_base + U, nodes.data(),
                       bounds.data(), hot.data(), index.data());
    for (uint32_t s = U; s < T; ++s) {
        out.hot[s] = hot[slot_base + s];
        out.index[s] = index[slot_base + s];
    }
    out.nodes.assign(nodes.begin() + node_base, nodes.end());
    out.unculled = U;
    out.depth = t.depth;
    out.obj.has = 1;
    out.obj.root = C ? node_base : kNoNode;
    out.obj.ubegin = slot_base;
    out.obj.ucount = U;
    out.obj.gamma = up(C ? gamma : 0.0);
    return out;
}

// The refit of `built` (emulate_device_build's result at these bases, for other positions of the same
// faces) on the faces as they now stand, step for step as accel_refit_device runs it.  false: some
// face changed between culled and unculled (the caller rebuilds).
inline bool emulate_refit(const std::vector<Hot>& faces, const Built& built, uint32_t node_base, uint32_t slot_base, Built* out) {
    const uint32_t T = (uint32_t)faces.size(), U = built.unculled, C = T - U;
    // margin pass: flags, (alpha, beta), max gamma and the counts
    std::vector<double> ab(2 * (size_t)T);
    std::vector<char> unculled(T);
    double gamma = 0.0;
    uint32_t nc = 0, nu = 0;
    for (uint32_t f = 0; f < T; ++f) {
        const FaceMargin m = face_margin_of(faces[f]);
        unculled[f] = !m.culled;
        ab[2 * (size_t)f] = m.alpha;
        ab[2 * (size_t)f + 1] = m.beta;
        (m.culled ? nc : nu) += 1;
        if (m.culled) gamma = std::fmax(gamma, m.gamma);
    }
    // the hierarchy's arrays as they are on the device (global slots and node ids)
    std::vector<Hot> hot((size_t)slot_base + T);
    std::vector<uint32_t> index((size_t)slot_base + T);
    std::copy(built.hot.begin(), built.hot.end(), hot.begin() + slot_base);
    std::copy(built.index.begin(), built.index.end(), index.begin() + slot_base);
    // check pass: every listed face still unculled, its record copy refreshed; the counts unchanged
    bool status = false;
    for (uint32_t k = 0; k < U; ++k) {
        const uint32_t f = index[slot_base + k];
        if (f < T && unculled[f]) hot[slot_base + k] = faces[f];
        else status = true;
    }
    if (status || nc != C || nu != U) return false;
    // levels, deepest first: the sorted order is the index array from the first culled slot, bias 0
    const TreeLayout t = tree_layout(C);
    std::vector<Node> nodes((size_t)node_base + t.nodes);
    std::vector<NodeBounds> bounds(nodes.size());
    for (uint32_t level = t.depth; level-- > 0;)
        for (uint32_t j = 0; j < (1u << level); ++j)
            level_node(t, level, j, index.data() + slot_base + U, 0u, faces.data(), ab.data(), node_base, slot_base + U, nodes.data(),
                       bounds.data(), hot.data(), index.data());
    out->hot.assign(hot.begin() + slot_base, hot.end());
    out->index.assign(index.begin() + slot_base, index.end());
    out->nodes.assign(nodes.begin() + node_base, nodes.end());
    out->unculled = U;
    out->depth = t.depth;
    std::memset(&out->obj, 0, sizeof out->obj);
    out->obj.has = 1;
    out->obj.root = C ? node_base : kNoNode;
    out->obj.ubegin = slot_base;
    out->obj.ucount = U;
    out->obj.gamma = up(C ? gamma : 0.0);
    return true;
}

// accel::check on one object's own arrays (local node ids and slots)
inline const char* check_one(const std::vector<Hot>& faces, const Built& b) {
    const uint32_t T = (uint32_t)faces.size();
    return check(faces.data(), &T, 1, 1, &b.obj, b.nodes.data(), b.nodes.size(), b.hot.data(), b.index.data(), b.index.size());
}

// ---- checker cases ----------------------------------------------------------------------------
// The named corruptions of a valid tree; each must make the checker name `expect`.
struct Corruption {
    const char* name;
    const char* expect;
};
inline constexpr Corruption kCorruptions[] = {
    {"swapped_children", "left child's minimum index"},
    {"shrunk_h", "does not contain its faces"},
    {"lowered_alpha", "alpha is below"},
    {"leaf_out_of_order", "not in ascending index"},
    {"duplicated_slot", "not a permutation"},
    {"wrong_min_index", "is not its subtree's minimum"},
    {"wrong_right_min", "right_min"},
    {"lowered_gamma", "gamma is below"},
    {"unculled_into_tree", "unculled"},
};

// 0: the corruption does not apply to this tree (no inner node, no leaf of two faces ...)
inline int corrupt(const std::vector<Hot>& faces, const Built& good, const Corruption& c) {
    Built b = good;
    const std::string name = c.name;
    int inner = -1, leaf2 = -1;
    for (size_t i = 0; i < b.nodes.size(); ++i) {
        if (!(b.nodes[i].left & kLeafBit)) inner = inner < 0 ? (int)i : inner;
        else if (b.nodes[i].right >= 2) leaf2 = leaf2 < 0 ? (int)i : leaf2;
    }
    if (name == "swapped_children") {
        if (inner < 0) return 0;
        std::swap(b.nodes[inner].left, b.nodes[inner].right);
    } else if (name == "shrunk_h") {
        if (b.nodes.empty()) return 0;
        Node& n = b.nodes[b.nodes.size() / 2];
        int ax = 0;
        for (int j = 1; j < 3; ++j) ax = n.h[j] > n.h[ax] ? j : ax;
        n.h[ax] *= 0.5f;
    } else if (name == "lowered_alpha") {
        if (b.nodes.empty()) return 0;
        b.nodes[0].alpha *= 0.5f;
    } else if (name == "leaf_out_of_order") {
        if (leaf2 < 0) return 0;
        const uint32_t s = b.nodes[leaf2].left & ~kLeafBit;
        std::swap(b.hot[s], b.hot[s + 1]);
        std::swap(b.index[s], b.index[s + 1]);
    } else if (name == "duplicated_slot") {
        if (b.index.size() < 2) return 0;
        b.index[1] = b.index[0];
        b.hot[1] = b.hot[0];
    } else if (name == "wrong_min_index") {
        if (b.nodes.empty()) return 0;
        b.nodes.back().min_index += 1;
    } else if (name == "wrong_right_min") {
        if (inner < 0) return 0;
        b.nodes[inner].right_min += 1;
    } else if (name == "lowered_gamma") {
        if (b.nodes.empty()) return 0;
        b.obj.gamma *= 0.5f;
    } else if (name == "unculled_into_tree") {
        if (!b.obj.ucount) return 0;
        b.obj.ucount -= 1;  // (the last unculled face is claimed for the tree)
    }
    const char* got = check_one(faces, b);
    if (got && std::strstr(got, c.expect)) return 1;
    std::printf("  corruption %s: the checker said \"%s\", expected \"%s\"\n", c.name, got ? got : "(nothing)", c.expect);
    return -1;
}

// ---- threading --------------------------------------------------------------------------------
// [0, n) dealt over at most 16 threads in contiguous blocks: part(begin, end, r) fills one block's
// partial result r; the partial results come back in block order for the caller to sum.
template <class R, class Part>
std::vector<R> deal(size_t n, Part part) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::max<size_t>(1, std::min<size_t>({hw ? hw : 1u, 16u, n / 64 + 1}));
    std::vector<R> out(nt);
    std::vector<std::thread> th;
    const size_t chunk = (n + nt - 1) / nt;
    for (size_t k = 0; k < nt; ++k)
        th.emplace_back([&, k] { part(std::min(n, k * chunk), std::min(n, (k + 1) * chunk), out[k]); });
    for (auto& t : th) t.join();
    return out;
}

// ---- the walk through one tree against the scan -------------------------------------------------
// (a namespace of its own: accel_walk_main and accel_refit_async_main have wider Results)
namespace single_tree {

struct Result {
    uint64_t mismatch = 0, fallback = 0, hits = 0;
};

inline void run_range(const std::vector<Hot>& hot, const Built& b, const std::vector<Ray>& rays, size_t begin, size_t end, Result& res) {
    for (size_t i = begin; i < end; ++i) {
        const Ray& r = rays[i];
        const F3 o{r.o[0], r.o[1], r.o[2]}, d{r.d[0], r.d[1], r.d[2]};
        HostStack st;
        int got = accel_first_face(b.obj, b.nodes.data(), b.index.data(), r.o, r.d, st,
                                   [&](uint32_t slot) { return exact_test(b.hot[slot], o, d); });
        const int want = scan(hot, o, d);
        if (got == kAccelFallback) {
            got = want;  // (the caller's scan)
            ++res.fallback;
        }
        if (want >= 0) ++res.hits;
        if (got != want && res.mismatch++ < 5)
            std::printf("  mismatch ray %zu: walk %d scan %d  o=(%g %g %g) d=(%g %g %g)\n", i, got, want, r.o[0], r.o[1], r.o[2],
                        r.d[0], r.d[1], r.d[2]);
    }
}

inline void run(const std::vector<Hot>& hot, const Built& b, const std::vector<Ray>& rays, Result& res) {
    const auto part = [&](size_t begin, size_t end, Result& q) { run_range(hot, b, rays, begin, end, q); };
    for (const Result& q : deal<Result>(rays.size(), part)) {
        res.mismatch += q.mismatch;
        res.fallback += q.fallback;
        res.hits += q.hits;
    }
}

}  // namespace single_tree

}  // namespace accel_emul
