// accel_walk_main.cpp — the ray-query hierarchy on the CPU: the builder (accel_build.cpp) and the
// walk the kernel runs (accel_walk.hpp), against a linear scan with one shared f32 predicate.
// No GPU, no HIP.  Compile with -ffp-contract=off.
//
//   accel_walk_main <sphere2000.bin> <sphere20000.bin> [rays]
//
// The .bin files hold T x 9 float32 face positions (a, b, c per face) of
// meshgen.displaced_sphere(T, 42); the soup, the cube and the sliver mesh are generated here.
// Per mesh it prints one line of figures; tests/test_accel_host.py asserts on them:
//   mismatch   rays whose walk result differs from the scan's                     (a)
//   violation  (ray, face) pairs the predicate passes whose leaf or one of its ancestors fails
//              the node test (face not unculled, ray not a fallback ray)          (b)
//   rebuild    1 when a second build gave the same bytes                          (c)
//   deep       1 when the builder refused a tree deeper than a too-small stack    (d)
//   tests_per_ray, unculled, fallback_in_range                                    (e)
// Then sphere2000 and the sliver mesh again, moved and scaled with their rays (moved_suite): the
// same figures (a), (b) and the fallback counts, min(rays, 20000) rays each.
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

using namespace eray::accel;

namespace {

struct F3 {
    float x, y, z;
};
F3 sub(F3 a, F3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
F3 cross(F3 s, F3 o) { return {s.y * o.z - s.z * o.y, s.z * o.x - s.x * o.z, s.x * o.y - s.y * o.x}; }
float dot0(F3 a, F3 b) {
    float acc = 0.0f;
    acc = acc + a.x * b.x;
    acc = acc + a.y * b.y;
    acc = acc + a.z * b.z;
    return acc;
}

// The record of face (a, b, c): e1 = b - a, e2 = c - a, n = e1 x e2 (primitives.rs:44-46).
Hot make_hot(const float* p) {
    const F3 a{p[0], p[1], p[2]}, b{p[3], p[4], p[5]}, c{p[6], p[7], p[8]};
    const F3 e1 = sub(b, a), e2 = sub(c, a), n = cross(e1, e2);
    return Hot{{e1.x, e1.y, e1.z, e2.x, e2.y, e2.z, n.x, n.y, n.z, a.x, a.y, a.z}};
}

// Triangle::intersects with the precomputed record (hit.hpp exact_test), plain f32.
bool exact_test(const Hot& r, F3 o, F3 d) {
    const F3 e1{r.q[0], r.q[1], r.q[2]}, e2{r.q[3], r.q[4], r.q[5]}, n{r.q[6], r.q[7], r.q[8]}, a{r.q[9], r.q[10], r.q[11]};
    if (dot0(n, d) > 0.0f) return false;
    const float det = -dot0(d, n);
    if (!(det >= 1e-6f)) return false;
    const float invdet = 1.0f / det;
    const F3 ao = sub(o, a), dao = cross(ao, d);
    const float u = dot0(e2, dao) * invdet, v = -dot0(e1, dao) * invdet, t = dot0(ao, n) * invdet;
    return t >= 0.0f && u >= 0.0f && v >= 0.0f && (u + v) <= 1.0f;
}

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

std::mt19937_64 g_rng(12345);
double uni(double lo, double hi) { return std::uniform_real_distribution<double>(lo, hi)(g_rng); }
double gauss() { return std::normal_distribution<double>(0.0, 1.0)(g_rng); }

Ray mk(const double* o, const double* d) {
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
void sphere_rays(std::vector<Ray>& out, size_t n, double far, double scale) {
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
void adversarial_rays(std::vector<Ray>& out, const std::vector<float>& pos, size_t n) {
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
        if (i < 48) (i & 1 ? o : d)[(i >> 1) % 3] = bad[(i >> 3) % 3];
        else d[0] = d[1] = d[2] = 0.0;
        out.push_back(mk(o, d));
    }
}

struct Result {
    uint64_t mismatch = 0, violation = 0, fallback = 0, fallback_in_range = 0, face_tests = 0, hits = 0, pairs = 0;
    uint32_t stack_high = 0;
};

int scan(const std::vector<Hot>& hot, F3 o, F3 d) {
    for (size_t f = 0; f < hot.size(); ++f)
        if (exact_test(hot[f], o, d)) return (int)f;
    return -1;
}

void run_range(const std::vector<Hot>& hot, const Built& b, const std::vector<Ray>& rays, size_t property_rays, size_t begin,
               size_t end, Result& res) {
    // parents and the leaf of every culled face, for the property check
    std::vector<uint32_t> parent(b.nodes.size(), kNoNode), leaf_of(hot.size(), kNoNode);
    for (uint32_t i = 0; i < b.nodes.size(); ++i) {
        const Node& n = b.nodes[i];
        if (n.left & kLeafBit) {
            for (uint32_t j = 0; j < n.right; ++j) leaf_of[b.index[(n.left & ~kLeafBit) + j]] = i;
        } else {
            parent[n.left] = i;
            parent[n.right] = i;
        }
    }
    std::vector<char> unculled(hot.size(), 0);
    for (uint32_t j = 0; j < b.obj.ucount; ++j) unculled[b.index[b.obj.ubegin + j]] = 1;
    for (size_t i = begin; i < end; ++i) {
        const Ray& r = rays[i];
        const F3 o{r.o[0], r.o[1], r.o[2]}, d{r.d[0], r.d[1], r.d[2]};
        HostStack st;
        Counters cnt;
        int got = accel_first_face(b.obj, b.nodes.data(), b.index.data(), r.o, r.d, st,
                                   [&](uint32_t slot) { return exact_test(b.hot[slot], o, d); }, &cnt);
        const bool fb = got == kAccelFallback;
        const int want = scan(hot, o, d);
        if (fb) {
            got = want;  // (the caller's scan)
            ++res.fallback;
            if (r.in_range) ++res.fallback_in_range;
        }
        res.face_tests += cnt.face_tests;
        res.stack_high = st.high > res.stack_high ? st.high : res.stack_high;
        if (want >= 0) ++res.hits;
        if (got != want) {
            if (res.mismatch++ < 5)
                std::printf("  mismatch ray %zu: walk %d scan %d  o=(%g %g %g) d=(%g %g %g)\n", i, got, want, r.o[0], r.o[1],
                            r.o[2], r.d[0], r.d[1], r.d[2]);
        }
        if (i >= property_rays || fb) continue;
        float o1, dinf;
        accel_covered(r.o, r.d, o1, dinf);
        for (size_t f = 0; f < hot.size(); ++f) {
            if (unculled[f] || !exact_test(hot[f], o, d)) continue;
            ++res.pairs;
            for (uint32_t nd = leaf_of[f]; nd != kNoNode; nd = parent[nd])
                if (!accel_node_visit(b.nodes[nd], r.o, r.d, o1, dinf, b.obj.gamma)) {
                    if (res.violation++ < 5)
                        std::printf("  violation ray %zu face %zu node %u  o=(%g %g %g) d=(%g %g %g)\n", i, f, nd, r.o[0],
                                    r.o[1], r.o[2], r.d[0], r.d[1], r.d[2]);
                    break;
                }
        }
    }
}

// the rays dealt over a few threads (contiguous blocks), the figures summed
void run(const std::vector<Hot>& hot, const Built& b, const std::vector<Ray>& rays, size_t property_rays, Result& res) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::max<size_t>(1, std::min<size_t>({hw ? hw : 1u, 16u, rays.size() / 64 + 1}));
    std::vector<Result> part(nt);
    std::vector<std::thread> th;
    const size_t chunk = (rays.size() + nt - 1) / nt;
    for (size_t k = 0; k < nt; ++k)
        th.emplace_back([&, k] {
            run_range(hot, b, rays, property_rays, std::min(rays.size(), k * chunk), std::min(rays.size(), (k + 1) * chunk),
                      part[k]);
        });
    for (auto& t : th) t.join();
    for (const Result& q : part) {
        res.mismatch += q.mismatch;
        res.violation += q.violation;
        res.fallback += q.fallback;
        res.fallback_in_range += q.fallback_in_range;
        res.face_tests += q.face_tests;
        res.hits += q.hits;
        res.pairs += q.pairs;
        res.stack_high = std::max(res.stack_high, q.stack_high);
    }
}

bool same_bytes(const Built& x, const Built& y) {
    return x.nodes.size() == y.nodes.size() && x.hot.size() == y.hot.size() && x.index == y.index &&
           (x.nodes.empty() || !std::memcmp(x.nodes.data(), y.nodes.data(), x.nodes.size() * sizeof(Node))) &&
           (x.hot.empty() || !std::memcmp(x.hot.data(), y.hot.data(), x.hot.size() * sizeof(Hot))) &&
           !std::memcmp(&x.obj, &y.obj, sizeof(Object)) && x.depth == y.depth;
}

bool suite(const char* name, const std::vector<float>& pos, size_t nrays, size_t property_rays) {
    const uint32_t T = (uint32_t)(pos.size() / 9);
    std::vector<Hot> hot(T);
    for (uint32_t f = 0; f < T; ++f) hot[f] = make_hot(&pos[9 * (size_t)f]);
    Built b, b2, b3;
    const char* why = "";
    if (!build_object(hot.data(), T, 0, 0, kStackDepth, &b, &why)) {
        std::printf("%s: build refused: %s\n", name, why);
        return false;
    }
    build_object(hot.data(), T, 0, 0, kStackDepth, &b2, &why);
    const bool rebuild = same_bytes(b, b2);
    // a stack too small for this tree must be refused (one level short of what it needs)
    const bool deep = b.depth < 2 || !build_object(hot.data(), T, 0, 0, b.depth - 1, &b3, &why);
    uint32_t bound = 1;
    for (uint64_t leaves = kLeafFaces; leaves < T; leaves *= 2) ++bound;  // ceil(log2(T / leaf)) + 1
    // the slots are a permutation of the faces, byte copies of their records
    std::vector<char> seen(T, 0);
    bool perm = b.index.size() == T;
    for (size_t s = 0; perm && s < b.index.size(); ++s) {
        perm = b.index[s] < T && !seen[b.index[s]] && !std::memcmp(&b.hot[s], &hot[b.index[s]], sizeof(Hot));
        if (perm) seen[b.index[s]] = 1;
    }
    // the sphere distribution alone first (the cap is stated for it), then the adversarial rays
    std::vector<Ray> rays;
    sphere_rays(rays, nrays, 1.0, 1.0);
    Result cap;
    run(hot, b, rays, 0, cap);
    const double per_ray = rays.empty() ? 0.0 : (double)cap.face_tests / (double)rays.size();
    std::vector<Ray> adv;
    sphere_rays(adv, nrays / 8, 1.0, 1e-3);
    sphere_rays(adv, nrays / 8, 1.0, 1e3 / 4.5);  // (|d|2 <= 1e3: the unscaled dir is at most 3 + sqrt(3) long)
    sphere_rays(adv, nrays / 8, 1e3 / 3.0, 1.0 / 1e3);
    adversarial_rays(adv, pos, nrays);
    Result r;
    run(hot, b, adv, property_rays, r);
    Result p;
    run(hot, b, std::vector<Ray>(rays.begin(), rays.begin() + std::min(rays.size(), property_rays)), property_rays, p);
    std::printf(
        "suite=%s faces=%u nodes=%zu depth=%u depth_bound=%u unculled=%u rays=%zu mismatch=%llu violation=%llu "
        "pairs=%llu rebuild=%d deep=%d perm=%d tests_per_ray=%.2f sphere_hits=%llu fallback=%llu fallback_in_range=%llu "
        "stack_high=%u\n",
        name, T, b.nodes.size(), b.depth, bound, b.unculled, rays.size() + adv.size(),
        (unsigned long long)(cap.mismatch + r.mismatch + p.mismatch), (unsigned long long)(r.violation + p.violation),
        (unsigned long long)(r.pairs + p.pairs), (int)rebuild, (int)deep, (int)perm, per_ray, (unsigned long long)cap.hits,
        (unsigned long long)(cap.fallback + r.fallback), (unsigned long long)(cap.fallback_in_range + r.fallback_in_range),
        std::max(cap.stack_high, r.stack_high));
    return cap.mismatch + r.mismatch + p.mismatch + r.violation + p.violation == 0 && rebuild && deep && perm &&
           b.depth <= bound;
}

// The mesh moved to x * s + t and the sphere distribution's rays moved with it (start * s + t,
// direction * s * k), both in double before the rounding to f32: long directions (step 5 of the
// margin proof, where rounding alone can lift det over 1e-6) and meshes far from the origin (the
// |a|1 term of beta).  Every such ray is finite with |o|1 and |d|inf far inside accel_covered's
// range, so in_range is true by construction: none may fall back.
// Every other ray has suite()'s long direction (kLong times the unit distribution's) under the
// same s * k.  With s = 1e-2 and k = 1 a face's n shrinks by 1e-4 and a unit-distribution direction
// by 1e-2: det = -d . n is at most 6e-8 on sphere2000 and Triangle::intersects' det >= 1e-6 fails
// every face, so only the long rays give that setting pairs to check.
constexpr double kLong = 1e3 / 4.5;
bool moved_suite(const char* name, const std::vector<float>& unit, double s, double t, double k, size_t nrays) {
    const uint32_t T = (uint32_t)(unit.size() / 9);
    std::vector<float> pos(unit.size());
    for (size_t i = 0; i < unit.size(); ++i) pos[i] = (float)((double)unit[i] * s + t);
    std::vector<Hot> hot(T);
    for (uint32_t f = 0; f < T; ++f) hot[f] = make_hot(&pos[9 * (size_t)f]);
    Built b;
    const char* why = "";
    if (!build_object(hot.data(), T, 0, 0, kStackDepth, &b, &why)) {
        std::printf("%s: build refused: %s\n", name, why);
        return false;
    }
    std::vector<Ray> rays;
    for (size_t i = 0; i < nrays; ++i) {
        double v[3] = {gauss(), gauss(), gauss()};
        const double l = std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]);
        double o[3], d[3];
        for (int c = 0; c < 3; ++c) {
            const double start = 3.0 * v[c] / l;
            o[c] = start * s + t;
            d[c] = (uni(-1, 1) - start) * (i % 2 ? kLong : 1.0) * s * k;
        }
        Ray r = mk(o, d);
        r.in_range = true;
        rays.push_back(r);
    }
    Result r;
    run(hot, b, rays, rays.size(), r);
    std::printf(
        "suite=%s faces=%u nodes=%zu depth=%u unculled=%u rays=%zu mismatch=%llu violation=%llu pairs=%llu "
        "sphere_hits=%llu fallback=%llu fallback_in_range=%llu stack_high=%u\n",
        name, T, b.nodes.size(), b.depth, b.unculled, rays.size(), (unsigned long long)r.mismatch,
        (unsigned long long)r.violation, (unsigned long long)r.pairs, (unsigned long long)r.hits,
        (unsigned long long)r.fallback, (unsigned long long)r.fallback_in_range, r.stack_high);
    return r.mismatch + r.violation + r.fallback == 0;
}

bool load(const char* path, std::vector<float>& pos) {
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

std::vector<float> soup(uint32_t T, double spread, double size) {
    std::vector<float> pos(9 * (size_t)T);
    for (uint32_t f = 0; f < T; ++f) {
        const double c[3] = {uni(-spread, spread), uni(-spread, spread), uni(-spread, spread)};
        for (int k = 0; k < 9; ++k) pos[9 * (size_t)f + k] = (float)(c[k % 3] + uni(-size, size));
    }
    return pos;
}

// slivers (one edge 1e-4 .. 1e-7 of the others), zero-area faces and a few huge ones among a soup
std::vector<float> slivers(uint32_t T) {
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

std::vector<float> cube() {
    static const float v[8][3] = {{-1, -1, -1}, {1, -1, -1}, {1, 1, -1}, {-1, 1, -1}, {-1, -1, 1}, {1, -1, 1}, {1, 1, 1}, {-1, 1, 1}};
    static const int q[6][4] = {{0, 3, 2, 1}, {4, 5, 6, 7}, {0, 1, 5, 4}, {2, 3, 7, 6}, {1, 2, 6, 5}, {0, 4, 7, 3}};
    std::vector<float> pos;
    for (auto& f : q)
        for (int t = 0; t < 2; ++t)
            for (int k : {0, 1 + t, 2 + t})
                for (int j = 0; j < 3; ++j) pos.push_back(v[f[k]][j]);
    return pos;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 3) {
        std::fprintf(stderr, "usage: %s sphere2000.bin sphere20000.bin [rays]\n", argv[0]);
        return 2;
    }
    const size_t nrays = argc > 3 ? (size_t)std::atoll(argv[3]) : 100000;
    std::vector<float> s2k, s20k;
    if (!load(argv[1], s2k) || !load(argv[2], s20k)) {
        std::fprintf(stderr, "cannot read the meshes\n");
        return 2;
    }
    bool ok = true;
    ok &= suite("sphere2000", s2k, nrays, nrays);
    ok &= suite("sphere20000", s20k, nrays, nrays / 10);
    ok &= suite("soup300", soup(300, 1.0, 0.2), nrays, nrays);
    ok &= suite("cube", cube(), nrays, nrays);
    ok &= suite("slivers", slivers(600), nrays, nrays);
    // (s, t, k) of moved_suite, in this order in the suites' names: _m0 .. _m4
    static const double moves[5][3] = {{1, 0, 1e6}, {1, 1000, 1}, {1, 1000, 1e5}, {1e-2, 5, 1e4}, {1e-2, 0, 1}};
    const std::vector<float> sliver_mesh = slivers(600);
    for (int m = 0; m < 5; ++m) {
        const size_t n = std::min<size_t>(nrays, 20000);
        ok &= moved_suite(("sphere2000_m" + std::to_string(m)).c_str(), s2k, moves[m][0], moves[m][1], moves[m][2], n);
        ok &= moved_suite(("slivers_m" + std::to_string(m)).c_str(), sliver_mesh, moves[m][0], moves[m][1], moves[m][2], n);
    }
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
