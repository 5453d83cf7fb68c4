// accel_refit_async_main.cpp — the refit that runs on the stream (accel_dev.hip accel_refit_enqueue)
// emulated on the CPU with the headers its kernels share (accel_margin.hpp, accel_layout.hpp), the
// checker (accel_check.cpp) and the walk the kernel runs (accel_walk.hpp).  No GPU, no HIP.  Compile
// with -ffp-contract=off.
//
//   accel_refit_async_main <sphere2000.bin> [rays]
//
// A scene of two covered objects is built on meshes A (emulate_device_build, as
// tests/cpp/accel_refit_main.cpp; its generators and ray sets, copied) and refitted through ONE
// workspace that is never cleared except by the documented resets (the accumulators and counters):
// the margin pass, the check of the unculled lists, the level passes whatever the verdict, the
// verdict (accel::refit_keeps) and the object record (accel::refit_object).
//   reuse=...         A -> B -> C through the reused workspace: same=1 when nodes, slots, indices and
//                     records equal a synchronous-style refit from A straight to C (emulate_refit),
//                     check=1 when accel::check accepts the scene, top=1 when the order of
//                     refit_top_levels_kernel gives the bytes of the per-level order
//   class_change=...  B -> a mesh with one face's class changed -> B: only=1 when the verdict fails
//                     that object and no other, mismatch: rays (dispatched by the records' `has`)
//                     that differ from the linear scan, healed=1 when the last refit's bytes are
//                     those of a refit that never saw the bad mesh
// tests/test_accel_refit_async_host.py asserts on the figures.
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

int scan(const std::vector<Hot>& hot, F3 o, F3 d) {
    for (size_t f = 0; f < hot.size(); ++f)
        if (exact_test(hot[f], o, d)) return (int)f;
    return -1;
}

// The device build of one object (accel_dev.hip), step for step on the host.
Built emulate_device_build(const std::vector<Hot>& faces, uint32_t node_base, uint32_t slot_base) {
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

// The synchronous refit of one object (accel_refit_device, as tests/cpp/accel_refit_main.cpp emulates
// it): the reference the refit on the stream must equal byte for byte.  false: a class change.
bool emulate_refit(const std::vector<Hot>& faces, const Built& built, uint32_t node_base, uint32_t slot_base, Built* out) {
    const uint32_t T = (uint32_t)faces.size(), U = built.unculled, C = T - U;
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
    std::vector<Hot> hot((size_t)slot_base + T);
    std::vector<uint32_t> index((size_t)slot_base + T);
    std::copy(built.hot.begin(), built.hot.end(), hot.begin() + slot_base);
    std::copy(built.index.begin(), built.index.end(), index.begin() + slot_base);
    bool status = false;
    for (uint32_t k = 0; k < U; ++k) {
        const uint32_t f = index[slot_base + k];
        if (f < T && unculled[f]) hot[slot_base + k] = faces[f];
        else status = true;
    }
    if (status || nc != C || nu != U) return false;
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

std::vector<Hot> records(const std::vector<float>& pos) {
    std::vector<Hot> hot(pos.size() / 9);
    for (size_t f = 0; f < hot.size(); ++f) hot[f] = make_hot(&pos[9 * f]);
    return hot;
}

// ---- the scene as the device holds it, and the refit's persistent workspace -----------------
struct Layout {  // what the refit reads of accel_dev.hip's DevObj
    uint32_t faces, gbegin, index, C, U, node_base, full, extra;
};

struct Arrays {  // the hierarchy's four device arrays
    std::vector<Object> objs;
    std::vector<Node> nodes;
    std::vector<Hot> hot;
    std::vector<uint32_t> index;
};

bool same_bytes(const Arrays& a, const Arrays& b) {
    return a.objs.size() == b.objs.size() && a.nodes.size() == b.nodes.size() && a.hot.size() == b.hot.size() && a.index == b.index &&
           !std::memcmp(a.objs.data(), b.objs.data(), sizeof(Object) * a.objs.size()) &&
           (a.nodes.empty() || !std::memcmp(a.nodes.data(), b.nodes.data(), sizeof(Node) * a.nodes.size())) &&
           (a.hot.empty() || !std::memcmp(a.hot.data(), b.hot.data(), sizeof(Hot) * a.hot.size()));
}

struct Scene {
    std::vector<std::vector<Hot>> faces;  // per object, the records as they now stand
    std::vector<Layout> layout;
    std::vector<Built> built;  // the build's, per object (the synchronous reference starts from them)
    Arrays a;
};

// RefitWorkspace.  Only the accumulators and the counters are reset per refit; the flags, the
// margins and the bounds start as garbage and keep whatever the last refit left.
struct Workspace {
    std::vector<double> gamma;                       // DevAcc (a refit reads its gamma alone)
    std::vector<uint32_t> culled, unculled, status;  // DevCount
    std::vector<uint32_t> flags;
    std::vector<double> ab;
    std::vector<NodeBounds> bounds;
    std::vector<uint32_t> verdict;
    uint32_t refits = 0;
    explicit Workspace(const Scene& s) {
        const size_t n = s.layout.size(), F = s.a.index.size();
        gamma.assign(n, NAN);
        culled.assign(n, 0xdeadbeefu);
        unculled.assign(n, 0xdeadbeefu);
        status.assign(n, 0xdeadbeefu);
        flags.assign(F, 0xdeadbeefu);
        ab.assign(2 * F, NAN);
        bounds.resize(s.a.nodes.size());
        if (!bounds.empty()) std::memset(bounds.data(), 0xff, sizeof(NodeBounds) * bounds.size());
        verdict.assign(n, 1u);
    }
};

// The device build of every object, node and slot bases running on as on the device.
Scene build_scene(const std::vector<std::vector<float>>& pos) {
    Scene s;
    uint32_t node_base = 0, slot = 0;
    for (size_t o = 0; o < pos.size(); ++o) {
        s.faces.push_back(records(pos[o]));
        const uint32_t T = (uint32_t)s.faces[o].size();
        Built b = emulate_device_build(s.faces[o], node_base, slot);
        const TreeLayout t = tree_layout(T - b.unculled);
        s.layout.push_back(Layout{T, slot, (uint32_t)o, T - b.unculled, b.unculled, node_base, t.full, t.extra});
        s.a.objs.push_back(b.obj);
        s.a.nodes.insert(s.a.nodes.end(), b.nodes.begin(), b.nodes.end());
        s.a.hot.insert(s.a.hot.end(), b.hot.begin(), b.hot.end());
        s.a.index.insert(s.a.index.end(), b.index.begin(), b.index.end());
        node_base += (uint32_t)b.nodes.size();
        slot += T;
        s.built.push_back(std::move(b));
    }
    return s;
}

void set_faces(Scene& s, const std::vector<std::vector<float>>& pos) {
    for (size_t o = 0; o < pos.size(); ++o) s.faces[o] = records(pos[o]);
}

// accel_refit_enqueue, kernel for kernel.  top: the levels below first_deep in
// refit_top_levels_kernel's order (per object, kTopBlock lanes per level), else every level in
// refit_level_kernel's (per level, every object).
void refit_async(Scene& s, Workspace& w, bool top) {
    const uint32_t n = (uint32_t)s.layout.size();
    for (uint32_t o = 0; o < n; ++o) {  // refit_reset_kernel
        w.gamma[o] = 0.0;
        w.culled[o] = w.unculled[o] = w.status[o] = 0u;
    }
    for (uint32_t o = 0; o < n; ++o) {  // margin_kernel
        const Layout& ob = s.layout[o];
        for (uint32_t k = 0; k < ob.faces; ++k) {
            const FaceMargin m = face_margin_of(s.faces[o][k]);
            const size_t g = (size_t)ob.gbegin + k;
            w.flags[g] = m.culled ? 0u : 1u;
            w.ab[2 * g] = m.alpha;
            w.ab[2 * g + 1] = m.beta;
            (m.culled ? w.culled[o] : w.unculled[o]) += 1;
            if (m.culled) w.gamma[o] = std::fmax(w.gamma[o], m.gamma);
        }
    }
    for (uint32_t o = 0; o < n; ++o) {  // refit_check_kernel
        const Layout& ob = s.layout[o];
        for (uint32_t k = 0; k < ob.U; ++k) {
            const uint32_t slot = ob.gbegin + k, f = s.a.index[slot];
            if (f < ob.faces && w.flags[ob.gbegin + f] != 0u) s.a.hot[slot] = s.faces[o][f];
            else w.status[o] |= 1u;
        }
    }
    uint32_t max_depth = 0, max_full = 0;
    for (const Layout& ob : s.layout) {
        max_depth = std::max(max_depth, tree_layout(ob.C).depth);
        if (ob.C) max_full = std::max(max_full, ob.full);
    }
    auto lane = [&](uint32_t o, uint32_t level, uint32_t j) {
        const Layout& ob = s.layout[o];
        const TreeLayout t{ob.C, ob.full, ob.extra, 0u, 0u};
        level_node(t, level, j, s.a.index.data() + ob.gbegin + ob.U, 0u, s.faces[o].data(), w.ab.data() + 2 * (size_t)ob.gbegin,
                   ob.node_base, ob.gbegin + ob.U, s.a.nodes.data(), w.bounds.data(), s.a.hot.data(), s.a.index.data());
    };
    if (!s.a.nodes.empty()) {
        const uint32_t first_deep = top ? refit_first_deep(max_full) : 0u;
        for (uint32_t level = max_depth; level-- > first_deep;) {  // refit_level_kernel: whole workgroups of lanes
            const uint32_t lanes = (uint32_t)((((1ull << level) + kTopBlock - 1) / kTopBlock) * kTopBlock);
            for (uint32_t o = 0; o < n; ++o)
                for (uint32_t j = 0; j < lanes; ++j) lane(o, level, j);
        }
        if (first_deep)  // refit_top_levels_kernel
            for (uint32_t o = 0; o < n; ++o)
                for (uint32_t level = std::min(first_deep, max_depth); level-- > 0;)
                    for (uint32_t j = 0; j < kTopBlock; ++j) lane(o, level, j);
    }
    for (uint32_t o = 0; o < n; ++o) {  // refit_object_kernel
        const Layout& ob = s.layout[o];
        const bool keeps = refit_keeps(w.culled[o], w.unculled[o], w.status[o], ob.C, ob.U);
        s.a.objs[ob.index] = refit_object(keeps, ob.C, ob.U, ob.node_base, ob.gbegin, keeps && ob.C ? w.gamma[o] : 0.0);
        w.verdict[o] = keeps ? 1u : 0u;
    }
    ++w.refits;
}

// The scene's arrays after a synchronous-style refit of every object from the build straight to
// the faces as they now stand.  false: some object changed class.
bool reference_refit(const Scene& s, Arrays* out) {
    *out = Arrays{};
    for (size_t o = 0; o < s.layout.size(); ++o) {
        Built r;
        if (!emulate_refit(s.faces[o], s.built[o], s.layout[o].node_base, s.layout[o].gbegin, &r)) return false;
        out->objs.push_back(r.obj);
        out->nodes.insert(out->nodes.end(), r.nodes.begin(), r.nodes.end());
        out->hot.insert(out->hot.end(), r.hot.begin(), r.hot.end());
        out->index.insert(out->index.end(), r.index.begin(), r.index.end());
    }
    return true;
}

const char* check_scene(const Scene& s) {
    std::vector<Hot> all;
    std::vector<uint32_t> sizes;
    for (const std::vector<Hot>& f : s.faces) {
        all.insert(all.end(), f.begin(), f.end());
        sizes.push_back((uint32_t)f.size());
    }
    return check(all.data(), sizes.data(), sizes.size(), 1, s.a.objs.data(), s.a.nodes.data(), s.a.nodes.size(), s.a.hot.data(),
                 s.a.index.data(), s.a.index.size());
}

struct Result {
    uint64_t mismatch = 0, hits = 0, scanned = 0;
};

// Object::intersects per object as the query kernels dispatch it: through the hierarchy where the
// record says has, else (and for a fallback ray) the scan over the object's faces.
void run_range(const Scene& s, const std::vector<Ray>& rays, size_t begin, size_t end, Result& res) {
    for (size_t i = begin; i < end; ++i) {
        const Ray& r = rays[i];
        const F3 o{r.o[0], r.o[1], r.o[2]}, d{r.d[0], r.d[1], r.d[2]};
        for (size_t k = 0; k < s.faces.size(); ++k) {
            const int want = scan(s.faces[k], o, d);
            int got;
            if (s.a.objs[k].has) {
                HostStack st;
                got = accel_first_face(s.a.objs[k], s.a.nodes.data(), s.a.index.data(), r.o, r.d, st,
                                       [&](uint32_t slot) { return exact_test(s.a.hot[slot], o, d); });
                if (got == kAccelFallback) got = want;  // (the caller's scan)
            } else {
                got = scan(s.faces[k], o, d);
                ++res.scanned;
            }
            if (want >= 0) ++res.hits;
            if (got != want && res.mismatch++ < 5) std::printf("  mismatch ray %zu object %zu: got %d scan %d\n", i, k, got, want);
        }
    }
}

Result run(const Scene& s, const std::vector<Ray>& rays) {
    const unsigned hw = std::thread::hardware_concurrency();
    const size_t nt = std::max<size_t>(1, std::min<size_t>({hw ? hw : 1u, 16u, rays.size() / 64 + 1}));
    std::vector<Result> part(nt);
    std::vector<std::thread> th;
    const size_t chunk = (rays.size() + nt - 1) / nt;
    for (size_t k = 0; k < nt; ++k)
        th.emplace_back([&, k] { run_range(s, rays, std::min(rays.size(), k * chunk), std::min(rays.size(), (k + 1) * chunk), part[k]); });
    for (auto& t : th) t.join();
    Result res;
    for (const Result& q : part) {
        res.mismatch += q.mismatch;
        res.hits += q.hits;
        res.scanned += q.scanned;
    }
    return res;
}

std::vector<Ray> make_rays(const std::vector<float>& pos, size_t nrays) {
    std::vector<Ray> rays;
    sphere_rays(rays, nrays, 1.0, 1.0);
    sphere_rays(rays, nrays / 8, 1.0, 1e-3);
    sphere_rays(rays, nrays / 8, 1.0, 1e3 / 4.5);
    sphere_rays(rays, nrays / 8, 1e3 / 3.0, 1.0 / 1e3);
    adversarial_rays(rays, pos, nrays);
    return rays;
}

bool all_kept(const Workspace& w) {
    return std::all_of(w.verdict.begin(), w.verdict.end(), [](uint32_t v) { return v == 1u; });
}

using Meshes = std::vector<std::vector<float>>;

// A -> B -> C through one workspace, in both launch orders, against the refit from A straight to C.
bool reuse(const char* name, const Meshes& A, const Meshes& B, const Meshes& C) {
    Arrays got[2];
    bool kept = true;
    const char* bad = nullptr;
    uint32_t refits = 0;
    for (int top = 0; top < 2; ++top) {
        Scene s = build_scene(A);
        Workspace w(s);
        set_faces(s, B);
        refit_async(s, w, top != 0);
        kept = kept && all_kept(w);
        set_faces(s, C);
        refit_async(s, w, top != 0);
        kept = kept && all_kept(w);
        refits = w.refits;
        got[top] = s.a;
        if (top) {
            Arrays want;
            const bool ref = reference_refit(s, &want);
            bad = check_scene(s);
            if (bad) std::printf("  %s: the refitted scene: %s\n", name, bad);
            const bool same = ref && same_bytes(got[1], want), tops = same_bytes(got[0], got[1]);
            uint32_t faces = 0;
            for (const Layout& ob : s.layout) faces += ob.faces;
            std::printf("reuse=%s objects=%zu faces=%u nodes=%zu refits=%u kept=%d same=%d check=%d top=%d\n", name, s.layout.size(), faces,
                        s.a.nodes.size(), refits, (int)kept, (int)same, (int)!bad, (int)tops);
            return kept && same && !bad && tops && refits == 2;
        }
    }
    return false;
}

// B -> bad (object `obj`'s face changed by `change`, which returns the face or -1) -> B.
template <typename Change>
bool class_change(const char* name, const Meshes& A, const Meshes& B, uint32_t obj, size_t nrays, bool top, Change change) {
    Scene s = build_scene(A);
    Workspace w(s);
    set_faces(s, B);
    refit_async(s, w, top);
    const bool kept_b = all_kept(w);
    const Arrays at_b = s.a;
    Meshes bad = B;
    const int face = change(s.faces[obj], bad[obj]);
    set_faces(s, bad);
    refit_async(s, w, top);  // (the level passes run to the end whatever the verdict)
    bool only = face >= 0;
    for (uint32_t o = 0; o < s.layout.size(); ++o)
        only = only && w.verdict[o] == (o == obj ? 0u : 1u) && s.a.objs[o].has == (o == obj ? 0u : 1u);
    const std::vector<Ray> rays = make_rays(B[0], nrays);
    const Result r = run(s, rays);
    set_faces(s, B);
    refit_async(s, w, top);
    const bool healed = all_kept(w) && same_bytes(s.a, at_b);
    const char* chk = check_scene(s);
    std::printf("class_change=%s object=%u face=%d kept_before=%d only=%d rays=%zu mismatch=%llu hits=%llu scanned=%llu healed=%d check=%d "
                "refits=%u\n",
                name, obj, face, (int)kept_b, (int)only, rays.size(), (unsigned long long)r.mismatch, (unsigned long long)r.hits,
                (unsigned long long)r.scanned, (int)healed, (int)!chk, w.refits);
    return kept_b && only && r.mismatch == 0 && healed && !chk && w.refits == 3;
}

void scale_face(float* p, double s) {  // about its centroid
    double c[3];
    for (int j = 0; j < 3; ++j) c[j] = ((double)p[j] + p[3 + j] + p[6 + j]) / 3.0;
    for (int k = 0; k < 9; ++k) p[k] = (float)(c[k % 3] + (p[k] - c[k % 3]) * s);
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

// A smooth displacement of `amp` per vertex position (shared vertices stay shared).
std::vector<float> displaced(const std::vector<float>& pos, double amp) {
    std::vector<float> out(pos.size());
    for (size_t v = 0; v < pos.size(); v += 3)
        for (int j = 0; j < 3; ++j) out[v + j] = (float)(pos[v + j] + amp * std::sin(2.5 * pos[v + (j + 1) % 3] + 0.3));
    return out;
}

// The sliver mesh's plain faces moved rigidly, each by a smooth function of its centroid; the
// slivers, the zero-area faces and the huge ones stay where they are, among faces that moved.
std::vector<float> slivers_moved(const std::vector<float>& pos, double amp) {
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

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s sphere2000.bin [rays]\n", argv[0]);
        return 2;
    }
    const size_t nrays = argc > 2 ? (size_t)std::atoll(argv[2]) : 50000;
    std::vector<float> s2k;
    if (!load(argv[1], s2k)) {
        std::fprintf(stderr, "cannot read the mesh\n");
        return 2;
    }
    bool ok = true;
    // every mesh behind a small first object, so that its node and slot bases are not zero
    const std::vector<float> first = soup(37, 0.5, 0.1);
    const std::vector<float> firstB = displaced(first, 0.02), firstC = displaced(first, -0.015);
    ok &= reuse("sphere2000", {first, s2k}, {firstB, displaced(s2k, 0.03)}, {firstC, displaced(s2k, -0.02)});
    const std::vector<float> sl = slivers(600);
    ok &= reuse("slivers", {first, sl}, {firstB, slivers_moved(sl, 0.05)}, {firstC, slivers_moved(sl, -0.04)});
    // 1100: levels 0 .. 8 complete and a pairs level 9, all of it inside refit_top_levels_kernel
    for (uint32_t T : {1u, 4u, 5u, 65u, 513u, 1100u}) {
        const std::vector<float> a = soup(T, 0.8, 0.06);
        ok &= reuse(("soup" + std::to_string(T)).c_str(), {first, a}, {firstB, displaced(a, 0.02)}, {firstC, displaced(a, -0.03)});
    }
    // class changes, in either direction, in a scene of the sphere and a crowded soup
    const std::vector<float> crowd = soup(600, 0.25, 0.15);
    // (the crowded soup has faces close to the margin's threshold: it moves by the largest of these
    // amplitudes that keeps every face's class, which the refits to B below then confirm)
    std::vector<float> crowdB = crowd;
    double crowd_amp = 0.0;
    for (double amp : {0.01, 0.003, 0.001, 0.0003, 0.0001}) {
        const std::vector<float> moved = displaced(crowd, amp);
        const std::vector<Hot> a = records(crowd), b = records(moved);
        bool same = true;
        for (size_t f = 0; f < a.size(); ++f) same = same && face_margin_of(a[f]).culled == face_margin_of(b[f]).culled;
        if (same) {
            crowdB = moved;
            crowd_amp = amp;
            break;
        }
    }
    std::printf("crowd_amp=%g\n", crowd_amp);
    ok &= crowd_amp > 0.0;
    const Meshes A{s2k, crowd}, B{displaced(s2k, 0.03), crowdB};
    ok &= class_change("culled_face_scaled_until_n1_is_4", A, B, 0, nrays, true, [](const std::vector<Hot>& rec, std::vector<float>& pos) {
        const int f = 11;
        if (!face_margin_of(rec[f]).culled) return -1;
        for (int i = 0; i < 40; ++i) {
            const Hot r = make_hot(&pos[9 * f]);
            if (std::fabs((double)r.q[6]) + std::fabs((double)r.q[7]) + std::fabs((double)r.q[8]) >= 4.0) return f;
            scale_face(&pos[9 * f], 2.0);
        }
        return -1;
    });
    ok &= class_change("nan_vertex_on_a_culled_face", A, B, 0, nrays, false, [](const std::vector<Hot>& rec, std::vector<float>& pos) {
        const int f = 1234;
        if (!face_margin_of(rec[f]).culled) return -1;
        pos[9 * f + 4] = NAN;
        return f;
    });
    ok &= class_change("unculled_face_of_the_crowded_soup_shrunk", A, B, 1, nrays, true, [](const std::vector<Hot>& rec, std::vector<float>& pos) {
        for (int f = 0; f < (int)rec.size(); ++f) {
            if (face_margin_of(rec[f]).culled) continue;
            for (int i = 0; i < 40; ++i) {
                scale_face(&pos[9 * f], 0.5);
                if (face_margin_of(make_hot(&pos[9 * f])).culled) return f;
            }
            return -1;
        }
        return -1;
    });
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
