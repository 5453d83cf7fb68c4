// accel_build.cpp — see accel_build.hpp.
#include "accel_build.hpp"

#include <algorithm>
#include <cmath>
#include <cstring>

namespace eray {
namespace accel {
namespace {

struct V3 {
    double x, y, z;
};
V3 e1_of(const Hot& r) { return {r.q[0], r.q[1], r.q[2]}; }
V3 e2_of(const Hot& r) { return {r.q[3], r.q[4], r.q[5]}; }
V3 a_of(const Hot& r) { return {r.q[9], r.q[10], r.q[11]}; }

struct Ctx {
    const Hot* faces;
    const std::vector<FaceMargin>* fm;
    std::vector<double> cx, cy, cz;  // centroids, by original index
    std::vector<uint32_t> ids;       // culled faces, permuted by the splits
    Built* out;
    uint32_t node_base, slot_base, max_depth;
    uint32_t depth = 0;
    bool too_deep = false;
};

// The node of ids[lo .. hi) at `level` (root: 1); returns its local index.
uint32_t build_node(Ctx& c, uint32_t lo, uint32_t hi, uint32_t level) {
    if (level > c.max_depth) {
        c.too_deep = true;
        return 0;
    }
    c.depth = std::max(c.depth, level);
    const uint32_t me = (uint32_t)c.out->nodes.size();
    c.out->nodes.push_back(Node{});
    const uint32_t count = hi - lo;
    double blo[3] = {INFINITY, INFINITY, INFINITY}, bhi[3] = {-INFINITY, -INFINITY, -INFINITY};
    double alpha = 0.0, beta = 0.0;
    uint32_t min_index = 0xffffffffu;
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t f = c.ids[k];
        const Hot& r = c.faces[f];
        const V3 a = a_of(r), e1 = e1_of(r), e2 = e2_of(r);
        const V3 p[3] = {a, {a.x + e1.x, a.y + e1.y, a.z + e1.z}, {a.x + e2.x, a.y + e2.y, a.z + e2.z}};
        for (const V3& v : p) {
            const double q[3] = {v.x, v.y, v.z};
            for (int j = 0; j < 3; ++j) {
                blo[j] = std::min(blo[j], q[j]);
                bhi[j] = std::max(bhi[j], q[j]);
            }
        }
        alpha = std::max(alpha, (*c.fm)[f].alpha);
        beta = std::max(beta, (*c.fm)[f].beta);
        min_index = std::min(min_index, f);
    }
    Node n{};
    for (int j = 0; j < 3; ++j) {
        n.c[j] = (float)(0.5 * (blo[j] + bhi[j]));
        n.h[j] = up(std::max(bhi[j] - (double)n.c[j], (double)n.c[j] - blo[j]));
    }
    n.alpha = up(alpha);
    n.beta = up(beta);
    n.min_index = min_index;
    if (count <= kLeafFaces) {
        std::sort(c.ids.begin() + lo, c.ids.begin() + hi);
        n.left = kLeafBit | (c.slot_base + (uint32_t)c.out->hot.size());
        n.right = count;
        n.right_min = 0xffffffffu;
        for (uint32_t k = lo; k < hi; ++k) {
            c.out->hot.push_back(c.faces[c.ids[k]]);
            c.out->index.push_back(c.ids[k]);
        }
        c.out->nodes[me] = n;
        return me;
    }
    // widest axis of the centroids, then the median by (centroid, index)
    double clo[3] = {INFINITY, INFINITY, INFINITY}, chi[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (uint32_t k = lo; k < hi; ++k) {
        const uint32_t f = c.ids[k];
        const double q[3] = {c.cx[f], c.cy[f], c.cz[f]};
        for (int j = 0; j < 3; ++j) {
            clo[j] = std::min(clo[j], q[j]);
            chi[j] = std::max(chi[j], q[j]);
        }
    }
    int axis = 0;
    for (int j = 1; j < 3; ++j)
        if (chi[j] - clo[j] > chi[axis] - clo[axis]) axis = j;
    const std::vector<double>& key = axis == 0 ? c.cx : axis == 1 ? c.cy : c.cz;
    const uint32_t mid = lo + count / 2;
    std::nth_element(c.ids.begin() + lo, c.ids.begin() + mid, c.ids.begin() + hi, [&](uint32_t x, uint32_t y) {
        return key[x] < key[y] || (key[x] == key[y] && x < y);
    });
    const uint32_t l = build_node(c, lo, mid, level + 1);
    const uint32_t r = c.too_deep ? 0 : build_node(c, mid, hi, level + 1);
    if (c.too_deep) return me;
    const uint32_t lmin = c.out->nodes[l].min_index, rmin = c.out->nodes[r].min_index;
    const bool left_first = lmin < rmin;
    n.left = c.node_base + (left_first ? l : r);
    n.right = c.node_base + (left_first ? r : l);
    n.right_min = left_first ? rmin : lmin;
    c.out->nodes[me] = n;
    return me;
}

}  // namespace

FaceMargin face_margin(const Hot& r) { return face_margin_of(r); }

bool build_object(const Hot* faces, uint32_t T, uint32_t node_base, uint32_t slot_base, uint32_t max_depth, Built* out,
                  const char** why) {
    *out = Built{};
    std::memset(&out->obj, 0, sizeof out->obj);
    std::vector<FaceMargin> fm(T);
    Ctx c;
    c.faces = faces;
    c.fm = &fm;
    c.out = out;
    c.node_base = node_base;
    c.slot_base = slot_base;
    c.max_depth = max_depth;
    c.cx.resize(T);
    c.cy.resize(T);
    c.cz.resize(T);
    double gamma = 0.0;
    for (uint32_t f = 0; f < T; ++f) {
        fm[f] = face_margin(faces[f]);
        if (!fm[f].culled) {  // ascending index: the unculled list
            out->hot.push_back(faces[f]);
            out->index.push_back(f);
            continue;
        }
        const V3 a = a_of(faces[f]), e1 = e1_of(faces[f]), e2 = e2_of(faces[f]);
        c.cx[f] = a.x + (e1.x + e2.x) / 3.0;
        c.cy[f] = a.y + (e1.y + e2.y) / 3.0;
        c.cz[f] = a.z + (e1.z + e2.z) / 3.0;
        c.ids.push_back(f);
        gamma = std::max(gamma, fm[f].gamma);
    }
    out->unculled = (uint32_t)out->hot.size();
    out->obj.has = 1;
    out->obj.root = kNoNode;
    out->obj.ubegin = slot_base;
    out->obj.ucount = out->unculled;
    out->obj.gamma = up(gamma);
    if (!c.ids.empty()) {
        build_node(c, 0, (uint32_t)c.ids.size(), 1);
        if (c.too_deep) {
            *out = Built{};
            if (why) *why = "the hierarchy would be deeper than the traversal stack";
            return false;
        }
        out->obj.root = node_base;
        out->depth = c.depth;
    }
    return true;
}

bool fits_tree_layout(const Built& b, uint32_t faces) {
    const TreeLayout t = tree_layout(faces - b.unculled);
    return b.nodes.size() == t.nodes && b.depth == t.depth;
}

bool build_scene(const Hot* faces, const uint32_t* sizes, size_t nobj, uint32_t min_faces, bool refittable, SceneBuilt* out,
                 size_t* bad_object, const char** why) {
    *out = SceneBuilt{};
    out->objs.resize(nobj);
    if (nobj) std::memset(out->objs.data(), 0, sizeof(Object) * nobj);
    uint32_t begin = 0, blocks = 0, culled = 0;
    for (size_t i = 0; i < nobj; begin += sizes[i], ++i) {
        const uint32_t n = sizes[i];
        if (n < min_faces) continue;
        Built b;
        *bad_object = i;
        *why = "too many nodes";
        if (out->nodes.size() + 2 * (size_t)n > 0x7fffffffu || out->hot.size() + n > 0x7fffffffu) return false;
        const uint32_t node_base = (uint32_t)out->nodes.size(), slot_base = (uint32_t)out->hot.size();
        if (!build_object(faces + begin, n, node_base, slot_base, kStackDepth, &b, why)) return false;
        if (refittable) {
            *why = "the tree is not the shape its face count lays out";
            if (!fits_tree_layout(b, n)) return false;
            const uint32_t C = n - b.unculled;
            const TreeLayout t = tree_layout(C);
            out->layout.push_back(gpu::AccelDevLayout{begin, n, slot_base, blocks, (uint32_t)i, C, b.unculled, culled, node_base, t.full,
                                                      t.extra, 1u});
            blocks += (n + 255u) / 256u;  // (accel_dev.hip's workgroups of 256 faces)
            culled += C;
        }
        out->objs[i] = b.obj;
        out->nodes.insert(out->nodes.end(), b.nodes.begin(), b.nodes.end());
        out->hot.insert(out->hot.end(), b.hot.begin(), b.hot.end());
        out->index.insert(out->index.end(), b.index.begin(), b.index.end());
        ++out->objects;
        out->max_depth = std::max(out->max_depth, b.depth);
        out->faces += n;
        out->unculled += b.unculled;
    }
    *why = "";
    return true;
}

}  // namespace accel
}  // namespace eray
