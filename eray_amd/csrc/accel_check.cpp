// accel_check.cpp — see accel_check.hpp.
#include "accel_check.hpp"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

#include "accel_margin.hpp"

namespace eray {
namespace accel {
namespace {

thread_local char g_msg[256];

const char* fail(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    std::vsnprintf(g_msg, sizeof g_msg, fmt, ap);
    va_end(ap);
    return g_msg;
}

struct Agg {  // of a subtree
    double lo[3], hi[3], alpha, beta;
    uint32_t min_index, depth;
};

struct Walk {
    const Hot* faces;  // the object's
    const std::vector<FaceMargin>* fm;
    const Node* nodes;
    size_t nnodes;
    const Hot* hot;
    const uint32_t* index;
    uint32_t leaf_begin, leaf_end;  // the object's culled slots
    std::vector<char>* visited;     // per node of the scene
    std::vector<char>* in_leaf;     // per slot of the scene
    size_t obj;
    uint32_t claimed = 0;
    const char* err = nullptr;

    Agg node(uint32_t id, uint32_t level) {
        Agg a{{INFINITY, INFINITY, INFINITY}, {-INFINITY, -INFINITY, -INFINITY}, 0.0, 0.0, 0xffffffffu, level};
        if (id >= nnodes) return err = fail("object %zu: node index %u outside the %zu nodes", obj, id, nnodes), a;
        if ((*visited)[id]) return err = fail("node %u is reachable more than once", id), a;
        (*visited)[id] = 1;
        if (level > 2 * kStackDepth) return err = fail("object %zu: deeper than %u levels at node %u", obj, 2 * kStackDepth, id), a;
        const Node& n = nodes[id];
        if (n.left & kLeafBit) {
            const uint32_t first = n.left & ~kLeafBit, count = n.right;
            if (count < 1 || count > kLeafFaces) return err = fail("leaf %u holds %u faces (1 .. %u allowed)", id, count, kLeafFaces), a;
            if (first < leaf_begin || first > leaf_end || count > leaf_end - first)
                return err = fail("leaf %u's slots [%u, %u) leave its object's culled slots [%u, %u)", id, first, first + count,
                                  leaf_begin, leaf_end), a;
            for (uint32_t k = 0; k < count; ++k) {
                const uint32_t s = first + k, f = index[s];
                if ((*in_leaf)[s]) return err = fail("slot %u is in more than one leaf (leaf %u)", s, id), a;
                (*in_leaf)[s] = 1;
                ++claimed;
                if (k && index[s - 1] >= f) return err = fail("leaf %u's faces are not in ascending index (%u before %u)", id, index[s - 1], f), a;
                const Hot& r = faces[f];
                for (int j = 0; j < 3; ++j) {
                    const double p = r.q[9 + j];
                    for (double v : {p, p + (double)r.q[j], p + (double)r.q[3 + j]}) {
                        a.lo[j] = std::fmin(a.lo[j], v);
                        a.hi[j] = std::fmax(a.hi[j], v);
                    }
                }
                a.alpha = std::fmax(a.alpha, (*fm)[f].alpha);
                a.beta = std::fmax(a.beta, (*fm)[f].beta);
                a.min_index = f < a.min_index ? f : a.min_index;
            }
        } else {
            const Agg l = node(n.left, level + 1);
            if (err) return a;
            const Agg r = node(n.right, level + 1);
            if (err) return a;
            if (!(l.min_index < r.min_index))
                return err = fail("inner node %u: its left child's minimum index %u is not below its right child's %u", id,
                                  l.min_index, r.min_index), a;
            if (n.right_min != r.min_index)
                return err = fail("inner node %u: right_min %u is not its right child's minimum index %u", id, n.right_min, r.min_index), a;
            for (int j = 0; j < 3; ++j) {
                a.lo[j] = std::fmin(l.lo[j], r.lo[j]);
                a.hi[j] = std::fmax(l.hi[j], r.hi[j]);
            }
            a.alpha = std::fmax(l.alpha, r.alpha);
            a.beta = std::fmax(l.beta, r.beta);
            a.min_index = l.min_index;
            a.depth = l.depth > r.depth ? l.depth : r.depth;
        }
        if (n.min_index != a.min_index)
            return err = fail("node %u: min_index %u is not its subtree's minimum %u", id, n.min_index, a.min_index), a;
        for (int j = 0; j < 3; ++j)  // (written so that a NaN fails)
            if (!((double)n.c[j] - (double)n.h[j] <= a.lo[j] && (double)n.c[j] + (double)n.h[j] >= a.hi[j]))
                return err = fail("node %u: its box [c - h, c + h] does not contain its faces on axis %d", id, j), a;
        if (!((double)n.alpha >= a.alpha)) return err = fail("node %u: alpha is below its subtree's maximum", id), a;
        if (!((double)n.beta >= a.beta)) return err = fail("node %u: beta is below its subtree's maximum", id), a;
        return a;
    }
};

}  // namespace

const char* check(const Hot* faces, const uint32_t* sizes, size_t nobj, uint32_t min_faces, const Object* objs,
                  const Node* nodes, size_t nnodes, const Hot* hot, const uint32_t* index, size_t nslots) {
    std::vector<char> visited(nnodes, 0), in_leaf(nslots, 0), owned(nslots, 0);
    size_t begin = 0;
    for (size_t i = 0; i < nobj; begin += sizes[i], ++i) {
        const uint32_t T = sizes[i];
        const Object& ob = objs[i];
        if (T < min_faces) {
            if (ob.has) return fail("object %zu has %u faces, fewer than min_faces %u, but has == %u", i, T, min_faces, ob.has);
            continue;
        }
        if (ob.has != 1) return fail("object %zu of %u faces has no record (has == %u)", i, T, ob.has);
        if (ob.ubegin > nslots || T > nslots - ob.ubegin || ob.ucount > T)
            return fail("object %zu: its slots [%u, %u + %u) or its %u unculled faces do not fit", i, ob.ubegin, ob.ubegin, T, ob.ucount);
        const Hot* of = faces + begin;
        std::vector<char> seen(T, 0);
        for (uint32_t k = 0; k < T; ++k) {
            const uint32_t s = ob.ubegin + k, f = index[s];
            if (owned[s]) return fail("object %zu: slot %u belongs to an earlier object too", i, s);
            owned[s] = 1;
            if (f >= T || seen[f]) return fail("object %zu: its slots are not a permutation of its faces (slot %u: face %u)", i, s, f);
            seen[f] = 1;
            if (std::memcmp(&hot[s], &of[f], sizeof(Hot))) return fail("object %zu: slot %u is not a byte copy of face %u's record", i, s, f);
        }
        std::vector<FaceMargin> fm(T);
        uint32_t u = 0;
        double gamma = 0.0;
        for (uint32_t f = 0; f < T; ++f) {
            fm[f] = face_margin_of(of[f]);
            if (fm[f].culled) {
                gamma = std::fmax(gamma, fm[f].gamma);
                continue;
            }
            if (u >= ob.ucount || index[ob.ubegin + u] != f)
                return fail("object %zu: the unculled list is not the unculled faces in ascending index (face %u, entry %u)", i, f, u);
            ++u;
        }
        if (u != ob.ucount) return fail("object %zu: the unculled list holds %u faces, %u are unculled", i, ob.ucount, u);
        if (!((double)ob.gamma >= gamma)) return fail("object %zu: gamma is below its culled faces' maximum", i);
        const uint32_t C = T - u;
        if (!C) {
            if (ob.root != kNoNode) return fail("object %zu: every face is unculled but root is %u", i, ob.root);
            continue;
        }
        Walk w;
        w.faces = of;
        w.fm = &fm;
        w.nodes = nodes;
        w.nnodes = nnodes;
        w.hot = hot;
        w.index = index;
        w.leaf_begin = ob.ubegin + u;
        w.leaf_end = ob.ubegin + T;
        w.visited = &visited;
        w.in_leaf = &in_leaf;
        w.obj = i;
        const Agg a = w.node(ob.root, 1);
        if (w.err) return w.err;
        if (w.claimed != C) return fail("object %zu: its leaves hold %u of its %u culled faces", i, w.claimed, C);
        uint32_t bound = 1;
        for (uint64_t leaves = kLeafFaces; leaves < C; leaves *= 2) ++bound;
        if (a.depth > bound || a.depth > kStackDepth)
            return fail("object %zu: %u levels, above the balanced bound %u or the stack's %u", i, a.depth, bound, kStackDepth);
    }
    for (size_t k = 0; k < nnodes; ++k)
        if (!visited[k]) return fail("node %zu is not reachable from any object", k);
    return nullptr;
}

}  // namespace accel
}  // namespace eray
