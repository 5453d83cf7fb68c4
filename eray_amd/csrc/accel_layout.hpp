// accel_layout.hpp — the device-side builder's arithmetic (accel_dev.hip), host/device-neutral so
// that tests/cpp/accel_dev_main.cpp runs the same code on the CPU: the Morton key of a centroid,
// the tree's layout from the number of culled faces alone, and the leaf / inner-node functions.
//
// ORDER.  The culled faces of an object are sorted by (key, index): key = 63 bits, 21 per axis of
// the centroid a + (e1 + e2) / 3 quantised in double within the object's centroid bounds (a
// zero-extent axis: code 0).
//
// TOPOLOGY.  The balanced split of that order with the host builder's arithmetic: a range of
// count <= kLeafFaces is a leaf, otherwise mid = lo + count / 2.  The counts of one level differ by
// at most one (count of node j of level L = floor((C + rev_L(j)) / 2^L)), so with
//     F = the first level whose smallest count floor(C / 2^F) is <= kLeafFaces
// levels 0 .. F are complete (2^L nodes, heap numbering 2^L - 1 + j) and at most one more level
// exists: the two leaves under every node of level F that still holds kLeafFaces + 1 faces.  There
// are `extra` = C - kLeafFaces * 2^F such nodes when floor(C / 2^F) == kLeafFaces; the one at
// position j starts at lo = kLeafFaces * j + (how many of them precede it), so its children are
// numbered 2^(F+1) - 1 + 2 (lo - kLeafFaces j) and the next.  Node count and depth are the host
// build's for the same C.  The host build numbers the same shape in recursion order instead
// (PreOrder below): with it level_node refits a host-built tree, whose leaves lie in range order.
#pragma once

#include "accel_margin.hpp"
#include "accel_walk.hpp"

namespace eray {
namespace gpu {

// A covered object as the device builder laid it out (accel_dev.hip; 48 B, uploaded as it stands).
// The refittable host build (accel_build.hpp build_scene) derives the same record from its results;
// cbase is the build's alone.  numbering: how the tree's nodes are numbered — 0 level by level (the
// device build), 1 in recursion order (the host build); one value per scene.
struct AccelDevLayout {
    uint32_t hot_begin, faces, gbegin, block_begin;
    uint32_t index, C, U, cbase;                 // C, U, cbase: the culled / unculled counts, first sorted position
    uint32_t node_base, full, extra, numbering;  // (TreeLayout, LevelOrder / PreOrder below)
};
static_assert(sizeof(AccelDevLayout) == 48, "the kernels' record");

}  // namespace gpu

namespace accel {

// 21 bits of v spread to every third bit
ERAY_HD uint64_t spread3(uint64_t v) {
    v &= 0x1fffffull;
    v = (v | v << 32) & 0x1f00000000ffffull;
    v = (v | v << 16) & 0x1f0000ff0000ffull;
    v = (v | v << 8) & 0x100f00f00f00f00full;
    v = (v | v << 4) & 0x10c30c30c30c30c3ull;
    v = (v | v << 2) & 0x1249249249249249ull;
    return v;
}

// c in [lo, hi] to 0 .. 2^21 - 1
ERAY_HD uint32_t morton_code(double c, double lo, double hi) {
    const double ext = hi - lo;
    if (!(ext > 0.0)) return 0u;
    const double q = (c - lo) / ext * 2097152.0;
    if (!(q > 0.0)) return 0u;
    return q >= 2097151.0 ? 2097151u : (uint32_t)q;
}

ERAY_HD void centroid_of(const Hot& r, double* c) {
    c[0] = (double)r.q[9] + ((double)r.q[0] + (double)r.q[3]) / 3.0;
    c[1] = (double)r.q[10] + ((double)r.q[1] + (double)r.q[4]) / 3.0;
    c[2] = (double)r.q[11] + ((double)r.q[2] + (double)r.q[5]) / 3.0;
}

ERAY_HD uint64_t morton_key(const double* c, const double* lo, const double* hi) {
    return spread3(morton_code(c[0], lo[0], hi[0])) << 2 | spread3(morton_code(c[1], lo[1], hi[1])) << 1 |
           spread3(morton_code(c[2], lo[2], hi[2]));
}

// The tree of C culled faces.
struct TreeLayout {
    uint32_t C;
    uint32_t full;   // F: levels 0 .. F are complete (C > 0)
    uint32_t extra;  // nodes of level F that split once more
    uint32_t nodes;
    uint32_t depth;  // levels (0: no tree)
};

ERAY_HD TreeLayout tree_layout(uint32_t C) {
    TreeLayout t{C, 0u, 0u, 0u, 0u};
    if (!C) return t;
    while ((C >> t.full) > kLeafFaces) ++t.full;
    if ((C >> t.full) == kLeafFaces) t.extra = C - (kLeafFaces << t.full);
    t.nodes = (2u << t.full) - 1u + 2u * t.extra;
    t.depth = t.full + 1u + (t.extra ? 1u : 0u);
    return t;
}

// Node j of the complete level L: its range [lo, lo + n) of the sorted order.
ERAY_HD void node_range(uint32_t C, uint32_t L, uint32_t j, uint32_t& lo, uint32_t& n) {
    lo = 0;
    n = C;
    for (uint32_t k = L; k-- > 0;) {
        const uint32_t half = n / 2;
        if ((j >> k) & 1u) {
            lo += half;
            n -= half;
        } else {
            n = half;
        }
    }
}

ERAY_HD uint32_t node_id(uint32_t L, uint32_t j) { return (1u << L) - 1u + j; }

// The local ids of the children of the inner node j of level L starting at lo (left half first).
ERAY_HD uint32_t first_child(const TreeLayout& t, uint32_t L, uint32_t j, uint32_t lo) {
    return L < t.full ? node_id(L + 1, 2 * j) : node_id(t.full + 1, 0) + 2u * (lo - kLeafFaces * j);
}

// tree_layout(n).nodes for n >= 1 without the loop: with b = floor(log2 n) (n > kLeafFaces), n >> (b - 2)
// is in 4 .. 7; when it is kLeafFaces = 4 the complete levels end at F = b - 2 and n - (4 << F) nodes
// split once more, otherwise at F = b - 1 (n >> F is 2 or 3) and none does.
static_assert(kLeafFaces == 4, "subtree_nodes' closed form");
ERAY_HD uint32_t subtree_nodes(uint32_t n) {
    if (n <= kLeafFaces) return 1u;
    const uint32_t b = 31u - (uint32_t)__builtin_clz(n);
    const bool four = (n >> (b - 2u)) == kLeafFaces;
    const uint32_t F = four ? b - 2u : b - 1u;
    return (2u << F) - 1u + (four ? 2u * (n - (kLeafFaces << F)) : 0u);
}

// NUMBERING.  Which local id the node j of the complete level L gets, and its two children (the
// first half's first), is a compile-time policy of level_node; the topology, the ranges and the
// slots are the same under both.  Either way every id is a function of C, L and j alone.
//
// LevelOrder: the device builder's (accel_dev.hip level_kernel), level by level as described above.
struct LevelOrder {
    static ERAY_HD uint32_t id(uint32_t, uint32_t L, uint32_t j) { return node_id(L, j); }
    static ERAY_HD void children(const TreeLayout& t, uint32_t L, uint32_t j, uint32_t lo, uint32_t, uint32_t, uint32_t& c0,
                                 uint32_t& c1) {
        c0 = first_child(t, L, j, lo);
        c1 = c0 + 1u;
    }
};

// PreOrder: the host builder's (accel_build.cpp build_node pushes a node, then its first half's
// subtree, then its second half's).  The root is 0; a node `me` over n faces has its first child at
// me + 1 and its second at me + 1 + subtree_nodes(n / 2).  id() walks the halves node_range walks:
// O(L) steps per lane, no table, no scratch.
struct PreOrder {
    static ERAY_HD uint32_t id(uint32_t C, uint32_t L, uint32_t j) {
        uint32_t me = 0, n = C;
        for (uint32_t k = L; k-- > 0;) {
            const uint32_t half = n / 2;
            if ((j >> k) & 1u) {
                me += 1u + subtree_nodes(half);
                n -= half;
            } else {
                me += 1u;
                n = half;
            }
        }
        return me;
    }
    // me: id(C, L, j); n: the node's count (node_range), above kLeafFaces
    static ERAY_HD void children(const TreeLayout&, uint32_t, uint32_t, uint32_t, uint32_t n, uint32_t me, uint32_t& c0,
                                 uint32_t& c1) {
        c0 = me + 1u;
        c1 = c0 + subtree_nodes(n / 2);
    }
};

// A node's real box and margins before rounding (temporary, one per node).
struct NodeBounds {
    double lo[3], hi[3], alpha, beta;
};

// c, h, alpha, beta rounded as the host builder rounds them: [c - h, c + h] holds [lo, hi].
ERAY_HD void round_node(const NodeBounds& b, Node& n) {
    for (int j = 0; j < 3; ++j) {
        n.c[j] = (float)(0.5 * (b.lo[j] + b.hi[j]));
        const double p = b.hi[j] - (double)n.c[j], q = (double)n.c[j] - b.lo[j];
        n.h[j] = up(p > q ? p : q);
    }
    n.alpha = up(b.alpha);
    n.beta = up(b.beta);
}

// The leaf of ids[0 .. count) (1 <= count <= kLeafFaces original indices, any order): sorted
// ascending, copied with their records to slots [slot, slot + count), with the box of the faces'
// vertices (a, a + e1, a + e2) in double.  alpha_beta[2 f], [2 f + 1]: the margins of face f.
ERAY_HD void make_leaf(const uint32_t* ids, uint32_t count, const Hot* faces, const double* alpha_beta, uint32_t slot,
                       Hot* hot, uint32_t* index, Node& node, NodeBounds& nb) {
    uint32_t s[kLeafFaces];
    for (uint32_t k = 0; k < kLeafFaces; ++k) s[k] = k < count ? ids[k] : 0xffffffffu;
    for (uint32_t a = 1; a < kLeafFaces; ++a)  // (insertion sort of four words)
        for (uint32_t b = a; b > 0 && s[b] < s[b - 1]; --b) {
            const uint32_t t = s[b];
            s[b] = s[b - 1];
            s[b - 1] = t;
        }
    for (int j = 0; j < 3; ++j) {
        nb.lo[j] = INFINITY;
        nb.hi[j] = -INFINITY;
    }
    nb.alpha = 0.0;
    nb.beta = 0.0;
    for (uint32_t k = 0; k < kLeafFaces; ++k) {
        if (k >= count) break;
        const uint32_t f = s[k];
        const Hot r = faces[f];
        hot[slot + k] = r;
        index[slot + k] = f;
        for (int j = 0; j < 3; ++j) {
            const double a = r.q[9 + j];
            const double v[3] = {a, a + (double)r.q[j], a + (double)r.q[3 + j]};
            for (int i = 0; i < 3; ++i) {
                nb.lo[j] = v[i] < nb.lo[j] ? v[i] : nb.lo[j];
                nb.hi[j] = v[i] > nb.hi[j] ? v[i] : nb.hi[j];
            }
        }
        const double al = alpha_beta[2 * (size_t)f], be = alpha_beta[2 * (size_t)f + 1];
        nb.alpha = al > nb.alpha ? al : nb.alpha;
        nb.beta = be > nb.beta ? be : nb.beta;
    }
    round_node(nb, node);
    node.left = kLeafBit | slot;
    node.right = count;
    node.min_index = s[0];
    node.right_min = 0xffffffffu;
}

// The inner node over children l and r (global ids; their nodes and bounds are written): `left`
// is the child with the smaller minimum index.
ERAY_HD void make_inner(uint32_t l, uint32_t r, const Node* nodes, const NodeBounds* bounds, Node& node, NodeBounds& nb) {
    const NodeBounds x = bounds[l], y = bounds[r];
    for (int j = 0; j < 3; ++j) {
        nb.lo[j] = x.lo[j] < y.lo[j] ? x.lo[j] : y.lo[j];
        nb.hi[j] = x.hi[j] > y.hi[j] ? x.hi[j] : y.hi[j];
    }
    nb.alpha = x.alpha > y.alpha ? x.alpha : y.alpha;
    nb.beta = x.beta > y.beta ? x.beta : y.beta;
    round_node(nb, node);
    const uint32_t lmin = nodes[l].min_index, rmin = nodes[r].min_index;
    const bool left_first = lmin < rmin;
    node.left = left_first ? l : r;
    node.right = left_first ? r : l;
    node.min_index = left_first ? lmin : rmin;
    node.right_min = left_first ? rmin : lmin;
}

// One lane's work at `level` (0: the root) of the tree t, lane j: node j of a complete level, or
// (level == t.full + 1) the two leaves under node j of level t.full when it splits once more.
// Levels are run deepest first, so an inner node finds its children written.  sorted: the culled
// faces in (key, index) order, each entry its original index + id_bias; slot0: the slot of
// sorted[0]; nodes / bounds are the scene's, the tree's node k at node_base + k, k by Numbering.
// Every node id, range and slot below comes from C, full, extra, level and j; none from a face
// value or from what `sorted` holds (accel_dev.hip accel_refit_enqueue relies on it).
template <class Numbering = LevelOrder>
ERAY_HD void level_node(const TreeLayout& t, uint32_t level, uint32_t j, const uint32_t* sorted, uint32_t id_bias,
                        const Hot* faces, const double* alpha_beta, uint32_t node_base, uint32_t slot0, Node* nodes,
                        NodeBounds* bounds, Hot* hot, uint32_t* index) {
    const bool pairs = level == t.full + 1;
    if (!t.C || (level > t.full && !(pairs && t.extra))) return;
    const uint32_t L = pairs ? t.full : level;
    if (j >= (1u << L)) return;
    uint32_t lo, n;
    node_range(t.C, L, j, lo, n);
    const uint32_t me = Numbering::id(t.C, L, j);
    uint32_t first[2] = {lo, lo + n / 2}, count[2] = {n, 0u}, id[2] = {node_base + me, 0u};
    uint32_t leaves = n <= kLeafFaces ? 1u : 0u;
    uint32_t c0 = 0, c1 = 0;  // the children, local ids
    if (n > kLeafFaces) Numbering::children(t, L, j, lo, n, me, c0, c1);
    if (pairs) {
        if (n <= kLeafFaces) return;
        leaves = 2;
        count[0] = n / 2;
        count[1] = n - n / 2;
        id[0] = node_base + c0;
        id[1] = node_base + c1;
    }
    for (uint32_t k = 0; k < 2; ++k) {
        if (k >= leaves) break;
        uint32_t f[kLeafFaces];
        for (uint32_t q = 0; q < kLeafFaces; ++q) f[q] = q < count[k] ? sorted[first[k] + q] - id_bias : 0u;
        Node nd;
        NodeBounds nb;
        make_leaf(f, count[k], faces, alpha_beta, slot0 + first[k], hot, index, nd, nb);
        nodes[id[k]] = nd;
        bounds[id[k]] = nb;
    }
    if (leaves) return;
    Node nd;
    NodeBounds nb;
    make_inner(node_base + c0, node_base + c1, nodes, bounds, nd, nb);
    nodes[id[0]] = nd;
    bounds[id[0]] = nb;
}

// The refit's verdict on one covered object (accel_dev.hip refit_object_kernel, and the host's
// comparison in accel_refit_device): the topology laid out for C culled and U unculled faces still
// fits when the margin pass counted the same classes and the check pass found every listed
// unculled face still unculled (status 0).  Counts and flags only: no face value is looked at, so
// NaN, infinite or huge faces (which have no provable margin: unculled) simply change the counts.
ERAY_HD bool refit_keeps(uint32_t culled, uint32_t unculled, uint32_t status, uint32_t C, uint32_t U) {
    return status == 0u && culled == C && unculled == U;
}

// The object record after a refit on the stream: on a pass what the build writes (object_kernel);
// otherwise has = 0, and the query kernels scan the object as without a hierarchy until a later
// refit passes.  gamma: the max gamma_f of the culled faces as the margin pass reduced it.
ERAY_HD Object refit_object(bool keeps, uint32_t C, uint32_t U, uint32_t node_base, uint32_t slot_base, double gamma) {
    Object r{};
    if (!keeps) return r;
    r.has = 1;
    r.root = C ? node_base : kNoNode;
    r.ubegin = slot_base;
    r.ucount = U;
    r.gamma = up(C ? gamma : 0.0);
    return r;
}

// Levels 0 .. kTopLevels - 1 of a tree hold at most kTopBlock nodes each: one workgroup of
// kTopBlock lanes runs them in one launch (refit_top_levels_kernel), deepest first with a barrier
// between levels.  The pairs level full + 1 has one lane per node of level `full`, so it fits as
// well when full < kTopLevels.  first_deep: the shallowest level that per-level launches ran
// (kTopLevels when some tree has a complete level kTopLevels, else kTopLevels + 1: level kTopLevels
// is then at most the pairs level of trees with full == kTopLevels - 1).
constexpr uint32_t kTopBlock = 256, kTopLevels = 9;
static_assert((1u << (kTopLevels - 1)) == kTopBlock, "the last top level fills the workgroup");
ERAY_HD uint32_t refit_first_deep(uint32_t max_full) { return max_full >= kTopLevels ? kTopLevels : kTopLevels + 1u; }

}  // namespace accel
}  // namespace eray
