// accel_walk.hpp — the ray-query hierarchy's records and its walk, for the host and the device
// alike (no HIP type, no HIP call): rays.hip runs it one lane per ray, tests/cpp/accel_walk_main.cpp
// runs the same code on the CPU.  The builder is accel_build.hpp.
//
// WHAT IS SEARCHED.  Object::intersects (object.rs:63-78) returns the first face BY INDEX whose
// Triangle::intersects passes in f32 — not the nearest one.  The walk therefore keeps `best`, the
// smallest passing original index so far, skips every subtree whose smallest index is >= best,
// descends into the child with the smaller minimum first and, in a leaf (ascending indices), stops
// at the first pass or at an index >= best.  The face test itself is the caller's callable on the
// caller's records, so u, v, t are the bits the scan would give.
//
// WHEN A NODE MAY BE SKIPPED.  exact_test (hit.hpp) passing in f32 does not mean that the real line
// meets the real triangle: near det = 1e-6 rounding decides.  accel_build.hpp derives, per face f,
// numbers alpha_f, beta_f, gamma_f such that for every ray (o, d) the proof covers
//
//     exact_test passes  ==>  the real line {o + s d} passes within
//                             rho_f(o, d) = |d|inf * (alpha_f * |o|1 + beta_f) + gamma_f
//                             (Euclidean) of a point of the face's box,
//
// with 1-norms and inf-norms of the ray's floats.  A node stores the box of its faces as a centre c
// and half extents h (floats; [c - h, c + h] holds the real box) and alpha, beta as the maxima
// over its subtree; gamma is kept per object.  The node is visited unless the line provably
// misses the box inflated by 2 * rho per axis (the factor 2 is the builder's safety factor; a point
// within rho of the box in the Euclidean norm lies in the box inflated by rho per axis).
//
// THE NODE TEST divides nothing.  A line misses a box exactly when one of the three axes d x e_k
// separates them (projected along d the box is a hexagon whose edge normals are these axes; a zero
// component of d makes the corresponding tests the plain slab tests, d = 0 passes them all):
//     |m_i d_j - m_j d_i|  >  H_i |d_j| + H_j |d_i|        m = o - c, H = h + 2 rho, (i, j) != k.
// In f32 the left side carries at most 3u S, S = |m_i d_j| + |m_j d_i|, of rounding (u = 2^-24: one
// for m, one per product, one for the difference) and the right side at most 5u R relative (H's
// sum, the products, the sum), each plus 2^-148 of underflow.  The node is skipped only when
//     L > R + 1e-6 * (S + R) + 1e-36
// (1e-6 > 16u), evaluated so that a NaN or an infinity anywhere makes the comparison false: such a
// node is visited.
//
// WHICH RAYS THE PROOF COVERS (accel_covered): every component finite, |o|1 <= kAccelStartMax and
// kAccelDirMin <= |d|inf <= kAccelDirMax (without ERAY_RAYS_NORMALIZE, dir has any length; the
// range keeps every product of the node test far from overflow).  Every other ray is a FALLBACK
// ray: the walk returns kAccelFallback and the caller scans the object's faces in index order, as
// without a hierarchy.  Faces without a margin that holds over that whole range are UNCULLED
// (accel_build.hpp): every ray tests them first, in index order.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ERAY_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define ERAY_HD inline
#endif

namespace eray {
namespace accel {

// A face record as the kernels read it (internal.hpp TriHot, byte for byte):
//   e1.xyz e2.x | e2.yz n.xy | n.z a.xyz
struct alignas(16) Hot {
    float q[12];
};

constexpr uint32_t kLeafBit = 0x80000000u;
constexpr uint32_t kNoNode = 0xffffffffu;
constexpr uint32_t kLeafFaces = 4;  // at most this many faces in a leaf
// The walk's stack: one entry per level below the root at most (the walk pushes one sibling per
// level it descends).  The builder refuses a deeper tree; a balanced split of 2^26 faces (the
// scene limit) into leaves of kLeafFaces is 25 levels deep.
constexpr uint32_t kStackDepth = 32;
constexpr int kAccelFallback = -2;
constexpr float kAccelDirMin = 0x1p-40f, kAccelDirMax = 0x1p40f;
constexpr float kAccelStartMax = 0x1p40f;

struct alignas(16) Node {  // 48 B, three 16-B words
    float c[3], alpha;     // box centre; max alpha_f of the subtree
    float h[3], beta;      // half extents (rounded up); max beta_f of the subtree
    uint32_t left;         // inner: the child with the smaller minimum index; leaf: kLeafBit | first slot
    uint32_t right;        // inner: the other child; leaf: the number of faces (1 .. kLeafFaces)
    uint32_t min_index;    // smallest original face index of the subtree
    uint32_t right_min;    // inner: that of `right`
};
static_assert(sizeof(Node) == 48, "three 16-B words per node");

// Per scene object, 32 B.  Slots index the leaf-ordered face copies and their original indices;
// node indices are into the scene's node array.
struct alignas(16) Object {
    uint32_t has;     // 1: the object is searched through this record
    uint32_t root;    // kNoNode: every face is unculled
    uint32_t ubegin;  // the unculled faces' slots, ascending original index
    uint32_t ucount;
    float gamma;      // max gamma_f of the culled faces
    uint32_t pad[3];
};
static_assert(sizeof(Object) == 32, "two 16-B words per object");

// (diagnostics of the CPU program; the kernel passes none)
struct Counters {
    uint64_t face_tests = 0, node_tests = 0, fallback = 0;
};

ERAY_HD float accel_abs(float x) { return x < 0.0f ? -x : x; }  // (NaN stays NaN)

// Does the margin proof cover ray (o, d) for this object?  Written so that NaN fails.
ERAY_HD bool accel_covered(const float* o, const float* d, float& o1, float& dinf) {
    o1 = accel_abs(o[0]) + accel_abs(o[1]) + accel_abs(o[2]);
    const float ax = accel_abs(d[0]), ay = accel_abs(d[1]), az = accel_abs(d[2]);
    dinf = ax > ay ? ax : ay;
    dinf = az > dinf ? az : dinf;
    // (a NaN component: ax + ay + az is NaN and the last comparison fails)
    return o1 <= kAccelStartMax && dinf >= kAccelDirMin && dinf <= kAccelDirMax && (ax + ay + az) <= 3.0f * kAccelDirMax;
}

// The node test above: false only when the line provably misses the node's inflated box.
ERAY_HD bool accel_node_visit(const Node& n, const float* o, const float* d, float o1, float dinf, float gamma) {
    const float rho2 = 2.0f * (dinf * (n.alpha * o1 + n.beta) + gamma);
    const float m[3] = {o[0] - n.c[0], o[1] - n.c[1], o[2] - n.c[2]};
    const float H[3] = {n.h[0] + rho2, n.h[1] + rho2, n.h[2] + rho2};
    bool miss = false;
    for (int k = 0; k < 3; ++k) {
        const int i = k == 0 ? 1 : 0, j = k == 2 ? 1 : 2;
        const float p = m[i] * d[j], q = m[j] * d[i];
        const float L = accel_abs(p - q), S = accel_abs(p) + accel_abs(q);
        const float R = H[i] * accel_abs(d[j]) + H[j] * accel_abs(d[i]);
        miss = miss || (L > R + 1e-6f * (S + R) + 1e-36f);
    }
    return !miss;
}

// The first face by original index that `test` passes, or -1; kAccelFallback for a ray the proof
// does not cover.  test(slot) runs the exact test on the leaf-ordered record `slot` and keeps its
// u, v, t when it passes: every face the walk tests has an index below `best`, so every pass is
// the new best.  Stack: push(uint32_t), pop() -> uint32_t, empty().
template <class Stack, class FaceTest>
ERAY_HD int accel_first_face(const Object& ob, const Node* nodes, const uint32_t* face_index, const float* o,
                             const float* d, Stack& stack, FaceTest&& test, Counters* cnt = nullptr) {
    float o1, dinf;
    if (!accel_covered(o, d, o1, dinf)) {
        if (cnt) ++cnt->fallback;
        return kAccelFallback;
    }
    uint32_t best = 0xffffffffu;
    for (uint32_t j = 0; j < ob.ucount; ++j) {
        if (cnt) ++cnt->face_tests;
        if (test(ob.ubegin + j)) {
            best = face_index[ob.ubegin + j];
            break;
        }
    }
    uint32_t node = ob.root;
    while (node != kNoNode) {
        const Node n = nodes[node];
        node = kNoNode;
        if (cnt) ++cnt->node_tests;
        if (n.min_index < best && accel_node_visit(n, o, d, o1, dinf, ob.gamma)) {
            if (n.left & kLeafBit) {
                const uint32_t first = n.left & ~kLeafBit;
                for (uint32_t j = 0; j < n.right; ++j) {
                    const uint32_t idx = face_index[first + j];
                    if (idx >= best) break;
                    if (cnt) ++cnt->face_tests;
                    if (test(first + j)) {
                        best = idx;
                        break;
                    }
                }
            } else {
                if (n.right_min < best) stack.push(n.right);
                node = n.left;
            }
        }
        if (node == kNoNode && !stack.empty()) node = stack.pop();
    }
    return best == 0xffffffffu ? -1 : (int)best;
}

}  // namespace accel
}  // namespace eray
