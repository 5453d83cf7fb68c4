// accel_build.hpp — builder of the ray-query hierarchy (accel_walk.hpp), plain host C++: no HIP
// call, no HIP type.  Input: one object's face records as the kernels read them (TriHot bytes).
// Output: the nodes, a leaf-ordered byte copy of the records and the faces' original indices.
//
// THE TRIANGLE is the stored record's: (a, a + e1, a + e2) with the stored floats, evaluated in
// double — not the mesh's original b and c, which the kernels never see.
//
// THE MARGIN (what accel_walk.hpp's node test relies on).  u = 2^-24; |.|1, |.|2, |.|inf norms;
// w = o - a; N = e1 x e2 in reals, n the stored normal; D = -d.N the real determinant;
// g_u = e2.(w x d), g_v = -e1.(w x d) the real numerators of u and v.  exact_test (hit.hpp)
// computes in f32 (no fused operation):
//     det_f = -dot0(d, n)                     and requires det_f >= 1e-6
//     G_u = dot0(e2, cross(fl(o - a), d))     u_f = fl(G_u * fl(1 / det_f))       (v likewise)
// and passes only if u_f >= 0, v_f >= 0, fl(u_f + v_f) <= 1 — so u_f + v_f <= 1 + u.
//  1. det.  The three products and two sums of dot0 give |det_f - (-d.n)| <= 2.01u |d|inf |n|1 +
//     u det_f.  With dn = |n - e1 x e2|1 (measured here in double, whatever produced n):
//         |det_f - D| <= kappa |d|inf + 1.01u det_f,     kappa = 2.01u |n|1 + 1.001 dn + 1e-30
//     (the last term: products that underflow).  For rays with kappa |d|inf <= 0.2e-6 <= 0.2 det_f
//     (longer directions: step 5) this gives D >= 0.75 det_f > 0.
//  2. numerators.  fl(o - a) is within u of w per component, each cross component adds two
//     products and a difference, dot0 three products and two sums: every term of the expansion is
//     off by at most 6.1u of its magnitude, so
//         |G_u - g_u| <= 8u |e2|1 |w|1 |d|inf,       |G_v - g_v| <= 8u |e1|1 |w|1 |d|inf.
//  3. the point Q = a + u_f e1 + v_f e2 lies within u max(|e1|2, |e2|2) of the triangle.  For
//     c = (Q - o) x d:  c.d = 0, c.e2 = u_f D - g_u =: r_u, c.e1 = -(v_f D - g_v) =: -r_v, hence
//     c = (r_u (e1 x d) + r_v (e2 x d)) / D and
//         dist(Q, line) = |c|2 / |d|2 <= (|r_u| |e1|2 + |r_v| |e2|2) / D.
//     r_u = u_f (D - det_f) + (u_f det_f - G_u) + (G_u - g_u); the middle term is the two roundings
//     of the division, at most 2.02u |G_u| <= 2.03u det_f.  With u_f <= 1 + u:
//         |r_u| <= 1.001 kappa |d|inf + 3.1u det_f + 8u |e2|1 |w|1 |d|inf.
//  4. dividing by D >= 0.75 det_f >= 0.75e-6, with |w|1 <= |o|1 + |a|1:
//         dist(triangle, line) <= rho_f = |d|inf (alpha_f |o|1 + beta_f) + gamma_f
//         alpha_f = 8u (|e2|1 |e1|2 + |e1|1 |e2|2) / 0.75e-6
//         beta_f  = 1.001 kappa (|e1|2 + |e2|2) / 0.75e-6 + alpha_f |a|1
//         gamma_f = 5.2u (|e1|2 + |e2|2) + 1e-30
//     The walk inflates a node's box by 2 rho (a safety factor of 2 over this derivation, which
//     also covers the f32 evaluation of rho itself).
//
//  5. long directions.  The threshold 1e-6 is absolute, so step 1 covers a face only up to
//     |d|inf <= 0.2e-6 / kappa; beyond it rounding alone can lift det over 1e-6 and the test's
//     outcome says nothing about the line.  But rho_f grows with |d|inf, and the line contains o:
//         2 rho_f >= 2 |d|inf alpha_f (|o|1 + |a|1) >= 2 |d|inf alpha_f |o - a|2,
//     so once 1.9 alpha_f |d|inf >= 1 the vertex a of the face's box is within 2 rho_f / 1.05 of the
//     line whatever the test said (the 5 % pay for the f32 evaluation of rho).  A face with
//         kappa_f <= 1.9 alpha_f * 0.2e-6                                            (*)
//     is therefore covered for every |d|inf: by steps 1-4 up to 0.2e-6 / kappa_f, trivially above.
//     (For n = fl(e1 x e2), kappa <= (2.01 sqrt 3 + 3.01) u |e1|2 |e2|2 and the right side is at
//     least 8.1u |e1|2 |e2|2, so (*) holds; dn is measured all the same.)
//
// UNCULLED FACES.  A face goes under the tree only if its record and margins are finite, (*) holds
// and alpha_f <= kAlphaMax; the others form the object's unculled list, tested first by every ray
// in index order.  alpha_f > kAlphaMax = 1/4 means 2 rho_f > |o - a| / 2 for a unit direction: the
// margin is as wide as the scene and a node holding the face is never skipped — the cube's faces
// (|n|1 = 4, alpha = 5.1) are cheaper in a list.  No face is dropped: |n|2 < 1e-6 cannot pass for a
// unit direction, but can for a longer one.
//
// THE TREE.  A balanced median split (nth_element, ties by index) of the culled faces' centroids
// on the widest axis, down to leaves of at most kLeafFaces faces in ascending index: depth at most
// ceil(log2(T / kLeafFaces)) + 1.  build_object refuses a tree deeper than `max_depth` (the
// kernel's stack, accel_walk.hpp kStackDepth).  Same input, same bytes out.
#pragma once

#include <cstdint>
#include <vector>

#include "accel_layout.hpp"
#include "accel_margin.hpp"
#include "accel_walk.hpp"

namespace eray {
namespace accel {

// (kAlphaMax, FaceMargin and the margin's arithmetic: accel_margin.hpp, shared with the device build)
FaceMargin face_margin(const Hot& r);

struct Built {
    std::vector<Node> nodes;      // node 0 is the root (when there is one); indices are global
    std::vector<Hot> hot;         // unculled faces first, then the leaves' faces
    std::vector<uint32_t> index;  // the original index of every slot
    Object obj;
    uint32_t depth = 0;           // levels, 0: no tree
    uint32_t unculled = 0;
};

// Builds the hierarchy of `faces[0 .. T)`; node and slot indices in the output start at node_base /
// slot_base (the caller concatenates the objects of a scene).  False, with *why, when the tree
// would be deeper than max_depth.
bool build_object(const Hot* faces, uint32_t T, uint32_t node_base, uint32_t slot_base, uint32_t max_depth, Built* out,
                  const char** why);

// Is b (build_object's result for `faces` faces) the tree that accel_layout.hpp lays out for its
// culled count?  The refit's kernels take every node id and range from tree_layout(C): only such a
// tree may get an AccelDevLayout.
bool fits_tree_layout(const Built& b, uint32_t faces);

// A scene's hierarchy: what eray_scene_build_ray_accel uploads and reports.
struct SceneBuilt {
    std::vector<Object> objs;      // one per object of the scene, zero for those below min_faces
    std::vector<Node> nodes;       // the covered objects' arrays, concatenated in scene order
    std::vector<Hot> hot;
    std::vector<uint32_t> index;
    std::vector<gpu::AccelDevLayout> layout;  // per covered object, when refittable (numbering 1)
    uint32_t objects = 0, max_depth = 0;      // covered objects; levels of the deepest tree
    uint64_t faces = 0, unculled = 0;         // faces of the covered objects; those in unculled lists
};

// build_object for every object of at least min_faces faces of a scene: `faces` holds the objects'
// records one after another, sizes[i] of object i.  False, with the object and *why, when the scene
// would pass 0x7fffffff slots or nodes, a tree would be deeper than kStackDepth or, for refittable,
// a tree is not fits_tree_layout's.
bool build_scene(const Hot* faces, const uint32_t* sizes, size_t nobj, uint32_t min_faces, bool refittable, SceneBuilt* out,
                 size_t* bad_object, const char** why);

}  // namespace accel
}  // namespace eray
