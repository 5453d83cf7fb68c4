// accel_refit_hosttree_main.cpp — the refit of a HOST-built ray-query hierarchy
// (eray_scene_build_ray_accel_refittable; accel_dev.hip's refit kernels in their recursion-order
// instantiation) on the CPU: accel_build.cpp's build_object on a mesh A, then the refit emulated
// step for step as accel_refit_device runs it — the margin pass, the check of the unculled list,
// accel_layout.hpp's level_node<PreOrder> over the hierarchy's own index array, the object record —
// on A itself and on a deformed mesh B of the same faces, the checker (accel_check.cpp) and the walk
// the kernel runs (accel_walk.hpp).  The meshes, the ray sets, the named corruptions and the walk are
// accel_emul.hpp's.  No GPU, no HIP.  Compile with -ffp-contract=off.
//
//   accel_refit_hosttree_main <sphere2000.bin> [rays]
//
// One line for the numbering:
//   ids        trees (C = 1 .. 5000) whose arithmetic ids were compared with a recursion that numbers
//              as build_node does; id_errors / range_errors / coverage_errors / count_errors: nodes
//              whose id or range differs, ids not hit exactly once, C whose closed-form node count
//              differs from tree_layout's
// Per mesh one line of figures; tests/test_accel_refit_hosttree_host.py asserts on them:
//   identity   1 when the refit with B = A reproduces the build's nodes, record copies, indices and
//              object record byte for byte
//   check      1 when accel::check accepts the refitted tree against B's faces
//   mismatch   rays whose walk through the refitted tree differs from the linear scan over B
//   topology   1 when the index array and every node's left, right, min_index and right_min words are
//              the build's (they depend on face indices only)
//   moved      nodes whose bytes differ between A's tree and the refitted one (the refit did work)
//   caught     how many of the named corruptions of the refitted tree the checker names
// one line per class change that the refit must refuse (detected=1), and one line for a scene of three
// objects, the middle one below min_faces, built by accel_build.cpp's build_scene as
// eray_scene_build_ray_accel_refittable builds it:
//   slices     1 when every covered object's slice of the concatenated arrays and its record are
//              build_object's alone at those bases, and the uncovered object's record is zero
//   layout     1 when every AccelDevLayout field is what the scene's sizes and tree_layout give
//   refit      1 when the refit of the unmoved scene through that layout, emulated as the kernels run
//              it over the scene's arrays, reproduces them byte for byte
//   c0, extra0, c2, extra2: the covered objects' culled counts and nodes of level `full` that split
#include "accel_emul.hpp"

using namespace eray::accel;
using namespace accel_emul;
using namespace accel_emul::single_tree;

namespace {

std::vector<std::string> g_caught;  // the corruptions that some mesh exercised and the checker named

// ---- the numbering ------------------------------------------------------------------------------
struct IdCheck {
    uint32_t C;
    TreeLayout t;
    uint32_t next = 0;
    uint64_t id_errors = 0, range_errors = 0;
    // build_node's order: the node, its first half's subtree, its second half's; returns the id
    uint32_t walk(uint32_t lo, uint32_t n, uint32_t L, uint32_t j) {
        const uint32_t me = next++;
        if (L <= t.full) {  // a node of a complete level: its id and range by arithmetic
            uint32_t alo, an;
            node_range(C, L, j, alo, an);
            range_errors += alo != lo || an != n;
            id_errors += PreOrder::id(C, L, j) != me;
        }
        if (n <= kLeafFaces) return me;
        const uint32_t half = n / 2;
        uint32_t c0, c1;
        PreOrder::children(t, L, j, lo, n, me, c0, c1);
        const uint32_t l = walk(lo, half, L + 1, 2 * j), r = walk(lo + half, n - half, L + 1, 2 * j + 1);
        id_errors += (c0 != l) + (c1 != r);
        return me;
    }
};

bool check_ids(uint32_t max_c) {
    uint64_t id_errors = 0, range_errors = 0, coverage_errors = 0, count_errors = 0;
    for (uint32_t C = 1; C <= max_c; ++C) {
        IdCheck k{C, tree_layout(C)};
        k.walk(0, C, 0, 0);
        id_errors += k.id_errors;
        range_errors += k.range_errors;
        count_errors += k.next != k.t.nodes || subtree_nodes(C) != k.t.nodes;
        // the ids the kernels compute, level by level: every one of 0 .. nodes - 1 exactly once
        std::vector<uint32_t> seen(k.t.nodes, 0u);
        const auto mark = [&](uint32_t id) {
            if (id < seen.size()) ++seen[id];
            else ++coverage_errors;
        };
        for (uint32_t L = 0; L <= k.t.full; ++L)
            for (uint32_t j = 0; j < (1u << L); ++j) {
                const uint32_t me = PreOrder::id(C, L, j);
                mark(me);
                uint32_t lo, n;
                node_range(C, L, j, lo, n);
                if (L == k.t.full && n > kLeafFaces) {  // the pairs level
                    uint32_t c0, c1;
                    PreOrder::children(k.t, L, j, lo, n, me, c0, c1);
                    mark(c0);
                    mark(c1);
                }
            }
        for (uint32_t s : seen) coverage_errors += s != 1u;
    }
    std::printf("ids=%u id_errors=%llu range_errors=%llu coverage_errors=%llu count_errors=%llu\n", max_c,
                (unsigned long long)id_errors, (unsigned long long)range_errors, (unsigned long long)coverage_errors,
                (unsigned long long)count_errors);
    return !id_errors && !range_errors && !coverage_errors && !count_errors;
}

// ---- the refit of a host-built tree --------------------------------------------------------------
// accel_emul.hpp's emulate_refit with the one difference the kernels have: level_node numbers the
// nodes in recursion order.  `built` is build_object's result at these bases.
bool emulate_refit_preorder(const std::vector<Hot>& faces, const Built& built, uint32_t node_base, uint32_t slot_base, Built* out) {
    const uint32_t T = (uint32_t)faces.size(), U = built.unculled, C = T - U;
    std::vector<double> ab(2 * (size_t)T);
    std::vector<char> unculled(T);
    double gamma = 0.0;
    uint32_t nc = 0, nu = 0;
    for (uint32_t f = 0; f < T; ++f) {  // margin pass
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
    for (uint32_t k = 0; k < U; ++k) {  // check pass
        const uint32_t f = index[slot_base + k];
        if (f < T && unculled[f]) hot[slot_base + k] = faces[f];
        else status = true;
    }
    if (!refit_keeps(nc, nu, status ? 1u : 0u, C, U)) return false;
    if (!fits_tree_layout(built, T)) return false;  // (what build_scene checks before it records a layout)
    const TreeLayout t = tree_layout(C);
    std::vector<Node> nodes((size_t)node_base + t.nodes);
    std::vector<NodeBounds> bounds(nodes.size());
    for (uint32_t level = t.depth; level-- > 0;)  // levels, deepest first
        for (uint32_t j = 0; j < (1u << level); ++j)
            level_node<PreOrder>(t, level, j, index.data() + slot_base + U, 0u, faces.data(), ab.data(), node_base, slot_base + U,
                                 nodes.data(), bounds.data(), hot.data(), index.data());
    out->hot.assign(hot.begin() + slot_base, hot.end());
    out->index.assign(index.begin() + slot_base, index.end());
    out->nodes.assign(nodes.begin() + node_base, nodes.end());
    out->unculled = U;
    out->depth = t.depth;
    out->obj = refit_object(true, C, U, node_base, slot_base, gamma);
    return true;
}

bool host_build(const std::vector<Hot>& faces, uint32_t node_base, uint32_t slot_base, Built* out) {
    const char* why = "";
    if (build_object(faces.data(), (uint32_t)faces.size(), node_base, slot_base, kStackDepth, out, &why)) return true;
    std::printf("  build_object: %s\n", why);
    return false;
}

bool same_bytes(const Built& a, const Built& b) {
    return a.nodes.size() == b.nodes.size() && a.hot.size() == b.hot.size() && a.index == b.index &&
           (a.nodes.empty() || !std::memcmp(a.nodes.data(), b.nodes.data(), sizeof(Node) * a.nodes.size())) &&
           (a.hot.empty() || !std::memcmp(a.hot.data(), b.hot.data(), sizeof(Hot) * a.hot.size())) &&
           !std::memcmp(&a.obj, &b.obj, sizeof(Object)) && a.unculled == b.unculled && a.depth == b.depth;
}

// The host build on A, the refit on A and on B (the same faces, moved), at bases other than zero.
bool suite(const char* name, const std::vector<float>& posA, const std::vector<float>& posB, size_t nrays) {
    const uint32_t node_base = 5, slot_base = 300;
    const std::vector<Hot> A = records(posA), B = records(posB);
    const uint32_t T = (uint32_t)A.size();
    Built built;
    if (!host_build(A, node_base, slot_base, &built)) return false;
    bool same_class = true;
    for (uint32_t f = 0; f < T; ++f) same_class = same_class && face_margin_of(A[f]).culled == face_margin_of(B[f]).culled;
    Built same, refit;
    const bool identity = emulate_refit_preorder(A, built, node_base, slot_base, &same) && same_bytes(same, built);
    const bool kept = emulate_refit_preorder(B, built, node_base, slot_base, &refit);
    if (!same_class || !kept) {
        std::printf("%s: same_class=%d kept=%d: the deformation must keep every face's class\n", name, (int)same_class, (int)kept);
        return false;
    }
    bool topology = refit.index == built.index && refit.nodes.size() == built.nodes.size();
    size_t moved = 0;
    for (size_t i = 0; topology && i < refit.nodes.size(); ++i) {
        const Node &x = refit.nodes[i], &y = built.nodes[i];
        topology = x.left == y.left && x.right == y.right && x.min_index == y.min_index && x.right_min == y.right_min;
        moved += std::memcmp(&x, &y, sizeof(Node)) != 0;
    }
    // the checker and the walk take an object's own arrays: local node ids and slots
    Built local = refit;
    for (Node& n : local.nodes) {
        if (n.left & kLeafBit) n.left -= slot_base;
        else n.left -= node_base, n.right -= node_base;
    }
    local.obj.ubegin = 0;
    if (local.obj.root != kNoNode) local.obj.root = 0;
    const char* bad = check_one(B, local);
    if (bad) std::printf("  %s: the refitted tree: %s\n", name, bad);
    int caught = 0, failed = 0;
    for (const Corruption& c : kCorruptions) {
        const int r = bad ? 0 : corrupt(B, local, c);
        if (r > 0) {
            ++caught;
            if (std::find(g_caught.begin(), g_caught.end(), c.name) == g_caught.end()) g_caught.push_back(c.name);
        }
        failed += r < 0;
    }
    const std::vector<Ray> rays = make_rays(posB, nrays);
    Result r;
    if (!bad) run(B, local, rays, r);  // (an invalid tree may not be walked)
    std::printf(
        "suite=%s faces=%u nodes=%zu depth=%u unculled=%u rays=%zu mismatch=%llu hits=%llu fallback=%llu check=%d identity=%d "
        "topology=%d moved=%zu caught=%d corruption_failed=%d\n",
        name, T, refit.nodes.size(), refit.depth, refit.unculled, rays.size(), (unsigned long long)r.mismatch,
        (unsigned long long)r.hits, (unsigned long long)r.fallback, (int)!bad, (int)identity, (int)topology, moved, caught, failed);
    return !bad && identity && topology && !failed && r.mismatch == 0;
}

// A class change the refit must refuse: the host build on A, then B = A with one face changed by
// `change` (which returns the face it changed, or -1 when the mesh has none of the kind).
template <typename Change>
bool refused(const char* name, const std::vector<float>& posA, Change change) {
    const std::vector<Hot> A = records(posA);
    Built built, out;
    if (!host_build(A, 0, 0, &built)) return false;
    std::vector<float> posB = posA;
    const int face = change(A, posB);
    const bool detected = face >= 0 && !emulate_refit_preorder(records(posB), built, 0, 0, &out);
    std::printf("class_change=%s face=%d detected=%d\n", name, face, (int)detected);
    return detected;
}

// ---- a scene through build_scene ------------------------------------------------------------------
// The first faces of a soup that hold exactly `culled` culled ones.
std::vector<Hot> soup_with_culled(uint32_t culled) {
    const std::vector<Hot> all = records(soup(2 * culled + 64, 0.8, 0.06));
    std::vector<Hot> out;
    for (uint32_t f = 0, c = 0; f < all.size() && c < culled; ++f) {
        out.push_back(all[f]);
        c += face_margin_of(all[f]).culled;
    }
    return out;
}

// The refit kernels' passes over a scene's arrays (accel_dev.hip accel_refit_device), every id and
// range from the layout records: false on a class change.
bool emulate_scene_refit(const std::vector<Hot>& faces, const std::vector<eray::gpu::AccelDevLayout>& layout, uint32_t max_depth,
                         SceneBuilt* sc) {
    std::vector<double> ab(2 * sc->hot.size());
    std::vector<NodeBounds> bounds(sc->nodes.size());
    std::vector<double> gamma(layout.size(), 0.0);
    for (size_t o = 0; o < layout.size(); ++o) {  // margin and check passes
        const eray::gpu::AccelDevLayout& ob = layout[o];
        std::vector<char> unculled(ob.faces);
        uint32_t nc = 0, nu = 0, status = 0;
        for (uint32_t k = 0; k < ob.faces; ++k) {
            const FaceMargin m = face_margin_of(faces[ob.hot_begin + k]);
            unculled[k] = !m.culled;
            ab[2 * (size_t)(ob.gbegin + k)] = m.alpha;
            ab[2 * (size_t)(ob.gbegin + k) + 1] = m.beta;
            (m.culled ? nc : nu) += 1;
            if (m.culled) gamma[o] = std::fmax(gamma[o], m.gamma);
        }
        for (uint32_t k = 0; k < ob.U; ++k) {
            const uint32_t slot = ob.gbegin + k, f = sc->index[slot];
            if (f < ob.faces && unculled[f]) sc->hot[slot] = faces[ob.hot_begin + f];
            else status = 1;
        }
        if (!refit_keeps(nc, nu, status, ob.C, ob.U)) return false;
    }
    for (uint32_t level = max_depth; level-- > 0;)  // levels, deepest first, every covered object
        for (const eray::gpu::AccelDevLayout& ob : layout) {
            const TreeLayout t{ob.C, ob.full, ob.extra, 0u, 0u};
            for (uint32_t j = 0; j < (1u << level); ++j)
                level_node<PreOrder>(t, level, j, sc->index.data() + ob.gbegin + ob.U, 0u, faces.data() + ob.hot_begin,
                                     ab.data() + 2 * (size_t)ob.gbegin, ob.node_base, ob.gbegin + ob.U, sc->nodes.data(), bounds.data(),
                                     sc->hot.data(), sc->index.data());
        }
    for (size_t o = 0; o < layout.size(); ++o)
        sc->objs[layout[o].index] = refit_object(true, layout[o].C, layout[o].U, layout[o].node_base, layout[o].gbegin, gamma[o]);
    return true;
}

bool scene_of_three() {
    // C just above kLeafFaces << 6 (a pairs level), a few faces, C an exact kLeafFaces << 6
    const std::vector<std::vector<Hot>> parts = {soup_with_culled((kLeafFaces << 6) + 3), records(soup(10, 0.8, 0.06)),
                                                 soup_with_culled(kLeafFaces << 6)};
    const uint32_t min_faces = 64;
    std::vector<Hot> faces;
    std::vector<uint32_t> sizes;
    for (const std::vector<Hot>& p : parts) {
        faces.insert(faces.end(), p.begin(), p.end());
        sizes.push_back((uint32_t)p.size());
    }
    SceneBuilt sc;
    size_t bad_object = 0;
    const char* why = "";
    if (!build_scene(faces.data(), sizes.data(), sizes.size(), min_faces, true, &sc, &bad_object, &why)) {
        std::printf("  build_scene: object %zu: %s\n", bad_object, why);
        return false;
    }
    // what the records must say, from the sizes, the faces' classes and tree_layout alone
    bool slices = sc.objs.size() == sizes.size(), layout = true;
    uint32_t begin = 0, gbegin = 0, blocks = 0, cbase = 0, node_base = 0, covered = 0, depth = 0, c[3] = {}, extra[3] = {};
    for (size_t i = 0; slices && i < sizes.size(); begin += sizes[i], ++i) {
        const uint32_t n = sizes[i];
        static const Object none{};
        if (n < min_faces) {
            slices = !std::memcmp(&sc.objs[i], &none, sizeof(Object));
            continue;
        }
        uint32_t C = 0;
        for (uint32_t k = 0; k < n; ++k) C += face_margin_of(faces[begin + k]).culled;
        const TreeLayout t = tree_layout(C);
        c[i] = C;
        extra[i] = t.extra;
        Built alone;
        slices = host_build(parts[i], node_base, gbegin, &alone) && alone.nodes.size() == t.nodes && alone.hot.size() == n &&
                 sc.nodes.size() >= (size_t)node_base + t.nodes && sc.hot.size() >= (size_t)gbegin + n && sc.index.size() == sc.hot.size() &&
                 !std::memcmp(&sc.nodes[node_base], alone.nodes.data(), sizeof(Node) * t.nodes) &&
                 !std::memcmp(&sc.hot[gbegin], alone.hot.data(), sizeof(Hot) * n) &&
                 !std::memcmp(&sc.index[gbegin], alone.index.data(), 4 * (size_t)n) && !std::memcmp(&sc.objs[i], &alone.obj, sizeof(Object));
        const eray::gpu::AccelDevLayout want{begin, n, gbegin, blocks, (uint32_t)i, C, n - C, cbase, node_base, t.full, t.extra, 1u};
        layout = layout && covered < sc.layout.size() && !std::memcmp(&sc.layout[covered], &want, sizeof want);
        ++covered;
        gbegin += n;
        blocks += (n + 255u) / 256u;
        cbase += C;
        node_base += t.nodes;
        depth = std::max(depth, t.depth);
    }
    slices = slices && sc.nodes.size() == node_base && sc.hot.size() == gbegin;
    layout = layout && sc.layout.size() == covered && sc.objects == covered && sc.max_depth == depth && sc.faces == gbegin &&
             sc.unculled == gbegin - cbase;
    // the refit of the unmoved scene: the nodes start from zero, so every one must be written
    SceneBuilt again = sc;
    std::fill(again.nodes.begin(), again.nodes.end(), Node{});
    std::memset(again.objs.data(), 0, sizeof(Object) * again.objs.size());
    const bool refit = slices && layout && emulate_scene_refit(faces, sc.layout, sc.max_depth, &again) &&
                       !std::memcmp(again.nodes.data(), sc.nodes.data(), sizeof(Node) * sc.nodes.size()) &&
                       !std::memcmp(again.hot.data(), sc.hot.data(), sizeof(Hot) * sc.hot.size()) && again.index == sc.index &&
                       !std::memcmp(again.objs.data(), sc.objs.data(), sizeof(Object) * sc.objs.size());
    std::printf("scene=three_objects objects=%u faces=%u nodes=%zu depth=%u c0=%u extra0=%u c2=%u extra2=%u slices=%d layout=%d refit=%d\n",
                sc.objects, gbegin, sc.nodes.size(), sc.max_depth, c[0], extra[0], c[2], extra[2], (int)slices, (int)layout, (int)refit);
    return slices && layout && refit;
}

}  // namespace

int main(int argc, char** argv) {
    if (argc < 2) {
        std::fprintf(stderr, "usage: %s sphere2000.bin [rays]\n", argv[0]);
        return 2;
    }
    const size_t nrays = argc > 2 ? (size_t)std::atoll(argv[2]) : 100000;
    std::vector<float> s2k;
    if (!load(argv[1], s2k)) {
        std::fprintf(stderr, "cannot read the mesh\n");
        return 2;
    }
    bool ok = check_ids(5000);
    ok &= suite("sphere2000", s2k, displaced(s2k, 0.05), nrays);
    const std::vector<float> sl = slivers(3000);
    ok &= suite("slivers3000", sl, slivers_moved(sl, 0.05), nrays);
    // 9 .. 19: the smallest sizes at which the two halves' subtrees differ in node count
    for (uint32_t T : {1u, 4u, 5u, 9u, 10u, 11u, 13u, 19u, 65u, 513u}) {
        const std::vector<float> a = soup(T, 0.8, 0.06);
        ok &= suite(("soup" + std::to_string(T) + "h").c_str(), a, displaced(a, 0.05), 1024);
    }
    std::string names;
    for (const std::string& n : g_caught) names += (names.empty() ? "" : ",") + n;
    std::printf("corruptions_named=%s\n", names.c_str());
    ok &= g_caught.size() == sizeof kCorruptions / sizeof kCorruptions[0];
    // class changes, in either direction (accel_refit_main's three)
    ok &= refused("culled_face_scaled_until_n1_is_4", s2k, [](const std::vector<Hot>& A, std::vector<float>& pos) {
        const int f = 11;
        if (!face_margin_of(A[f]).culled) return -1;
        for (int i = 0; i < 40; ++i) {
            const Hot r = make_hot(&pos[9 * f]);
            if (std::fabs((double)r.q[6]) + std::fabs((double)r.q[7]) + std::fabs((double)r.q[8]) >= 4.0) return f;
            scale_face(&pos[9 * f], 2.0);
        }
        return -1;
    });
    ok &= refused("nan_vertex_on_a_culled_face", s2k, [](const std::vector<Hot>& A, std::vector<float>& pos) {
        const int f = 1234;
        if (!face_margin_of(A[f]).culled) return -1;
        pos[9 * f + 4] = NAN;
        return f;
    });
    ok &= refused("unculled_face_of_the_crowded_soup_shrunk", soup(600, 0.25, 0.15), [](const std::vector<Hot>& A, std::vector<float>& pos) {
        for (int f = 0; f < (int)A.size(); ++f) {
            if (face_margin_of(A[f]).culled) continue;
            for (int i = 0; i < 40; ++i) {
                scale_face(&pos[9 * f], 0.5);
                if (face_margin_of(make_hot(&pos[9 * f])).culled) return f;
            }
            return -1;
        }
        return -1;
    });
    ok &= scene_of_three();  // (last: its meshes draw from the generator after every figure above)
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
