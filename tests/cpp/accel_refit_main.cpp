// accel_refit_main.cpp — the refit of a device-built ray-query hierarchy (accel_dev.hip
// accel_refit_device) on the CPU: accel_emul.hpp's emulate_device_build on a mesh A, then its
// emulate_refit on a deformed mesh B of the same faces (the margin pass, the check of the unculled
// list, level_node over the hierarchy's own index array, the object record), the checker
// (accel_check.cpp) and the walk the kernel runs (accel_walk.hpp).  The emulations, the ray sets,
// the meshes and the named corruptions are the header's; this program adds the suite at non-zero
// bases and the class changes the refit must refuse.  No GPU, no HIP.  Compile with
// -ffp-contract=off.
//
//   accel_refit_main <sphere2000.bin> [rays]
//
// Per mesh one line of figures; tests/test_accel_refit_host.py asserts on them:
//   check      1 when accel::check accepts the refitted tree against B's faces
//   mismatch   rays whose walk through the refitted tree differs from the linear scan over B
//   identity   1 when the refit with B = A reproduces nodes, slots, indices and the object record
//              byte for byte
//   moved      nodes whose bytes differ between A's tree and the refitted one (the refit did work)
//   caught     how many of the named corruptions of the refitted tree the checker names
// and one line per class change that the refit must refuse (detected=1).
#include "accel_emul.hpp"

using namespace eray::accel;
using namespace accel_emul;
using namespace accel_emul::single_tree;

namespace {

std::vector<std::string> g_caught;  // the corruptions that some mesh exercised and the checker named

bool same_bytes(const Built& a, const Built& b) {
    return a.nodes.size() == b.nodes.size() && a.hot.size() == b.hot.size() && a.index == b.index &&
           (a.nodes.empty() || !std::memcmp(a.nodes.data(), b.nodes.data(), sizeof(Node) * a.nodes.size())) &&
           (a.hot.empty() || !std::memcmp(a.hot.data(), b.hot.data(), sizeof(Hot) * a.hot.size())) &&
           !std::memcmp(&a.obj, &b.obj, sizeof(Object)) && a.unculled == b.unculled && a.depth == b.depth;
}

// The build on A, the refit on B (the same faces, moved), at node / slot bases other than zero.
bool suite(const char* name, const std::vector<float>& posA, const std::vector<float>& posB, size_t nrays) {
    const uint32_t node_base = 5, slot_base = 300;
    const std::vector<Hot> A = records(posA), B = records(posB);
    const uint32_t T = (uint32_t)A.size();
    const Built built = emulate_device_build(A, node_base, slot_base);
    // the precondition of a kept topology, from the margins alone: the same faces are unculled
    bool same_class = true;
    for (uint32_t f = 0; f < T; ++f) same_class = same_class && face_margin_of(A[f]).culled == face_margin_of(B[f]).culled;
    Built same, refit;
    const bool kept_same = emulate_refit(A, built, node_base, slot_base, &same);
    const bool identity = kept_same && same_bytes(same, built);
    const bool kept = emulate_refit(B, built, node_base, slot_base, &refit);
    if (!same_class || !kept) {
        std::printf("%s: same_class=%d kept=%d: the deformation must keep every face's class\n", name, (int)same_class, (int)kept);
        return false;
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
    size_t moved = 0;
    for (size_t i = 0; i < refit.nodes.size(); ++i) moved += std::memcmp(&refit.nodes[i], &built.nodes[i], sizeof(Node)) != 0;
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
        "moved=%zu caught=%d corruption_failed=%d\n",
        name, T, refit.nodes.size(), refit.depth, refit.unculled, rays.size(), (unsigned long long)r.mismatch,
        (unsigned long long)r.hits, (unsigned long long)r.fallback, (int)!bad, (int)identity, moved, caught, failed);
    return !bad && identity && !failed && r.mismatch == 0;
}

// A class change the refit must refuse: the build on A, then B = A with one face changed by `change`
// (which returns the face it changed, or -1 when the mesh has none of the kind).
template <typename Change>
bool refused(const char* name, const std::vector<float>& posA, Change change) {
    const std::vector<Hot> A = records(posA);
    const Built built = emulate_device_build(A, 0, 0);
    std::vector<float> posB = posA;
    const int face = change(A, posB);
    Built out;
    const bool detected = face >= 0 && !emulate_refit(records(posB), built, 0, 0, &out);
    std::printf("class_change=%s face=%d detected=%d\n", name, face, (int)detected);
    return detected;
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
    bool ok = true;
    ok &= suite("sphere2000", s2k, displaced(s2k, 0.03), nrays);
    const std::vector<float> sl = slivers(600);
    ok &= suite("slivers", sl, slivers_moved(sl, 0.05), nrays);
    for (uint32_t T : {1u, 4u, 5u, 65u, 513u}) {
        const std::vector<float> a = soup(T, 0.8, 0.06);
        ok &= suite(("soup" + std::to_string(T) + "b").c_str(), a, displaced(a, 0.02), 2000);
    }
    std::string names;
    for (const std::string& n : g_caught) names += (names.empty() ? "" : ",") + n;
    std::printf("corruptions_named=%s\n", names.c_str());
    ok &= g_caught.size() == sizeof kCorruptions / sizeof kCorruptions[0];
    // class changes, in either direction
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
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
