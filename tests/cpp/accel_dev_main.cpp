// accel_dev_main.cpp — the device-side builder of the ray-query hierarchy on the CPU:
// accel_emul.hpp's emulate_device_build (the headers the kernels share: margins, Morton keys, the
// level layout, make_leaf / make_inner through level_node; std::stable_sort for the radix sort)
// against the host builder, the checker (accel_check.cpp) and the walk the kernel runs
// (accel_walk.hpp).  The emulation, the ray sets, the meshes and the checker's named corruptions
// are the header's; this program adds the meshes with tied keys and zero extent, the layout's
// arithmetic against the recursion it replaces, and the suite.  No GPU, no HIP.  Compile with
// -ffp-contract=off.
//
//   accel_dev_main <sphere2000.bin> <sphere20000.bin> [rays]
//
// Per mesh one line of figures; tests/test_accel_dev_host.py asserts on them:
//   check_dev / check_host  1 when accel::check accepts the emulated build / build_object's
//   mismatch   rays whose walk result through the emulated tree differs from the scan's
//   same_shape 1 when node count, depth and unculled count equal the host build's
//   caught     how many of the named corruptions of the valid tree the checker names
#include "accel_emul.hpp"

using namespace eray::accel;
using namespace accel_emul;
using namespace accel_emul::single_tree;

namespace {

std::vector<std::string> g_caught;  // the corruptions that some mesh exercised and the checker named

bool suite(const char* name, const std::vector<float>& pos, size_t nrays) {
    const uint32_t T = (uint32_t)(pos.size() / 9);
    const std::vector<Hot> hot = records(pos);
    Built host;
    const char* why = "";
    if (!build_object(hot.data(), T, 0, 0, kStackDepth, &host, &why)) {
        std::printf("%s: build refused: %s\n", name, why);
        return false;
    }
    const Built dev = emulate_device_build(hot, 0, 0);
    const char* bad_dev = check_one(hot, dev);
    const char* bad_host = nullptr;
    if (bad_dev) std::printf("  %s: the emulated device build: %s\n", name, bad_dev);
    const bool check_dev = !bad_dev;
    bad_host = check_one(hot, host);
    if (bad_host) std::printf("  %s: the host build: %s\n", name, bad_host);
    const bool same_shape = dev.nodes.size() == host.nodes.size() && dev.depth == host.depth && dev.unculled == host.unculled &&
                            !std::memcmp(&dev.obj, &host.obj, sizeof(Object));
    // the same build at non-zero bases (several objects in a scene) is the same tree, shifted
    const Built moved = emulate_device_build(hot, 7, 1000);
    bool shifted = moved.nodes.size() == dev.nodes.size() && moved.index == dev.index && moved.obj.ubegin == 1000 &&
                   (dev.nodes.empty() || moved.obj.root == 7);
    for (size_t i = 0; shifted && i < dev.nodes.size(); ++i) {
        const Node &a = dev.nodes[i], &b = moved.nodes[i];
        const bool leaf = a.left & kLeafBit;
        shifted = !std::memcmp(a.c, b.c, 32) && a.min_index == b.min_index && a.right_min == b.right_min &&
                  b.left == a.left + (leaf ? 1000u : 7u) && b.right == a.right + (leaf ? 0u : 7u);
    }
    int caught = 0, failed = 0;
    for (const Corruption& c : kCorruptions) {
        const int r = corrupt(hot, dev, c);
        if (r > 0) {
            ++caught;
            if (std::find(g_caught.begin(), g_caught.end(), c.name) == g_caught.end()) g_caught.push_back(c.name);
        }
        failed += r < 0;
    }
    const std::vector<Ray> rays = make_rays(pos, nrays);
    Result r;
    if (check_dev) run(hot, dev, rays, r);  // (an invalid tree may not be walked)
    std::printf(
        "suite=%s faces=%u nodes=%zu depth=%u unculled=%u rays=%zu mismatch=%llu hits=%llu fallback=%llu check_dev=%d "
        "check_host=%d same_shape=%d shifted=%d caught=%d corruption_failed=%d\n",
        name, T, dev.nodes.size(), dev.depth, dev.unculled, rays.size(), (unsigned long long)r.mismatch,
        (unsigned long long)r.hits, (unsigned long long)r.fallback, (int)check_dev, (int)!bad_host, (int)same_shape, (int)shifted,
        caught, failed);
    return check_dev && !bad_host && same_shape && shifted && !failed && r.mismatch == 0;
}

// faces in groups of 8 that share one centroid exactly (one triangle, its vertices permuted and
// its winding kept or flipped): the Morton keys tie and the index decides
std::vector<float> tied(uint32_t groups) {
    std::vector<float> pos;
    static const int perm[8][3] = {{0, 1, 2}, {1, 2, 0}, {2, 0, 1}, {0, 2, 1}, {2, 1, 0}, {1, 0, 2}, {0, 1, 2}, {1, 2, 0}};
    for (uint32_t g = 0; g < groups; ++g) {
        const std::vector<float> t = soup(1, 1.0, 0.2);
        for (auto& p : perm)
            for (int k : p)
                for (int j = 0; j < 3; ++j) pos.push_back(t[3 * k + j]);
    }
    return pos;
}

// every vertex in the plane z = 0.25: the centroids' extent on that axis is zero
std::vector<float> planar(uint32_t T) {
    std::vector<float> pos = soup(T, 1.0, 0.2);
    for (size_t k = 2; k < pos.size(); k += 3) pos[k] = 0.25f;
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
    // the layout's arithmetic against the recursion it replaces, for every small count
    for (uint32_t C = 0; C <= 5000 && ok; ++C) {
        struct Rec {
            static void go(uint32_t n, uint32_t level, uint32_t& nodes, uint32_t& depth) {
                ++nodes;
                depth = std::max(depth, level);
                if (n <= kLeafFaces) return;
                go(n / 2, level + 1, nodes, depth);
                go(n - n / 2, level + 1, nodes, depth);
            }
        };
        uint32_t nodes = 0, depth = 0;
        if (C) Rec::go(C, 1, nodes, depth);
        const TreeLayout t = tree_layout(C);
        if (t.nodes != nodes || t.depth != depth) {
            std::printf("layout: C=%u gives %u nodes / %u levels, the recursion %u / %u\n", C, t.nodes, t.depth, nodes, depth);
            ok = false;
        }
    }
    std::printf("layout=%d\n", (int)ok);
    ok &= suite("sphere2000", s2k, nrays);
    ok &= suite("sphere20000", s20k, nrays);
    ok &= suite("soup300", soup(300, 1.0, 0.2), nrays);
    ok &= suite("cube", cube(), nrays);
    ok &= suite("slivers", slivers(600), nrays);
    ok &= suite("tied256", tied(32), nrays);
    ok &= suite("planar200", planar(200), nrays);
    for (uint32_t T : {1u, 4u, 5u, 8u, 9u, 64u, 65u, 513u}) ok &= suite(("soup" + std::to_string(T) + "b").c_str(), soup(T, 0.8, 0.06), 2000);
    std::string names;
    for (const std::string& n : g_caught) names += (names.empty() ? "" : ",") + n;
    std::printf("corruptions_named=%s\n", names.c_str());
    ok &= g_caught.size() == sizeof kCorruptions / sizeof kCorruptions[0];
    std::printf(ok ? "OK\n" : "FAILED\n");
    return ok ? 0 : 1;
}
