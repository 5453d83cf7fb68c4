// accel_walk_main.cpp — the ray-query hierarchy on the CPU: the builder (accel_build.cpp) and the
// walk the kernel runs (accel_walk.hpp), against a linear scan with one shared f32 predicate.
// The predicate, the scan, the ray sets and the meshes are accel_emul.hpp's; this program adds the
// property check of the nodes (b) and the moved suites.  No GPU, no HIP.  Compile with
// -ffp-contract=off; it links with accel_build.cpp alone.
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
#include "accel_emul.hpp"

using namespace eray::accel;
using namespace accel_emul;

namespace {

struct Result {
    uint64_t mismatch = 0, violation = 0, fallback = 0, fallback_in_range = 0, face_tests = 0, hits = 0, pairs = 0;
    uint32_t stack_high = 0;
};

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
    const auto part = [&](size_t begin, size_t end, Result& q) { run_range(hot, b, rays, property_rays, begin, end, q); };
    for (const Result& q : deal<Result>(rays.size(), part)) {
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
    const std::vector<Hot> hot = records(pos);
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
    const std::vector<Hot> hot = records(pos);
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
