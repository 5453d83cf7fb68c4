// accel_refit_async_main.cpp — the refit that runs on the stream (accel_dev.hip accel_refit_enqueue)
// emulated on the CPU, kernel for kernel, with the headers its kernels share (accel_margin.hpp,
// accel_layout.hpp), the checker (accel_check.cpp) and the walk the kernel runs (accel_walk.hpp).
// The device build, the synchronous refit it is compared with, the ray sets and the meshes are
// accel_emul.hpp's; this program adds the scene, the persistent workspace, refit_async and the
// dispatch of queries by the records' `has`.  No GPU, no HIP.  Compile with -ffp-contract=off.
//
//   accel_refit_async_main <sphere2000.bin> [rays]
//
// A scene of two covered objects is built on meshes A (emulate_device_build) and refitted through
// ONE workspace that is never cleared except by the documented resets (the accumulators and
// counters): the margin pass, the check of the unculled lists, the level passes whatever the
// verdict, the verdict (accel::refit_keeps) and the object record (accel::refit_object).
//   reuse=...         A -> B -> C through the reused workspace: same=1 when nodes, slots, indices and
//                     records equal a synchronous-style refit from A straight to C (emulate_refit),
//                     check=1 when accel::check accepts the scene, top=1 when the order of
//                     refit_top_levels_kernel gives the bytes of the per-level order
//   class_change=...  B -> a mesh with one face's class changed -> B: only=1 when the verdict fails
//                     that object and no other, mismatch: rays (dispatched by the records' `has`)
//                     that differ from the linear scan, healed=1 when the last refit's bytes are
//                     those of a refit that never saw the bad mesh
// tests/test_accel_refit_async_host.py asserts on the figures.
#include "accel_emul.hpp"

using namespace eray::accel;
using namespace accel_emul;

namespace {

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
    const auto part = [&](size_t begin, size_t end, Result& q) { run_range(s, rays, begin, end, q); };
    Result res;
    for (const Result& q : deal<Result>(rays.size(), part)) {
        res.mismatch += q.mismatch;
        res.hits += q.hits;
        res.scanned += q.scanned;
    }
    return res;
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
