// Engine::build_ray_accel(min_faces, on_device, refittable) of the C++ host (include/eray/engine.hpp)
// on the GPU: an Engine builds the host-split hierarchy refittable, moves its 1500-face sphere in
// place and refits — the topology is kept (no rebuild) — and cast_rays gives the records of a
// freshly built Engine with the moved sphere.
//
//   test_refit_hosttree
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <vector>

#include "eray/eray.hpp"

using namespace eray;

static int g_failed = 0, g_run = 0;
#define CHECK(cond)                                                                         \
    do {                                                                                    \
        if (!(cond)) {                                                                      \
            std::fprintf(stderr, "  %s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #cond); \
            ++g_failed;                                                                     \
        }                                                                                   \
    } while (0)

static void test(const char* name, const std::function<void()>& fn) {
    ++g_run;
    const int before = g_failed;
    try {
        fn();
    } catch (const std::exception& e) {
        std::fprintf(stderr, "  exception: %s\n", e.what());
        ++g_failed;
    }
    std::printf("%s %s\n", g_failed == before ? "ok  " : "FAIL", name);
}

// every field of every record, bit for bit
static bool same_hits(const std::vector<std::optional<RaycastHit>>& a, const std::vector<std::optional<RaycastHit>>& b) {
    if (a.size() != b.size()) return false;
    for (size_t i = 0; i < a.size(); ++i) {
        if (a[i].has_value() != b[i].has_value()) return false;
        if (!a[i]) continue;
        const RaycastHit &x = *a[i], &y = *b[i];
        const float fx[] = {x.position.x, x.position.y, x.position.z, x.normal.x, x.normal.y, x.normal.z, x.uv[0], x.uv[1], x.u, x.v};
        const float fy[] = {y.position.x, y.position.y, y.position.z, y.normal.x, y.normal.y, y.normal.z, y.uv[0], y.uv[1], y.u, y.v};
        if (x.object != y.object || x.face_index != y.face_index || std::memcmp(fx, fy, sizeof fx)) return false;
    }
    return true;
}

static std::vector<Ray> rays_toward_origin(size_t n) {
    std::vector<Ray> rays;
    for (size_t i = 0; i < n; ++i) {
        const float a = 0.7f * (float)i, b = 1.3f * (float)i;
        const Vector3 s(3.0f * std::cos(a) * std::cos(b), 3.0f * std::sin(b), 3.0f * std::sin(a) * std::cos(b));
        const Vector3 t(std::sin(2.1f * (float)i), std::sin(3.7f * (float)i), std::sin(5.3f * (float)i));
        rays.push_back(Ray::make(s, Vector3(t.x - s.x, t.y - s.y, t.z - s.z)));
    }
    return rays;
}

// a latitude / longitude sphere of radius 0.9, faces in a scrambled order, outward
static Object<Built> sphere(uint32_t rings, uint32_t segs) {
    Object<Built> o;
    auto P = [&](uint32_t i, uint32_t j) {
        const float th = 3.14159265f * (float)i / (float)rings, ph = 6.2831853f * (float)(j % segs) / (float)segs;
        return Vector3(0.9f * std::sin(th) * std::cos(ph), 0.9f * std::cos(th), 0.9f * std::sin(th) * std::sin(ph));
    };
    auto face = [&](Vector3 a, Vector3 b, Vector3 c) {
        Triangle t;
        t.pos = {a, b, c};
        t.normal = {a, b, c};
        t.uv = {{{0.0f, 0.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}}};
        o.faces.push_back(t);
    };
    for (uint32_t i = 0; i < rings; ++i)
        for (uint32_t j = 0; j < segs; ++j) {
            if (i > 0) face(P(i, j), P(i, j + 1), P(i + 1, j + 1));
            if (i + 1 < rings) face(P(i, j), P(i + 1, j + 1), P(i + 1, j));
        }
    for (size_t k = 0; k < o.faces.size(); ++k) std::swap(o.faces[k], o.faces[(k * 7919u + 13u) % o.faces.size()]);
    o.bbox = {Vector3(-0.9f, -0.9f, -0.9f), Vector3(0.9f, 0.9f, 0.9f)};
    return o;
}

// the sphere moved and smoothly displaced, face by face (the order is the semantics)
static Object<Built> moved(Object<Built> o) {
    auto f = [](Vector3 p) {
        return Vector3(p.x + 0.1f + 0.03f * std::sin(2.5f * p.y), p.y - 0.05f + 0.03f * std::sin(2.5f * p.z),
                       p.z + 0.03f * std::sin(2.5f * p.x));
    };
    for (Triangle& t : o.faces)
        for (int k = 0; k < 3; ++k) t.pos[k] = f(t.pos[k]);
    o.bbox = {Vector3(-0.9f, -0.9f, -0.9f), Vector3(1.1f, 0.9f, 0.9f)};
    return o;
}

int main() {
    test("build_ray_accel(refittable) + update_object + refit_ray_accel keeps the host-built tree", [&] {
        const Object<Built> s0 = sphere(26, 30), s1 = moved(s0);
        const size_t T = s0.faces.size();
        Camera cam;
        cam.center = Vector3(0.0f, 0.0f, 5.0f);
        cam.width = 64;  // (the engines' 64 x 64 image)
        const std::vector<Ray> rays = rays_toward_origin(3000);
        Engine fresh({64, 64}, 0, 0);
        fresh.scene().set_camera(cam).add_object(s1);
        const auto want = fresh.cast_rays(rays);
        // (the engines share the device's context: `fresh` is not used again once `engine` uploads)
        size_t hit = 0;
        for (auto& h : want) hit += h.has_value();
        CHECK(hit >= 500 && hit + 500 <= rays.size());

        Engine engine({64, 64}, 0, 0);
        engine.scene().set_camera(cam).add_object(s0);
        const auto before = engine.cast_rays(rays);
        CHECK(!same_hits(before, want));
        const Engine::RayAccelInfo plain = engine.build_ray_accel();
        const Engine::RayAccelInfo built = engine.build_ray_accel(0, false, true);
        CHECK(built.objects == 1 && built.faces == T);  // the host build's figures
        CHECK(built.nodes == plain.nodes && built.max_depth == plain.max_depth && built.unculled_faces == plain.unculled_faces &&
              built.device_bytes == plain.device_bytes);
        CHECK(same_hits(engine.cast_rays(rays), before));
        engine.update_object(0, s1);
        const Engine::RayAccelRefitInfo r = engine.refit_ray_accel();
        CHECK(!r.rebuilt && r.refitted == 1);
        CHECK(r.accel.objects == 1 && r.accel.faces == T && r.accel.nodes == built.nodes && r.accel.max_depth == built.max_depth &&
              r.accel.device_bytes == built.device_bytes && r.accel.unculled_faces == built.unculled_faces);
        CHECK(same_hits(engine.cast_rays(rays), want));
        CHECK(same_hits(engine.cast_rays(rays, 0), want));
        engine.update_object(0, s0);  // and back: still refittable
        const Engine::RayAccelRefitInfo back = engine.refit_ray_accel();
        CHECK(!back.rebuilt && back.refitted == 1);
        CHECK(same_hits(engine.cast_rays(rays), before));
        bool threw = false;
        try {
            engine.build_ray_accel(0, true, true);  // the device build is always refittable
        } catch (const Failure& e) {
            threw = e.status == ERAY_E_INVALID_ARGUMENT;
        }
        CHECK(threw);
        CHECK(same_hits(engine.cast_rays(rays), before));
    });

    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
