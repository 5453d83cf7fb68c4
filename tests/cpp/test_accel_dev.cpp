// Engine::build_ray_accel(min_faces, on_device = true) of the C++ host (include/eray/engine.hpp) on
// the GPU: cast_rays gives the same records through the device-built hierarchy as before any
// build and as through the host-built one, on a generated 1500-face sphere.
//
//   test_accel_dev
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

int main() {
    test("build_ray_accel(0, true): a 1500-face sphere, built on the device", [&] {
        Object<Built> s = sphere(26, 30);
        const size_t T = s.faces.size();
        Camera cam;
        cam.center = Vector3(0.0f, 0.0f, 5.0f);
        Engine engine({64, 64}, 0, 0);
        engine.scene().set_camera(cam).add_object(std::move(s));
        const std::vector<Ray> rays = rays_toward_origin(3000);
        const auto before = engine.cast_rays(rays);
        size_t hit = 0;
        for (auto& h : before) hit += h.has_value();
        CHECK(hit >= 500 && hit + 500 <= rays.size());
        const Engine::RayAccelInfo host = engine.build_ray_accel();
        CHECK(same_hits(engine.cast_rays(rays), before));
        const Engine::RayAccelInfo info = engine.build_ray_accel(0, true);
        CHECK(info.objects == 1 && info.faces == T && info.unculled_faces == host.unculled_faces);
        CHECK(info.nodes == host.nodes && info.max_depth == host.max_depth && info.device_bytes == host.device_bytes);
        CHECK(same_hits(engine.cast_rays(rays), before));
        CHECK(same_hits(engine.cast_rays(rays, 0), before));
        engine.drop_ray_accel();
        CHECK(same_hits(engine.cast_rays(rays), before));
    });

    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
