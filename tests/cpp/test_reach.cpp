// Engine::reaches_light of the C++ host (include/eray/engine.hpp) on the GPU, on a hand-derived
// pair: one triangle in the plane z = 0 between a start at z = 1 and a target at z = -1 blocks the
// ray (the hit lies at distance 1, the target at distance 2: 1 > 2 is false); with the target at
// z = 0.5, in front of the triangle, the same hit lies farther than the target (1 > 0.5) and the
// ray reaches it.
//
//   test_reach
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
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

int main() {
    test("reaches_light: one face between start and target blocks, a nearer target is reached", [] {
        // a = (0,0,0), b = (1,0,0), c = (0,1,0): e1 x e2 = (0,0,1); the ray from (0.25, 0.25, 1)
        // along -z has det = 1 and t = 1, so the hit is (0.25, 0.25, 0), at distance 1 from the start
        Object<Built> tri;
        Triangle t;
        t.pos = {Vector3(0, 0, 0), Vector3(1, 0, 0), Vector3(0, 1, 0)};
        t.normal = {Vector3(0, 0, 1), Vector3(0, 0, 1), Vector3(0, 0, 1)};
        t.uv = {{{0.0f, 0.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}}};
        tri.faces.push_back(t);
        tri.bbox = {Vector3(0, 0, 0), Vector3(1, 1, 0)};
        Engine engine({16, 16}, 0, 0);
        engine.scene().add_object(std::move(tri));
        const Vector3 start(0.25f, 0.25f, 1.0f);
        const Ray down = Ray::make(start, Vector3(0, 0, -2.0f));
        const std::vector<Ray> rays = {down, down, Ray::make(Vector3(2.0f, 2.0f, 1.0f), Vector3(0, 0, -1.0f)),
                                       Ray::make(Vector3(0.25f, 0.25f, -1.0f), Vector3(0, 0, 1.0f))};
        const std::vector<Vector3> targets = {Vector3(0.25f, 0.25f, -1.0f), Vector3(0.25f, 0.25f, 0.5f),
                                              Vector3(2.0f, 2.0f, -1.0f), Vector3(0.25f, 0.25f, 1.0f)};
        for (bool accel : {false, true}) {
            if (accel) CHECK(engine.build_ray_accel(1).objects == 1);
            const std::vector<bool> r = engine.reaches_light(rays, targets);
            CHECK(r.size() == 4);
            if (r.size() != 4) continue;
            CHECK(!r[0]);  // blocked: the face lies between
            CHECK(r[1]);   // the target lies in front of the face
            CHECK(r[2]);   // the ray passes beside the face: nothing hit
            CHECK(r[3]);   // from behind: backface culling (primitives.rs:48-51), nothing hit
        }
        CHECK(engine.reaches_light({}, {}).empty());
        bool threw = false;
        try {
            engine.reaches_light(rays, {});
        } catch (const std::exception&) {
            threw = true;
        }
        CHECK(threw);
    });

    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
