// Engine::cast_rays of the C++ host (include/eray/engine.hpp) on the GPU: the hand-derived
// one-face hit record and its backface miss, and the cube's centre ray (face 1 on
// the shared diagonal, u = 0.5).
//
//   test_rays [--root REPO]
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

int main(int argc, char** argv) {
    std::string root = ".";
    for (int i = 1; i < argc; ++i)
        if (!std::strcmp(argv[i], "--root") && i + 1 < argc) root = argv[++i];

    test("cast_rays: one face, hand-derived record and the backface miss", [] {
        // a = (0,0,0), b = (1,0,0), c = (0,1,0), normals (0,0,1), uvs (0,0) (1,0) (0,1):
        // e1 x e2 = (0,0,1); the ray from (0.25, 0.25, 1) along -z has det = 1, t = 1, u = v = 0.25
        Object<Built> tri;
        Triangle t;
        t.pos = {Vector3(0, 0, 0), Vector3(1, 0, 0), Vector3(0, 1, 0)};
        t.normal = {Vector3(0, 0, 1), Vector3(0, 0, 1), Vector3(0, 0, 1)};
        t.uv = {{{0.0f, 0.0f}, {1.0f, 0.0f}, {0.0f, 1.0f}}};
        tri.faces.push_back(t);
        tri.bbox = {Vector3(0, 0, 0), Vector3(1, 1, 0)};
        Engine engine({16, 16}, 0, 0);
        engine.scene().add_object(std::move(tri));
        const std::vector<Ray> rays = {Ray::make(Vector3(0.25f, 0.25f, 1.0f), Vector3(0, 0, -2.0f)),
                                       Ray::make(Vector3(0.25f, 0.25f, -1.0f), Vector3(0, 0, 1.0f))};
        CHECK(rays[0].dir.x == 0.0f && rays[0].dir.y == 0.0f && rays[0].dir.z == -1.0f);  // Ray::new normalises
        for (int object : {-1, 0}) {
            const auto hits = engine.cast_rays(rays, object);
            CHECK(hits.size() == 2);
            CHECK(hits[0].has_value());
            if (hits[0]) {
                const RaycastHit& h = *hits[0];
                CHECK(h.object == 0 && h.face_index == 0);
                CHECK(h.position.x == 0.25f && h.position.y == 0.25f && h.position.z == 0.0f);
                CHECK(h.normal.x == 0.0f && h.normal.y == 0.0f && h.normal.z == 1.0f);
                CHECK(h.u == 0.25f && h.v == 0.25f && h.uv[0] == 0.25f && h.uv[1] == 0.25f);
            }
            CHECK(!hits[1].has_value());  // backface culling (primitives.rs:48-51)
        }
        CHECK(engine.cast_rays({}).empty());
    });

    test("cast_rays: the cube's centre ray hits face 1", [&] {
        Object<Building> cube = load_obj(root + "/objects/cube.obj");
        Camera cam;
        cam.center = Vector3(0.0f, 0.0f, 5.0f);
        Engine engine({256, 256}, 0, 0);
        engine.scene().set_camera(cam).add_object(build(std::move(cube)));
        // Camera::pixel_to_ray(0.5, 0.5) of that camera: start (0,0,5), dir (0,0,-1)
        const auto hits = engine.cast_rays({Ray::make(cam.center, Vector3(0.0f, 0.0f, -1.0f))});
        CHECK(hits.size() == 1 && hits[0].has_value());
        if (hits.size() == 1 && hits[0]) {
            CHECK(hits[0]->object == 0 && hits[0]->face_index == 1);
            CHECK(hits[0]->u == 0.5f);
            CHECK(hits[0]->position.x == 0.0f && hits[0]->position.y == 0.0f && hits[0]->position.z == 1.0f);
        }
    });

    std::printf("%d tests, %d failed checks\n", g_run, g_failed);
    return g_failed ? 1 : 0;
}
