// engine.hpp — the render side of the C++ host: Vector, Camera, Light, Material, Object,
// Scene and Engine with the reference's builder API (src/lib/{camera,light,material,object,
// scene,engine}.rs), rendering through the C-ABI (include/eray_hip.h) on the current Device.
#pragma once

#include <array>
#include <map>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include "graph.hpp"
#include "image.hpp"

namespace eray {

struct Vector3 {
    float x = 0.0f, y = 0.0f, z = 0.0f;
    Vector3() = default;
    Vector3(float x_, float y_, float z_) : x(x_), y(y_), z(z_) {}
};

struct Fov {  // camera.rs:8-12 Fov(f32, f32)
    float a = 60.0f, b = 60.0f;
    float ratio() const { return a / b; }
};

// camera.rs:15-38 (target / up are not used by the render path)
struct Camera {
    Vector3 center{0.0f, 0.0f, 0.0f};
    Fov fov{60.0f, 60.0f};
    uint32_t width = 1024;
    float z_dist = 1.0f;
    // camera.rs:36-38: (width, (width as f32 / fov.ratio()) as u32)
    std::pair<uint32_t, uint32_t> size() const;
};

struct Transform {  // transform.rs: only the translation reaches the path
    Vector3 translation;
    Transform apply_translation(Vector3 t) const { return Transform{t}; }
};

enum class LightVariant { Point, Ambient };  // light.rs:20-25

struct Light {  // light.rs:7-16
    Transform transform;
    LightVariant variant = LightVariant::Point;
    Color color{1.0f, 1.0f, 1.0f};
    float brightness = 1.0f;
};

// material.rs:96-104
enum class StandardMaterialOutput { Color, Diffuse, Specular, SpecularPower, Reflection };

// material.rs:13-94: a validated graph and the outputs that feed the renderer
class Material {
public:
    Material() = default;
    Material(shader::Graph<shader::Validated> graph, std::map<StandardMaterialOutput, shader::Name> selected);
    // material.rs:35-53: runs the graph once (until an input changes)
    shader::Status update();
    // material.rs:96-112: set a graph input (Missing(Input, name) if absent)
    shader::Status set_input(const shader::Name& name, shader::SocketValue value);
    // the selected outputs as device images (IColor for Color, IValue for the others; any
    // other kind is ignored, as Material::get does)
    eray_material device_material() const;
    const shader::Graph<shader::Validated>& graph() const { return graph_; }

private:
    std::map<StandardMaterialOutput, shader::Name> selected_;
    shader::Graph<shader::Validated> graph_;
    bool recompute_ = true;
};

struct Building {};  // object.rs typestate
struct Built {};

struct Triangle {  // primitives.rs: positions, vertex normals, uvs of a face
    std::array<Vector3, 3> pos, normal;
    std::array<std::array<float, 2>, 3> uv;
};

// object.rs:30-52
template <class State>
struct Object {
    std::vector<Vector3> vertices, normals;
    std::vector<std::array<float, 2>> uvs;
    std::vector<Triangle> faces;
    std::array<Vector3, 2> bbox{};  // (0,0,0)-(0,0,0) for loaded meshes (object.rs:306-315)
    Material material;
};

// object.rs:101-186 Object::load_obj (the reference's dialect; its panics become Failure with
// ERAY_E_PARSE / ERAY_E_IO)
Object<Building> load_obj(const std::string& path);
// object.rs:213-230 Object::build: "Missing vertices" / "Missing normals" -> Failure with
// ERAY_E_BUILD
Object<Built> build(Object<Building> object);

// scene.rs:12-54
class Scene {
public:
    Scene& set_camera(Camera camera);
    Scene& add_light(Light light);
    Scene& add_object(Object<Built> object);
    const Camera& camera() const { return camera_; }
    std::vector<Object<Built>>& objects() { return objects_; }
    const std::vector<Light>& lights() const { return lights_; }

private:
    Camera camera_{};
    std::vector<Light> lights_;
    std::vector<Object<Built>> objects_;
    friend class Engine;
    bool dirty_ = true;
};

// raycasting.rs:9-21: a start and a direction; Ray::make is Ray::new (the direction normalised,
// vector.rs:150-158), an aggregate Ray{start, dir} keeps dir as given (a Ray's stored dir)
struct Ray {
    Vector3 start, dir;
    static Ray make(Vector3 start, Vector3 dir);
};

// raycasting.rs:43-54 RaycastHit, with the hit's uv (object.rs:70-72) and barycentric u, v
// (primitives.rs:60-61) in place of the material bundle Material::get derives from the uv
struct RaycastHit {
    uint32_t object = 0;      // index in Scene::objects()
    uint32_t face_index = 0;  // relative to the object's first face
    Vector3 position, normal;
    std::array<float, 2> uv{};
    float u = 0.0f, v = 0.0f;
};

// engine.rs:13-98
class Engine {
public:
    // Engine::new((width, height), bounces, anti_aliasing)
    Engine(std::pair<uint32_t, uint32_t> size, uint32_t bounces, uint32_t anti_aliasing);
    Scene& scene() { scene_.dirty_ = true; return scene_; }
    // engine.rs:46-81: renders on the GPU; the f32 image (Image<Color>) is copied back
    const Image<Color>& render();
    // engine.rs:86-98: render + save_as_ppm (the PPM bytes come from the device, fused)
    const Image<Color>& render_to_path(const std::string& path);
    // object.rs:58-81 Object::intersects for each ray, on the GPU (eray_cast_rays): object -1 the
    // scene's closest object as cast_ray selects it (by the camera's centre, engine.rs:116-126),
    // k >= 0 Object k alone; nullopt is a miss
    std::vector<std::optional<RaycastHit>> cast_rays(const std::vector<Ray>& rays, int object = -1);
    // engine.rs:218-228 Engine::reaches_light for each shadow ray and its light position, on the
    // GPU (eray_rays_reach_light): true unless the first object in scene order that the ray hits
    // is hit no farther from the ray's start than the target lies.  cast_ray's own shadow ray of a
    // hit at P with normal N is Ray::make(P + N * 0.1, L - P) with target L (engine.rs:136-141).
    std::vector<bool> reaches_light(const std::vector<Ray>& rays, const std::vector<Vector3>& targets);
    // A hierarchy for cast_rays over the objects of at least min_faces faces (0: the library's
    // default), built from the uploaded scene (eray_scene_build_ray_accel): the same hits, found
    // without scanning every face.  It lasts until the scene changes (scene() marks it changed:
    // the next upload drops it) or drop_ray_accel.  on_device builds it on the GPU from the resident
    // records (eray_scene_build_ray_accel_device) instead of on the host: the same hits either way.
    // refittable (the three-argument form; false in the other) is the host build with what a refit needs kept beside it
    // (eray_scene_build_ray_accel_refittable): refit_ray_accel then keeps this tree's topology.  With
    // on_device it is a failure (ERAY_E_INVALID_ARGUMENT): a device build is always refittable.
    // The hierarchy also speeds up render(): with anti-aliasing or bounces the shadow and reflected
    // rays of every pixel search the covered objects through it (ERAY_HAS_TRACE_RAY_ACCEL; the same
    // image, bit for bit) — what pays for objects whose bounding box is real, i.e. lets those rays in.
    struct RayAccelInfo {
        uint32_t objects, max_depth;
        uint64_t nodes, faces, unculled_faces, device_bytes;
        float build_ms;
    };
    RayAccelInfo build_ray_accel(uint32_t min_faces = 0, bool on_device = false);
    RayAccelInfo build_ray_accel(uint32_t min_faces, bool on_device, bool refittable);
    void drop_ray_accel();
    // New geometry for object `index` of the scene in place (eray_scene_update_object): the faces
    // (positions, normals, uvs) and the bounding box of `object` replace the scene object's; the
    // face count must be the same, the scene object's material, the lights and the other objects
    // stay.  Unlike scene(), this does not mark the scene changed: nothing else is uploaded again.
    // Every later render and query answers as for a scene built with the new object.  A hierarchy
    // is not used again until refit_ray_accel or build_ray_accel.  Failure with
    // ERAY_E_INVALID_ARGUMENT for an index that is no object or another face count.
    void update_object(size_t index, const Object<Built>& object);
    // The hierarchy made valid for the current geometry (eray_scene_refit_ray_accel): after
    // update_object alone, on a device-built or refittable host-built hierarchy, the tree's topology is kept and its boxes,
    // margins and face copies are recomputed (the same hits; pruning weakens as the mesh moves away
    // from the geometry the tree was split for); otherwise it is rebuilt, by the refittable host
    // build when that made it, else on the device.
    struct RayAccelRefitInfo {
        RayAccelInfo accel;
        uint32_t refitted;  // objects whose topology was kept
        bool rebuilt;
    };
    RayAccelRefitInfo refit_ray_accel();
    // The anti-aliasing jitter stream's key (eray_render_params::aa_seed).  The reference draws
    // from the OS-seeded thread_rng; a new Engine picks a random seed likewise, and fixing it
    // makes anti-aliased renders reproducible.
    void set_aa_seed(uint64_t seed) { aa_seed_ = seed; }
    uint64_t aa_seed() const { return aa_seed_; }

private:
    void upload();
    Image<Color> image_;
    Scene scene_;
    uint32_t bounces_, anti_aliasing_;
    uint64_t aa_seed_ = 0;
    std::shared_ptr<DeviceBuffer> rgb_, ppm_;
};

}  // namespace eray
