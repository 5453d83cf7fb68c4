// owners.hpp — move-only owners of the HIP resources the C-ABI layer holds (host code only: no
// kernel sees these types).  Each destructor releases its resource; each converts to the raw
// handle or pointer it owns, so launch parameters are filled as from raw fields.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

#include "accel_layout.hpp"
#include "accel_walk.hpp"

struct eray_ctx;

namespace eray {
namespace gpu {

// A HIP handle (a pointer type) released by Destroy.
template <typename H, hipError_t (*Destroy)(H)>
class Handle {
public:
    Handle() = default;
    Handle(Handle&& o) noexcept : h_(std::exchange(o.h_, nullptr)) {}
    Handle& operator=(Handle&& o) noexcept {
        if (this != &o) {
            reset();
            h_ = std::exchange(o.h_, nullptr);
        }
        return *this;
    }
    ~Handle() { reset(); }
    void reset() {
        if (h_) (void)Destroy(h_);
        h_ = nullptr;
    }
    operator H() const { return h_; }
    H* put() {  // for the creating call (releases what it held)
        reset();
        return &h_;
    }

private:
    H h_ = nullptr;
};

struct Event : Handle<hipEvent_t, hipEventDestroy> {
    hipError_t create(unsigned flags = hipEventDefault) { return hipEventCreateWithFlags(put(), flags); }
};
struct Stream : Handle<hipStream_t, hipStreamDestroy> {
    hipError_t create(unsigned flags) { return hipStreamCreateWithFlags(put(), flags); }
    hipError_t create(unsigned flags, int priority) { return hipStreamCreateWithPriority(put(), flags, priority); }
};
using Graph = Handle<hipGraph_t, hipGraphDestroy>;
using GraphExec = Handle<hipGraphExec_t, hipGraphExecDestroy>;

// A captured launch plan with the key it was captured for (capi_frames.cpp ensure_graph).
struct FrameGraph {
    Graph graph;
    GraphExec exec;  // (destroyed before its graph)
    std::vector<unsigned char> key;
    uint64_t used = 0;
};

// `cap` elements of T, released by Free (device or pinned host memory).
template <typename T, hipError_t (*Free)(void*)>
class Buffer {
public:
    Buffer() = default;
    Buffer(Buffer&& o) noexcept : p_(std::exchange(o.p_, nullptr)), cap(std::exchange(o.cap, 0)) {}
    Buffer& operator=(Buffer&& o) noexcept {
        if (this != &o) {
            (void)release();
            p_ = std::exchange(o.p_, nullptr);
            cap = std::exchange(o.cap, 0);
        }
        return *this;
    }
    ~Buffer() { (void)release(); }
    hipError_t release() {
        const hipError_t e = p_ ? Free(p_) : hipSuccess;
        p_ = nullptr;
        cap = 0;
        return e;
    }
    operator T*() const { return p_; }
    T* operator->() const { return p_; }

protected:
    T* p_ = nullptr;

public:
    size_t cap = 0;  // elements
};

template <typename T>
struct DeviceBuf : Buffer<T, hipFree> {
    hipError_t alloc(size_t n) {  // n >= 1 elements, replacing what it held
        hipError_t e = this->release();
        if (e == hipSuccess) e = hipMalloc((void**)&this->p_, n * sizeof(T));
        if (e == hipSuccess) this->cap = n;
        return e;
    }
    // At least `need` elements: nothing when they fit, else ctx's stream is synchronised, the old
    // allocation freed and max(need, 1) elements allocated (contents are not kept).  An eray
    // status; defined in ctx.hpp.
    int ensure(eray_ctx* ctx, size_t need);
};

// The scene's ray-query hierarchy on the device (accel_walk.hpp; capi_rays.cpp
// eray_scene_build_ray_accel and eray_scene_build_ray_accel_device): per object its record, the nodes, the leaf-ordered copies of the
// face records (TriHot bytes) and their original indices.  `valid` falls with any geometry change
// (a stale tree is never used; eray_scene_refit_ray_accel makes it valid again); the memory is
// released by drop() or with the owner.  (AccelDevLayout, a covered object as a refit takes it:
// accel_layout.hpp.)

// What eray_scene_refit_ray_accel_async works in (accel_dev.hip accel_refit_workspace): one device
// allocation that lives from the first eligible call outside a capture until the next build or
// drop — the uploaded layout, the accumulators and counters, per face the flag and (alpha, beta),
// per node the double bounds, per covered object the verdict, and the count of refits executed.
struct RefitWorkspace {
    DeviceBuf<unsigned char> mem;
    size_t o_objs = 0, o_acc = 0, o_cnt = 0, o_flags = 0, o_ab = 0, o_bounds = 0, o_verdict = 0, o_refits = 0;
    size_t bytes = 0;
    uint32_t ncov = 0, blocks = 0, first_deep = 0;
    bool ready() const { return (unsigned char*)mem != nullptr; }
    void release() {
        (void)mem.release();
        bytes = 0;
        ncov = blocks = first_deep = 0;
    }
};

struct RayAccel {
    DeviceBuf<accel::Object> objs;
    DeviceBuf<accel::Node> nodes;
    DeviceBuf<accel::Hot> hot;
    DeviceBuf<uint32_t> index;
    bool valid = false;
    // counts every event after which a launch plan that holds the arrays' addresses must not be
    // replayed: a build, a drop (a rebuilding refit does both), eray_scene_add_object and
    // eray_scene_reset.  Part of the general tracer's plan keys (capi_frames.cpp).  A refit that
    // keeps the topology rewrites the arrays in place and does not count; nor does
    // eray_scene_update_object, which only clears `valid` until that refit (meanwhile the tracer's
    // plans are keyed without a hierarchy).  It outlives drop().
    uint64_t gen = 0;
    uint32_t covered = 0;  // objects the last build gave a hierarchy
    // what the last build covered (eray_debug_ray_accel_check): its min_faces, node and slot counts
    uint32_t min_faces = 0;
    size_t node_count = 0, slot_count = 0;
    // which builder made it (kNone: never built, or dropped) and, for the device builder and the
    // refittable host build (eray_scene_build_ray_accel_refittable), its host-side layout and depth:
    // what eray_scene_refit_ray_accel needs to rewrite the levels of the same topology
    enum Builder : uint32_t { kNone = 0, kHost = 1, kDevice = 2, kHostRefittable = 3 };
    bool refittable() const { return builder == kDevice || builder == kHostRefittable; }
    Builder builder = kNone;
    std::vector<AccelDevLayout> layout;
    uint32_t max_depth = 0;
    // eray_scene_add_object or eray_scene_reset happened since the build: `objs` holds a record per
    // object of the scene as it was, so the arrays fit the old scene only — a refit rebuilds
    bool scene_changed = false;
    // the async refit's workspace (fits `layout`: released with it) and whether it runs the upper
    // levels in one launch (a setting of eray_debug_set_refit_top_levels: it outlives drop())
    RefitWorkspace refit;
    bool refit_top_levels = true;
    size_t device_bytes() const {  // of the four arrays as allocated
        return sizeof(accel::Object) * objs.cap + sizeof(accel::Node) * nodes.cap + sizeof(accel::Hot) * hot.cap + 4 * index.cap;
    }
    void drop() {
        refit.release();
        ++gen;
        covered = 0;
        valid = false;
        min_faces = 0;
        node_count = slot_count = 0;
        builder = kNone;
        layout.clear();
        max_depth = 0;
        scene_changed = false;
        (void)objs.release();
        (void)nodes.release();
        (void)hot.release();
        (void)index.release();
    }
};

// Pinned host memory; allocated with hipHostMallocMapped, `dev` is its device address.
template <typename T>
struct PinnedBuf : Buffer<T, hipHostFree> {
    T* dev = nullptr;
    hipError_t alloc(size_t n, unsigned flags = hipHostMallocDefault) {
        dev = nullptr;
        hipError_t e = this->release();
        if (e == hipSuccess) e = hipHostMalloc((void**)&this->p_, n * sizeof(T), flags);
        if (e == hipSuccess) this->cap = n;
        if (e == hipSuccess && (flags & hipHostMallocMapped)) e = hipHostGetDevicePointer((void**)&dev, this->p_, 0);
        return e;
    }
};

}  // namespace gpu
}  // namespace eray
