// accel_dev.hpp — the device-side builder of the ray-query hierarchy (accel_dev.hip): the same
// records as accel_build.hpp's host builder (accel_walk.hpp Object / Node, leaf-ordered TriHot
// copies, the index array), built on a stream from the resident face records.  Host interface
// only; capi_rays.cpp's eray_scene_build_ray_accel_device owns the context side.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>
#include <vector>

#include "internal.hpp"
#include "owners.hpp"

namespace eray {
namespace gpu {

struct AccelDevObject {  // an object that gets a hierarchy
    uint32_t index;      // in the scene
    uint32_t hot_begin;  // its first record in the scene's TriHot array
    uint32_t faces;
};

struct AccelDevInfo {
    uint32_t max_depth = 0;
    uint64_t nodes = 0, unculled = 0;
};

// Builds the hierarchy of `covered` (scene order) into ra (objs: nobj records, zero for the other
// objects) on stream s and waits for it.  One device-to-host copy: 16 B of counters per covered
// object (culled, unculled, status); no face record leaves the device.  Temporaries are released
// before it returns.  *refuse (when set on return, with hipSuccess) names why the scene is not
// supported; ra is then left dropped.
hipError_t accel_build_device(const TriHot* d_hot, const std::vector<AccelDevObject>& covered, size_t nobj, RayAccel& ra,
                              hipStream_t s, AccelDevInfo* info, const char** refuse);

// Refits a hierarchy that accel_build_device built, or a host build whose layout build_scene recorded
// (accel_build.hpp; eray_scene_build_ray_accel_refittable: numbering 1) (ra.layout, ra.max_depth, its four arrays) to
// the records d_hot now holds, on stream s, and waits for it: the topology, the slots and the
// unculled lists stay; every margin, box, min_index, record copy and gamma is recomputed by the
// build's functions.  The same one device-to-host copy as the build.  *kept is false (ra's arrays
// partly rewritten, not to be used) when some face changed between culled and unculled: the caller
// rebuilds.  Temporaries (flags, margins, per-node double bounds) are released before it returns.
hipError_t accel_refit_device(const TriHot* d_hot, RayAccel& ra, hipStream_t s, AccelDevInfo* info, bool* kept);

// The same refit without the host in it (eray_scene_refit_ray_accel_async).  accel_refit_workspace
// allocates ra.refit for ra.layout, uploads the layout and waits (not during a capture);
// accel_refit_enqueue then only launches kernels on s — the reset of the accumulators, the margin and
// check passes, the levels (those of at most kBlock nodes in one launch per default), and
// refit_object_kernel, which takes the verdict per covered object and writes its record: has = 0 where
// a face changed class, so that queries scan that object until a later refit passes.  No copy, no
// wait, no allocation: capturable.  accel_refit_status waits for s and reads the count of executed
// refits and how many covered objects passed the last one.
hipError_t accel_refit_workspace(RayAccel& ra, hipStream_t s);
hipError_t accel_refit_enqueue(const TriHot* d_hot, RayAccel& ra, hipStream_t s);
hipError_t accel_refit_status(const RayAccel& ra, hipStream_t s, uint32_t* refits, uint32_t* kept);

}  // namespace gpu
}  // namespace eray
