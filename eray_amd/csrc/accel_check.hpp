// accel_check.hpp — checker of a ray-query hierarchy (accel_walk.hpp) whichever builder made it,
// plain host C++: no HIP call, no HIP type.  It verifies what the walk relies on, not how the
// tree was split, so the host builder's (accel_build.hpp) and the device builder's (accel_dev.hip)
// output both pass.
//
// Per object of at least min_faces faces (its slots are [ubegin, ubegin + size)):
//   - the slots are a permutation of its faces, each `hot` slot a byte copy of its record;
//   - the unculled list is exactly the faces face_margin leaves unculled, in ascending index;
//   - every leaf holds 1 .. kLeafFaces faces in ascending index, inside the object's slots;
//   - every node's min_index is its subtree's minimum; an inner node's left child has the smaller
//     minimum and right_min is the right child's;
//   - in double, [c - h, c + h] contains every vertex (a, a + e1, a + e2) of every face of the
//     subtree; alpha and beta are at least the subtree's maxima, the object's gamma the object's;
//   - the depth is within ceil(log2(C / kLeafFaces)) + 1 for C culled faces and within kStackDepth.
// Every node of the scene is reached exactly once; smaller objects have has == 0.
#pragma once

#include <cstddef>
#include <cstdint>

#include "accel_walk.hpp"

namespace eray {
namespace accel {

// nullptr when every invariant holds, else the first violated one (a message that stays valid
// until the calling thread's next call).  faces: the scene's records, object after object
// (sizes[0 .. nobj)); objs: nobj records; nodes, hot / index: the hierarchy's arrays.
const char* check(const Hot* faces, const uint32_t* sizes, size_t nobj, uint32_t min_faces, const Object* objs,
                  const Node* nodes, size_t nnodes, const Hot* hot, const uint32_t* index, size_t nslots);

}  // namespace accel
}  // namespace eray
