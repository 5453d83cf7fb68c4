// bins.hpp — the screen bins' device arrays as the C-ABI layer holds them, their allocation and
// the launch chain that builds a camera's bins (bins.hip).  Host code only: no kernel sees these
// types.
#pragma once

#include "internal.hpp"
#include "owners.hpp"

namespace eray {
namespace gpu {

// Device arrays of the binned objects' screen bins for one layout (bin_layout.hpp: camera size,
// row phase, the binned objects), all preallocated: a camera's bins are rebuilt on the stream with
// no host round trip.  Bin key = k * nbins + bin for binned object k; a bin's entries (face
// relative to the object, pixel mask, intersection record) are unordered — the frame kernel keeps
// the smallest face index that hits, which is the reference's first hit (object.rs:63-78).  Each
// array is released with the struct; whoever drops one synchronises the streams that use it first.
struct BinBuffers : BinLayout {
    DeviceBuf<unsigned long long> first;  // SetupParams::first_local (T)
    DeviceBuf<unsigned long long> boff;   // SetupParams::boff (kSetupMaxBlocks + 1)
    DeviceBuf<uint32_t> count;            // per key (nb * nbins + 1), zero between builds
    DeviceBuf<uint32_t> start;            // per key + 1
    DeviceBuf<uint32_t> kbegin;           // tri_begin per binned object
    DeviceBuf<uint32_t> kobj;             // object index per binned object
    DeviceBuf<uint32_t> n;                // entries found (device counter, reset by the finaliser)
    DeviceBuf<uint32_t> done;             // workgroup counter of the finaliser
    DeviceBuf<uint32_t> acc;              // rectangle accumulators of the non-empty bins (a line per object)
    DeviceBuf<uint32_t> part;             // 10 per finaliser workgroup: its end objects' partials
    DeviceBuf<uint32_t> ekey;             // unscattered entries (cap)
    DeviceBuf<uint32_t> eface;
    DeviceBuf<unsigned long long> emask;
    DeviceBuf<uint32_t> erank;            // the entry's place among its bin's entries (count's old value)
    DeviceBuf<BinEntry> ent;              // bin entries in key order (cap)
    // detail sub-block list of the rendered rows
    DeviceBuf<uint8_t> dflags;            // listed sub-blocks whose bin holds more than one chunk
    DeviceBuf<uint8_t> dflags_light;      // ... and the other listed ones
    DeviceBuf<uint32_t> dpacked;
    DeviceBuf<uint32_t> dlist;
    DeviceBuf<uint32_t> dlight;           // the light ones, appended to dlist after the heavy ones
    DeviceBuf<uint32_t> dcount;           // [heavy, light] counts
    DeviceBuf<uint8_t> docc;
    DeviceBuf<uint32_t> sortq;            // bins to sort by face index (bins.hip bin_sort_kernel)
    DeviceBuf<uint32_t> nsort;            // their count, zero between builds
    DeviceBuf<unsigned char> temp;        // hipcub scratch
    size_t temp_bytes = 0;
};
// (Re)allocates `b` for T triangles, nb binned objects (kbegin / kobj: host arrays), a W x H
// camera, row phase and `rows` rendered rows, entry capacity `cap` (synchronises `s` first); the
// detail lists of `ncam` cameras (a multi-camera setup, SetupParams::ncam).  On failure `b` is
// left empty.
hipError_t bins_alloc(BinBuffers& b, uint32_t T, uint32_t nb, const uint32_t* kbegin, const uint32_t* kobj, uint32_t W,
                      uint32_t H, uint32_t phase, uint32_t tiles_x, uint32_t rows, size_t cap, hipStream_t s,
                      uint32_t ncam = 1);
// After launch_camera_setup: the bins of the setup's camera, the binned objects' rectangles
// narrowed to their non-empty bins and their bin views in the descriptors (or none when the
// entries overflow the capacity: the frame kernel then scans those objects through LDS tiles),
// and the detail sub-block list of rows [row0, row0 + rows) with CamState::total_sub.
hipError_t launch_bins_build(const SetupParams& sp, BinBuffers& b, uint32_t tiles_x, bool ordered, hipStream_t s);

}  // namespace gpu
}  // namespace eray
