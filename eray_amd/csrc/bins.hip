// bins.hip — screen bins of the large objects' faces for the frame kernel's primary-ray scan,
// rebuilt per camera entirely on the device.  A bin is one 16 x 4 pixel sub-block: exactly one
// wave's pixels.
//
// The per-face pixel rectangles (face_rect.hpp, setup.hip) say which bins a face can be hit in.
// For objects too large to scan per wave (> kDirectMax faces) the frame kernel reads, for its
// sub-block's bin, the faces that can be hit there and runs the exact tests on those only: a face
// outside the bin's list cannot be hit by any ray of the bin.  The list need not be in index
// order: the frame kernel keeps, per pixel, the smallest face index whose Triangle::intersects
// passes, which is the reference's first hit (object.rs:63-78).
//
// Each entry also carries the bin's pixels the face may cover (bin_pixels: the four culling
// bounds solved per pixel row), so the frame kernel only tests (face, pixel) pairs that can hit.
// The general tracer's setup (SetupParams::keep_all) masks the pixels any of whose jittered
// anti-aliasing rays may pass instead (bin_pixels_jittered; trace.hip).
//
// Per camera, after camera_setup_kernel (each binned face's bin rectangle and its number of units,
// bin rows or bins): exclusive scan of the units -> the pair pass (bin_segments_kernel /
// bin_pairs_kernel, bin_pairs.hpp) computes the (face, bin) pairs' pixel masks and appends the non-empty
// pairs (wave-aggregated slot counter) with a per-bin count -> exclusive scan of the counts ->
// each entry scattered to its bin (one 64-B BinEntry line: record, mask, face) -> the counts
// zeroed for the next camera, the binned objects' rectangles narrowed to their non-empty bins,
// their bin views in the descriptors -> the detail sub-block list.
// Buffers are preallocated (bins_alloc); if the pairs exceed the capacity the bins are dropped
// for that camera (the frame kernel scans those objects through LDS tiles instead, still exact)
// and CamState reports the count, so the host can grow the capacity.
//
// This unit keeps the allocation and the launch chain; its device code, in the old order:
// bin_walk.hpp (the unit walk and the entry append), bin_pairs.hpp (the pair pass), bin_place.hpp
// (scatter, sort, finaliser), bin_detail.hpp (the detail sub-block lists).  Sizes: bin_layout.hpp.
#include <algorithm>
#include <mutex>

#include <hipcub/hipcub.hpp>

#include "bins.hpp"
#include "internal.hpp"

#include "bin_walk.hpp"
#include "bin_pairs.hpp"
#include "bin_place.hpp"
#include "bin_detail.hpp"

namespace eray {
namespace gpu {
namespace {

constexpr uint32_t kPairGrid = 2048;  // workgroups of the grid-stride pair and scatter loops

// Workgroups of kBinWG threads of kernel `k` resident at once on the device (occupancy API, per
// kernel slot), kPairGrid if unknown.
uint32_t resident_grid(const void* k, int slot) {
    static std::mutex mu;
    static int per_cu[3] = {-1, -1, -1}, cus = -1;
    std::lock_guard<std::mutex> lock(mu);
    if (cus < 0) {
        int dev = 0;
        if (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0)
            cus = 0;
    }
    if (per_cu[slot] < 0 && hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu[slot], k, kBinWG, 0) != hipSuccess)
        per_cu[slot] = 0;
    return cus > 0 && per_cu[slot] > 0 ? (uint32_t)(cus * per_cu[slot]) : kPairGrid;
}

}  // namespace

hipError_t bins_alloc(BinBuffers& b, uint32_t T, uint32_t nb, const uint32_t* kbegin, const uint32_t* kobj, uint32_t W,
                      uint32_t H, uint32_t phase, uint32_t tiles_x, uint32_t rows, size_t cap, hipStream_t s,
                      uint32_t ncam) {
    hipError_t e = hipStreamSynchronize(s);  // the buffers may be in use by enqueued work
    if (e != hipSuccess) return e;
    b = BinBuffers{};
    const BinLayout l = bin_layout(T, nb, W, H, phase, tiles_x, rows, cap, ncam);
    auto fill = [&]() -> hipError_t {
        auto some = [](size_t n) { return n ? n : (size_t)1; };
        if ((e = b.first.alloc(some(T))) != hipSuccess || (e = b.boff.alloc(kSetupMaxBlocks + 1)) != hipSuccess ||
            (e = b.count.alloc(l.keys + 1)) != hipSuccess || (e = b.start.alloc(l.keys + 1)) != hipSuccess ||
            (e = b.kbegin.alloc(some(nb))) != hipSuccess || (e = b.kobj.alloc(some(nb))) != hipSuccess ||
            (e = b.n.alloc(kShards * kShardStride)) != hipSuccess || (e = b.done.alloc(1)) != hipSuccess ||
            (e = b.acc.alloc(some(kAccStride * (size_t)nb))) != hipSuccess || (e = b.part.alloc(l.part_words)) != hipSuccess ||
            (e = b.ekey.alloc(some(cap))) != hipSuccess || (e = b.eface.alloc(some(cap))) != hipSuccess ||
            (e = b.emask.alloc(some(cap))) != hipSuccess || (e = b.erank.alloc(some(cap))) != hipSuccess ||
            (e = b.ent.alloc(some(cap))) != hipSuccess || (e = b.dflags.alloc(some(l.nsub))) != hipSuccess ||
            (e = b.dpacked.alloc(some(l.nsub))) != hipSuccess || (e = b.dflags_light.alloc(some(l.nsub))) != hipSuccess ||
            (e = b.dlight.alloc(some(l.nsub))) != hipSuccess || (e = b.dcount.alloc(2)) != hipSuccess ||
            (e = b.dlist.alloc(some(l.dlist_len))) != hipSuccess || (e = b.docc.alloc(some(l.docc_len))) != hipSuccess ||
            (e = b.sortq.alloc(some(l.keys))) != hipSuccess || (e = b.nsort.alloc(2)) != hipSuccess)
            return e;
        // counters zero between builds (each build leaves them so)
        if ((e = hipMemsetAsync(b.count, 0, sizeof(uint32_t) * (l.keys + 1), s)) != hipSuccess ||
            (e = hipMemsetAsync(b.n, 0, sizeof(uint32_t) * kShards * kShardStride, s)) != hipSuccess ||
            (e = hipMemsetAsync(b.nsort, 0, 2 * sizeof(uint32_t), s)) != hipSuccess ||
            (e = hipMemsetAsync(b.done, 0, sizeof(uint32_t), s)) != hipSuccess ||
            (e = hipMemsetAsync(b.acc, 0, sizeof(uint32_t) * kAccStride * nb, s)) != hipSuccess ||
            (e = hipMemcpyAsync(b.kbegin, kbegin, sizeof(uint32_t) * nb, hipMemcpyHostToDevice, s)) != hipSuccess ||
            (e = hipMemcpyAsync(b.kobj, kobj, sizeof(uint32_t) * nb, hipMemcpyHostToDevice, s)) != hipSuccess)
            return e;
        // hipcub scratch: the larger of the two device-wide passes
        size_t t2 = 0, t3 = 0;
        if ((e = hipcub::DeviceScan::ExclusiveSum(nullptr, t2, (uint32_t*)nullptr, (uint32_t*)nullptr, (int)(l.keys + 1), s)) !=
                hipSuccess ||
            (e = hipcub::DeviceSelect::Flagged(nullptr, t3, (uint32_t*)nullptr, (uint8_t*)nullptr, (uint32_t*)nullptr,
                                               (uint32_t*)nullptr, (int)std::max<size_t>(l.nsub, 1), s)) != hipSuccess)
            return e;
        b.temp_bytes = std::max(t2, t3);
        if ((e = b.temp.alloc(some(b.temp_bytes))) != hipSuccess) return e;
        return hipStreamSynchronize(s);  // the host arrays above are the caller's
    };
    if ((e = fill()) != hipSuccess) {
        b = BinBuffers{};
        return e;
    }
    static_cast<BinLayout&>(b) = l;
    return hipSuccess;
}

hipError_t launch_bins_build(const SetupParams& sp, BinBuffers& b, uint32_t tiles_x, bool ordered, hipStream_t s) {
    hipError_t e;
    const size_t keys = b.keys;
    size_t tb = b.temp_bytes;
    const bool multi = sp.ncam > 1;
    const uint32_t ncam = multi ? sp.ncam : 1u;
    if (sp.T) {  // (a multi-camera build may set up fewer cameras than the buffers hold)
        const uint32_t nparts = setup_blocks(sp.T), chunk = (sp.T + nparts - 1) / nparts;  // as camera_setup_kernel
        auto* k = bin_segments(sp) ? bin_segments_kernel : sp.keep_all ? bin_pairs_kernel<true> : bin_pairs_kernel<false>;
        // exactly the resident workgroups (each wave walks a fixed share of the units: a second
        // round of workgroups would double the pass)
        const uint32_t pgrid = resident_grid(reinterpret_cast<const void*>(k), bin_segments(sp) ? 2 : sp.keep_all ? 1 : 0);
        k<<<pgrid, kBinWG, 0, s>>>(sp.cull, sp.range, b.first, b.boff, nparts, chunk, sp.fkey, sp.T, sp.W, sp.H, sp.phase,
                                       b.bins_x, b.nbins, (uint32_t)b.cap, b.n, b.count, b.ekey, b.eface, b.emask, b.erank);
        if ((e = hipGetLastError()) != hipSuccess) return e;
    }
    tb = b.temp_bytes;
    if ((e = hipcub::DeviceScan::ExclusiveSum(b.temp, tb, (uint32_t*)b.count, (uint32_t*)b.start, (int)(keys + 1), s)) != hipSuccess)
        return e;
    bin_scatter_kernel<<<kPairGrid, kBinWG, 0, s>>>(b.n, (uint32_t)b.cap, b.ekey, b.eface, b.emask, b.erank, b.start,
                                                    b.kbegin, b.nbins, sp.hot, multi ? sp.T1 : 0u, b.ent);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const uint32_t per = b.fin_per, fgrid = b.fin_grid;  // at most kFinGrid workgroups, each over `per` consecutive keys
    bins_finalize_kernel<false><<<fgrid, kBinWG, 0, s>>>(per, b.start, b.nb, b.bins_x, b.nbins, sp.W, sp.H, b.phase,
                                                         b.acc, b.part, b.done, b.n, (uint32_t)b.cap, b.kobj, sp.objs,
                                                         b.ent, b.count, b.sortq, b.nsort, sp.state, ncam, nullptr, 1u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bin_sort_kernel<<<kSortGrid, kBinWG, 0, s>>>(b.sortq, b.nsort, b.start, b.ent, (uint32_t)keys);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    bins_finalize_kernel<true><<<1, kBinWG, 0, s>>>(per, b.start, b.nb, b.bins_x, b.nbins, sp.W, sp.H, b.phase, b.acc,
                                                    b.part, b.done, b.n, (uint32_t)b.cap, b.kobj, sp.objs, b.ent, b.count,
                                                    b.sortq, b.nsort, sp.state, ncam, sp.path_union,
                                                    sp.union_nobj ? sp.union_nobj : 1u);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    if (!b.nsub) return hipSuccess;
    const uint32_t n = (uint32_t)b.nsub;
    if (ordered) {
        detail_flags_kernel<<<(n + kBinWG - 1) / kBinWG, kBinWG, 0, s>>>(sp.objs, sp.nobj, sp.W, sp.row0, sp.rows,
                                                                        sp.band_shift, sp.band_mask, sp.band_stride,
                                                                        b.bins_x, b.phase, tiles_x, n, sp.keep_all ? kTraceHeavyMin : 64u, b.dflags,
                                                                        b.dflags_light, b.dpacked, b.docc);
        if ((e = hipGetLastError()) != hipSuccess) return e;
        tb = b.temp_bytes;
        uint32_t *packed = b.dpacked, *dcount = b.dcount;
        if ((e = hipcub::DeviceSelect::Flagged(b.temp, tb, packed, (uint8_t*)b.dflags, (uint32_t*)b.dlist, dcount, (int)n, s)) !=
            hipSuccess)
            return e;
        tb = b.temp_bytes;
        if ((e = hipcub::DeviceSelect::Flagged(b.temp, tb, packed, (uint8_t*)b.dflags_light, (uint32_t*)b.dlight, dcount + 1, (int)n,
                                               s)) != hipSuccess)
            return e;
        detail_append_kernel<<<std::max<uint32_t>(1u, std::min<uint32_t>(1024u, (n + kBinWG - 1) / kBinWG)), kBinWG, 0,
                               s>>>(b.dlight, b.dcount, b.dlist, sp.state);
        return hipGetLastError();
    }
    detail_list_kernel<<<dim3((n + kBinWG - 1) / kBinWG, ncam), kBinWG, 0, s>>>(
        sp.objs, multi ? sp.nobj1 : sp.nobj, sp.W, sp.row0, sp.rows, sp.band_shift, sp.band_mask, sp.band_stride, b.bins_x,
        b.phase, tiles_x, n, b.dlist, b.docc, sp.state);
    return hipGetLastError();
}

}  // namespace gpu
}  // namespace eray
