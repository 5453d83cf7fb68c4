// bin_layout.hpp — the sizes of the screen bins (bins.hip) for one layout: bin columns and rows,
// keys, the detail lists' lengths, the shard region and the finaliser's grid.  Index arithmetic
// with no HIP header or call, so the allocation and the launch chain (bins.hip), the setups
// (capi_setup.cpp), the kernels (through internal.hpp) and the stand-alone checker
// (tests/cpp/bin_layout_main.cpp, built with the host sanitizers) share it.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include "band_rows.hpp"

namespace eray::gpu {

// Screen bins of large objects' faces: kBinW x kBinH pixels (one wave's 16 x 4 sub-block).
constexpr uint32_t kBinW = 16, kBinH = 4;
constexpr int kBinWG = 256;  // threads per workgroup of the bins' kernels
// The entry list's slot counter is sharded: device-scope atomics execute at the memory side, and
// one word (or one 64-B line) takes about 88 returning atomics per microsecond (MI355X_MICROARCH.md
// dequeue row), so one counter bumped once per 256 pairs serialised the pair pass (C5's four-camera
// build: ~115k bumps, 1.3-1.8 ms).  Workgroup b appends to shard b % kShards, which owns entries
// [s * region, (s + 1) * region) (region = cap / kShards); its counter sits kShardStride words
// from the next one (a line of its own).  Pairs are dealt to the workgroups in 256-pair chunks
// round-robin, so the shards fill evenly.
constexpr uint32_t kShards = 32, kShardStride = 32;
// binned object k's rectangle accumulator: acc + kAccStride * k (a line per object: the
// finaliser's per-workgroup atomics on different objects do not share a line)
constexpr uint32_t kAccStride = 16;
constexpr uint32_t kFinGrid = 512;  // workgroups of the finaliser's per-key pass

// Bins start at camera rows phase + k * kBinH - kBinH (phase = the first rendered row % kBinH, so
// a rendered sub-block is one bin): the bin row of camera row y, the bin column of pixel column x.
ERAY_HD_PLAIN inline uint32_t bin_phase(uint32_t row0) { return row0 % kBinH; }
ERAY_HD_PLAIN inline uint32_t bin_row(uint32_t y, uint32_t phase) { return (y + kBinH - phase) / kBinH; }
ERAY_HD_PLAIN inline uint32_t bin_col(uint32_t x) { return x / kBinW; }
ERAY_HD_PLAIN inline uint32_t bin_cols(uint32_t W) { return (W + kBinW - 1) / kBinW; }  // bin columns of a frame
// the 64 x 4 pixel blocks across a frame (four sub-blocks each)
ERAY_HD_PLAIN inline uint32_t frame_tiles_x(uint32_t W) { return (W + 63) / 64; }
// entries of one shard of an entry list of `cap`
ERAY_HD_PLAIN inline uint32_t shard_region(uint32_t cap) { return cap / kShards; }

struct BinLayout {
    uint32_t T = 0, nb = 0, phase = 0;  // faces, binned objects, row phase (as given)
    size_t cap = 0;                     // entry capacity (as given)
    uint32_t bins_x = 0, bins_y = 0, nbins = 0;
    size_t keys = 0;                    // nb * nbins: bin key = k * nbins + bin for binned object k
    uint32_t subs_y = 0;                // sub-block rows of the rendered rows
    size_t nsub = 0;                    // sub-blocks of one camera's detail list (padded rows)
    size_t dlist_len = 0, docc_len = 0; // every camera's list and occupancy bytes
    size_t part_words = 0;
    uint32_t region = 0;                // a shard's entries
    uint32_t fin_per = 0, fin_grid = 0; // the finaliser: at most kFinGrid workgroups, each over fin_per consecutive keys
};

// T faces, nb binned objects, a W x H camera, row phase, tiles_x blocks across and `rows` rendered
// rows, entry capacity `cap`, the detail lists of `ncam` cameras.
inline BinLayout bin_layout(uint32_t T, uint32_t nb, uint32_t W, uint32_t H, uint32_t phase, uint32_t tiles_x,
                            uint32_t rows, size_t cap, uint32_t ncam) {
    BinLayout l;
    l.T = T;
    l.nb = nb;
    l.phase = phase;
    l.cap = cap;
    l.bins_x = bin_cols(W);
    l.bins_y = H ? bin_row(H - 1, phase) + 1 : 1;
    l.nbins = l.bins_x * l.bins_y;
    l.keys = (size_t)nb * l.nbins;
    l.subs_y = (rows + kBinH - 1) / kBinH;
    l.nsub = 4 * (size_t)tiles_x * l.subs_y;
    l.dlist_len = l.nsub * ncam;
    l.docc_len = (size_t)tiles_x * l.subs_y * ncam;
    const size_t wgs = (l.keys + kBinWG - 1) / kBinWG;
    l.part_words = 10 * (wgs > 1 ? wgs : 1);
    l.region = shard_region((uint32_t)cap);
    const size_t span = (size_t)kFinGrid * kBinWG, per = (l.keys + span - 1) / span * kBinWG;
    l.fin_per = (uint32_t)(per > (size_t)kBinWG ? per : (size_t)kBinWG);
    const size_t grid = (l.keys + l.fin_per - 1) / l.fin_per;
    l.fin_grid = (uint32_t)(grid > 1 ? grid : 1);
    return l;
}

}  // namespace eray::gpu
