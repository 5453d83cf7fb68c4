// gather_plan.hpp — the planning of the multi-GPU gathers (comm.cpp): which rows a rank holds, its
// rectangles and their layout, which rank assembles which frame, where every pack, header and
// transfer of a batch lies in a rank's buffer, and the verdicts every rank reaches alike.  Index
// arithmetic with no HIP header or call, so comm.cpp and its kernels (gather_coded.hpp, gather_scene.hpp),
// the host-only diagnostics (gather_debug.cpp) and the stand-alone checker (tests/cpp/gather_plan_main.cpp,
// built with the host sanitizers) share it.  Internal linkage, as when it stood in comm.cpp: the
// kernels take RankLayout, Roots, HeaderSpots and XferHeader by value, so their symbols name these types.
#pragma once

#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <vector>

#include "../../include/eray_hip.h"
#include "band_rows.hpp"

namespace {
constexpr int kMaxCodedRanks = 64;  // the ranks a gather serves (include/eray_hip.h; HeaderSpots, the scratch layout)

// camera rows of `rank` in the interleaved band split (eray_band_rows)
ERAY_HD_PLAIN uint32_t band_rows_of(uint32_t height, uint32_t band_rows, uint32_t nranks, uint32_t rank) {
    if (!band_rows || !nranks || rank >= nranks) return 0;
    const uint32_t bands = height / band_rows, tail = height % band_rows;  // the last band may be short
    uint32_t rows = (bands / nranks + (rank < bands % nranks ? 1u : 0u)) * band_rows;
    if (tail && bands % nranks == rank) rows += tail;  // the short band, band index `bands`
    return rows;
}

// A valid row split of `height` rows over `nranks` (> 0) ranks: interleaved bands of a power of
// two >= 4 rows (as eray_render's bands, capi_frames.cpp), or equal blocks.
inline bool row_split_ok(uint32_t height, uint32_t band_rows, uint32_t nranks) {
    return band_rows ? band_rows >= 4 && !(band_rows & (band_rows - 1)) : height % nranks == 0;
}

// ---- scene-camera gather: only the objects' pixel rectangles travel --------------------------
// The frame kernel writes engine.rs:212's miss colour at every pixel outside the objects' pixel
// rectangles (ObjGeom::rect: no primary ray there can hit any face, the same conservative bounds
// the kernel culls with).  So when every rank's local rows are its renders of the scene camera,
// the frame on rank 0 is the miss colour except inside those rectangles, and only their bytes need
// to cross xGMI.  The rectangles are fixed per camera: each rank states its own (rank-local rows,
// 16-pixel column groups) once, one all-gather exchanges them (the only host synchronisation),
// and every later gather enqueues a pack kernel, fixed-size point-to-point transfers and, on rank
// 0, one assembly kernel — no host round trip, so a serving loop can capture it in a graph.
constexpr int kPlanRects = 8;
struct GatherRect {        // one rectangle of a rank's rows, 32 B
    int32_t l0, l1;        // local rows (inclusive)
    int32_t c0, c1;        // 16-pixel column groups (inclusive)
    uint32_t off;          // byte offset of its first row in the rank's per-frame pack
    uint32_t row_bytes;    // 48 * (c1 - c0 + 1)
    uint32_t first;        // its first packed row among the rank's (pack kernel)
    uint32_t pad;
};
struct RankLayout {        // a rank's rectangles and its share of rank 0's receive buffer
    GatherRect r[kPlanRects];
    uint32_t nrect, bytes;  // bytes per frame (a multiple of 48)
    uint64_t off;           // per-frame offset of the rank's block (prefix sum of bytes)
    uint32_t rows, packed_rows;
    uint32_t pad[2];
};
// Which rank assembles frame k of a batch of B: rank 0, or (ERAY_GATHER_ROTATE_ROOT) rank k % n,
// which spreads the assembly's frame writes and the inbound xGMI bytes of a stream of frames over
// every GPU instead of piling them on rank 0.  A rank's pack of the batch holds its frames grouped
// by root (one transfer per rank pair moves each group); the frames it assembles itself are packed
// straight into its receive area.
struct Roots {
    uint32_t B, n;  // n == 0: every frame's root is rank 0
    ERAY_HD_PLAIN uint32_t root(uint32_t k) const { return n ? k % n : 0u; }
    ERAY_HD_PLAIN uint32_t index(uint32_t k) const { return n ? k / n : k; }  // among its root's frames
    ERAY_HD_PLAIN uint32_t count(uint32_t r) const {
        return n ? (r < B ? (B - 1u - r) / n + 1u : 0u) : (r ? 0u : B);
    }
    ERAY_HD_PLAIN uint32_t before(uint32_t r) const {  // frames whose root is below r
        return n ? (B / n) * r + (B % n < r ? B % n : r) : 0u;
    }
    // frame k's slot in rank `me`'s send area (frames of other roots, grouped by root)
    ERAY_HD_PLAIN uint32_t send_slot(uint32_t k, uint32_t me) const {
        const uint32_t r = root(k);
        return before(r) - (r > me ? count(me) : 0u) + index(k);
    }
    // roots with frames (0 .. roots() - 1), and root r's group among me's send groups
    ERAY_HD_PLAIN uint32_t roots() const { return n ? (B < n ? B : n) : 1u; }
    ERAY_HD_PLAIN uint32_t group(uint32_t r, uint32_t me) const {
        const uint32_t R = roots();
        return (r < R ? r : R) - (me < r && me < R ? 1u : 0u);
    }
};

// Every transfer of the scene-camera gather ends with its sender's header: the sender's verdict
// on its own arguments and the source (kind, key) of the frames it packed.  A root assembles its
// frames only when every header it uses says ERAY_OK and the plan's source; otherwise it writes
// none of them and raises the plan's fault word, which the context's next eray_gather_frames
// reports — a rank that could not use its arguments still takes part in the transfers, and its
// stale bytes never become a frame.
struct XferHeader {
    int32_t status;
    uint32_t kind, key_lo, key_hi;
};
constexpr size_t kHdr = sizeof(XferHeader);
static_assert(kHdr == 16, "one 16-B word");
ERAY_HD_PLAIN inline bool header_ok(const XferHeader& h, uint32_t kind, uint64_t key) {
    return h.status == 0 && h.kind == kind && h.key_lo == (uint32_t)key && h.key_hi == (uint32_t)(key >> 32);
}
// Rank q's block in a receive area of `mine` frames: its packs (mine x bytes), then its header.
ERAY_HD_PLAIN inline uint64_t recv_block(const RankLayout& L, uint32_t q, uint32_t mine) {
    return (uint64_t)mine * L.off + kHdr * q;
}

// A rank's record in the plan exchange: [status, source kind, key low, key high | nrect, then
// nrect x (l0, l1, c0, c1)] — every rank learns every rank's status and source, so all of them
// accept the plan or all fail together.
constexpr int kXchgHead = 4;
constexpr int kXchgInts = kXchgHead + 1 + 4 * kPlanRects;

// The local rows of rank `rank` (rows, camera row of local row j): interleaved bands (band > 0)
// or the rank's block of PPM file rows (camera rows [H - (rank+1) h, H - rank h)).
struct RankRows {
    uint32_t row0, rows, shift, stride;
};
inline RankRows rank_rows(uint32_t H, uint32_t band, uint32_t N, uint32_t rank) {
    if (!band) {
        const uint32_t h = H / N;
        return RankRows{H - (rank + 1) * h, h, 31u, 0u};
    }
    uint32_t shift = 0;
    while ((1u << shift) < band) ++shift;
    return RankRows{rank * band, band_rows_of(H, band, N, rank), shift, N * band};
}

// This rank's rectangles: the objects' pixel rectangles in its local rows and 16-pixel column
// groups, overlapping ones merged (as camera_setup_kernel merges the detail rectangles), more than
// kPlanRects merged into the last.
inline std::vector<std::array<int32_t, 4>> my_rects(const std::vector<std::array<int32_t, 4>>& rects, const RankRows& rr,
                                                    uint32_t W) {
    std::vector<std::array<int32_t, 4>> out;
    for (const auto& q : rects) {
        int32_t x0 = std::max(q[0], 0), x1 = std::min(q[1], (int32_t)W - 1), l0, l1;
        if (x0 > x1 || q[2] > q[3]) continue;
        eray::gpu::band_local_range(rr.row0, rr.shift, rr.stride, q[2], q[3], &l0, &l1);
        l0 = std::max(l0, 0);
        l1 = std::min(l1, (int32_t)rr.rows - 1);
        if (l0 > l1) continue;
        std::array<int32_t, 4> r{l0, l1, x0 / 16, x1 / 16};
        if (out.size() == (size_t)kPlanRects) {
            auto& z = out.back();
            z = {std::min(z[0], r[0]), std::max(z[1], r[1]), std::min(z[2], r[2]), std::max(z[3], r[3])};
        } else {
            out.push_back(r);
        }
    }
    for (bool merged = true; merged;) {
        merged = false;
        for (size_t a = 0; a < out.size() && !merged; ++a)
            for (size_t b = a + 1; b < out.size() && !merged; ++b) {
                auto &x = out[a], &y = out[b];
                if (x[0] > y[1] || y[0] > x[1] || x[2] > y[3] || y[2] > x[3]) continue;
                x = {std::min(x[0], y[0]), std::max(x[1], y[1]), std::min(x[2], y[2]), std::max(x[3], y[3])};
                out.erase(out.begin() + (std::ptrdiff_t)b);
                merged = true;
            }
    }
    return out;
}

// The rectangle part of an exchange record (nrect, then the rectangles).
inline void write_rects(const std::vector<std::array<int32_t, 4>>& mine, int32_t* rec) {
    rec[0] = (int32_t)mine.size();
    for (size_t i = 0; i < mine.size(); ++i)
        for (int q = 0; q < 4; ++q) rec[1 + 4 * i + q] = mine[i][q];
}

inline RankLayout layout_of(const int32_t* rec, uint32_t rows) {
    RankLayout R{};
    R.nrect = (uint32_t)std::min(std::max(rec[0], 0), kPlanRects);
    R.rows = rows;
    uint32_t off = 0, first = 0;
    for (uint32_t i = 0; i < R.nrect; ++i) {
        GatherRect& g = R.r[i];
        g.l0 = rec[1 + 4 * i];
        g.l1 = rec[2 + 4 * i];
        g.c0 = rec[3 + 4 * i];
        g.c1 = rec[4 + 4 * i];
        g.off = off;
        g.row_bytes = 48u * (uint32_t)(g.c1 - g.c0 + 1);
        g.first = first;
        first += (uint32_t)(g.l1 - g.l0 + 1);
        off += g.row_bytes * (uint32_t)(g.l1 - g.l0 + 1);
    }
    R.bytes = off;
    R.packed_rows = first;
    return R;
}

// The ranks' blocks in rank order (RankLayout::off: prefix sums); returns every rank's bytes per frame.
inline uint64_t place_ranks(std::vector<RankLayout>& ranks) {
    uint64_t total = 0;
    for (RankLayout& R : ranks) {
        R.off = total;
        total += R.bytes;
    }
    return total;
}
// The plan's rank table from every rank's rectangle record (rank q's at recs + q * stride) and its
// rows in the split (H, band, N = ranks->size()); returns the total.
inline uint64_t rank_table(const int32_t* recs, size_t stride, uint32_t H, uint32_t band, std::vector<RankLayout>* ranks) {
    const uint32_t N = (uint32_t)ranks->size();
    for (uint32_t q = 0; q < N; ++q) (*ranks)[q] = layout_of(recs + q * stride, rank_rows(H, band, N, q).rows);
    return place_ranks(*ranks);
}

// The headers a rank writes into its buffer: one after each send group, one after its own packs.
struct HeaderSpots {
    uint64_t off[kMaxCodedRanks + 1];
    uint32_t n;
};

// One rank's part of a batch of B frames: where its packs go in its buffer, how much buffer it
// needs, and its point-to-point transfers (offsets into the buffer).  Its receive area holds, for
// each of the `mine` frames it assembles, every rank's pack and then that rank's header (rank q's
// block at recv_block: mine * off_q + 16 q, frame j at + j * bytes_q, the layout
// gather_assemble_kernel reads); its send area the frames of the other roots, grouped by root,
// each group followed by this rank's header, so each (rank, root) pair is one transfer.
struct Xfer {
    uint32_t peer;
    bool send;
    size_t off, bytes;
};
struct Schedule {
    Roots R;
    uint32_t mine;             // frames this rank assembles
    size_t send_base, own;     // its send area; its own packs' block in the receive area
    size_t need;               // buffer bytes
    std::vector<Xfer> ops;
    HeaderSpots hdr;           // where this rank writes its header (after each send group, after its own packs)
    std::vector<uint64_t> peer_hdr;  // per rank: its header in this rank's receive area (~0: not used)
};
inline Schedule schedule(const std::vector<RankLayout>& ranks, uint64_t total, uint32_t rank, uint32_t B, bool rotate) {
    Schedule S;
    const uint32_t N = (uint32_t)ranks.size();
    S.R = Roots{B, rotate ? N : 0u};
    S.mine = S.R.count(rank);
    const RankLayout& me = ranks[rank];
    S.send_base = (size_t)S.mine * total + kHdr * N;
    S.own = recv_block(me, rank, S.mine);
    S.hdr.n = 0;
    S.peer_hdr.assign(N, ~0ull);
    size_t groups = 0;
    for (uint32_t q = 0; q < N; ++q) {
        if (q != rank && S.R.count(q) && me.bytes) {
            const size_t off = S.send_base + (size_t)(S.R.before(q) - (q > rank ? S.mine : 0u)) * me.bytes +
                               kHdr * S.R.group(q, rank);
            const size_t bytes = (size_t)S.R.count(q) * me.bytes;
            S.ops.push_back({q, true, off, bytes + kHdr});
            S.hdr.off[S.hdr.n++] = off + bytes;
            ++groups;
        }
        if (S.mine && ranks[q].bytes) {
            const size_t off = recv_block(ranks[q], q, S.mine), bytes = (size_t)S.mine * ranks[q].bytes;
            if (q != rank) S.ops.push_back({q, false, off, bytes + kHdr});
            S.peer_hdr[q] = off + bytes;
        }
    }
    if (S.mine) S.hdr.off[S.hdr.n++] = S.own + (size_t)S.mine * me.bytes;
    S.need = S.send_base + (size_t)(B - S.mine) * me.bytes + kHdr * groups;
    return S;
}

// The re-plan decision of eray_gather_frames' scene-camera transport.  Its inputs are the state
// every rank holds alike when the ranks make the same calls (SPMD): the shared arguments, whether
// the cached plan was made for them (by an exchange whose verdict every rank shares), and the
// context's latest scene-camera or camera-path render — never this rank's own buffers or their
// tags, so a rank whose `local` is unusable enters the same collectives as its peers.
inline bool gather_replan(bool cached, uint32_t plan_kind, uint64_t plan_key, uint32_t cur_kind, uint64_t cur_key) {
    return !cached || plan_kind != cur_kind || plan_key != cur_key;
}

// Every rank's verdict on a plan exchange from the same records (so all accept the plan or all
// fail together): the first rank's failure, or a source other than this rank's.  status: this
// rank's own verdict, which it keeps (its message is already set).  Returns the verdict's code;
// *failed is the rank whose failure it is, or -1 (accepted, or ranks whose sources differ).
inline int plan_verdict(const int32_t* all, int nranks, int status, const int32_t* mine, int* failed) {
    *failed = -1;
    for (int q = 0; q < nranks && status == ERAY_OK; ++q)
        if (all[(size_t)q * kXchgInts] != ERAY_OK) return *failed = q, all[(size_t)q * kXchgInts];
    if (status != ERAY_OK) return status;
    for (int q = 0; q < nranks; ++q) {
        const int32_t* o = all + (size_t)q * kXchgInts;
        if (o[1] != mine[1] || o[2] != mine[2] || o[3] != mine[3]) return ERAY_E_INVALID_ARGUMENT;
    }
    return ERAY_OK;
}
}  // namespace
