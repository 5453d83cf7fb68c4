// gather_debug.cpp — the host-only diagnostics of the multi-GPU gather's planning (tests): C
// wrappers of gather_plan.hpp, with no HIP call and no HIP header.  The hooks that launch kernels
// (eray_debug_unband, eray_debug_coded_unband, eray_debug_scene_gather*) are comm.cpp's.
#include <cstdint>
#include <cstring>
#include <vector>

#include "../../include/eray_hip.h"
#include "gather_plan.hpp"

namespace eray::gpu {
int set_error(eray_ctx* ctx, int code, const char* fmt, ...);  // capi.cpp (declared in ctx.hpp, which includes HIP)
}
using eray::gpu::set_error;

namespace {
// The schedule of eray_debug_gather_* for packs of rank_bytes[q] bytes per frame (no plan).
Schedule debug_schedule(const uint32_t* rank_bytes, uint32_t nranks, uint32_t rank, uint32_t nframes, uint32_t rotate,
                        std::vector<RankLayout>* ranks_out = nullptr) {
    std::vector<RankLayout> ranks(nranks, RankLayout{});
    for (uint32_t q = 0; q < nranks; ++q) ranks[q].bytes = rank_bytes[q];
    const uint64_t total = place_ranks(ranks);
    if (ranks_out) *ranks_out = ranks;
    return schedule(ranks, total, rank, nframes, rotate != 0);
}
bool debug_schedule_args(const uint32_t* rank_bytes, uint32_t nranks, uint32_t rank) {
    return rank_bytes && nranks && nranks <= (uint32_t)kMaxCodedRanks && rank < nranks;
}
}  // namespace

extern "C" {

// Diagnostics (tests, host only): rank `rank`'s share of the scene-camera gather of `nranks` ranks
// for objects whose pixel rectangles are `rects` (n x (x0, x1, y0, y1), camera rows) — the layout
// exchange_plan builds from that rank's record.  out (4 + 8 * 8 words): rows, nrect, bytes per
// frame, packed rows, then per rectangle l0, l1, c0, c1 (local rows, 16-pixel column groups), its
// byte offset in the rank's per-frame pack, its row bytes, its first packed row, 0.
int eray_debug_gather_layout(const int32_t* rects, uint32_t n, uint32_t height, uint32_t width, uint32_t band_rows,
                             uint32_t nranks, uint32_t rank, uint32_t* out) {
    if ((n && !rects) || !out || !nranks || rank >= nranks || width % 16 || !row_split_ok(height, band_rows, nranks))
        return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "gather layout: bad arguments");
    std::vector<std::array<int32_t, 4>> rs;
    for (uint32_t i = 0; i < n; ++i) rs.push_back({rects[4 * i], rects[4 * i + 1], rects[4 * i + 2], rects[4 * i + 3]});
    const RankRows rr = rank_rows(height, band_rows, nranks, rank);
    int32_t rec[kXchgInts - kXchgHead] = {};
    write_rects(my_rects(rs, rr, width), rec);
    const RankLayout R = layout_of(rec, rr.rows);
    std::memset(out, 0, sizeof(uint32_t) * (4 + 8 * kPlanRects));
    out[0] = R.rows;
    out[1] = R.nrect;
    out[2] = R.bytes;
    out[3] = R.packed_rows;
    for (uint32_t i = 0; i < R.nrect; ++i) {
        const GatherRect& g = R.r[i];
        const uint32_t v[8] = {(uint32_t)g.l0, (uint32_t)g.l1, (uint32_t)g.c0, (uint32_t)g.c1, g.off, g.row_bytes, g.first, 0u};
        std::memcpy(out + 4 + 8 * i, v, sizeof v);
    }
    return ERAY_OK;
}

// Diagnostics (tests, host only): rank `rank`'s schedule for a batch of `nframes` frames when the
// ranks' packs are rank_bytes[q] bytes per frame (rank order = receive-area order) — what
// eray_gather_frames' pack kernel and point-to-point transfers do.  out (u64): buffer bytes,
// frames this rank assembles, number of transfers T; then per frame k its pack's offset in the
// buffer; then per rank q where q's packs of this rank's frames start (frame j: + j * bytes_q);
// then per transfer: peer, 1 = send / 0 = receive, offset, bytes (each transfer ends with its
// sender's 16-B header); then the number of headers this rank writes and their offsets (T + 1
// slots); then per rank q the offset of q's header in this rank's receive area (~0: unused).
int eray_debug_gather_schedule(const uint32_t* rank_bytes, uint32_t nranks, uint32_t rank, uint32_t nframes,
                               uint32_t rotate, uint64_t* out, uint32_t cap) {
    if (!debug_schedule_args(rank_bytes, nranks, rank) || !out || cap < 5u + nframes + 12u * nranks)
        return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "gather schedule: bad arguments");
    std::vector<RankLayout> ranks;
    const Schedule S = debug_schedule(rank_bytes, nranks, rank, nframes, rotate, &ranks);
    const uint64_t bytes = rank_bytes[rank];
    out[0] = S.need;
    out[1] = S.mine;
    out[2] = S.ops.size();
    for (uint32_t k = 0; k < nframes; ++k) {
        const uint32_t r = S.R.root(k);
        out[3 + k] = r == rank ? S.own + S.R.index(k) * bytes
                               : S.send_base + S.R.send_slot(k, rank) * bytes + (bytes ? kHdr * S.R.group(r, rank) : 0);
    }
    for (uint32_t q = 0; q < nranks; ++q) out[3 + nframes + q] = recv_block(ranks[q], q, S.mine);
    uint64_t* o = out + 3 + nframes + nranks;
    for (const Xfer& x : S.ops) {
        o[0] = x.peer;
        o[1] = x.send ? 1u : 0u;
        o[2] = x.off;
        o[3] = x.bytes;
        o += 4;
    }
    *o++ = S.hdr.n;
    for (uint32_t i = 0; i < S.hdr.n; ++i) *o++ = S.hdr.off[i];
    for (uint32_t q = 0; q < nranks; ++q) *o++ = S.peer_hdr[q];
    return ERAY_OK;
}

// Diagnostics (tests, host only): the headers rank `rank` writes into its transfer buffer `buf`
// (host memory of the schedule's size) — its verdict `status` and its frames' source (kind, key).
int eray_debug_gather_write_headers(const uint32_t* rank_bytes, uint32_t nranks, uint32_t rank, uint32_t nframes,
                                    uint32_t rotate, int32_t status, uint32_t kind, uint64_t key, uint8_t* buf) {
    if (!debug_schedule_args(rank_bytes, nranks, rank) || !buf)
        return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "gather headers: bad arguments");
    const Schedule S = debug_schedule(rank_bytes, nranks, rank, nframes, rotate);
    const XferHeader h{status, kind, (uint32_t)key, (uint32_t)(key >> 32)};
    for (uint32_t i = 0; i < S.hdr.n; ++i) std::memcpy(buf + S.hdr.off[i], &h, kHdr);
    return ERAY_OK;
}

// Diagnostics (tests, host only): a root's verdict on its received batch (gather_assemble_kernel's
// check, on a host copy of its buffer): ERAY_OK when every header it uses says ERAY_OK and the
// plan's source (kind, key), else ERAY_E_INVALID_ARGUMENT (the root writes none of the frames).
int eray_debug_gather_check(const uint32_t* rank_bytes, uint32_t nranks, uint32_t rank, uint32_t nframes,
                            uint32_t rotate, uint32_t kind, uint64_t key, const uint8_t* buf) {
    if (!debug_schedule_args(rank_bytes, nranks, rank) || !buf)
        return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "gather check: bad arguments");
    const Schedule S = debug_schedule(rank_bytes, nranks, rank, nframes, rotate);
    for (uint32_t q = 0; q < nranks; ++q) {
        if (S.peer_hdr[q] == ~0ull) continue;
        XferHeader h;
        std::memcpy(&h, buf + S.peer_hdr[q], kHdr);
        if (!header_ok(h, kind, key))
            return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "gather: a rank could not use its frames");
    }
    return ERAY_OK;
}

// Diagnostics (tests, host only): eray_gather_frames' re-plan decision (gather_replan) — from the
// cached plan's state and the context's latest render, the only inputs it has.
int eray_debug_gather_replan(uint32_t cached, uint32_t plan_kind, uint64_t plan_key, uint32_t cur_kind, uint64_t cur_key) {
    return gather_replan(cached != 0, plan_kind, plan_key, cur_kind, cur_key) ? 1 : 0;
}

// Diagnostics (tests, host only): a new plan's verdict on this rank (exchange_plan's): records
// holds every rank's (status, kind, key low, key high), `rank`'s own among them.
int eray_debug_plan_verdict(const int32_t* records, uint32_t nranks, uint32_t rank) {
    if (!records || !nranks || nranks > (uint32_t)kMaxCodedRanks || rank >= nranks)
        return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "plan verdict: bad arguments");
    std::vector<int32_t> all((size_t)kXchgInts * nranks, 0);
    for (uint32_t q = 0; q < nranks; ++q) std::memcpy(all.data() + (size_t)q * kXchgInts, records + 4 * q, 4 * sizeof(int32_t));
    const int32_t* mine = all.data() + (size_t)rank * kXchgInts;
    if (mine[0] != ERAY_OK) set_error(nullptr, mine[0], "plan verdict: this rank's own failure");
    int failed;
    const int code = plan_verdict(all.data(), (int)nranks, mine[0], mine, &failed);
    if (code == ERAY_OK || mine[0] != ERAY_OK) return code;  // (worded as exchange_plan words them)
    return failed >= 0 ? set_error(nullptr, code, "scene-camera gather: rank %d could not use its frames (status %d)", failed, code)
                       : set_error(nullptr, code, "scene-camera gather: the ranks' frames come from different cameras or paths");
}

}  // extern "C"
