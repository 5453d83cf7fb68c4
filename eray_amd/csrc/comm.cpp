// comm.cpp — the multi-GPU frame gather of the C-ABI, over RCCL.
//
// Every pixel is independent (engine.rs:52-78), so a frame shards by row tiles across the GPUs of
// a node, one process (one eray context) per GPU: rank r renders the r-th block of PPM file rows
// (camera rows [H - (r+1) h, H - r h); eray_render's fused out_ppm writes them in file order), and
// one gather concatenates the blocks on rank 0 in rank order — the PPM body Image::save_as_ppm
// writes (image.rs:48-74).  u8 rows, 4x fewer bytes than f32.  With interleaved bands (equal work
// per rank) the rows travel coded (uniform 64-pixel segments as one word) by point-to-point
// transfers into rank 0, which writes each file row from them.
//
// Here: the RCCL transport, the plan exchange and the entry points.  The planning is gather_plan.hpp
// (HIP-free; its host-only diagnostics gather_debug.cpp), the kernels gather_coded.hpp and gather_scene.hpp.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <cstring>
#include <new>
#include <string>
#include <vector>

#include "ctx.hpp"
#include "gather_plan.hpp"
#include "gather_coded.hpp"
#include "gather_scene.hpp"

static_assert(ERAY_COMM_ID_BYTES == NCCL_UNIQUE_ID_BYTES, "unique id size");

// What an assembly takes of its plan: the frame's split and source, and on the device every rank's layout and the fault word.
struct PlanFrames {
    uint32_t H = 0, W = 0, band = 0, nranks = 0, kind = 0;
    uint64_t key = 0;
    RankLayout* d_ranks = nullptr;  // (the plan's: in the context's scratch)
    int32_t* d_fault = nullptr;
};
// eray_gather_frames' plan, which the context owns (eray_ctx::gather_plan).
struct eray::gpu::GatherPlan : PlanFrames {
    void* comm = nullptr;
    PinnedBuf<int32_t> fault;      // mapped host word (d_fault on the device): a root met a failed or foreign header
    Event asm_ev;                  // after the last assembly enqueued outside a graph capture
    bool asm_pending = false;      // ... whose fault word has not been read yet
    uint32_t rank = 0;
    bool valid = false;
    std::vector<RankLayout> ranks;
    uint64_t total = 0;            // every rank's bytes per frame
    DeviceBuf<uint8_t> buf;        // [receive area: its frames x every rank's packs | send area: its packs]
    // batch sizes whose transfer buffers every rank has confirmed since the plan was made (a new
    // size's first call agrees on that before any transfer)
    std::vector<uint32_t> batches;
};
void eray::gpu::GatherPlanDelete::operator()(GatherPlan* P) const { delete P; }

namespace {
// The context's collective scratch (eray_ctx::d_coll, allocated with the context):
// status and count words at kScrWords, the plan exchange's records at kScrXchg, the plan's rank
// table (the assembly kernels' RankLayout array) at kScrRanks.
constexpr size_t kScrWords = 0, kScrXchg = 1024, kScrRanks = kScrXchg + 12288;
static_assert(4 * (kMaxCodedRanks + 2) <= kScrXchg, "status words");
static_assert(kScrXchg + sizeof(int32_t) * kXchgInts * (kMaxCodedRanks + 1) <= kScrRanks, "plan records");
static_assert(kScrRanks + sizeof(RankLayout) * kMaxCodedRanks <= eray::gpu::kCollScratchBytes, "rank table");

int nccl_error(eray_ctx* ctx, const char* what, ncclResult_t r) {
    return set_error(ctx, ERAY_E_HIP, "%s: %s", what, ncclGetErrorString(r));
}

// Every rank's status word, all-gathered through the collective scratch (one stream
// synchronisation): this rank's own failure, else the first failing rank's, else ERAY_OK — the
// same outcome on every rank, so they all go on to the next collective or all return.
int agree(eray_ctx* ctx, ncclComm_t c, int nranks, int status, const char* what) {
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    int32_t* words = reinterpret_cast<int32_t*>(ctx->d_coll + kScrWords);
    const int32_t mine = status;
    std::vector<int32_t> all((size_t)nranks);
    hipError_t he;
    if ((he = hipMemcpyAsync(words, &mine, 4, hipMemcpyHostToDevice, s)) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    const ncclResult_t r = ncclAllGather(words, words + 1, 1, ncclInt32, c, s);
    if (r != ncclSuccess) return nccl_error(ctx, what, r);
    if ((he = hipMemcpyAsync(all.data(), words + 1, 4u * (size_t)nranks, hipMemcpyDeviceToHost, s)) != hipSuccess ||
        (he = hipStreamSynchronize(s)) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    if (status != ERAY_OK) return status;
    for (int q = 0; q < nranks; ++q)
        if (all[(size_t)q] != ERAY_OK)
            return set_error(ctx, all[(size_t)q], "%s: rank %d could not take part (status %d)", what, q, all[(size_t)q]);
    return ERAY_OK;
}
}  // namespace

extern "C" {

int eray_comm_unique_id(uint8_t* id) {
    if (!id) return set_error(nullptr, ERAY_E_INVALID_ARGUMENT, "id is null");
    ncclUniqueId u;
    const ncclResult_t r = ncclGetUniqueId(&u);
    if (r != ncclSuccess) return nccl_error(nullptr, "ncclGetUniqueId", r);
    std::memcpy(id, u.internal, NCCL_UNIQUE_ID_BYTES);
    return ERAY_OK;
}

int eray_comm_init(eray_ctx* ctx, int nranks, int rank, const uint8_t* id, void** nccl_comm) {
    if (!ctx || !id || !nccl_comm || nranks < 1 || rank < 0 || rank >= nranks)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "comm_init: bad arguments");
    *nccl_comm = nullptr;
    if (int st = eray_synchronize(ctx)) return st;  // selects the context's device
    ncclUniqueId u;
    std::memcpy(u.internal, id, NCCL_UNIQUE_ID_BYTES);
    ncclComm_t c = nullptr;
    const ncclResult_t r = ncclCommInitRank(&c, nranks, u, rank);
    if (r != ncclSuccess) return nccl_error(ctx, "ncclCommInitRank", r);
    *nccl_comm = c;
    return ERAY_OK;
}

int eray_comm_destroy(void* nccl_comm) {
    if (!nccl_comm) return ERAY_OK;
    const ncclResult_t r = ncclCommDestroy((ncclComm_t)nccl_comm);
    return r == ncclSuccess ? ERAY_OK : nccl_error(nullptr, "ncclCommDestroy", r);
}

uint32_t eray_band_rows(uint32_t height, uint32_t band_rows, uint32_t nranks, uint32_t rank) {
    return band_rows_of(height, band_rows, nranks, rank);
}

int eray_gather_rows(eray_ctx* ctx, void* nccl_comm, const uint8_t* local, uint8_t* frame, uint32_t height,
                     uint32_t width, uint32_t band_rows) {
    if (!ctx || !nccl_comm) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: null context or comm");
    ncclComm_t c = (ncclComm_t)nccl_comm;
    int nranks = 0, rank = 0;
    ncclResult_t r = ncclCommCount(c, &nranks);
    if (r == ncclSuccess) r = ncclCommUserRank(c, &rank);
    if (r != ncclSuccess) return nccl_error(ctx, "gather: communicator", r);
    if (!row_split_ok(height, band_rows, (uint32_t)nranks))
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "%s",
                         band_rows ? "gather: band_rows must be a power of two >= 4"
                                   : "gather: height does not split into equal blocks");
    if (nranks > kMaxCodedRanks)  // (shared arguments: every rank returns here)
        return set_error(ctx, ERAY_E_UNSUPPORTED, "gather: more than 64 ranks");
    const size_t row_bytes = (size_t)width * 3u;
    const uint32_t rows = band_rows ? band_rows_of(height, band_rows, (uint32_t)nranks, 0) : height / (uint32_t)nranks;
    const size_t bytes = (size_t)rows * row_bytes;
    if (!bytes) return ERAY_OK;  // (shared arguments: every rank returns here)
    // this rank's verdict on its own buffers: a failing rank still takes part in the status
    // exchange below, and every rank returns an error before any rows move
    int status = ERAY_OK;
    if (!local) status = set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: local rows are null");
    else if (rank == 0 && !frame) status = set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: frame is null");
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    hipError_t he;
    if (!band_rows) {
        // every rank's status (one word each, all-gathered, one stream synchronisation), then the
        // rows: rank order = PPM file order, rank r's block lands at frame + r * bytes on rank 0 (in
        // place when rank 0's local rows already sit at frame + 0)
        if (int st = agree(ctx, c, nranks, status, "gather")) return st;
        r = ncclGather(local, rank == 0 ? frame : nullptr, bytes, ncclUint8, 0, c, s);
        if (r != ncclSuccess) return nccl_error(ctx, "ncclGather", r);
        return ERAY_OK;
    }
    {
        // bands, coded (see seg_classify_kernel): every rank encodes its rows; the packed counts
        // reach every host (one all-gather of a word each, then a stream synchronisation: the
        // point-to-point sizes must be known to post them); rank 0 receives every rank's code
        // words and packed segments and decodes the frame
        const uint32_t S = (width + kSegPx - 1) / kSegPx, G = rows * S;
        const uint32_t mine = band_rows_of(height, band_rows, (uint32_t)nranks, (uint32_t)rank);
        CodedBufs b;
        b.count = reinterpret_cast<uint32_t*>(ctx->d_coll + kScrWords);
        b.counts = b.count + 1;
        if (status == ERAY_OK && !coded_bufs(ctx, G, rank == 0 ? (uint32_t)nranks : 1u, &b))
            status = set_error(ctx, ERAY_E_OUT_OF_MEMORY, "gather: staging buffer");
        // the packed-segment counts carry the ranks' verdicts: a rank that cannot use its buffers
        // (or allocate its staging) sends kCountFailed, and every rank returns an error before the
        // transfers
        if (status == ERAY_OK) {
            he = encode_rows(local, mine, rows, width, S, b.code, b.packed, b, s);
            if (he != hipSuccess) status = set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
        }
        if (status != ERAY_OK && (he = hipMemsetAsync(b.count, 0xff, 4, s)) != hipSuccess)
            return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
        r = ncclAllGather(b.count, b.counts, 1, ncclUint32, c, s);
        if (r != ncclSuccess) return nccl_error(ctx, "ncclAllGather", r);
        std::vector<uint32_t> counts((size_t)nranks);
        if ((he = hipMemcpyAsync(counts.data(), b.counts, 4u * (size_t)nranks, hipMemcpyDeviceToHost, s)) != hipSuccess ||
            (he = hipStreamSynchronize(s)) != hipSuccess)
            return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
        if (status != ERAY_OK) return status;
        for (int q = 0; q < nranks; ++q)
            if (counts[(size_t)q] == kCountFailed)
                return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: rank %d could not use its buffers", q);
        RankOffsets off{};
        for (int k = 1; k < nranks; ++k) off.v[k] = off.v[k - 1] + counts[(size_t)k - 1];
        if (nranks > 1) {
            if ((r = ncclGroupStart()) != ncclSuccess) return nccl_error(ctx, "ncclGroupStart", r);
            if (rank == 0) {
                for (int k = 1; k < nranks && r == ncclSuccess; ++k) {
                    r = ncclRecv(b.code + (size_t)k * G, G, ncclUint32, k, c, s);
                    if (r == ncclSuccess && counts[(size_t)k])
                        r = ncclRecv(b.packed + (size_t)off.v[k] * kSegBytes, (size_t)counts[(size_t)k] * kSegBytes,
                                     ncclUint8, k, c, s);
                }
            } else {
                r = ncclSend(b.code, G, ncclUint32, 0, c, s);
                if (r == ncclSuccess && counts[(size_t)rank])
                    r = ncclSend(b.packed, (size_t)counts[(size_t)rank] * kSegBytes, ncclUint8, 0, c, s);
            }
            const ncclResult_t r2 = ncclGroupEnd();
            if (r != ncclSuccess) return nccl_error(ctx, "ncclSend/ncclRecv", r);
            if (r2 != ncclSuccess) return nccl_error(ctx, "ncclGroupEnd", r2);
        }
        if (rank == 0) {
            seg_decode_kernel<<<height, 256, 0, s>>>(b.code, b.packed, off, frame, height, width, S, band_rows,
                                                     (uint32_t)nranks, rows);
            if ((he = hipGetLastError()) != hipSuccess) return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
        }
        return ERAY_OK;
    }
}

}  // extern "C"

namespace {
// The source of the n frames local + k * stride (k < n) as this context last rendered them
// (tag_frames); every frame must have the same one.
int frames_source(eray_ctx* ctx, const uint8_t* local, uint64_t stride, uint32_t n, FrameSource* out) {
    if (!ctx || !out) return ERAY_E_INVALID_ARGUMENT;
    *out = FrameSource{};
    for (uint32_t k = 0; k < n; ++k) {
        const uintptr_t a = reinterpret_cast<uintptr_t>(local) + (uintptr_t)(k * stride);
        const eray_ctx::SlotTag* t = nullptr;
        for (auto it = ctx->slot_tags.rbegin(); it != ctx->slot_tags.rend(); ++it)
            if (it->ppm == a) {
                t = &*it;
                break;
            }
        if (!t)
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: frame %u at %p was not rendered by this context", k,
                             (const void*)a);
        if (k == 0) {
            *out = t->src;
        } else if (t->src.kind != out->kind || t->src.key != out->key) {
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: frames 0 and %u come from different renders", k);
        }
    }
    if (out->kind == kSrcOther)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                         "gather: the frames were rendered with anti-aliasing, bounces or brute force (no pixel rectangles)");
    return ERAY_OK;
}

// The pixel rectangles of `src` (waits for their host copy): the last scene-camera setup when it
// is src's (same camera, scene and rows), or the union of camera path src.key's cameras while it
// is among the last kUnionRing paths.
int source_layout(eray_ctx* ctx, const FrameSource& src, SceneLayout* out) {
    if (!ctx || !out) return ERAY_E_INVALID_ARGUMENT;
    auto same_rows = [](const FrameSource& a, const FrameSource& b) {
        return a.W == b.W && a.H == b.H && a.row0 == b.row0 && a.rows == b.rows && a.band_shift == b.band_shift &&
               a.band_stride == b.band_stride;
    };
    out->src = src;
    out->rects.clear();
    const size_t nobj = ctx->objects.size();
    if (src.kind == kSrcScene) {
        const FrameSource& s = ctx->setup_src;
        if (s.kind != kSrcScene || s.key != src.key || !same_rows(s, src))
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                             "gather: the scene camera's last setup is not the one these frames were rendered with");
        if (ctx->state_pending) {
            HIP_TRY(ctx, hipEventSynchronize(ctx->state_ev));
            state_arrived(ctx);
        }
        for (size_t i = 0; i < nobj; ++i) {
            const int32_t* r = ctx->h_objs_state[i].g.rect;
            out->rects.push_back({r[0], r[1], r[2], r[3]});
        }
        return ERAY_OK;
    }
    if (src.kind == kSrcPath) {
        const uint32_t e = (uint32_t)(src.key % kUnionRing);
        if (ctx->union_seq[e] != src.key || !same_rows(ctx->union_src[e], src))
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                             "gather: these camera-path frames are older than the last %u paths", kUnionRing);
        // (the union covers the objects of the scene the path was rendered from; a scene change
        // since makes the path's frames ungatherable, as their objects no longer exist)
        if (ctx->union_nobj[e] != nobj || ctx->union_gen[e] != ctx->scene_gen || nobj > ctx->union_cap())
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                             "gather: the scene changed after these camera-path frames were rendered");
        HIP_TRY(ctx, hipEventSynchronize(ctx->union_ev[e]));
        const int32_t* u = ctx->h_union + (size_t)e * 4 * ctx->union_cap();
        for (size_t i = 0; i < nobj; ++i)
            out->rects.push_back({u[2 * i], u[2 * nobj + 2 * i], u[2 * i + 1], u[2 * nobj + 2 * i + 1]});
        return ERAY_OK;
    }
    return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: frames of an unknown source");
}
// The source of the scene camera's last setup (diagnostics: eray_debug_scene_gather).
int scene_setup_source(eray_ctx* ctx, FrameSource* out) {
    if (!ctx || !out) return ERAY_E_INVALID_ARGUMENT;
    if (ctx->setup_src.kind != kSrcScene)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "no setup of the scene camera: render it first");
    *out = ctx->setup_src;
    return ERAY_OK;
}

// Exchanges the ranks' records for a new plan (a collective: every rank calls it at the same
// point, one stream synchronisation).  `status` is this rank's verdict (ERAY_OK, or the error it
// met looking up its frames' source and rectangles); on success every rank holds every rank's
// layout, otherwise every rank returns an error.
int exchange_plan(eray_ctx* ctx, ncclComm_t c, int nranks, int rank, uint32_t H, uint32_t W, uint32_t band,
                  const eray::gpu::FrameSource& src, int status, const std::vector<std::array<int32_t, 4>>& rects,
                  GatherPlan* P) {
    P->valid = false;
    P->batches.clear();
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    hipError_t he;
    // (the records travel through the context's collective scratch: nothing to allocate before
    // the all-gather, so this rank always takes part)
    int32_t* xchg = reinterpret_cast<int32_t*>(ctx->d_coll + kScrXchg);
    if (status == ERAY_OK && !P->fault) {  // the roots' fault word (a failure here is this rank's verdict)
        if (P->fault.alloc(1, hipHostMallocMapped) != hipSuccess) {
            (void)P->fault.release();
            status = set_error(ctx, ERAY_E_OUT_OF_MEMORY, "gather plan: fault word");
        } else {
            *P->fault = 0;
            P->d_fault = P->fault.dev;
        }
    }
    if (status == ERAY_OK && !P->asm_ev && P->asm_ev.create(hipEventDisableTiming) != hipSuccess)
        status = set_error(ctx, ERAY_E_HIP, "gather plan: assembly event");
    int32_t rec[kXchgInts] = {};
    rec[0] = status;
    rec[1] = (int32_t)src.kind;
    rec[2] = (int32_t)(uint32_t)src.key;
    rec[3] = (int32_t)(uint32_t)(src.key >> 32);
    if (status == ERAY_OK) write_rects(my_rects(rects, rank_rows(H, band, (uint32_t)nranks, (uint32_t)rank), W), rec + kXchgHead);
    std::vector<int32_t> all((size_t)kXchgInts * (size_t)nranks);
    if ((he = hipMemcpyAsync(xchg, rec, sizeof rec, hipMemcpyHostToDevice, s)) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    const ncclResult_t r = ncclAllGather(xchg, xchg + kXchgInts, kXchgInts, ncclInt32, c, s);
    if (r != ncclSuccess) return nccl_error(ctx, "ncclAllGather (gather plan)", r);
    if ((he = hipMemcpyAsync(all.data(), xchg + kXchgInts, sizeof(int32_t) * all.size(), hipMemcpyDeviceToHost, s)) !=
            hipSuccess ||
        (he = hipStreamSynchronize(s)) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    int failed;
    if (const int st = plan_verdict(all.data(), nranks, status, rec, &failed)) {
        if (status != ERAY_OK) return st;  // (this rank's own failure: its message is set)
        return failed >= 0 ? set_error(ctx, st, "scene-camera gather: rank %d could not use its frames (status %d)", failed, st)
                           : set_error(ctx, st, "scene-camera gather: the ranks' frames come from different cameras or paths");
    }
    P->ranks.assign((size_t)nranks, RankLayout{});
    P->total = rank_table(all.data() + kXchgHead, kXchgInts, H, band, &P->ranks);
    // the rank table lives in the scratch: the previous plan's assemblies (on any stream) read it
    // until they finish, so the device drains first (a re-plan is once per camera)
    P->d_ranks = reinterpret_cast<RankLayout*>(ctx->d_coll + kScrRanks);
    if ((he = hipDeviceSynchronize()) != hipSuccess ||
        (he = hipMemcpy(P->d_ranks, P->ranks.data(), sizeof(RankLayout) * (size_t)nranks, hipMemcpyHostToDevice)) !=
            hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    P->comm = (void*)c;
    P->kind = src.kind;
    P->key = src.key;
    P->H = H;
    P->W = W;
    P->band = band;
    P->nranks = (uint32_t)nranks;
    P->rank = (uint32_t)rank;
    P->valid = true;
    return ERAY_OK;
}

// The plan's transfer buffer grown to `bytes` (the first call of a batch size): the new buffer is
// allocated before the old one is released, so a failure leaves the plan as it was.
int grow(eray_ctx* ctx, GatherPlan* P, size_t bytes) {
    if (bytes <= P->buf.cap && P->buf) return ERAY_OK;
    DeviceBuf<uint8_t> nb;
    hipError_t he = hipDeviceSynchronize();  // (the old buffer's transfers are done, on whichever stream)
    if (he == hipSuccess) he = nb.alloc(std::max<size_t>(bytes, 256));
    if (he != hipSuccess) return set_error(ctx, ERAY_E_OUT_OF_MEMORY, "%s", hipGetErrorString(he));
    P->buf = std::move(nb);  // (releases the old one)
    return ERAY_OK;
}

// The three launches of a rank's part of a batch, on its buffer `buf` with its schedule S: its header at each of
// its spots; its B frames' packs (frame k at local + k * local_stride); a root's S.mine frames from its receive area.
hipError_t enqueue_headers(uint8_t* buf, const Schedule& S, const XferHeader& h, hipStream_t s) {
    gather_header_kernel<<<1, 64, 0, s>>>(buf, S.hdr, h);
    return hipGetLastError();
}
hipError_t enqueue_pack(const uint8_t* local, uint64_t local_stride, uint8_t* buf, const Schedule& S, const RankLayout& me,
                        uint32_t W, uint32_t B, uint32_t rank, hipStream_t s) {
    gather_pack_kernel<<<dim3(me.packed_rows, B), 256, 0, s>>>(local, local_stride, buf + S.send_base, buf + S.own, me, W,
                                                               S.R, rank);
    return hipGetLastError();
}
hipError_t enqueue_assemble(const uint8_t* buf, const Schedule& S, const PlanFrames& F, uint8_t* frames,
                            uint64_t frame_stride, hipStream_t s) {
    gather_assemble_kernel<<<dim3(F.H, S.mine), 256, 0, s>>>(buf, F.d_ranks, S.mine, frames, frame_stride, F.H, F.W, F.band,
                                                             F.nranks, F.kind, F.key, F.d_fault);
    return hipGetLastError();
}

// Pack (every rank), transfer, assemble (each frame's root) `B` frames with plan P.  status != OK
// (this rank's own arguments are unusable): its headers carry the status and it runs only the
// plan's transfers, so the other ranks' matching sends and receives complete and their roots
// refuse the batch — no kernel touches the caller's buffers.
int scene_gather(eray_ctx* ctx, ncclComm_t c, GatherPlan& P, const Schedule& S, const uint8_t* local,
                 uint64_t local_stride, uint8_t* frames, uint64_t frame_stride, uint32_t B, int status = ERAY_OK) {
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    const RankLayout& me = P.ranks[P.rank];
    const bool fail_safe = status != ERAY_OK;
    hipError_t he;
    const XferHeader h{status, P.kind, (uint32_t)P.key, (uint32_t)(P.key >> 32)};
    if (S.hdr.n && (he = enqueue_headers(P.buf, S, h, s)) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    if (me.bytes && !fail_safe && (he = enqueue_pack(local, local_stride, P.buf, S, me, P.W, B, P.rank, s)) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    if (!S.ops.empty()) {
        ncclResult_t r = ncclGroupStart();
        if (r != ncclSuccess) return nccl_error(ctx, "ncclGroupStart", r);
        for (size_t i = 0; i < S.ops.size() && r == ncclSuccess; ++i) {
            const Xfer& x = S.ops[i];
            r = x.send ? ncclSend(P.buf + x.off, x.bytes, ncclUint8, (int)x.peer, c, s)
                       : ncclRecv(P.buf + x.off, x.bytes, ncclUint8, (int)x.peer, c, s);
        }
        const ncclResult_t r2 = ncclGroupEnd();
        if (r != ncclSuccess) return nccl_error(ctx, "ncclSend/ncclRecv", r);
        if (r2 != ncclSuccess) return nccl_error(ctx, "ncclGroupEnd", r2);
    }
    if (S.mine && !fail_safe) {
        if ((he = enqueue_assemble(P.buf, S, P, frames, frame_stride, s)) != hipSuccess)
            return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
        // the next call reads the fault word once this assembly is done (not under a graph capture,
        // whose replays' refusals the first call after them reads)
        hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
        if (hipStreamIsCapturing(s, &cap) == hipSuccess && cap == hipStreamCaptureStatusNone &&
            hipEventRecord(P.asm_ev, s) == hipSuccess)
            P.asm_pending = true;
    }
    return ERAY_OK;
}

}  // namespace

extern "C" {

int eray_gather_frames(eray_ctx* ctx, void* nccl_comm, const uint8_t* local, uint64_t local_stride, uint8_t* frames,
                       uint64_t frame_stride, uint32_t nframes, uint32_t height, uint32_t width, uint32_t band_rows,
                       uint32_t flags) {
    if (!ctx || !nccl_comm) return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: null context or comm");
    if (flags & ~(uint32_t)(ERAY_GATHER_SCENE_CAMERA | ERAY_GATHER_ROTATE_ROOT))
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: unknown flags");
    const bool rotate = (flags & ERAY_GATHER_ROTATE_ROOT) != 0;
    if (rotate && !(flags & ERAY_GATHER_SCENE_CAMERA))
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "gather: rotating roots need ERAY_GATHER_SCENE_CAMERA");
    if (int st = use_device(ctx)) return st;
    ncclComm_t c = (ncclComm_t)nccl_comm;
    int nranks = 0, rank = 0;
    ncclResult_t r = ncclCommCount(c, &nranks);
    if (r == ncclSuccess) r = ncclCommUserRank(c, &rank);
    if (r != ncclSuccess) return nccl_error(ctx, "gather: communicator", r);
    if (!nframes || !height || !width) return ERAY_OK;
    if (flags & ERAY_GATHER_SCENE_CAMERA) {
        // The transport is chosen from arguments every rank shares (flags, the frame size, the
        // split), never from this rank's own pointers or state, so all ranks take the same path.
        if (width % 16 || !row_split_ok(height, band_rows, (uint32_t)nranks))
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                             "scene-camera gather: width must be a multiple of 16 and the rows a valid split");
        if (nranks > kMaxCodedRanks)
            return set_error(ctx, ERAY_E_UNSUPPORTED, "scene-camera gather: more than 64 ranks");
        // This rank's verdict on its own arguments and frames.  Whatever it is, the rank takes
        // part in the same collectives as the others (chosen from the shared arguments and the
        // shared render history, gather_replan), then returns its error.
        const bool assembles = rotate ? (uint32_t)rank < nframes : rank == 0;
        const bool aligned = ((reinterpret_cast<uintptr_t>(local) | local_stride) & 15) == 0 &&
                             (!assembles || ((reinterpret_cast<uintptr_t>(frames) | frame_stride) & 15) == 0);
        int status = ERAY_OK;
        if (!local || (assembles && !frames) || !aligned)
            status = set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                               "scene-camera gather: null or unaligned (16 B) buffers or strides");
        // what the plan is for: the context's latest render of the scene camera or of a camera path
        const eray::gpu::FrameSource cur = ctx->gather_src;
        if (status == ERAY_OK && cur.kind != eray::gpu::kSrcScene && cur.kind != eray::gpu::kSrcPath)
            status = set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                               "scene-camera gather: this context has rendered neither its scene camera nor a "
                               "camera path");
        // this rank's frames must be frames of that render, over this rank's share
        eray::gpu::FrameSource src;
        if (status == ERAY_OK) status = frames_source(ctx, local, local_stride, nframes, &src);
        if (status == ERAY_OK && (src.kind != cur.kind || src.key != cur.key))
            status = set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                               "scene-camera gather: the frames are not of this context's latest scene-camera "
                               "or camera-path render");
        const RankRows rr = rank_rows(height, band_rows, (uint32_t)nranks, (uint32_t)rank);
        if (status == ERAY_OK && (src.W != width || src.H != height || src.row0 != rr.row0 || src.rows != rr.rows ||
                                  src.band_shift != rr.shift || (band_rows && src.band_stride != rr.stride)))
            status = set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                               "scene-camera gather: the frames cover other rows or another frame size than "
                               "this rank's share");
        if (!ctx->gather_plan) ctx->gather_plan.reset(new (std::nothrow) GatherPlan());
        GatherPlan* const P = ctx->gather_plan.get();
        if (!P) {  // no plan object: this rank still takes part in the (first) exchange, with its error
            GatherPlan tmp;
            set_error(ctx, ERAY_E_OUT_OF_MEMORY, "gather plan");
            const int st = exchange_plan(ctx, c, nranks, rank, height, width, band_rows, cur, ERAY_E_OUT_OF_MEMORY, {}, &tmp);
            return st ? st : ERAY_E_OUT_OF_MEMORY;
        }
        hipStream_t s = (hipStream_t)eray_get_stream(ctx);
        // a failed or foreign batch met by one of this context's earlier assemblies: read once that
        // assembly is done (reported after this call's own collectives)
        bool faulted = false;
        if (P->fault) {
            hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
            const bool capturing = hipStreamIsCapturing(s, &cap) != hipSuccess || cap != hipStreamCaptureStatusNone;
            if (P->asm_pending && !capturing) {
                const hipError_t he = hipEventSynchronize(P->asm_ev);
                if (he != hipSuccess && status == ERAY_OK)
                    status = set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
                P->asm_pending = false;
            }
            if (!P->asm_pending) faulted = __atomic_exchange_n((int32_t*)P->fault, 0, __ATOMIC_RELAXED) != 0;
        }
        const bool cached = P->valid && P->comm == (void*)c && P->H == height && P->W == width &&
                            P->band == band_rows && P->nranks == (uint32_t)nranks && P->rank == (uint32_t)rank;
        if (gather_replan(cached, P->kind, P->key, cur.kind, cur.key)) {  // a new plan: every rank exchanges
            eray::gpu::SceneLayout L;
            if (status == ERAY_OK) status = source_layout(ctx, src, &L);
            if (int st = exchange_plan(ctx, c, nranks, rank, height, width, band_rows, cur, status, L.rects, P)) return st;
        }
        const Schedule S = schedule(P->ranks, P->total, (uint32_t)rank, nframes, rotate);
        if (std::find(P->batches.begin(), P->batches.end(), nframes) == P->batches.end()) {
            // a batch size's first call: every rank's transfer buffer for it, agreed on before any
            // transfer (a rank that cannot allocate makes every rank return instead of leaving its
            // peers' sends and receives waiting)
            std::string keep = status != ERAY_OK ? eray_last_error(ctx) : std::string();
            const int gst = grow(ctx, P, S.need);
            if (status != ERAY_OK) set_error(ctx, status, "%s", keep.c_str());  // (the first failure's message)
            if (int st = agree(ctx, c, nranks, gst, "scene-camera gather: transfer buffer")) return status ? status : st;
            P->batches.push_back(nframes);
        }
        std::string msg = status != ERAY_OK ? eray_last_error(ctx) : std::string();
        const int st = scene_gather(ctx, c, *P, S, local, local_stride, frames, frame_stride, nframes, status);
        if (status != ERAY_OK) return set_error(ctx, status, "%s", msg.c_str());
        if (st) return st;
        if (S.mine) untag_range(ctx, (uintptr_t)frames, (size_t)(S.mine - 1) * frame_stride + (size_t)height * width * 3u);
        if (faulted)
            return set_error(ctx, ERAY_E_INVALID_ARGUMENT,
                             "scene-camera gather: an earlier batch assembled here had a rank that could not "
                             "use its frames; its frames were left unwritten");
        return ERAY_OK;
    }
    for (uint32_t k = 0; k < nframes; ++k)  // one frame at a time through eray_gather_rows
        if (int st = eray_gather_rows(ctx, nccl_comm, local ? local + k * local_stride : nullptr,
                                      frames ? frames + k * frame_stride : nullptr, height, width, band_rows))
            return st;
    return ERAY_OK;
}

// Diagnostics (tests): the scene-camera gather of a batch of `nframes` frames by N ranks,
// simulated on one GPU with the real pack and assembly kernels and each rank's schedule (its
// point-to-point transfers as device copies between the ranks' buffers).  The context has
// rendered the scene camera's whole frame (its setup's rectangles stand for every rank's);
// staging holds frame k of rank q's padded local PPM block at (k * N + q) * rows_max rows
// (rows_max = rank 0's rows; band_rows > 0: bands, 0: blocks).  Root r's assembled frames land at
// frames + (frames of roots below r + j) * H W 3 — in batch order unless `rotate`.
int eray_debug_scene_gather_batch(eray_ctx* ctx, const uint8_t* staging, uint8_t* frames, uint32_t nframes,
                                  uint32_t height, uint32_t width, uint32_t band_rows, uint32_t nranks, uint32_t rotate) {
    if (!ctx || !staging || !frames || !nframes || !nranks || nranks > (uint32_t)kMaxCodedRanks || width % 16 ||
        !row_split_ok(height, band_rows, nranks))
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "scene gather: bad arguments");
    eray::gpu::FrameSource src;
    eray::gpu::SceneLayout L;
    if (int st = scene_setup_source(ctx, &src)) return st;
    if (int st = source_layout(ctx, src, &L)) return st;
    if (src.W != width || src.H != height || src.row0 != 0 || src.rows != height || src.band_shift != 31u)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "scene gather: render the whole scene-camera frame first");
    const uint32_t rows_max = rank_rows(height, band_rows, nranks, 0).rows;
    constexpr size_t kRec = kXchgInts - kXchgHead;
    std::vector<int32_t> recs(kRec * nranks, 0);  // every rank's rectangles, from the whole frame's
    for (uint32_t q = 0; q < nranks; ++q)
        write_rects(my_rects(L.rects, rank_rows(height, band_rows, nranks, q), width), recs.data() + kRec * q);
    std::vector<RankLayout> ranks(nranks);
    const uint64_t total = rank_table(recs.data(), kRec, height, band_rows, &ranks);
    std::vector<Schedule> S;
    std::vector<size_t> base;  // rank q's buffer inside buf
    size_t all = 0;
    for (uint32_t q = 0; q < nranks; ++q) {
        S.push_back(schedule(ranks, total, q, nframes, rotate != 0));
        base.push_back(all);
        all += (S.back().need + 255) & ~(size_t)255;
    }
    const size_t block = (size_t)rows_max * width * 3u, frame_bytes = (size_t)height * width * 3u;
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    DeviceBuf<RankLayout> d_ranks;  // (this batch's own table, buffer and fault word: not the context's plan)
    DeviceBuf<uint8_t> buf;
    DeviceBuf<int32_t> d_fault;
    hipError_t he = d_ranks.alloc(nranks);
    if (he == hipSuccess) he = buf.alloc(std::max<size_t>(all, 256));
    if (he == hipSuccess) he = d_fault.alloc(1);
    if (he == hipSuccess) he = hipMemsetAsync(d_fault, 0, sizeof(int32_t), s);
    const XferHeader hdr{ERAY_OK, src.kind, (uint32_t)src.key, (uint32_t)(src.key >> 32)};
    for (uint32_t q = 0; q < nranks && he == hipSuccess; ++q)  // every rank's headers
        if (S[q].hdr.n) he = enqueue_headers(buf + base[q], S[q], hdr, s);
    if (he == hipSuccess) he = hipMemcpyAsync(d_ranks, ranks.data(), sizeof(RankLayout) * nranks, hipMemcpyHostToDevice, s);
    for (uint32_t q = 0; q < nranks && he == hipSuccess; ++q)  // every rank packs its frames
        if (ranks[q].bytes)
            he = enqueue_pack(staging + q * block, nranks * block, buf + base[q], S[q], ranks[q], width, nframes, q, s);
    for (uint32_t q = 0; q < nranks && he == hipSuccess; ++q)  // each send meets its peer's receive
        for (const Xfer& x : S[q].ops) {
            if (!x.send) continue;
            const Xfer* m = nullptr;
            for (const Xfer& y : S[x.peer].ops)
                if (!y.send && y.peer == q) m = &y;
            if (!m || m->bytes != x.bytes) {
                he = hipErrorInvalidValue;
                break;
            }
            he = hipMemcpyAsync(buf + base[x.peer] + m->off, buf + base[q] + x.off, x.bytes, hipMemcpyDeviceToDevice, s);
            if (he != hipSuccess) break;
        }
    const PlanFrames F{height, width, band_rows, nranks, src.kind, src.key, d_ranks, d_fault};
    for (uint32_t r = 0; r < nranks && he == hipSuccess; ++r)  // every root assembles its frames
        if (S[r].mine) he = enqueue_assemble(buf + base[r], S[r], F, frames + S[r].R.before(r) * frame_bytes, frame_bytes, s);
    int32_t fault = 0;
    if (he == hipSuccess) he = hipMemcpyAsync(&fault, d_fault, sizeof fault, hipMemcpyDeviceToHost, s);
    if (he == hipSuccess) he = hipStreamSynchronize(s);
    if (he != hipSuccess) return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(he));
    return fault ? set_error(ctx, ERAY_E_INVALID_ARGUMENT, "scene gather: a root refused its batch") : ERAY_OK;
}

// One frame of eray_debug_scene_gather_batch (staging: the N ranks' blocks; frame: rank 0's).
int eray_debug_scene_gather(eray_ctx* ctx, const uint8_t* staging, uint8_t* frame, uint32_t height, uint32_t width,
                            uint32_t band_rows, uint32_t nranks) {
    return eray_debug_scene_gather_batch(ctx, staging, frame, 1, height, width, band_rows, nranks, 0);
}

// Diagnostics (tests): the coded banded gather of N ranks on one GPU — staging holds the N ranks'
// padded local PPM blocks; each is encoded into rank 0's code / packed layout as the point-to-
// point transfers would leave it, then decoded into frame.
int eray_debug_coded_unband(eray_ctx* ctx, const uint8_t* staging, uint8_t* frame, uint32_t height, uint32_t width,
                            uint32_t band_rows, uint32_t nranks) {
    if (!ctx || !staging || !frame || !band_rows || band_rows % 4 || !nranks || nranks > (uint32_t)kMaxCodedRanks)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "coded unband: bad arguments");
    if (!height || !width) return ERAY_OK;
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    const uint32_t rows = band_rows_of(height, band_rows, nranks, 0);
    const uint32_t S = (width + kSegPx - 1) / kSegPx, G = rows * S;
    CodedBufs b;
    b.count = reinterpret_cast<uint32_t*>(ctx->d_coll + kScrWords);
    if (!coded_bufs(ctx, G, nranks, &b))
        return set_error(ctx, ERAY_E_OUT_OF_MEMORY, "coded unband: staging buffer");
    RankOffsets off{};
    std::vector<uint32_t> counts(nranks);
    for (uint32_t k = 0; k < nranks; ++k) {
        if (k) off.v[k] = off.v[k - 1] + counts[k - 1];
        const uint8_t* local = staging + (size_t)k * rows * width * 3u;
        hipError_t e = encode_rows(local, band_rows_of(height, band_rows, nranks, k), rows, width, S,
                                   b.code + (size_t)k * G, b.packed + (size_t)off.v[k] * kSegBytes, b, s);
        if (e == hipSuccess) e = hipMemcpyAsync(&counts[k], b.count, 4, hipMemcpyDeviceToHost, s);
        if (e == hipSuccess) e = hipStreamSynchronize(s);
        if (e != hipSuccess) return set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(e));
    }
    seg_decode_kernel<<<height, 256, 0, s>>>(b.code, b.packed, off, frame, height, width, S, band_rows, nranks, rows);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ERAY_OK : set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(e));
}

// Diagnostics (tests): rank 0's reordering step of the banded gather alone — staging holds the N
// ranks' padded local PPM blocks as the collective would leave them.
int eray_debug_unband(eray_ctx* ctx, const uint8_t* staging, uint8_t* frame, uint32_t height, uint32_t width,
                      uint32_t band_rows, uint32_t nranks) {
    if (!ctx || !staging || !frame || !band_rows || band_rows % 4 || !nranks)
        return set_error(ctx, ERAY_E_INVALID_ARGUMENT, "unband: bad arguments");
    if (!height) return ERAY_OK;
    hipStream_t s = (hipStream_t)eray_get_stream(ctx);
    unband_rows_kernel<<<height, 256, 0, s>>>(staging, frame, height, width * 3u, band_rows, nranks,
                                               band_rows_of(height, band_rows, nranks, 0));
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? ERAY_OK : set_error(ctx, ERAY_E_HIP, "%s", hipGetErrorString(e));
}

}  // extern "C"
