// capi_debug.cpp — diagnostics of the frame path's setup on a context (ctx.hpp), not part of
// include/eray_hip.h: the screen bins of an object as the last setup built them (eray_debug_bin_*),
// the bins' capacity and the pair pass's form (eray_debug_set_bin_*), and the setup's device state
// (eray_debug_setup_state).  The tests read them; nothing in the library calls them.  Host code only.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <vector>

#include "ctx.hpp"

namespace {
// Object `index`'s place among the binned objects (*k) when it has screen bins to read: a binned
// object of a context whose bins exist.  False otherwise: the hooks then return
// ERAY_E_INVALID_ARGUMENT without a message.
bool binned_object(const eray_ctx* ctx, uint32_t index, uint32_t* k) {
    if (!ctx || index >= ctx->objects.size() || ctx->objects[index].T <= kDirectMax || !ctx->bins.start) return false;
    *k = binned_before(ctx, index);
    return true;
}
}  // namespace

extern "C" {

// The screen bins of object `index` as built for the last setup — out[0] bins, out[1] entries,
// out[2] (face, pixel) pairs (mask bits), out[3] most entries in one bin, out[4] non-empty bins,
// out[5] most pairs in one bin, out[6..9] the object's pixel rectangle (x0, x1, y0, y1; int32 as
// uint64), out[10] the bin with the most entries, out[11] / out[12] the bins of more than 64 /
// kTraceHeavyMin entries, out[13] the units the pair pass walked: the faces' bin-rectangle rows
// (segments) or their (face, bin) pairs (the tracer's setups, eray_debug_set_bin_form) (out: 14
// words).  Synchronises.
int eray_debug_bin_stats(eray_ctx* ctx, uint32_t index, uint64_t* out) {
    uint32_t k;
    if (!out || !binned_object(ctx, index, &k)) return ERAY_E_INVALID_ARGUMENT;
    const BinBuffers& b = ctx->bins;
    std::vector<uint32_t> start(b.nbins + 1);
    ObjectDesc d{};
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(start.data(), b.start + (size_t)k * b.nbins, start.size() * 4, hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&d, ctx->d_objs + index, sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin stats copy failed");
    const size_t n = start[b.nbins] - start[0];
    std::vector<unsigned long long> mask(n);  // the entries' masks (a strided copy out of the 64-B entries)
    if (n && hipMemcpy2D(mask.data(), 8, reinterpret_cast<const char*>(b.ent + start[0]) + offsetof(BinEntry, mask),
                         sizeof(BinEntry), 8, n, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin stats copy failed");
    uint64_t pairs = 0, most = 0, nonempty = 0, most_pairs = 0, most_at = 0, over64 = 0, over192 = 0;
    for (size_t i = 0; i < b.nbins; ++i) {
        const uint64_t e = start[i + 1] - start[i];
        over64 += e > 64;
        over192 += e > kTraceHeavyMin;
        if (e > most) most_at = i;
        most = e > most ? e : most;
        nonempty += e != 0;
        uint64_t pb = 0;
        for (uint32_t j = start[i]; j < start[i + 1]; ++j) pb += (uint64_t)__builtin_popcountll(mask[j - start[0]]);
        pairs += pb;
        most_pairs = pb > most_pairs ? pb : most_pairs;
    }
    out[0] = b.nbins;
    out[1] = n;
    out[2] = pairs;
    out[3] = most;
    out[4] = nonempty;
    out[5] = most_pairs;
    for (int q = 0; q < 4; ++q) out[6 + q] = (uint64_t)(int64_t)d.g.rect[q];
    out[10] = most_at;
    out[11] = over64;
    out[12] = over192;
    // out[13]: the units of the faces' bin rectangles (every object)
    unsigned long long pairs_all = 0;
    if (hipMemcpy(&pairs_all, b.boff + setup_blocks(ctx->total_tris), sizeof pairs_all, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin stats copy failed");
    out[13] = pairs_all;
    return ERAY_OK;
}

// The entries of bin `bin` of object `index` in bin order (faces relative to the object, pixel
// masks, pad words: a sorted bin's later-chunk mask unions, BinEntry), at most `cap`; *n = the
// bin's entry count; `pad` may be null.  Synchronises.
int eray_debug_bin_entries(eray_ctx* ctx, uint32_t index, uint32_t bin, uint32_t* tri, uint64_t* mask, uint32_t* pad,
                           uint32_t cap, uint32_t* n) {
    uint32_t k;
    if (!n || !binned_object(ctx, index, &k) || bin >= ctx->bins.nbins) return ERAY_E_INVALID_ARGUMENT;
    const BinBuffers& b = ctx->bins;
    uint32_t se[2];
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(se, b.start + (size_t)k * b.nbins + bin, 8, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin dump copy failed");
    *n = se[1] - se[0];
    const uint32_t m = std::min(*n, cap);
    std::vector<BinEntry> ent(m);
    if (m && hipMemcpy(ent.data(), b.ent + se[0], sizeof(BinEntry) * (size_t)m, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "bin dump copy failed");
    for (uint32_t i = 0; i < m; ++i) {
        tri[i] = ent[i].tri;
        mask[i] = ent[i].mask;
        if (pad) pad[i] = ent[i].pad;
    }
    return ERAY_OK;
}

// eray_debug_bin_entries without the pad words.
int eray_debug_bin_dump(eray_ctx* ctx, uint32_t index, uint32_t bin, uint32_t* tri, uint64_t* mask, uint32_t cap,
                        uint32_t* n) {
    return eray_debug_bin_entries(ctx, index, bin, tri, mask, nullptr, cap, n);
}

// The entry count of every bin of object `index` (bins.nbins of them, row-major over the camera's
// bin rows, at most `cap`); *nbins = the object's bin count.  Synchronises.
int eray_debug_bin_counts(eray_ctx* ctx, uint32_t index, uint32_t* counts, uint32_t cap, uint32_t* nbins) {
    uint32_t k;
    if (!nbins || !binned_object(ctx, index, &k)) return ERAY_E_INVALID_ARGUMENT;
    const BinBuffers& b = ctx->bins;
    *nbins = b.nbins;
    const uint32_t m = std::min(b.nbins, cap);
    std::vector<uint32_t> st((size_t)m + 1);
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        (m && hipMemcpy(st.data(), b.start + (size_t)k * b.nbins, sizeof(uint32_t) * ((size_t)m + 1),
                        hipMemcpyDeviceToHost) != hipSuccess))
        return set_error(ctx, ERAY_E_HIP, "bin counts copy failed");
    for (uint32_t i = 0; i < m; ++i) counts[i] = st[i + 1] - st[i];
    return ERAY_OK;
}

// The screen bins' entry capacity.  Setting it reallocates the bins at the next setup; a setup
// whose entries exceed it renders its binned objects through LDS tiles and the capacity grows once
// the host sees the count (tests).
int eray_debug_set_bin_capacity(eray_ctx* ctx, uint64_t entries) {
    if (!ctx || !entries) return ERAY_E_INVALID_ARGUMENT;
    ctx->bin_cap = std::min((size_t)entries, kMaxBinEntries);
    ctx->setup_key.clear();
    return ERAY_OK;
}

uint64_t eray_debug_bin_capacity(const eray_ctx* ctx) { return ctx ? (uint64_t)ctx->bins.cap : 0u; }

// The frame setups' pair pass walks every (face, bin) pair of the faces' bin rectangles
// (rect_pairs != 0) instead of the rectangles' rows (bins.hip bin_segments_kernel); the next setup
// rebuilds the bins (tests compare the two forms' entries).
int eray_debug_set_bin_form(eray_ctx* ctx, int rect_pairs) {
    if (!ctx) return ERAY_E_INVALID_ARGUMENT;
    ctx->rect_pairs = rect_pairs != 0;
    ctx->setup_key.clear();
    ctx->mc_layout.clear();
    return ERAY_OK;
}

// The last setup's device state (CamState, 192 B) and object `index`'s pixel rectangle as the
// frame kernel reads them (synchronises).
int eray_debug_setup_state(eray_ctx* ctx, uint32_t index, void* state_out, int32_t* rect_out) {
    if (!ctx || !state_out || !rect_out || index >= ctx->objects.size()) return ERAY_E_INVALID_ARGUMENT;
    ObjectDesc d{};
    if (hipStreamSynchronize(ctx->stream) != hipSuccess ||
        hipMemcpy(state_out, ctx->d_state, sizeof(CamState), hipMemcpyDeviceToHost) != hipSuccess ||
        hipMemcpy(&d, ctx->d_objs + index, sizeof d, hipMemcpyDeviceToHost) != hipSuccess)
        return set_error(ctx, ERAY_E_HIP, "setup state copy failed");
    std::memcpy(rect_out, d.g.rect, sizeof d.g.rect);
    return ERAY_OK;
}

}  // extern "C"
