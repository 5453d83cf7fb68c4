// Stand-alone checker of the frame calls' planning (eray_amd/csrc/frame_plan.hpp, the header
// capi_frames.cpp decides with before it touches the GPU): plain host code, no library to link,
// meant for the host sanitizers and a machine without a GPU:
//
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tests/cpp/frame_plan_main.cpp -o /tmp/frame_plan && /tmp/frame_plan
//
// Every expectation is a plain restatement written here (loops over rows, frames and slots), never
// the header's own function: which banded and contiguous calls reach only rows of the camera, which
// cameras fit the engine image, the statuses and the exact messages of every rejecting branch, the
// ring's argument rules, the frames per launch as the largest of {8, 4, 2, 1} within the slots and
// the pixel cap, that the plans' walks with the launch function render every frame of a call exactly
// once into its own ring slot without wrapping (the static ring's form and the camera paths'), and
// ring_frames' pointers and its beyond-the-cache flag.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../../eray_amd/csrc/frame_plan.hpp"

using namespace eray::gpu;

namespace {
int g_failed = 0;
long g_checks = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        ++g_checks;                                       \
        if (!(cond)) {                                    \
            ++g_failed;                                   \
            std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

char g_why[kWhyLen];

eray_render_params params(uint32_t iw, uint32_t ih, uint32_t row0, uint32_t rows) {
    eray_render_params rp;
    std::memset(&rp, 0, sizeof rp);
    rp.image_width = iw;
    rp.image_height = ih;
    rp.row0 = row0;
    rp.rows = rows;
    return rp;
}
int check(const eray_render_params& rp, uint32_t W, uint32_t H, uint32_t bounces = 0) {
    std::memset(g_why, '#', sizeof g_why);
    const int st = check_render_params(&rp, W, H, bounces, g_why, sizeof g_why);
    CHECK(std::memchr(g_why, 0, sizeof g_why) != nullptr, "the message is terminated");
    CHECK((st == ERAY_OK) == (g_why[0] == 0), "status %d with message '%.200s'", st, g_why);
    return st;
}
#define CHECK_WHY(text) CHECK(std::strcmp(g_why, text) == 0, "message '%s'", g_why)

// ---- rows
void banded_rows() {
    const uint32_t W = 16;
    for (uint32_t H = 4; H <= 64; ++H)
        for (uint32_t band_rows : {4u, 8u, 16u}) {
            uint32_t shift = 0;
            while ((1u << shift) != band_rows) ++shift;
            for (uint32_t stride = 0; stride <= 40; stride += 4)
                for (uint32_t row0 = 0; row0 <= H + 4; row0 += 4)
                    for (uint32_t rows = 0; rows <= H + 9; ++rows) {
                        eray_render_params rp = params(W, H, row0, rows);
                        rp.band_rows = band_rows;
                        rp.band_stride = stride;
                        bool inside = stride >= band_rows;
                        for (uint32_t j = 0; j < rows && inside; ++j) {
                            const uint32_t y = band_camera_row(row0, shift, band_rows - 1, stride, j);
                            // (eray_hip.h's own wording of the mapping)
                            CHECK(y == row0 + (j / band_rows) * stride + j % band_rows, "local row %u", j);
                            inside = y < H;
                        }
                        const int st = check(rp, W, H);
                        CHECK((st == ERAY_OK) == inside && (inside || st == ERAY_E_INVALID_ARGUMENT),
                              "H %u bands %u stride %u row0 %u rows %u: status %d", H, band_rows, stride, row0, rows, st);
                        const RowSpan rs = row_span(&rp);
                        CHECK(rs.row0 == row0 && rs.rows == rows && rs.band_shift == shift && rs.band_mask == band_rows - 1 &&
                                  rs.band_stride == stride, "row_span of bands %u", band_rows);
                    }
        }
    // misaligned band arguments, each alone (H 64, rows that would fit)
    struct Bad { uint32_t band_rows, stride, row0; };
    for (const Bad& b : {Bad{2, 8, 0}, Bad{6, 8, 0}, Bad{12, 12, 0}, Bad{1, 4, 0}, Bad{8, 10, 0}, Bad{8, 8, 2}, Bad{8, 8, 5},
                         Bad{8, 4, 0}, Bad{16, 12, 4}}) {
        eray_render_params rp = params(16, 64, b.row0, 1);
        rp.band_rows = b.band_rows;
        rp.band_stride = b.stride;
        CHECK(check(rp, 16, 64) == ERAY_E_INVALID_ARGUMENT, "bands %u stride %u row0 %u", b.band_rows, b.stride, b.row0);
    }
}
void contiguous_rows() {
    for (uint32_t H = 4; H <= 64; ++H)
        for (uint32_t row0 = 0; row0 <= H + 2; ++row0)
            for (uint32_t rows = 0; rows <= H + 2; ++rows) {
                const eray_render_params rp = params(16, H, row0, rows);
                const int st = check(rp, 16, H);
                bool inside = true;
                for (uint32_t j = 0; j < rows; ++j) inside = inside && row0 + j < H;
                // (no rows: any first row up to H itself)
                if (!rows) inside = row0 <= H;
                CHECK((st == ERAY_OK) == inside && (inside || st == ERAY_E_INVALID_ARGUMENT), "H %u rows [%u, +%u): status %d", H,
                      row0, rows, st);
                CHECK((st == ERAY_OK) == (row0 + rows <= H), "H %u rows [%u, +%u)", H, row0, rows);
                const RowSpan rs = row_span(&rp);
                for (uint32_t j = 0; j < rows; ++j)
                    CHECK(band_camera_row(rs.row0, rs.band_shift, rs.band_mask, rs.band_stride, j) == row0 + j, "row %u", j);
            }
    // a row range whose end is past 2^32 is refused (the sum is taken in 64 bits; the message's
    // end is the parent's 32-bit sum)
    const eray_render_params rp = params(16, 64, 0xffffffffu, 2);
    CHECK(check(rp, 16, 64) == ERAY_E_INVALID_ARGUMENT, "row0 2^32 - 1");
    CHECK_WHY("rows [4294967295, 1) exceed the camera height 64");
}

// ---- image fit, flags, bounces, messages
void image_fit() {
    uint8_t* const some_ppm = reinterpret_cast<uint8_t*>(uintptr_t(4096));
    for (uint32_t W = 1; W <= 20; ++W)
        for (uint32_t H = 1; H <= 20; ++H)
            for (uint32_t iw = 1; iw <= 20; ++iw)
                for (uint32_t ih = 1; ih <= 20; ++ih) {
                    eray_render_params rp = params(iw, ih, 0, 0);
                    const bool fits = (uint64_t)(H - 1) * iw + (W - 1) < (uint64_t)iw * ih;
                    const int st = check(rp, W, H);
                    CHECK(st == (fits ? ERAY_OK : ERAY_E_OUT_OF_BOUNDS), "camera %ux%u image %ux%u: status %d", W, H, iw, ih, st);
                    rp.out_ppm = some_ppm;
                    const int want = !fits ? ERAY_E_OUT_OF_BOUNDS : (W == iw && H == ih) ? ERAY_OK : ERAY_E_INVALID_ARGUMENT;
                    const int sp = check(rp, W, H);
                    CHECK(sp == want, "camera %ux%u image %ux%u with out_ppm: status %d", W, H, iw, ih, sp);
                }
    // an empty camera fits any image
    CHECK(check(params(1, 1, 0, 0), 0, 0) == ERAY_OK && check(params(1, 1, 0, 0), 0, 7) == ERAY_OK, "empty camera");
    eray_render_params rp = params(16, 16, 0, 16);
    for (uint32_t bit = 0; bit < 32; ++bit) {
        rp.flags = 1u << bit;
        CHECK(check(rp, 16, 16) == (bit < 7 ? ERAY_OK : ERAY_E_INVALID_ARGUMENT), "flag bit %u", bit);
    }
    rp.flags = 127u;  // every ERAY_RENDER_* flag of eray_hip.h
    CHECK(check(rp, 16, 16) == ERAY_OK, "all known flags");
    rp.flags = 127u | 128u;
    CHECK(check(rp, 16, 16) == ERAY_E_INVALID_ARGUMENT, "an unknown flag beside known ones");
    CHECK_WHY("unknown render flags 0xff");
    rp.flags = 0;
    rp.bounces = 16;
    CHECK(check(rp, 16, 16, 16) == ERAY_OK, "16 bounces");
    rp.bounces = 17;
    CHECK(check(rp, 16, 16, 17) == ERAY_E_UNSUPPORTED, "17 bounces");
    CHECK_WHY("bounces = 17: at most 16 reflection levels");
    CHECK(check(rp, 16, 16, 0) == ERAY_OK, "17 bounces asked, none in effect (no material reflects)");
    // the other rejecting branches' messages
    CHECK(check(params(16, 16, 8, 9), 16, 16) == ERAY_E_INVALID_ARGUMENT, "rows");
    CHECK_WHY("rows [8, 17) exceed the camera height 16");
    CHECK(check(params(12, 9, 0, 0), 13, 10) == ERAY_E_OUT_OF_BOUNDS, "fit");
    CHECK_WHY("camera size 13x10 does not fit the 12x9 engine image (Image::set panics)");
    rp = params(16, 32, 0, 0);
    rp.out_ppm = some_ppm;
    CHECK(check(rp, 16, 16) == ERAY_E_INVALID_ARGUMENT, "ppm");
    CHECK_WHY("fused PPM output needs camera size == image size; use eray_pack_ppm");
    rp = params(16, 64, 4, 8);
    rp.band_rows = 12;
    rp.band_stride = 16;
    CHECK(check(rp, 16, 64) == ERAY_E_INVALID_ARGUMENT, "bands");
    CHECK_WHY("bands: band_rows (12) must be a power of two >= 4, band_stride (16) and row0 (4) multiples of 4, "
              "band_stride >= band_rows");
    rp.band_rows = 8;
    rp.rows = 30;  // local row 29: camera row 4 + 3 * 16 + 5 = 57 of 40
    CHECK(check(rp, 16, 40) == ERAY_E_INVALID_ARGUMENT, "bands past the end");
    CHECK_WHY("bands: 30 local rows reach past the camera height 40");
    // order: bounces, flags, rows, fit, ppm
    rp = params(12, 9, 8, 9);
    rp.flags = 128u;
    rp.bounces = 17;
    CHECK(check(rp, 13, 10, 17) == ERAY_E_UNSUPPORTED, "bounces first");
    CHECK(check(rp, 13, 10, 0) == ERAY_E_INVALID_ARGUMENT && !std::strncmp(g_why, "unknown", 7), "then flags");
    rp.flags = 0;
    CHECK(check(rp, 13, 10, 0) == ERAY_E_INVALID_ARGUMENT && !std::strncmp(g_why, "rows", 4), "then rows");
    rp.rows = 1;
    CHECK(check(rp, 13, 10, 0) == ERAY_E_OUT_OF_BOUNDS, "then the fit");
    // a short buffer truncates and terminates
    char small[8];
    CHECK(check_render_params(&rp, 13, 10, 0, small, sizeof small) == ERAY_E_OUT_OF_BOUNDS && !std::strcmp(small, "camera "),
          "short buffer '%s'", small);
}

// ---- the ring's arguments
FrameParams frame(uint32_t cam_w, uint32_t rows, uint32_t max_tris = 12) {
    FrameParams p;
    std::memset(&p, 0, sizeof p);
    p.cam_w = cam_w;
    p.rows = rows;
    p.max_object_tris = max_tris;
    return p;
}
int ring_of(const eray_render_params& rp, const FrameParams& p, const eray_frame_ring* r, Ring* out) {
    std::memset(g_why, '#', sizeof g_why);
    const int st = make_ring(&rp, p, r, out, g_why, sizeof g_why);
    CHECK((st == ERAY_OK) == (g_why[0] == 0), "status %d with message '%.200s'", st, g_why);
    return st;
}
void ring_arguments() {
    const uint32_t W = 16, rows = 8;
    const uint64_t need[3] = {W * rows * 12u, W * rows * 3u, W * rows * 4u};  // all multiples of 16
    void* const some = reinterpret_cast<void*>(uintptr_t(4096));
    const FrameParams p = frame(W, rows);
    Ring ring;
    CHECK(ring_of(params(W, rows, 0, rows), p, nullptr, &ring) == ERAY_OK && ring.slots == 1 && ring.per_launch == 1 &&
              !ring.rgb && !ring.ppm && !ring.face, "no ring: one slot");
    for (uint32_t slots = 0; slots <= 130; ++slots) {
        bool pow2 = false;
        for (uint32_t k = 1; k <= 64; k *= 2) pow2 = pow2 || slots == k;
        const eray_frame_ring r{slots, 0, 0, 0, 0};
        const int st = ring_of(params(W, rows, 0, rows), p, &r, &ring);  // (no outputs: no stride asked)
        CHECK(st == (pow2 ? ERAY_OK : ERAY_E_INVALID_ARGUMENT), "slots %u: status %d", slots, st);
        if (pow2) CHECK(ring.slots == slots, "slots %u kept", slots);
        if (slots == 3) CHECK_WHY("ring: slots (3) must be a power of two <= 64");
        if (slots == 128) CHECK_WHY("ring: slots (128) must be a power of two <= 64");
    }
    // strides: bad ones count only for outputs that are there, and only with more than one slot
    for (uint32_t present = 0; present < 8; ++present)
        for (uint32_t slots : {1u, 2u, 64u})
            for (int bad = -1; bad < 3; ++bad)
                for (int how = 0; how < (bad < 0 ? 1 : 3); ++how) {
                    eray_render_params rp = params(W, rows, 0, rows);
                    if (present & 1) rp.out_rgb = static_cast<float*>(some);
                    if (present & 2) rp.out_ppm = static_cast<uint8_t*>(some);
                    if (present & 4) rp.out_face = static_cast<int32_t*>(some);
                    uint64_t stride[3] = {need[0], need[1] + 16, need[2] + 4096};
                    if (bad >= 0) stride[bad] = how == 0 ? need[bad] - 16 : how == 1 ? need[bad] + 8 : 0;
                    const eray_frame_ring r{slots, 0, stride[0], stride[1], stride[2]};
                    const bool refused = bad >= 0 && (present >> bad & 1) && slots > 1;
                    const int st = ring_of(rp, p, &r, &ring);
                    CHECK(st == (refused ? ERAY_E_INVALID_ARGUMENT : ERAY_OK), "present %u slots %u bad %d how %d: status %d", present,
                          slots, bad, how, st);
                    if (!refused)
                        CHECK(ring.rgb == (slots > 1 ? stride[0] : 0) && ring.ppm == (slots > 1 ? stride[1] : 0) &&
                                  ring.face == (slots > 1 ? stride[2] : 0), "strides kept (0 with one slot)");
                    if (refused && bad == 1 && how == 1 && present == 2 && slots == 2)
                        CHECK_WHY("ring: output 1's slot stride 392 must be a multiple of 16 of at least 384 bytes");
                }
    // frames per launch as asked: a power of two up to the slots
    for (uint32_t slots : {1u, 2u, 4u, 8u, 16u, 32u, 64u})
        for (uint32_t asked = 0; asked <= 130; ++asked) {
            bool ok = asked == 0;
            for (uint32_t k = 1; k <= slots; k *= 2) ok = ok || asked == k;
            const eray_frame_ring r{slots, asked, 0, 0, 0};
            const int st = ring_of(params(W, rows, 0, rows), p, &r, &ring);
            CHECK(st == (ok ? ERAY_OK : ERAY_E_INVALID_ARGUMENT), "slots %u frames_per_launch %u: status %d", slots, asked, st);
            if (ok && asked) CHECK(ring.per_launch == (slots == 1 ? 1u : asked), "slots %u asked %u: %u", slots, asked, ring.per_launch);
            if (slots == 4 && asked == 3) CHECK_WHY("ring: frames_per_launch (3) must be a power of two <= slots (4)");
            if (slots == 4 && asked == 8) CHECK_WHY("ring: frames_per_launch (8) must be a power of two <= slots (4)");
        }
}

// ---- the library's frames per launch
uint32_t plain_auto(uint64_t w, uint64_t rows, uint32_t slots, bool binned) {
    const uint64_t cap = binned ? 3840ull * 2160ull : 2ull * 3840ull * 2160ull;
    for (uint32_t F : {8u, 4u, 2u})
        if (F <= slots && F * w * rows <= cap) return F;
    return 1;
}
void frames_in_flight() {
    for (uint32_t w : {1u, 1919u, 1920u, 1921u, 3839u, 3840u, 3841u, 7680u})
        for (uint32_t rows : {1u, 539u, 540u, 541u, 1079u, 1080u, 1081u, 2159u, 2160u, 2161u, 4320u})
            for (uint32_t slots : {1u, 2u, 4u, 8u, 16u, 64u})
                for (uint32_t tris : {12u, 256u, 257u, 70000u}) {
                    const uint32_t want = plain_auto(w, rows, slots, tris > 256);
                    const FrameParams p = frame(w, rows, tris);
                    const eray_frame_ring r{slots, 0, 0, 0, 0};
                    Ring ring;
                    CHECK(ring_of(params(w, rows, 0, rows), p, &r, &ring) == ERAY_OK && ring.per_launch == want,
                          "%ux%u slots %u tris %u: %u frames per launch, not %u", w, rows, slots, tris, ring.per_launch, want);
                    // eray_frames_per_launch's path
                    const uint32_t F = frames_per_launch(false, slots, 0, w, rows, tris);
                    CHECK(F == want && F == ring.per_launch, "%ux%u slots %u tris %u: %u", w, rows, slots, tris, F);
                    CHECK(frames_per_launch(true, slots, 0, w, rows, tris) == 1, "the general tracer");
                    // the general tracer, and one slot, whatever was asked
                    for (uint32_t asked : {0u, 1u, 2u}) {
                        if (asked > slots) continue;
                        const eray_frame_ring ra{slots, asked, 0, 0, 0};
                        FrameParams g = p;
                        g.aa = 2;
                        CHECK(ring_of(params(w, rows, 0, rows), g, &ra, &ring) == ERAY_OK && ring.per_launch == 1, "anti-aliasing");
                        g.aa = 0;
                        g.bounces = 1;
                        CHECK(ring_of(params(w, rows, 0, rows), g, &ra, &ring) == ERAY_OK && ring.per_launch == 1, "bounces");
                        if (slots == 1) CHECK(ring_of(params(w, rows, 0, rows), p, &ra, &ring) == ERAY_OK && ring.per_launch == 1, "one slot");
                    }
                }
    CHECK(plain_auto(1920, 1080, 8, false) == 8 && plain_auto(3840, 2160, 8, false) == 2 && plain_auto(1920, 1080, 8, true) == 4 &&
              plain_auto(3840, 2160, 8, true) == 1 && plain_auto(1, 1, 64, true) == 8, "the restatement's own landmarks");
}

// ---- coverage: every frame of a call once, in its slot
// The launches of one call, recorded as the strategies of capi_frames.cpp make them: launch(ring
// frame, count) goes through ring_frames, whose PPM pointer tells the slot.
struct Coverage {
    Ring r;
    uint32_t frames, per_launch;
    std::vector<uint32_t> rendered;
    FrameParams p;
    uint8_t* base = reinterpret_cast<uint8_t*>(uintptr_t(1) << 20);
    uint32_t chunks = 0, rests = 0, chunk_frames = 0, plains = 0;
    Coverage(uint32_t slots, uint32_t per_launch, uint32_t frames)
        : frames(frames), per_launch(per_launch), rendered(frames, 0u), p(frame(16, 8)) {
        r.slots = slots;
        r.per_launch = per_launch;
        r.ppm = 384;
        p.out_ppm = base;
    }
    void launch(uint32_t ring_frame, uint32_t count) {
        CHECK(count >= 1 && count <= per_launch, "launch of %u frames (per launch %u)", count, per_launch);
        const FrameParams q = ring_frames(p, r, ring_frame, count);
        const uint64_t slot = (uint64_t)(q.out_ppm - base) / r.ppm;
        CHECK(q.nframes == count && (uint64_t)(q.out_ppm - base) % r.ppm == 0, "launch parameters");
        CHECK(slot == ring_frame % r.slots && slot + count <= r.slots, "frame %u x %u: slot %llu of %u", ring_frame, count,
              (unsigned long long)slot, r.slots);
        for (uint32_t k = 0; k < count; ++k) {
            CHECK(ring_frame + k < frames, "frame %u of %u", ring_frame + k, frames);
            if (ring_frame + k < frames) ++rendered[ring_frame + k];
        }
    }
    void done(const PlanShape& s, bool direct) {
        for (uint32_t f = 0; f < frames; ++f)
            CHECK(rendered[f] == 1, "slots %u per launch %u frames %u: frame %u rendered %u times", r.slots, per_launch, frames, f,
                  rendered[f]);
        CHECK(chunk_frames + plains == frames, "chunks %u rest %u plain %u of %u frames", chunks, rests, plains, frames);
        CHECK(plains <= (direct ? 0u : 1u) && rests <= 1, "plain %u rests %u", plains, rests);
        // what the plan is, restated: whole chunks of min(frames, 64), then the remainder
        const uint32_t chunk = frames < 64 ? frames : 64, whole = chunk ? frames / chunk : 0, left = chunk ? frames % chunk : 0;
        if (direct || frames >= 2) {
            CHECK(chunks == whole && s.chunk == chunk, "chunks %u of %u (%u frames)", chunks, s.chunk, frames);
            CHECK(rests == (left > (direct ? 0u : 1u) ? 1u : 0u) && plains == (direct ? 0u : left == 1 ? 1u : 0u), "remainder %u", left);
        } else {
            CHECK(!chunks && !rests && plains == frames, "fewer than two frames: plain");
        }
    }
};

void static_ring(uint32_t slots, uint32_t per_launch, uint32_t frames) {
    {  // captured graphs, as StaticRing: the frame's index in its chunk; plain with the call's count
        Coverage c(slots, per_launch, frames);
        const PlanShape s = graph_plan_shape(frames, true);
        const int st = walk_plan(
            s, frames,
            [&](uint32_t first, uint32_t count, bool rest) {
                CHECK(first % 64 == 0 && count == (rest ? s.rest : s.chunk), "chunk at %u", first);
                ++(rest ? c.rests : c.chunks);
                c.chunk_frames += count;
                for (uint32_t f = 0; f < count; ++f)
                    if (const uint32_t nf = launch_frames(f, count, per_launch)) {
                        CHECK((first + f) % slots == f % slots, "a chunk starts at slot 0");
                        c.launch(first + f, nf);  // (the product passes f: the same slot, checked above)
                    }
                return 0;
            },
            [&](uint32_t f) {
                ++c.plains;
                if (const uint32_t nf = launch_frames(f, frames, per_launch)) c.launch(f, nf);
                return 0;
            });
        CHECK(st == 0, "walk status");
        c.done(s, false);
    }
    {  // the null stream: no graphs, every frame through plain
        Coverage c(slots, per_launch, frames);
        const PlanShape s = graph_plan_shape(frames, false);
        CHECK(!s.chunk && !s.rest, "no chunks on the null stream");
        walk_plan(s, frames, [&](uint32_t, uint32_t, bool) { ++c.chunks; return 0; },
                  [&](uint32_t f) {
                      if (const uint32_t nf = launch_frames(f, frames, per_launch)) c.launch(f, nf);
                      return 0;
                  });
        for (uint32_t f = 0; f < frames; ++f) CHECK(c.rendered[f] == 1, "null stream: frame %u rendered %u times", f, c.rendered[f]);
        CHECK(!c.chunks, "null stream: no chunk");
    }
}

// The camera paths' form: body(first, f, count) renders ring frame first + f from the chunk's slot f
// (batches of K cameras within the chunk), plain(f) is a batch of one.
void camera_path(uint32_t slots, uint32_t asked, uint32_t K, uint32_t frames, bool direct) {
    uint32_t per_launch = asked;  // restated: the largest power of two up to `asked` that divides K
    while (K % per_launch) per_launch >>= 1;
    CHECK(fit_per_launch(asked, K) == per_launch && K % per_launch == 0, "per launch %u fitted to K %u", asked, K);
    if (!direct) per_launch = asked;  // (the batched path keeps the ring's; its batch is the chunk)
    Coverage c(slots, per_launch, frames);
    const PlanShape s = direct ? direct_plan_shape(frames) : graph_plan_shape(frames, true);
    const int st = walk_plan(
        s, frames,
        [&](uint32_t first, uint32_t count, bool rest) {
            ++(rest ? c.rests : c.chunks);
            c.chunk_frames += count;
            for (uint32_t f = 0; f < count; ++f)
                if (const uint32_t nf = launch_frames(f, count, per_launch)) {
                    if (direct) CHECK(f / K == (f + nf - 1) / K, "launch of slots [%u, +%u) spans two batches of %u", f, nf, K);
                    c.launch(first + f, nf);
                }
            return 0;
        },
        [&](uint32_t f) {
            ++c.plains;
            const uint32_t nf = launch_frames(0, 1, 1);
            CHECK(nf == 1, "a batch of one");
            c.launch(f, nf);
            return 0;
        });
    CHECK(st == 0, "walk status");
    c.done(s, direct);
}

void coverage() {
    std::vector<uint32_t> counts;
    for (uint32_t n = 0; n <= 200; ++n) counts.push_back(n);
    for (uint32_t n : {255u, 256u, 257u}) counts.push_back(n);
    for (uint32_t slots : {1u, 2u, 4u, 8u, 64u})
        for (uint32_t per_launch = 1; per_launch <= slots; per_launch *= 2)
            for (uint32_t frames : counts) {
                static_ring(slots, per_launch, frames);
                camera_path(slots, per_launch, 64, frames, false);
                for (uint32_t K : {1u, 2u, 4u, 8u, 16u}) camera_path(slots, per_launch, K, frames, true);
            }
    // a walk ends at the first status that is not 0
    int calls = 0;
    CHECK(walk_plan(graph_plan_shape(200, true), 200, [&](uint32_t, uint32_t, bool) { return ++calls == 2 ? -7 : 0; },
                    [&](uint32_t) { return ++calls, 0; }) == -7 && calls == 2, "stops at the failing chunk (%d calls)", calls);
    calls = 0;
    CHECK(walk_plan(graph_plan_shape(3, false), 3, [&](uint32_t, uint32_t, bool) { return 0; },
                    [&](uint32_t) { return ++calls == 2 ? -2 : 0; }) == -2 && calls == 2, "stops at the failing frame (%d calls)", calls);
}

// ---- ring_frames: pointers and the cache flag
void ring_pointers() {
    const uint64_t MiB = 1ull << 20;
    char* const base[3] = {reinterpret_cast<char*>(uintptr_t(1) << 32), reinterpret_cast<char*>(uintptr_t(2) << 32),
                           reinterpret_cast<char*>(uintptr_t(3) << 32)};
    for (uint32_t present = 0; present < 8; ++present)
        for (uint32_t slots : {1u, 4u, 64u})
            for (uint32_t f : {0u, 1u, 3u, 4u, 63u, 64u, 67u, 1000u}) {
                FrameParams p = frame(16, 8);
                p.launch_flags = kLaunchDense | kLaunchSharedDetail;
                if (present & 1) p.out_rgb = reinterpret_cast<float*>(base[0]);
                if (present & 2) p.out_ppm = reinterpret_cast<uint8_t*>(base[1]);
                if (present & 4) p.out_face = reinterpret_cast<int32_t*>(base[2]);
                Ring r;
                r.slots = slots;
                r.rgb = 1536;
                r.ppm = 400;
                r.face = 512;
                const FrameParams q = ring_frames(p, r, f, 1);
                const uint64_t slot = f % slots;
                CHECK(reinterpret_cast<char*>(q.out_rgb) == ((present & 1) ? base[0] + slot * 1536 : nullptr), "rgb of slot %llu",
                      (unsigned long long)slot);
                CHECK(reinterpret_cast<char*>(q.out_ppm) == ((present & 2) ? base[1] + slot * 400 : nullptr), "ppm of slot %llu",
                      (unsigned long long)slot);
                CHECK(reinterpret_cast<char*>(q.out_face) == ((present & 4) ? base[2] + slot * 512 : nullptr), "face of slot %llu",
                      (unsigned long long)slot);
                CHECK(q.rgb_stride == 1536 && q.ppm_stride == 400 && q.face_stride == 512 && q.nframes == 1, "strides");
                CHECK(q.launch_flags == (kLaunchDense | kLaunchSharedDetail), "a small ring: flags kept");
                CHECK(q.cam_w == 16 && q.rows == 8, "the rest kept");
            }
    // beyond the cache: slots x the present outputs' strides above 256 MiB, one byte either side
    struct Case { uint32_t slots, present; uint64_t rgb, ppm, face; bool beyond; };
    for (const Case& k : {Case{1, 1, 256 * MiB - 1, 0, 0, false}, Case{1, 1, 256 * MiB, 0, 0, false}, Case{1, 1, 256 * MiB + 1, 0, 0, true},
                          Case{1, 2, 0, 256 * MiB, 0, false}, Case{1, 2, 0, 256 * MiB + 1, 0, true},
                          Case{1, 4, 0, 0, 256 * MiB, false}, Case{1, 4, 0, 0, 256 * MiB + 1, true},
                          Case{4, 7, 32 * MiB, 16 * MiB, 16 * MiB, false}, Case{4, 7, 32 * MiB, 16 * MiB, 16 * MiB + 1, true},
                          Case{4, 7, 32 * MiB, 16 * MiB - 1, 16 * MiB + 1, false},
                          // an absent output's stride does not count
                          Case{4, 3, 32 * MiB, 16 * MiB, 400 * MiB, false}, Case{4, 6, 400 * MiB, 16 * MiB, 16 * MiB, false},
                          Case{64, 1, 4 * MiB, 0, 0, false}, Case{64, 1, 4 * MiB + 1, 0, 0, true}}) {
        FrameParams p = frame(16, 8);
        p.launch_flags = kLaunchDense;
        if (k.present & 1) p.out_rgb = reinterpret_cast<float*>(base[0]);
        if (k.present & 2) p.out_ppm = reinterpret_cast<uint8_t*>(base[1]);
        if (k.present & 4) p.out_face = reinterpret_cast<int32_t*>(base[2]);
        Ring r;
        r.slots = k.slots;
        r.rgb = k.rgb;
        r.ppm = k.ppm;
        r.face = k.face;
        const FrameParams q = ring_frames(p, r, 0, 1);
        uint64_t bytes = 0;
        for (uint32_t s = 0; s < k.slots; ++s) bytes += ((k.present & 1) ? k.rgb : 0) + ((k.present & 2) ? k.ppm : 0) + ((k.present & 4) ? k.face : 0);
        CHECK((bytes > 256 * MiB) == k.beyond, "the case's own sum");
        CHECK(q.launch_flags == (kLaunchDense | (k.beyond ? 1u << 16 : 0u)), "ring of %llu bytes: flags 0x%x", (unsigned long long)bytes,
              q.launch_flags);
    }
}

// ---- the unculled call's rectangle, the aligned predicate
void whole_frame() {
    for (uint32_t W = 1; W <= 130; ++W)
        for (uint32_t rows = 1; rows <= 40; ++rows) {
            FrameParams p = frame(W, rows);
            whole_frame_rect(W, rows, 2, &p);
            uint32_t cols = 0, subrows = 0;  // sub-blocks of 16 x 4 pixels that hold a pixel of the frame
            while (cols * 16 < W) ++cols;
            while (subrows * 4 < rows) ++subrows;
            CHECK(p.nrect == 1 && p.rects[0][0] == 0 && p.rects[0][2] == 0 && p.rects[0][1] == (int32_t)cols - 1 &&
                      p.rects[0][3] == (int32_t)subrows - 1 && p.total_sub == cols * subrows, "%u x %u: rectangle", W, rows);
            FrameParams e = frame(W, rows);
            whole_frame_rect(W, rows, 0, &e);
            CHECK(e.nrect == 0 && e.total_sub == 0, "no objects: no rectangle");
        }
    char* const a = reinterpret_cast<char*>(uintptr_t(1) << 20);
    for (uint32_t w = 1; w <= 64; ++w)
        for (int off = 0; off < 3 * 17; ++off) {
            const int o[3] = {off / 17 == 0 ? off % 17 : 0, off / 17 == 1 ? off % 17 : 0, off / 17 == 2 ? off % 17 : 0};
            const bool want = w % 16 == 0 && o[0] % 16 == 0 && o[1] % 16 == 0 && o[2] % 16 == 0;
            CHECK(rows_aligned(w, 8, a + o[0], a + o[1], a + o[2]) == want, "width %u offsets %d %d %d", w, o[0], o[1], o[2]);
        }
    CHECK(rows_aligned(16, 8, nullptr, nullptr, nullptr), "absent outputs are aligned");
    // the largest output's byte offsets stay within 32 bits: rows x width x 12 < 2^32
    CHECK(rows_aligned(16384, 21845, a, a, a) && !rows_aligned(16384, 21846, a, a, a), "32-bit offsets");
}
}  // namespace

int main() {
    banded_rows();
    contiguous_rows();
    image_fit();
    ring_arguments();
    frames_in_flight();
    coverage();
    ring_pointers();
    whole_frame();
    std::printf("frame_plan: %ld checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
