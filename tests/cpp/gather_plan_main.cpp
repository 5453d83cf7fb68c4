// Stand-alone checker of the multi-GPU gather's planning (eray_amd/csrc/gather_plan.hpp, the
// header comm.cpp and its kernels plan with): plain host code, no library to link, meant for the
// host sanitizers and a machine without a GPU:
//
//   g++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tests/cpp/gather_plan_main.cpp -o /tmp/gather_plan && /tmp/gather_plan
//
// Schedules (the conditions of tests/test_dist_rows.py test_gather_schedules_pair_up, for N = 1..8
// and for 63 and 64 ranks, rotating roots and not, some ranks without bytes): each send meets
// exactly one receive of the same size, the packs do not overlap and lie inside the buffer, each
// rank assembles the frames its rotation gives it, the sent bytes are the packs plus one 16-B
// header per transfer, and the headers written are one per send group plus one for a root — never
// more than HeaderSpots holds, and every header a root reads lies inside its buffer.
// Layouts (my_rects / layout_of / rank_table): 0, 1, 8, 9 and 20 rectangles (more than kPlanRects
// merge into the last), rectangles off every edge of the frame, empty ones, band splits whose
// last band is short — at most kPlanRects rectangles, all inside the rank's rows and the frame's
// column groups, disjoint, covering every pixel of the objects' rectangles in the rank's rows, and
// bytes = the sum of row_bytes x rows.
#include <cstdint>
#include <cstdio>
#include <utility>
#include <vector>

#include "../../eray_amd/csrc/gather_plan.hpp"

namespace {
int g_failed = 0;
#define CHECK(cond, ...)                                  \
    do {                                                  \
        if (!(cond)) {                                    \
            ++g_failed;                                   \
            std::printf("FAILED %s:%d %s  ", __FILE__, __LINE__, #cond); \
            std::printf(__VA_ARGS__);                     \
            std::printf("\n");                            \
        }                                                 \
    } while (0)

uint64_t g_seed = 0x9e3779b97f4a7c15ull;
uint32_t rnd(uint32_t n) {  // [0, n)
    g_seed = g_seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)((g_seed >> 33) % n);
}

// One batch: every rank's schedule for packs of nb[q] bytes per frame.
void check_schedules(const std::vector<uint32_t>& nb, uint32_t B, bool rotate) {
    const uint32_t N = (uint32_t)nb.size();
    std::vector<RankLayout> ranks(N, RankLayout{});
    for (uint32_t q = 0; q < N; ++q) ranks[q].bytes = nb[q];
    const uint64_t total = place_ranks(ranks);
    uint64_t sum = 0;
    for (uint32_t q = 0; q < N; ++q) {
        CHECK(ranks[q].off == sum, "N %u rank %u", N, q);
        sum += nb[q];
    }
    CHECK(total == sum, "N %u", N);
    std::vector<Schedule> S;
    for (uint32_t r = 0; r < N; ++r) S.push_back(schedule(ranks, total, r, B, rotate));
    for (uint32_t r = 0; r < N; ++r) {
        const Schedule& s = S[r];
        uint32_t mine = 0;
        for (uint32_t k = 0; k < B; ++k) mine += (rotate ? k % N : 0u) == r;
        CHECK(s.mine == mine, "N %u B %u rotate %d rank %u: mine %u", N, B, (int)rotate, r, s.mine);
        // where the pack kernel puts frame k (gather_pack_kernel's `out`)
        std::vector<std::pair<uint64_t, uint64_t>> spans;
        for (uint32_t k = 0; k < B; ++k) {
            const uint32_t root = s.R.root(k);
            const uint64_t off = root == r ? s.own + (uint64_t)s.R.index(k) * nb[r]
                                           : s.send_base + (uint64_t)s.R.send_slot(k, r) * nb[r] +
                                                 (nb[r] ? kHdr * s.R.group(root, r) : 0);
            spans.push_back({off, off + nb[r]});
        }
        std::sort(spans.begin(), spans.end());
        for (size_t i = 0; i + 1 < spans.size(); ++i)
            CHECK(spans[i].second <= spans[i + 1].first, "N %u B %u rotate %d rank %u: packs overlap", N, B, (int)rotate, r);
        CHECK(spans.empty() || spans.back().second <= s.need, "N %u B %u rotate %d rank %u: pack past need", N, B,
              (int)rotate, r);
        uint64_t sent = 0;
        uint32_t sends = 0;
        for (const Xfer& x : s.ops) {
            CHECK(x.peer < N && x.peer != r, "N %u B %u rank %u: peer %u", N, B, r, x.peer);
            CHECK(x.off + x.bytes <= s.need, "N %u B %u rotate %d rank %u: transfer past need", N, B, (int)rotate, r);
            if (!x.send || x.peer >= N) continue;
            ++sends;
            sent += x.bytes;
            uint32_t met = 0;
            size_t bytes = 0;
            for (const Xfer& y : S[x.peer].ops)
                if (!y.send && y.peer == r) {
                    ++met;
                    bytes = y.bytes;
                }
            CHECK(met == 1 && bytes == x.bytes, "N %u B %u rotate %d rank %u -> %u: %u receives", N, B, (int)rotate, r,
                  x.peer, met);
        }
        for (const Xfer& x : s.ops) {  // ... and each receive one send
            if (x.send || x.peer >= N) continue;
            uint32_t met = 0;
            for (const Xfer& y : S[x.peer].ops) met += y.send && y.peer == r && y.bytes == x.bytes;
            CHECK(met == 1, "N %u B %u rotate %d rank %u <- %u: %u sends", N, B, (int)rotate, r, x.peer, met);
        }
        CHECK(sent == (uint64_t)nb[r] * (B - s.mine) + kHdr * sends, "N %u B %u rotate %d rank %u: sent bytes", N, B,
              (int)rotate, r);
        CHECK(s.hdr.n == sends + (s.mine ? 1u : 0u), "N %u B %u rotate %d rank %u: %u headers", N, B, (int)rotate, r, s.hdr.n);
        CHECK(s.hdr.n <= (uint32_t)kMaxCodedRanks + 1u, "N %u B %u rank %u: %u headers", N, B, r, s.hdr.n);
        for (uint32_t i = 0; i < s.hdr.n && i <= (uint32_t)kMaxCodedRanks; ++i)
            CHECK(s.hdr.off[i] + kHdr <= s.need, "N %u B %u rotate %d rank %u: header %u past need", N, B, (int)rotate, r, i);
        CHECK(s.peer_hdr.size() == N, "N %u", N);
        for (uint32_t q = 0; q < N && q < s.peer_hdr.size(); ++q) {
            CHECK((s.peer_hdr[q] != ~0ull) == (s.mine && nb[q]), "N %u B %u rotate %d rank %u: peer header %u", N, B,
                  (int)rotate, r, q);
            if (s.peer_hdr[q] != ~0ull)
                CHECK(s.peer_hdr[q] + kHdr <= s.need, "N %u B %u rotate %d rank %u: peer header %u past need", N, B,
                      (int)rotate, r, q);
        }
    }
}

void schedule_cases() {
    for (uint32_t N = 1; N <= 8; ++N)
        for (uint32_t B : {1u, 2u, 3u, 7u, 8u, 12u})
            for (int rotate = 0; rotate < 2; ++rotate) {
                std::vector<uint32_t> nb(N);
                for (auto& b : nb) b = 48u * rnd(40);
                check_schedules(nb, B, rotate != 0);
            }
    for (uint32_t N : {63u, (uint32_t)kMaxCodedRanks})
        for (uint32_t B : {1u, 63u, 64u, 65u, 129u})
            for (int rotate = 0; rotate < 2; ++rotate)
                for (int zeros = 0; zeros < 3; ++zeros) {  // no rank, every third, all but one without bytes
                    std::vector<uint32_t> nb(N);
                    for (uint32_t q = 0; q < N; ++q) {
                        nb[q] = 48u * (1u + rnd(40));
                        if ((zeros == 1 && q % 3 == 1) || (zeros == 2 && q != N / 2)) nb[q] = 0;
                    }
                    check_schedules(nb, B, rotate != 0);
                }
}

// One rank's layout of `rects` (x0, x1, y0, y1; camera rows) in the split (H, band, N).
void check_layout(const std::vector<std::array<int32_t, 4>>& rects, uint32_t H, uint32_t W, uint32_t band, uint32_t N,
                  uint32_t rank) {
    const RankRows rr = rank_rows(H, band, N, rank);
    const std::vector<std::array<int32_t, 4>> mine = my_rects(rects, rr, W);
    CHECK(mine.size() <= (size_t)kPlanRects, "%zu rectangles", mine.size());
    int32_t rec[kXchgInts - kXchgHead] = {};
    if (mine.size() > (size_t)kPlanRects) return;  // (write_rects would leave the record)
    write_rects(mine, rec);
    const RankLayout L = layout_of(rec, rr.rows);
    CHECK(L.nrect == mine.size() && L.nrect <= (uint32_t)kPlanRects && L.rows == rr.rows, "nrect %u", L.nrect);
    uint64_t bytes = 0, rows = 0;
    for (uint32_t i = 0; i < L.nrect; ++i) {
        const GatherRect& g = L.r[i];
        CHECK(0 <= g.l0 && g.l0 <= g.l1 && g.l1 < (int32_t)rr.rows, "H %u band %u N %u rank %u: rows [%d, %d] of %u", H, band,
              N, rank, g.l0, g.l1, rr.rows);
        CHECK(0 <= g.c0 && g.c0 <= g.c1 && g.c1 < (int32_t)(W / 16), "columns [%d, %d]", g.c0, g.c1);
        CHECK(g.row_bytes == 48u * (uint32_t)(g.c1 - g.c0 + 1) && g.off == bytes && g.first == rows, "rectangle %u", i);
        rows += (uint64_t)(g.l1 - g.l0 + 1);
        bytes += (uint64_t)g.row_bytes * (uint64_t)(g.l1 - g.l0 + 1);
        for (uint32_t j = 0; j < i; ++j) {
            const GatherRect& o = L.r[j];
            CHECK(g.l0 > o.l1 || o.l0 > g.l1 || g.c0 > o.c1 || o.c0 > g.c1, "rectangles %u and %u overlap", j, i);
        }
    }
    CHECK(L.bytes == bytes && L.packed_rows == rows, "bytes %u rows %u", L.bytes, L.packed_rows);
    // every pixel of an object's rectangle in one of this rank's rows lies in a rectangle of the layout
    const uint32_t mask = band ? band - 1u : 0x7fffffffu;
    for (uint32_t j = 0; j < rr.rows; ++j) {
        const int32_t y = (int32_t)eray::gpu::band_camera_row(rr.row0, rr.shift, mask, rr.stride, j);
        CHECK(y >= 0 && y < (int32_t)H, "local row %u is camera row %d", j, y);
        for (const auto& q : rects) {
            if (q[0] > q[1] || y < q[2] || y > q[3]) continue;
            for (int32_t x = std::max(q[0], 0); x <= std::min(q[1], (int32_t)W - 1); ++x) {
                bool in = false;
                for (uint32_t i = 0; i < L.nrect; ++i)
                    in |= (int32_t)j >= L.r[i].l0 && (int32_t)j <= L.r[i].l1 && x / 16 >= L.r[i].c0 && x / 16 <= L.r[i].c1;
                CHECK(in, "H %u band %u N %u rank %u: pixel (%d, %d) of local row %u is in no rectangle", H, band, N, rank, x, y, j);
                if (!in) return;
            }
        }
    }
}

void layout_cases() {
    struct Split {
        uint32_t H, W, band, N;
    };
    // blocks; bands that divide the rows; bands whose last band is short (100 = 12 x 8 + 4, 37 = 9 x 4 + 1)
    const Split splits[] = {{96, 128, 0, 1}, {96, 128, 0, 4}, {96, 64, 8, 3}, {100, 128, 8, 3},
                            {37, 48, 4, 5},  {100, 96, 16, 7}, {20, 32, 32, 2}, {64, 1024, 4, 8}};
    for (const Split& sp : splits) {
        CHECK(row_split_ok(sp.H, sp.band, sp.N), "split %u %u %u", sp.H, sp.band, sp.N);
        uint32_t rows = 0;
        for (uint32_t r = 0; r < sp.N; ++r) rows += rank_rows(sp.H, sp.band, sp.N, r).rows;
        CHECK(rows == sp.H, "H %u band %u N %u: the ranks hold %u rows", sp.H, sp.band, sp.N, rows);
        const int32_t H = (int32_t)sp.H, W = (int32_t)sp.W;
        for (uint32_t count : {0u, 1u, 8u, 9u, 20u})
            for (int shape = 0; shape < 3; ++shape) {
                std::vector<std::array<int32_t, 4>> rects;
                for (uint32_t i = 0; i < count; ++i) {
                    int32_t x0, x1, y0, y1;
                    if (shape == 0) {  // small, mostly apart, inside the frame
                        x0 = (int32_t)rnd(sp.W);
                        x1 = std::min(x0 + (int32_t)rnd(20), W - 1);
                        y0 = (int32_t)rnd(sp.H);
                        y1 = std::min(y0 + (int32_t)rnd(6), H - 1);
                    } else {  // any size, off every edge of the frame; every fourth one empty
                        x0 = (int32_t)rnd(sp.W + 100) - 50;
                        x1 = x0 + (int32_t)rnd(sp.W);
                        y0 = (int32_t)rnd(sp.H + 100) - 50;
                        y1 = y0 + (int32_t)rnd(sp.H);
                        if (shape == 2 && i % 4 == 1) x0 = x1 + 1;
                        if (shape == 2 && i % 4 == 3) y0 = y1 + 1 + (int32_t)rnd(3);
                    }
                    rects.push_back({x0, x1, y0, y1});
                }
                if (shape == 2 && count >= 8) {  // one past each edge, and one wholly outside
                    rects[0] = {-30, 5, -30, 5};
                    rects[1] = {W - 5, W + 30, H - 5, H + 30};
                    rects[2] = {-9, W + 9, H / 2, H / 2};
                    rects[3] = {W / 2, W / 2, -9, H + 9};
                    rects[4] = {W, W + 10, 0, H - 1};
                    rects[5] = {0, W - 1, H, H + 10};
                    rects[6] = {-10, -1, -10, -1};
                }
                for (uint32_t r = 0; r < sp.N; ++r) check_layout(rects, sp.H, sp.W, sp.band, sp.N, r);
                // the plan's table from every rank's record
                constexpr size_t kRec = kXchgInts - kXchgHead;
                std::vector<int32_t> recs(kRec * sp.N, 0);
                for (uint32_t r = 0; r < sp.N; ++r)
                    write_rects(my_rects(rects, rank_rows(sp.H, sp.band, sp.N, r), sp.W), recs.data() + kRec * r);
                std::vector<RankLayout> table(sp.N);
                const uint64_t total = rank_table(recs.data(), kRec, sp.H, sp.band, &table);
                uint64_t sum = 0;
                for (uint32_t r = 0; r < sp.N; ++r) {
                    CHECK(table[r].off == sum && table[r].rows == rank_rows(sp.H, sp.band, sp.N, r).rows, "table rank %u", r);
                    sum += table[r].bytes;
                }
                CHECK(total == sum, "table total");
                check_schedules([&] {
                    std::vector<uint32_t> nb;
                    for (const RankLayout& R : table) nb.push_back(R.bytes);
                    return nb;
                }(), 5, shape != 0);
            }
    }
    CHECK(!row_split_ok(96, 3, 2) && !row_split_ok(96, 12, 2) && !row_split_ok(96, 2, 2) && !row_split_ok(97, 0, 2) &&
              row_split_ok(97, 4, 2) && row_split_ok(97, 0, 1),
          "row_split_ok");
}

void verdict_cases() {
    const uint32_t N = 5;
    std::vector<int32_t> all((size_t)kXchgInts * N, 0);
    auto rec = [&](uint32_t q) { return all.data() + (size_t)q * kXchgInts; };
    for (uint32_t q = 0; q < N; ++q) rec(q)[1] = 1, rec(q)[2] = 77, rec(q)[3] = 5;
    int failed = 9;
    CHECK(plan_verdict(all.data(), N, ERAY_OK, rec(2), &failed) == ERAY_OK && failed == -1, "all accept");
    rec(3)[0] = ERAY_E_OUT_OF_MEMORY;
    rec(4)[0] = ERAY_E_HIP;
    CHECK(plan_verdict(all.data(), N, ERAY_OK, rec(0), &failed) == ERAY_E_OUT_OF_MEMORY && failed == 3, "the first failure");
    CHECK(plan_verdict(all.data(), N, ERAY_E_HIP, rec(4), &failed) == ERAY_E_HIP && failed == -1, "its own failure");
    rec(3)[0] = rec(4)[0] = ERAY_OK;
    rec(1)[2] = 78;
    CHECK(plan_verdict(all.data(), N, ERAY_OK, rec(0), &failed) == ERAY_E_INVALID_ARGUMENT && failed == -1, "another source");
    CHECK(gather_replan(false, 1, 7, 1, 7) && !gather_replan(true, 1, 7, 1, 7) && gather_replan(true, 1, 7, 1, 8) &&
              gather_replan(true, 1, 7, 2, 7),
          "gather_replan");
    const XferHeader h{0, 2, 0x89abcdefu, 0x01234567u};
    CHECK(header_ok(h, 2, 0x0123456789abcdefull) && !header_ok(h, 1, 0x0123456789abcdefull) &&
              !header_ok(h, 2, 0x0123456789abcdeeull) && !header_ok(XferHeader{1, 2, 0x89abcdefu, 0x01234567u}, 2, 0x0123456789abcdefull),
          "header_ok");
}
}  // namespace

int main() {
    schedule_cases();
    layout_cases();
    verdict_cases();
    std::printf("gather_plan: %d failed checks\n", g_failed);
    return g_failed ? 1 : 0;
}
