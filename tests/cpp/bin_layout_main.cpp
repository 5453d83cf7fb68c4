// Stand-alone checker of the screen bins' sizing (eray_amd/csrc/bin_layout.hpp, the header the
// allocation, the launch chain, the setups and the kernels size the bins with): plain host code,
// no library to link, meant for the host sanitizers and a machine without a GPU:
//
//   g++ -std=c++17 -g -Wall -fsanitize=address,undefined -fno-sanitize-recover=undefined
//       tests/cpp/bin_layout_main.cpp -o /tmp/bin_layout && /tmp/bin_layout
//
// Sweeps W in {1, 15, 16, 17, 63, 64, 65, 1920, 65535, 65536}, H in {1, 3, 4, 5, 1080}, phase
// 0..3, rows in {1, 4, 5, H}, nb in {1, 3}, ncam in {1, 16}, cap in {32, 1 << 16} against plain
// restatements: bin row k holds camera rows [phase + 4 (k - 1), phase + 4 k), bin column k pixel
// columns [16 k, 16 k + 16) — every camera row maps to a bin row below bins_y and row H - 1 to
// the last one, every pixel column to a bin column below bins_x, every detail sub-block of the
// rendered rows to a bin below nbins; nsub is a multiple of 4; the finaliser's keys per workgroup
// are a multiple of the workgroup, its grid at most kFinGrid, covering the keys with no idle
// workgroup; the shards' regions fit the capacity.
#include <cstdint>
#include <cstdio>
#include <initializer_list>

#include "../../eray_amd/csrc/bin_layout.hpp"

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

// the bin row whose camera rows [phase + 4 (k - 1), phase + 4 k) hold y, found by counting
uint32_t plain_bin_row(uint32_t y, uint32_t phase) {
    uint32_t k = 0;
    while (y >= phase + 4 * k) ++k;
    return k;
}

void rows_and_columns(uint32_t W, uint32_t H, uint32_t phase) {
    const BinLayout l = bin_layout(1, 1, W, H, phase, frame_tiles_x(W), H, 32, 1);
    for (uint32_t y = 0; y < H; ++y) {
        CHECK(bin_row(y, phase) == plain_bin_row(y, phase), "W %u H %u phase %u row %u", W, H, phase, y);
        CHECK(bin_row(y, phase) < l.bins_y, "W %u H %u phase %u row %u", W, H, phase, y);
    }
    CHECK(bin_row(H - 1, phase) == l.bins_y - 1, "W %u H %u phase %u: %u bin rows", W, H, phase, l.bins_y);
    if (phase) return;  // (the columns do not depend on it)
    for (uint32_t x = 0; x < W; ++x) {
        const uint32_t k = bin_col(x);
        CHECK(16 * k <= x && x < 16 * k + 16 && k < l.bins_x, "W %u column %u: bin column %u of %u", W, x, k, l.bins_x);
    }
    CHECK(bin_col(W - 1) == l.bins_x - 1, "W %u: %u bin columns", W, l.bins_x);
}

// The detail sub-blocks of rendered rows [row0, row0 + rows) (row0 % 4 == phase), as the detail
// kernels enumerate them: sub-block (sx, sy) of 4 * tiles_x per row, camera row row0 + 4 sy.
void sub_blocks(const BinLayout& l, uint32_t W, uint32_t H, uint32_t tiles_x, uint32_t row0, uint32_t rows) {
    CHECK(bin_phase(row0) == l.phase, "row0 %u phase %u", row0, l.phase);
    CHECK(4 * l.subs_y >= rows && 4 * (l.subs_y - 1) < rows, "rows %u: %u sub-block rows", rows, l.subs_y);
    for (uint32_t sy = 0; sy < l.subs_y; ++sy) {
        const uint32_t y0 = band_camera_row(row0, 31u, 0x7fffffffu, 0u, sy * kBinH);
        CHECK(y0 < H, "row0 %u rows %u sy %u", row0, rows, sy);
        for (uint32_t sx = 0; sx < 4 * tiles_x; ++sx) {
            if (sx * kBinW >= W) continue;  // (the padding of the last 64-pixel block)
            const uint32_t bin = bin_row(y0, l.phase) * l.bins_x + sx;
            CHECK(bin < l.nbins, "W %u H %u row0 %u rows %u: sub-block (%u, %u) bin %u of %u", W, H, row0, rows, sx, sy,
                  bin, l.nbins);
        }
    }
}

void sweep() {
    const uint32_t Ws[] = {1, 15, 16, 17, 63, 64, 65, 1920, 65535, 65536}, Hs[] = {1, 3, 4, 5, 1080};
    const size_t caps[] = {32, (size_t)1 << 16};
    for (uint32_t W : Ws)
        for (uint32_t H : Hs)
            for (uint32_t phase = 0; phase < 4; ++phase) {
                rows_and_columns(W, H, phase);
                const uint32_t rows_in[] = {1, 4, 5, H};
                for (uint32_t rows_asked : rows_in)
                    for (uint32_t nb : {1u, 3u})
                        for (uint32_t ncam : {1u, 16u})
                            for (size_t cap : caps) {
                                const uint32_t tiles_x = frame_tiles_x(W);
                                // rendered rows of this phase inside the frame: from the first and from the last such row0
                                const uint32_t first0 = phase < H ? phase : (H - 1) / 4 * 4, rows = rows_asked < H - first0 ? rows_asked : H - first0;
                                const BinLayout l = bin_layout(1000, nb, W, H, phase, tiles_x, rows, cap, ncam);
                                CHECK(l.T == 1000 && l.nb == nb && l.phase == phase && l.cap == cap, "inputs kept");
                                CHECK(l.bins_x * 16 >= W && (l.bins_x - 1) * 16 < W, "W %u: %u bin columns", W, l.bins_x);
                                CHECK(l.nbins == l.bins_x * l.bins_y && l.keys == (size_t)nb * l.nbins, "keys");
                                CHECK(l.nsub % 4 == 0 && l.nsub == (size_t)4 * tiles_x * l.subs_y, "nsub %zu", l.nsub);
                                CHECK(l.dlist_len == l.nsub * ncam && 4 * l.docc_len == l.dlist_len, "detail lists");
                                CHECK(l.part_words >= 10 && l.part_words * kBinWG >= 10 * l.keys, "part words %zu", l.part_words);
                                CHECK(l.fin_per % kBinWG == 0 && l.fin_per >= (uint32_t)kBinWG, "per %u", l.fin_per);
                                CHECK(l.fin_grid >= 1 && l.fin_grid <= kFinGrid, "grid %u", l.fin_grid);
                                CHECK((size_t)l.fin_grid * l.fin_per >= l.keys, "keys %zu: grid %u x per %u", l.keys, l.fin_grid, l.fin_per);
                                CHECK(l.keys == 0 || (size_t)(l.fin_grid - 1) * l.fin_per < l.keys, "keys %zu: grid %u x per %u", l.keys,
                                      l.fin_grid, l.fin_per);
                                CHECK((size_t)l.region * kShards <= cap && ((size_t)l.region + 1) * kShards > cap, "cap %zu region %u", cap,
                                      l.region);
                                if (nb == 1 && ncam == 1 && cap == caps[0]) {
                                    if (phase < H) sub_blocks(l, W, H, tiles_x, first0, rows);
                                    // ... and the last rows of the frame that start a bin of this phase
                                    if (H > phase && (H - phase - 1) / 4 * 4 + phase != first0) {
                                        const uint32_t last0 = (H - phase - 1) / 4 * 4 + phase, rows2 = rows_asked < H - last0 ? rows_asked : H - last0;
                                        sub_blocks(bin_layout(1000, nb, W, H, phase, tiles_x, rows2, cap, ncam), W, H, tiles_x, last0, rows2);
                                    }
                                }
                            }
            }
}
}  // namespace

int main() {
    sweep();
    std::printf("bin_layout: %ld checks, %d failed checks\n", g_checks, g_failed);
    return g_failed ? 1 : 0;
}
