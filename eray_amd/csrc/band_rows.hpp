// band_rows.hpp — rank-local rows and camera rows of a banded render, for the kernels (through
// internal.hpp) and the gather's planning (gather_plan.hpp): no HIP header, so a host compiler takes it.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__)
#define ERAY_HD_PLAIN __host__ __device__  // (no forced inlining: as the functions were declared in place)
#else
#define ERAY_HD_PLAIN
#endif

namespace eray::gpu {

// Camera row of rank-local row j (FrameParams::band_shift; shifts and masks: no division in the
// kernels' per-pixel paths).
ERAY_HD_PLAIN inline uint32_t band_camera_row(uint32_t row0, uint32_t band_shift, uint32_t band_mask,
                                              uint32_t band_stride, uint32_t j) {
    return row0 + (j >> band_shift) * band_stride + (j & band_mask);
}
// The rank-local rows [*lo, *hi] whose camera rows lie in [y0, y1] (empty: *lo > *hi); the
// mapping is monotonic, so a camera row range is a local row range.
ERAY_HD_PLAIN inline void band_local_range(uint32_t row0, uint32_t band_shift, uint32_t band_stride, int32_t y0,
                                          int32_t y1, int32_t* lo, int32_t* hi) {
    if (band_shift >= 31) {
        *lo = y0 - (int32_t)row0;
        *hi = y1 - (int32_t)row0;
        return;
    }
    const int64_t B = (int64_t)1 << band_shift, S = band_stride, off = row0;
    auto floordiv = [](int64_t a, int64_t b) { return a >= 0 ? a / b : -((-a + b - 1) / b); };
    // first local row at or after camera row y0
    int64_t i = floordiv((int64_t)y0 - off, S), w = (int64_t)y0 - off - i * S;
    const int64_t l0 = w < B ? i * B + w : (i + 1) * B;
    // last local row at or before camera row y1
    i = floordiv((int64_t)y1 - off, S);
    w = (int64_t)y1 - off - i * S;
    const int64_t l1 = w < B ? i * B + w : i * B + B - 1;
    *lo = (int32_t)(l0 < -1 ? -1 : (l0 > 0x7fffffff ? 0x7fffffff : l0));
    *hi = (int32_t)(l1 < -1 ? -1 : (l1 > 0x7fffffff ? 0x7fffffff : l1));
}

}  // namespace eray::gpu
