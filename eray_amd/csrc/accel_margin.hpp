// accel_margin.hpp — the per-face margin of the ray-query hierarchy (the derivation is in
// accel_build.hpp) and the rounding `up`, for the host and the device alike: accel_build.cpp calls
// them per face on the CPU, accel_dev.hip one face per lane in FP64.  Every operation is a
// correctly rounded IEEE double operation (+ - * / sqrt, no fused multiply-add: the build sets
// -ffp-contract=off), so both sides decide culled / unculled alike and get the same alpha, beta,
// gamma bits.
#pragma once

#include <float.h>
#include <math.h>
#include <stdint.h>

#include "accel_walk.hpp"

namespace eray {
namespace accel {

constexpr double kAlphaMax = 0.25;

struct FaceMargin {
    double alpha, beta, gamma, kappa;
    bool culled;  // false: the face belongs to the unculled list
};

namespace margin {
constexpr double kU = 0x1p-24;
constexpr double kDetShare = 0.2e-6;  // kappa |d|inf may reach this much of the 1e-6 threshold
constexpr double kDetFloor = 0.75e-6;
constexpr double kMarginMax = 1e30;

struct V3 {
    double x, y, z;
};
ERAY_HD double n1(V3 v) { return ::fabs(v.x) + ::fabs(v.y) + ::fabs(v.z); }
ERAY_HD double n2(V3 v) { return ::sqrt(v.x * v.x + v.y * v.y + v.z * v.z); }
ERAY_HD bool finite(double x) { return ::fabs(x) <= DBL_MAX; }  // (NaN fails)
}  // namespace margin

// the smallest float >= x (x finite, >= 0), one step further for the double arithmetic before it
ERAY_HD float up(double x) {
    float f = (float)x;
    if ((double)f < x) f = ::nextafterf(f, INFINITY);
    return ::nextafterf(f, INFINITY);
}

// The margins of one face record (accel_build.hpp steps 1-5) and whether it may go under the tree.
ERAY_HD FaceMargin face_margin_of(const Hot& r) {
    using namespace margin;
    FaceMargin m{0.0, 0.0, 0.0, 0.0, false};
    bool fin = true;
    for (int k = 0; k < 12; ++k) fin = fin && ::fabsf(r.q[k]) <= FLT_MAX;
    if (!fin) return m;
    const V3 e1 = {r.q[0], r.q[1], r.q[2]}, e2 = {r.q[3], r.q[4], r.q[5]}, n = {r.q[6], r.q[7], r.q[8]},
             a = {r.q[9], r.q[10], r.q[11]};
    const V3 N = {e1.y * e2.z - e1.z * e2.y, e1.z * e2.x - e1.x * e2.z, e1.x * e2.y - e1.y * e2.x};
    const double dn = n1({n.x - N.x, n.y - N.y, n.z - N.z});
    const double E1 = n2(e1), E2 = n2(e2);
    m.kappa = 2.01 * kU * n1(n) + 1.001 * dn + 1e-30;
    m.alpha = 8.0 * kU * (n1(e2) * E1 + n1(e1) * E2) / kDetFloor;
    m.beta = 1.001 * m.kappa * (E1 + E2) / kDetFloor + m.alpha * n1(a);
    m.gamma = 5.2 * kU * (E1 + E2) + 1e-30;
    m.culled = m.kappa <= 1.9 * m.alpha * kDetShare && m.alpha <= kAlphaMax && finite(m.alpha) && finite(m.beta) &&
               finite(m.gamma) && m.alpha <= kMarginMax && m.beta <= kMarginMax && m.gamma <= kMarginMax;
    return m;
}

}  // namespace accel
}  // namespace eray
