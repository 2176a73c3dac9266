// What the estimators that bin |k| share (fb_power.hip, fb_bispec.hip): exact shell membership of a mode, the fp64 k^2 of a
// mode without contraction, the checks on a set of k edges and the fundamental wavenumbers of the box; and FB_TWO_PI, which
// fb_field_kernels.h and fb_api.hip take from here as well.
#pragma once
#include "fb_plan.h"
#include "fb_api_util.h"
#include <cmath>

#define FB_TWO_PI 6.283185307179586       // the double 2 * np.pi: the library's one literal of it beside fb_cola.hip's kTwoPi

namespace fb {

// the least double x >= 0 with sqrt(x) >= e (sqrt correctly rounded, as on the device and in numpy):
// np.digitize(sqrt(k2), e) = #{b : sq_threshold(e_b) <= k2}, decided without forming the root
inline double sq_threshold(double e) {
    if (e <= 0.0) return 0.0;
    double x = e * e;
    while (!(std::sqrt(x) >= e)) x = std::nextafter(x, INFINITY);
    for (;;) {
        const double d = std::nextafter(x, 0.0);
        if (x > 0.0 && std::sqrt(d) >= e) x = d; else break;
    }
    return x;
}

// k_perp^2 = a^2 + b^2 and k^2 = s + c^2 as numpy rounds them: every product and sum once, no fused multiply-add
__device__ __forceinline__ double sq2(double a, double b) {
#pragma clang fp contract(off)
    return a * a + b * b;
}
__device__ __forceinline__ double add_sq(double s, double c) {
#pragma clang fp contract(off)
    return s + c * c;
}

// kedges[0..n]: n bins.  The last edge may be inf.
inline int kshell_check_edges(const double* kedges, int n) {
    FB_REQUIRE(kedges[0] >= 0.0, "the first k edge must be >= 0");
    for (int q = 0; q < n; ++q) FB_REQUIRE(std::isfinite(kedges[q]), "k edges must be finite (the last may be inf)");
    for (int q = 1; q <= n; ++q) FB_REQUIRE(kedges[q] > kedges[q - 1], "k edges must be strictly ascending");
    return FB_OK;
}
// kf[a] = 2 * np.pi / L_a
inline void fill_kf(const fb_plan* p, double (&kf)[3]) {
    for (int q = 0; q < 3; ++q) kf[q] = FB_TWO_PI / p->L[q];
}

}  // namespace fb
