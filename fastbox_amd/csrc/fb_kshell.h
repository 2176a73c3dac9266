// Exact shell membership of a mode, shared by the estimators that bin |k| (fb_power.hip, fb_bispec.hip).
#pragma once
#include <cmath>

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

}  // namespace fb
