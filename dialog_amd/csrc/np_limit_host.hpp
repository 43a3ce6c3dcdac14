// np_limit_host.hpp -- the NORMAL_PLANE prefilter limit on the host (no HIP: also compiled alone
// by tests/cpp/np_limit_host.cpp and checked there against its brute-force definition).
#pragma once

#include <cmath>

namespace dlg {

// np_de_limit (np_dev.hpp) restated for the host: the smallest float lim with
// fl((1 - w) lim) >= thr as a double product; +inf when the prefilter does not apply (w < 0 or
// NaN, 1 - w <= 0), 0 for thr <= 0 (nothing passes), NaN for a NaN thr.  For 0 <= w < 1 it is
// finite or +inf and monotone non-decreasing in w, so the limit of the cloud's largest w bounds
// every point's (make_plan takes it for the prune margin).
inline float np_lim_max(double w, double thr) {
  if (!(w >= 0.0)) return INFINITY;
  const double omw = 1.0 - w;
  if (!(omw > 0.0)) return INFINITY;
  if (!(thr > 0.0)) return thr == thr ? 0.0f : NAN;
  float x = (float)(thr / omw);
  if (!(x == x)) return INFINITY;
  while (!(omw * (double)x >= thr) && x < INFINITY) x = std::nextafter(x, INFINITY);
  while (x > 0.0f) {
    const float y = std::nextafter(x, -INFINITY);
    if (omw * (double)y >= thr) x = y;
    else break;
  }
  return x;
}

}  // namespace dlg
