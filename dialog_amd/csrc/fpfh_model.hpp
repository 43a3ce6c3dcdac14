// fpfh_model.hpp -- the arithmetic of pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33>
// (PCL 1.8 features/impl/fpfh.hpp and pfh_tools' computePairFeatures, restated from memory: parity
// unpinned), for the host and the device alike.  All float unless marked double; build
// with -ffp-contract=off.
//
//   pair (p, n_p, q, n_q): d = q - p, f4 = sqrt((dx^2 + dy^2) + dz^2), 0: the pair fails;
//   a1 = (n_p . d) / f4, a2 = (n_q . d) / f4 (dots summed left to right);
//   acos(|a1|) > acos(|a2|): u = n_q, t = n_p, d = -d, f3 = -a2; else u = n_p, t = n_q, f3 = a1;
//   v = d x u, |v| = sqrt(its squared norm), 0: the pair fails; v /= |v|; w = u x v;
//   f2 = v . t, f1 = atan2(w . t, u . t).
//   acos and atan2 are the correctly rounded floats of the real functions; here the double
//   function's value cast to float, which differs only where the double value lies within its own
//   error of a float rounding boundary (tests/fpfh_ref.py marks those pairs unstable).
//   bins (double, d_pi = 1.0f / (2.0f * float(M_PI))): floor(11 ((f1 + M_PI) d_pi)),
//   floor(11 ((f2 + 1.0) 0.5)), floor(11 ((f3 + 1.0) 0.5)), each clamped to 0..10 (a NaN: bin 0).
//   SPFH bin = the c-fold sequential float sum of incr = 100.0f / float(m - 1), c = the pairs of the
//   point's m neighbours (itself excluded by index) that fell into the bin.
//   FPFH: the neighbours in (d2, index) order, those with d2 == 0 skipped; w = 1.0f / d2, val =
//   spfh[nbr][b] * w, hist[b] += val (float), sum_g += val (double), neighbour-major, bin-minor;
//   then hist[b] *= (float)(100.0 / sum_g) for every g with sum_g != 0.
//
// Plain C++ without HIP too (tests/cpp/fpfh_model_san.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "host_math.hpp"  // DLG_HD

namespace dlg {

constexpr int kFpfhBins = 11;
constexpr int kFpfhDim = 33;

DLG_HD inline bool fpfh_finite(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}
DLG_HD inline bool fpfh_finite3(float x, float y, float z) {
  return fpfh_finite(x) && fpfh_finite(y) && fpfh_finite(z);
}

DLG_HD inline float fpfh_acos(float x) { return (float)acos((double)x); }
DLG_HD inline float fpfh_atan2(float y, float x) { return (float)atan2((double)y, (double)x); }

// computePairFeatures; false: the pair fails (f[] = f1, f2, f3 unset)
DLG_HD inline bool fpfh_pair(const float p[3], const float np[3], const float q[3],
                             const float nq[3], float f[3]) {
  float d[3] = {q[0] - p[0], q[1] - p[1], q[2] - p[2]};
  const float f4 = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  if (f4 == 0.0f) return false;
  const float a1 = ((np[0] * d[0] + np[1] * d[1]) + np[2] * d[2]) / f4;
  const float a2 = ((nq[0] * d[0] + nq[1] * d[1]) + nq[2] * d[2]) / f4;
  const bool sw = fpfh_acos(fabsf(a1)) > fpfh_acos(fabsf(a2));
  float u[3], t[3];
  for (int k = 0; k < 3; ++k) {
    u[k] = sw ? nq[k] : np[k];
    t[k] = sw ? np[k] : nq[k];
    d[k] = sw ? -d[k] : d[k];
  }
  const float f3 = sw ? -a2 : a1;
  float v[3] = {d[1] * u[2] - d[2] * u[1], d[2] * u[0] - d[0] * u[2], d[0] * u[1] - d[1] * u[0]};
  const float vn = sqrtf((v[0] * v[0] + v[1] * v[1]) + v[2] * v[2]);
  if (vn == 0.0f) return false;
  v[0] /= vn; v[1] /= vn; v[2] /= vn;
  const float w[3] = {u[1] * v[2] - u[2] * v[1], u[2] * v[0] - u[0] * v[2],
                      u[0] * v[1] - u[1] * v[0]};
  f[1] = (v[0] * t[0] + v[1] * t[1]) + v[2] * t[2];
  const float wt = (w[0] * t[0] + w[1] * t[1]) + w[2] * t[2];
  const float ut = (u[0] * t[0] + u[1] * t[1]) + u[2] * t[2];
  f[0] = fpfh_atan2(wt, ut);
  f[2] = f3;
  return true;
}

DLG_HD inline int fpfh_clamp_bin(double x) {
  const double fl = floor(x);
  return !(fl >= 0.0) ? 0 : (fl > 10.0 ? 10 : (int)fl);
}

// the three bin indices (0..10 each) of a pair's features
DLG_HD inline void fpfh_bins(const float f[3], int b[3]) {
  const float d_pi = 1.0f / (2.0f * 3.14159274101257324f);  // float(M_PI)
  b[0] = fpfh_clamp_bin(11.0 * (((double)f[0] + 3.14159265358979323846) * (double)d_pi));
  b[1] = fpfh_clamp_bin(11.0 * (((double)f[1] + 1.0) * 0.5));
  b[2] = fpfh_clamp_bin(11.0 * (((double)f[2] + 1.0) * 0.5));
}

// a bin's value from its count: hist += incr, c times (m = the point's neighbours, itself included)
DLG_HD inline float fpfh_bin_value(int m, int c) {
  const float incr = 100.0f / (float)(m - 1);
  float s = 0.0f;
  for (int i = 0; i < c; ++i) s = s + incr;
  return s;
}

// ---- the double sums' certificate -------------------------------------------------------------
// A float v > 0 is an odd multiple of 2^lo(v).  If every value a sum takes is a multiple of 2^e and
// the values' total T stays below 2^(e + 53), every partial sum of them, in any order, is a multiple
// of 2^e below 2^(e + 53): a double holds it exactly, so the sum does not depend on the order.
// FpfhCert keeps e = the smallest lo over an entry's values; the test takes the largest of the
// entry's three computed sums for T, with 2^-16 to spare: a computed sum of k < 2^36 non-negative
// doubles is within k 2^-53 < 2^-17 of the real one, so a real total at or above the limit cannot
// pass, and one below it is computed exactly whatever the order -- every implementation takes the
// same decision.
struct FpfhCert {
  int lo = 1 << 20;
  bool bad = false;  // a value that is not finite (or negative): the literal loop
};
DLG_HD inline void fpfh_cert_add(FpfhCert& c, float v) {
  uint32_t b;
  __builtin_memcpy(&b, &v, 4);
  if ((b << 1) == 0u) return;  // (+-0 adds nothing)
  const int e = (int)((b >> 23) & 0xffu);
  if ((b >> 31) || e == 0xff) {
    c.bad = true;
    return;
  }
  const uint32_t mant = e ? ((b & 0x7fffffu) | 0x800000u) : (b & 0x7fffffu);
  const int lo = (e ? e - 150 : -149) + __builtin_ctz(mant);
  c.lo = lo < c.lo ? lo : c.lo;
}
// sum_max = the largest of the entry's three double sums (any order of summation)
DLG_HD inline bool fpfh_cert_holds(const FpfhCert& c, double sum_max) {
  if (c.bad) return false;
  if (c.lo == 1 << 20) return true;  // (no non-zero value)
  return sum_max * (1.0 + 0x1p-16) < ldexp(1.0, c.lo + 53);
}

// the scale of histogram g after the walk: hist[b] *= fpfh_scale(sum_g) where sum_g != 0
DLG_HD inline float fpfh_scale(double sum) { return (float)(100.0 / sum); }

// ---- host restatement: the literal loops (tests/cpp/fpfh_model_san.cpp) -----------------------
// the SPFH counts of point i over its neighbours nbr[0..m) (itself among them); returns the pairs
// that added to the histograms
inline int fpfh_spfh_counts(const float* xyz, const float* nrm, int i, const int32_t* nbr, int m,
                            int32_t counts[kFpfhDim]) {
  for (int b = 0; b < kFpfhDim; ++b) counts[b] = 0;
  int ok = 0;
  const float* np = nrm + 3 * (size_t)i;
  if (!fpfh_finite3(np[0], np[1], np[2])) return 0;
  for (int k = 0; k < m; ++k) {
    const int j = nbr[k];
    if (j == i) continue;
    const float* nq = nrm + 3 * (size_t)j;
    if (!fpfh_finite3(nq[0], nq[1], nq[2])) continue;
    float f[3];
    if (!fpfh_pair(xyz + 3 * (size_t)i, np, xyz + 3 * (size_t)j, nq, f)) continue;
    int b[3];
    fpfh_bins(f, b);
    for (int g = 0; g < 3; ++g) ++counts[kFpfhBins * g + b[g]];
    ++ok;
  }
  return ok;
}

// the weighting loop of one entry over its (d2, index)-ordered neighbours; spfh: rows of 33 floats
// by point; returns whether the certificate held (the sums are the literal ones either way)
inline bool fpfh_weight(const float* spfh, const int32_t* nbr, const float* d2, int m,
                        float hist[kFpfhDim]) {
  double sum[3] = {0.0, 0.0, 0.0};
  FpfhCert cert;
  for (int b = 0; b < kFpfhDim; ++b) hist[b] = 0.0f;
  for (int k = 0; k < m; ++k) {
    if (d2[k] == 0.0f) continue;
    const float w = 1.0f / d2[k];
    const float* row = spfh + (size_t)kFpfhDim * (size_t)nbr[k];
    for (int b = 0; b < kFpfhDim; ++b) {
      const float val = row[b] * w;
      hist[b] = hist[b] + val;
      sum[b / kFpfhBins] = sum[b / kFpfhBins] + (double)val;
      fpfh_cert_add(cert, val);
    }
  }
  for (int g = 0; g < 3; ++g)
    if (sum[g] != 0.0) {
      const float s = fpfh_scale(sum[g]);
      for (int b = 0; b < kFpfhBins; ++b) hist[kFpfhBins * g + b] = hist[kFpfhBins * g + b] * s;
    }
  const double s01 = sum[0] > sum[1] ? sum[0] : sum[1];
  return fpfh_cert_holds(cert, s01 > sum[2] ? s01 : sum[2]);
}

}  // namespace dlg
