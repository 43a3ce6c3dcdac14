// sor_model.hpp -- the summation arithmetic of pcl::StatisticalOutlierRemoval<PointXYZ>::
// applyFilterIndices (PCL 1.8 filters/impl/statistical_outlier_removal.hpp restated from memory:
// parity unpinned), for the host and the device alike: one definition of the literal
// loops, of the certificate that lets a sum run in any order, and of the threshold.
//
//   distance of an entry:  double s = 0; s += (double)term[k] over the mean_k terms
//                          sqrtf(d2[k]) in ascending order; (float)(s / (double)mean_k)
//   statistics:            double sum = 0, sq = 0 over the list in order:
//                          sum += (double)d; sq += (double)(d * d)   (a float product)
//   threshold:             mean = sum / valid; var = (sq - sum * sum / valid) / (valid - 1);
//                          mean + mul * sqrt(var), all double, nothing contracted
//
// The certificate.  The terms are non-negative floats.  Let Q = 2^q be the weight of the lowest
// set bit over the non-zero terms: every term is an integer multiple of Q.  If the integer sum of
// term / Q over all the terms is below 2^53, every partial sum of every subset is a multiple of Q
// below 2^53 Q, hence a double: no addition of the chain rounds, in any order, and a parallel
// reduction gives the bits of the literal loop.  A non-finite term fails it.
// Plain C++ without HIP too (tests/cpp/sor_model_san.cpp); build with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_math.hpp"  // DLG_HD

namespace dlg {

constexpr int kSorMaxMeanK = 255;
constexpr int kSorNoExp = 1 << 20;  // lowest-bit exponent of "no non-zero term yet"

DLG_HD inline uint32_t sor_bits(float t) {
  uint32_t u;
  memcpy(&u, &t, 4);
  return u;
}

// a finite float t >= 0 as sig * 2^exp (sig < 2^24; zero: sig 0)
DLG_HD inline void sor_decompose(float t, uint32_t* sig, int* exp) {
  const uint32_t u = sor_bits(t) & 0x7fffffffu;
  const uint32_t e = u >> 23, m = u & 0x7fffffu;
  *sig = e ? (m | 0x800000u) : m;
  *exp = (e ? (int)e : 1) - 150;
}

DLG_HD inline bool sor_finite(float t) { return (sor_bits(t) & 0x7f800000u) != 0x7f800000u; }

// the exponent of t's lowest set bit (kSorNoExp for zero; t finite)
DLG_HD inline int sor_low_exp(float t) {
  uint32_t sig;
  int exp;
  sor_decompose(t, &sig, &exp);
  return sig ? exp + __builtin_ctz(sig) : kSorNoExp;
}

// t / 2^q as an integer (q <= t's lowest-bit exponent); false when it reaches 2^53 (then *units
// is not written)
DLG_HD inline bool sor_units(float t, int q, uint64_t* units) {
  uint32_t sig;
  int exp;
  sor_decompose(t, &sig, &exp);
  if (!sig) { *units = 0; return true; }
  const int z = __builtin_ctz(sig);
  const int sh = exp + z - q;  // >= 0
  if (sh >= 53) return false;
  // odd * 2^sh < 2^53 exactly when odd < 2^(53 - sh); tested before the shift, which could
  // otherwise drop high bits (odd has up to 24 bits, sh up to 52) and pass a wrong count
  const uint64_t odd = sig >> z;
  if (odd >> (53 - sh)) return false;
  *units = odd << sh;
  return true;
}

// one step of a literal chain
DLG_HD inline double sor_chain(double acc, float t) { return acc + (double)t; }
// the float square of the statistics loop
DLG_HD inline float sor_square(float d) { return d * d; }
DLG_HD inline float sor_distance(double dist_sum, int mean_k) {
  return (float)(dist_sum / (double)mean_k);
}

// the literal loop over terms[0..n)
DLG_HD inline double sor_literal_sum(const float* terms, int64_t n) {
  double s = 0.0;
  for (int64_t i = 0; i < n; ++i) s = sor_chain(s, terms[i]);
  return s;
}

// the certificate over terms[0..n) (n < 2^31): true when the sum is order-independent; *q_out =
// the unit's exponent, *units_out = the exact sum in units (the sum itself is units * 2^q)
DLG_HD inline bool sor_certify(const float* terms, int64_t n, int* q_out, uint64_t* units_out) {
  int q = kSorNoExp;
  for (int64_t i = 0; i < n; ++i) {
    if (!sor_finite(terms[i])) return false;
    const int e = sor_low_exp(terms[i]);
    q = e < q ? e : q;
  }
  // hi / lo halves: 2^31 terms below 2^53 cannot overflow either
  uint64_t lo = 0, hi = 0;
  for (int64_t i = 0; i < n; ++i) {
    uint64_t u;
    if (!sor_units(terms[i], q, &u)) return false;
    lo += u & 0xffffffffu;
    hi += u >> 32;
  }
  hi += lo >> 32;
  lo &= 0xffffffffu;
  if (hi >> 21) return false;  // hi * 2^32 + lo >= 2^53
  *q_out = q == kSorNoExp ? 0 : q;
  *units_out = (hi << 32) | lo;
  return true;
}

// units * 2^q, exact (units < 2^53, q >= -149)
DLG_HD inline double sor_from_units(uint64_t units, int q) { return ldexp((double)units, q); }

struct SorThreshold {
  double mean, variance, stddev, threshold;
};
DLG_HD inline SorThreshold sor_threshold(double sum, double sq_sum, int64_t valid, double mul) {
  SorThreshold t;
  t.mean = sum / (double)valid;
  t.variance = (sq_sum - sum * sum / (double)valid) / ((double)valid - 1.0);
  t.stddev = sqrt(t.variance);
  t.threshold = t.mean + mul * t.stddev;
  return t;
}

// 1: entry removed
DLG_HD inline bool sor_removed(float d, double threshold, bool negative) {
  return negative ? (double)d <= threshold : (double)d > threshold;
}

}  // namespace dlg
