// sacia_model.hpp -- the arithmetic of dlg_sac_ia_align (include/dialog_ransac.h), shared by the
// kernels (sacia.hip), the host driver (sacia_host.cpp) and the host-only test program
// (tests/cpp/sacia_model_san.cpp builds it without HIP); restated in numpy by tests/sac_ia_ref.py.
// pcl::SampleConsensusInitialAlignment of PCL 1.8, restated from memory (parity unpinned,
// DESIGN.md section 2).  Build with -ffp-contract=off.
//
//   rand():            glibc's TYPE_3 additive feedback generator or MSVC's LCG (SaciaRng)
//   getRandomIndex(n): (int)(n * (rand() / (RAND_MAX + 1.0))), in double
//   selectSamples:     sacia_select -- draws until nr_samples are accepted; a draw is rejected when
//                      it equals an accepted index or lies closer than min_sample_distance (float
//                      sqrtf((dx^2 + dy^2) + dz^2)) to an accepted sample; 3 n consecutive
//                      rejections halve the call's own copy of the distance
//   findSimilarFeatures: the k nearest target descriptors in (d, index) order, d = FLANN's L2_Simple
//                      (sacia_feature_d2), then one getRandomIndex(k) picks the rank
//   estimate:          icp_model.hpp's exact moments of the nr_samples pairs, Horn, t = ct - R cs
//                      (sacia_estimate); e = the exponent of the pairs' largest |coordinate|
//   error:             per source point the term e <= thr ? e / thr : 1.0f of its squared distance e
//                      to the nearest target point (a NaN term counts as 1.0f), E = sum of
//                      trunc(term 2^48): an exact integer below 2^79
//   adoption:          in iteration order, a valid hypothesis is adopted when nothing has been
//                      scored yet or its E is strictly below the lowest so far
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "icp_model.hpp"

namespace dlg {

constexpr int kSaciaMaxSamples = 8;
constexpr int kSaciaMaxK = 32;
constexpr int kSaciaDim = 33;
enum { kSaciaRngGlibc = 0, kSaciaRngMsvc = 1 };

// rand() of glibc (TYPE_3: r_i = r_{i-31} + r_{i-3}, the first 310 outputs discarded) or of the
// Visual C++ runtime (s = s 214013 + 2531011, bits 16..30)
struct SaciaRng {
  int kind = kSaciaRngGlibc;
  uint32_t r[34] = {};
  int at = 0;          // glibc: the ring position of r_i
  uint32_t s = 1;      // MSVC
  double denom = 2147483648.0;  // RAND_MAX + 1.0

  void seed(int kind_, uint32_t seed_) {
    kind = kind_;
    if (kind == kSaciaRngMsvc) {
      s = seed_;
      denom = 32768.0;
      return;
    }
    denom = 2147483648.0;
    int64_t w = (int64_t)(int32_t)(seed_ == 0 ? 1u : seed_);
    r[0] = (uint32_t)w;
    for (int i = 1; i < 31; ++i) {
      w = (16807 * w) % 2147483647;
      if (w < 0) w += 2147483647;
      r[i] = (uint32_t)w;
    }
    for (int i = 31; i < 34; ++i) r[i] = r[i - 31];
    at = 0;  // r[at] holds r_{i-34}: the next value replaces it
    for (int i = 34; i < 344; ++i) (void)step();
  }
  uint32_t step() {  // r_i = r_{i-31} + r_{i-3} in a ring of 34
    const uint32_t v = r[(at + 3) % 34] + r[(at + 31) % 34];
    r[at] = v;
    at = (at + 1) % 34;
    return v;
  }
  int next() {
    if (kind == kSaciaRngMsvc) {
      s = s * 214013u + 2531011u;
      return (int)((s >> 16) & 0x7fffu);
    }
    return (int)(step() >> 1);
  }
  int index(int n) { return (int)((double)n * ((double)next() / denom)); }
};

DLG_HD inline bool sacia_finite(float x) {
  uint32_t b;
  __builtin_memcpy(&b, &x, 4);
  return (b & 0x7f800000u) != 0x7f800000u;
}

DLG_HD inline bool sacia_row_finite(const float* row) {
  bool ok = true;
  for (int j = 0; j < kSaciaDim; ++j) ok = ok && sacia_finite(row[j]);
  return ok;
}

// pcl::euclideanDistance of two points
inline float sacia_point_dist(const float* a, const float* b) {
  const float dx = a[0] - b[0], dy = a[1] - b[1], dz = a[2] - b[2];
  return std::sqrt((dx * dx + dy * dy) + dz * dz);
}

// selectSamples over the source records (xyz first, stride_f floats apart): fills sample[0..nr),
// counts the rand() calls into *draws and the halvings into *relaxations
inline void sacia_select(SaciaRng& rng, const float* xyz, int64_t stride_f, int n, int nr,
                         float min_sample_distance, int32_t* sample, int64_t* draws,
                         int32_t* relaxations) {
  int64_t without = 0;
  const int64_t max_without = 3 * (int64_t)n;
  int got = 0;
  while (got < nr) {
    const int idx = rng.index(n);
    ++*draws;
    bool valid = true;
    for (int i = 0; i < got; ++i) {
      const float d = sacia_point_dist(xyz + (int64_t)idx * stride_f, xyz + (int64_t)sample[i] * stride_f);
      if (idx == sample[i] || d < min_sample_distance) {
        valid = false;
        break;
      }
    }
    if (valid) {
      sample[got++] = idx;
      without = 0;
    } else {
      ++without;
    }
    if (without >= max_without) {
      min_sample_distance *= 0.5f;
      ++*relaxations;
      without = 0;
    }
  }
}

// FLANN's L2_Simple over 33 floats: r = 0; r += (a_j - b_j) * (a_j - b_j)
DLG_HD inline float sacia_feature_d2(const float* a, const float* b) {
  float r = 0.0f;
  for (int j = 0; j < kSaciaDim; ++j) {
    const float d = a[j] - b[j];
    r += d * d;
  }
  return r;
}

// (float)corr_dist_threshold_: out of float's range -> +inf
inline float sacia_threshold(double max_correspondence_distance) {
  // (at FLT_MAX + half an ulp the cast rounds to 2^128: out of range)
  if (max_correspondence_distance >= 0x1.ffffffp127) return INFINITY;
  return (float)max_correspondence_distance;
}

// TruncatedError of one squared distance (a NaN term, inf / inf, counts as 1.0f)
DLG_HD inline float sacia_term(float e, float thr) {
  const float t = e <= thr ? e / thr : 1.0f;
  return t != t ? 1.0f : t;
}

// trunc(term 2^48): the term is a float in [0, 1], the product is exact
DLG_HD inline uint64_t sacia_quantise(float term) {
  return (uint64_t)((double)term * 0x1p48);
}

// E as the records carry it: E = hi 2^24 + lo, lo < 2^24, from the sums of the low 24 bits and of
// the rest of the per-wave partial sums (sum_lo < 2^64, sum_hi < 2^56)
inline void sacia_error_words(uint64_t sum_lo, uint64_t sum_hi, uint64_t* hi, uint64_t* lo) {
  *lo = sum_lo & 0xFFFFFFull;
  *hi = sum_hi + (sum_lo >> 24);
}

// RN(E) 2^-48
inline double sacia_error_double(uint64_t hi, uint64_t lo) {
  // hi 2^24 + lo rounded once: hi < 2^55 may not be exact as a double, so round the 79-bit integer
  // through long arithmetic (Big of exact_refit.hpp)
  int64_t dig[2] = {(int64_t)lo, (int64_t)hi};
  return big_to_double(big_lin(dig)) * 0x1p-48;
}

inline bool sacia_error_less(uint64_t hi_a, uint64_t lo_a, uint64_t hi_b, uint64_t lo_b) {
  return hi_a < hi_b || (hi_a == hi_b && lo_a < lo_b);
}

// "guess.isApprox(Identity, 0.01f)", in double from the float entries:
// sum (g - I)^2 <= (double)(0.01f * 0.01f) * min(sum g^2, 4)
inline bool sacia_guess_is_identity(const float g[16]) {
  double diff = 0.0, norm = 0.0;
  for (int k = 0; k < 16; ++k) {
    const double v = (double)g[k], d = v - ((k % 5 == 0) ? 1.0 : 0.0);
    diff += d * d;
    norm += v * v;
  }
  const float p = 0.01f;
  const double p2 = (double)(p * p);
  return diff <= p2 * (norm < 4.0 ? norm : 4.0);
}

// the rigid estimate of nr pairs (w_i -> t_i): icp_model.hpp's exact moments with e = the exponent
// of the pairs' largest |coordinate|, Horn, t = ct - R cs, cast to float
inline void sacia_estimate(const float (*w)[3], const float (*t)[3], int nr, float T[16]) {
  float big = 0.0f;
  for (int i = 0; i < nr; ++i)
    for (int a = 0; a < 3; ++a) big = std::fmax(big, std::fmax(std::fabs(w[i][a]), std::fabs(t[i][a])));
  const int e = icp_qexp(big);
  const double sc = pow2d(kFastBits - e);
  int64_t dig[kIcpDigits] = {};
  IcpAcc acc;
  icp_acc_zero(acc);
  for (int i = 0; i < nr; ++i) {
    const double qw[3] = {icp_q(w[i][0], sc), icp_q(w[i][1], sc), icp_q(w[i][2], sc)};
    const double qt[3] = {icp_q(t[i][0], sc), icp_q(t[i][1], sc), icp_q(t[i][2], sc)};
    icp_acc_point(acc, qw, qt, 0.0);
  }
  icp_acc_flush(dig, acc);
  const IcpMoments mo = icp_moments(dig);
  double mse;
  icp_solve(mo, e, 0, T, &mse);
}

// the adoption walk over the records' errors in iteration order
struct SaciaBest {
  bool scored = false;
  uint64_t hi = 0, lo = 0;
  int best_iteration = -1;  // the adopted hypothesis (-1: none)
  // a scored hypothesis (the guess: adopt = false); true when it was adopted
  bool offer(int iteration, uint64_t e_hi, uint64_t e_lo, bool adopt) {
    const bool better = !scored || sacia_error_less(e_hi, e_lo, hi, lo);
    if (!better) return false;
    scored = true;
    hi = e_hi;
    lo = e_lo;
    if (adopt) best_iteration = iteration;
    return adopt;
  }
};

}  // namespace dlg
