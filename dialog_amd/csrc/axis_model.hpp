// axis_model.hpp -- isModelValid of the axis-constrained plane models (SACMODEL_PERPENDICULAR_PLANE,
// SACMODEL_PARALLEL_PLANE; PCL 1.8 sac_model_perpendicular_plane.hpp / sac_model_parallel_plane.hpp
// restated from memory: parity unpinned), for the host and the device alike.
//
// Both models are SACMODEL_PLANE with one more gate on a hypothesis: a plane whose normal is not
// within eps of the axis (perpendicular plane) or not perpendicular to it within eps (parallel
// plane) counts nothing and selects nothing.  The verdict is float arithmetic up to one number f
// (a predux-ordered dot product) and then a double comparison through acos / sin.  No device
// transcendental may decide it, so the host turns eps into float thresholds on f once per call
// (make_axis_test): the device compares floats.
//   perpendicular: f = A . Cn, A = normalized4(axis), Cn = normalized4(c0, c1, c2);
//                  theta = acos(clamp((double)f, -1, 1)), m = min(theta, M_PI - theta);
//                  invalid exactly when m > eps   <=>   t_lo < f < t_hi
//   parallel     : f = axis . Cn (the raw axis); invalid exactly when
//                  (double)|f| > |sin(eps)|       <=>   |f| > t_hi = the largest float <= |sin(eps)|
// A NaN f is valid either way (its NaN plane counts nothing anyway); eps <= 0 switches the gate off.
// Plain C++ without HIP too (the sanitizer program tests/cpp/axis_model_san.cpp); like
// host_math.hpp it must be built with -ffp-contract=off.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>

#include "host_math.hpp"  // DLG_HD

namespace dlg {

// pcl::SacModel values of the two models (DLG_SACMODEL_* in include/dialog_ransac.h)
constexpr int kModelPerpendicularPlane = 9, kModelParallelPlane = 15;
enum { kAxisNone = 0, kAxisPerpendicular = 1, kAxisParallel = 2 };

struct AxisTest {
  int mode;          // kAxisNone: every plane is valid
  float ax, ay, az;  // perpendicular: normalized4(axis); parallel: the caller's axis as given
  float t_lo, t_hi;  // the thresholds on f (above)
};

// Eigen Vector4f(v0, v1, v2, 0).normalized(): z = (v0^2 + v2^2) + (v1^2 + 0 * 0); z > 0 ? v / sqrt(z) : v
DLG_HD inline void normalized4(float v0, float v1, float v2, float o[3]) {
  const float z = (v0 * v0 + v2 * v2) + (v1 * v1 + 0.0f * 0.0f);
  o[0] = v0; o[1] = v1; o[2] = v2;
  if (z > 0.0f) {
    const float s = sqrtf(z);
    o[0] = v0 / s; o[1] = v1 / s; o[2] = v2 / s;
  }
}

// the verdict from f alone (mode != kAxisNone)
DLG_HD inline bool axis_verdict(const AxisTest& t, float f) {
  if (t.mode == kAxisPerpendicular) return !(f < t.t_hi && f > t.t_lo);
  return !(fabsf(f) > t.t_hi);
}

// isModelValid of a plane whose normalized4(c0, c1, c2) is (n0, n1, n2)
DLG_HD inline bool axis_valid_n(const AxisTest& t, float n0, float n1, float n2) {
  if (t.mode == kAxisNone) return true;
  return axis_verdict(t, (t.ax * n0 + t.az * n2) + (t.ay * n1 + 0.0f * 0.0f));
}

// isModelValid of the plane (c0, c1, c2, .)
DLG_HD inline bool axis_valid(const AxisTest& t, float c0, float c1, float c2) {
  if (t.mode == kAxisNone) return true;
  float n[3];
  normalized4(c0, c1, c2, n);
  return axis_valid_n(t, n[0], n[1], n[2]);
}

// isSampleGood + computeModelCoefficients of SampleConsensusModelPlane in PCL's op order
// (k_build_hyps builds every hypothesis with it; the host rebuilds an invalid winner's real
// coefficients from its kept samples with it).  false: a bad sample, c = NaN
DLG_HD inline bool sample_plane(const float p0[3], const float p1[3], const float p2[3], float c[4]) {
  const float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
  const float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
  const float r0 = a0 / b0, r1 = a1 / b1, r2 = a2 / b2;
  const bool good = (r0 != r1) || (r2 != r1);
  if (!good) {
    c[0] = c[1] = c[2] = c[3] = __builtin_nanf("");
    return false;
  }
  float c0 = a1 * b2 - a2 * b1;
  float c1 = a2 * b0 - a0 * b2;
  float c2 = a0 * b1 - a1 * b0;
  float c3 = 0.0f;
  // VectorXf::normalize(): Eigen 3.3 guards z > 0; squaredNorm = (c0^2 + c2^2) + (c1^2 + c3^2)
  const float z = (c0 * c0 + c2 * c2) + (c1 * c1 + c3 * c3);
  if (z > 0.0f) {
    const float sq = sqrtf(z);  // correctly rounded (-fhip-fp32-correctly-rounded-divide-sqrt)
    c0 = c0 / sq; c1 = c1 / sq; c2 = c2 / sq; c3 = c3 / sq;
  }
  const float dot = (c0 * p0[0] + c2 * p0[2]) + (c1 * p0[1] + c3 * 1.0f);
  c[0] = c0; c[1] = c1; c[2] = c2; c[3] = -1.0f * dot;
  return true;
}

// ---- host: the specification evaluated directly, and the thresholds derived from it ------------
// perpendicular plane, from rad_f = A . Cn
inline bool perpendicular_valid_direct(float rad_f, double eps) {
  double rad = (double)rad_f;
  if (rad < -1.0) rad = -1.0;
  else if (rad > 1.0) rad = 1.0;
  const double theta = acos(rad);
  const double alt = 3.14159265358979323846 - theta;  // M_PI
  const double m = alt < theta ? alt : theta;
  return !(m > eps);
}
// parallel plane, from dot_f = axis . Cn
inline bool parallel_valid_direct(float dot_f, double eps) {
  return !((double)fabsf(dot_f) > fabs(sin(eps)));
}
// isModelValid as the specification states it (no thresholds)
inline bool axis_valid_direct(int model, const float axis[3], double eps, const float c[3]) {
  if (!(eps > 0.0)) return true;
  float n[3], a[3] = {axis[0], axis[1], axis[2]};
  normalized4(c[0], c[1], c[2], n);
  if (model == kModelPerpendicularPlane) normalized4(axis[0], axis[1], axis[2], a);
  const float f = (a[0] * n[0] + a[2] * n[2]) + (a[1] * n[1] + 0.0f * 0.0f);
  return model == kModelPerpendicularPlane ? perpendicular_valid_direct(f, eps)
                                           : parallel_valid_direct(f, eps);
}

inline float bits_float(uint32_t b) {
  float f;
  std::memcpy(&f, &b, 4);
  return f;
}

// the float of smallest magnitude in [0, 1] (sign as given) that the perpendicular model accepts:
// bisection over bit patterns, assuming the verdict is monotone in |rad_f| on each side of 0
// (|rad_f| = 1 is always accepted: m = 0)
inline float perpendicular_threshold(double eps, bool negative) {
  const uint32_t sign = negative ? 0x80000000u : 0u;
  uint32_t lo = 0u, hi = 0x3F800000u;
  if (perpendicular_valid_direct(bits_float(sign | lo), eps)) return bits_float(sign | lo);
  while (hi - lo > 1u) {
    const uint32_t mid = lo + (hi - lo) / 2u;
    if (perpendicular_valid_direct(bits_float(sign | mid), eps)) hi = mid;
    else lo = mid;
  }
  return bits_float(sign | hi);
}

// the device's test for `model` with the caller's axis and eps (radians); kAxisNone for any other
// model and for eps <= 0
inline AxisTest make_axis_test(int model, const float axis[3], double eps) {
  AxisTest t;
  t.mode = kAxisNone;
  t.ax = t.ay = t.az = 0.0f;
  t.t_lo = t.t_hi = 0.0f;
  if (!(eps > 0.0)) return t;
  if (model == kModelPerpendicularPlane) {
    float a[3];
    normalized4(axis[0], axis[1], axis[2], a);
    t.mode = kAxisPerpendicular;
    t.ax = a[0]; t.ay = a[1]; t.az = a[2];
    t.t_hi = perpendicular_threshold(eps, false);
    t.t_lo = perpendicular_threshold(eps, true);
  } else if (model == kModelParallelPlane) {
    const double s = fabs(sin(eps));
    float f = (float)s;  // the largest float <= s: (double)x > s  <=>  x > f for a float x
    if ((double)f > s) f = std::nextafter(f, -INFINITY);
    t.mode = kAxisParallel;
    t.ax = axis[0]; t.ay = axis[1]; t.az = axis[2];
    t.t_hi = f;
    t.t_lo = -f;
  }
  return t;
}

}  // namespace dlg
