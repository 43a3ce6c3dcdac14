// icp_model.hpp -- the arithmetic of dlg_icp_align (include/dialog_ransac.h), shared by the device
// passes (icp.hip), the host driver (icp_host.cpp) and the host-only test program
// (tests/cpp/icp_model_san.cpp builds it without HIP); restated in numpy by tests/icp_ref.py.
//
// One iteration, given the m kept correspondences (w_i, t_i, d2_i) of the working cloud W and the
// target (any order):
//   e      = the binary exponent with F < 2^e, F = the larger of the target's and W's largest finite
//            |coordinate| (fast_qexp, exact_refit.hpp); e2 the same of the largest kept d2
//   q(v)   = trunc(v 2^(48 - e)), an integer |q| < 2^48
//   m, S_a = sum q(w_a), T_a = sum q(t_a), P_ab = sum q(w_a) q(t_b), D = sum trunc(d2 2^(48 - e2))
//   C_ab   = m P_ab - S_a T_b (exact, < 2^160), M_ab = RN(C_ab), cs_a = RN(S_a) / m 2^(e - 48), ct alike
//   mse    = RN(D) / m 2^(e2 - 48)
//   R      = Horn's closed form on M (icp_horn below), t = ct - R cs, T = (R | t) cast to float
// Accumulation, as exact_refit.hpp's: Q = q as a double, Q = hi 2^24 + lo (hi = floor(Q 2^-24),
// 0 <= lo < 2^24), q_a q_b = A 2^48 + B 2^24 + C with A = hi_a hi_b, B = hi_a lo_b + lo_a hi_b,
// C = lo_a lo_b, each < 2^49 in magnitude, summed with double FMAs in an IcpAcc (exact while every
// sum stays < 2^53: at most kIcpFlush entries between flushes); a flush splits every sum
// X = X0 + X1 2^24 (0 <= X0 < 2^24) and adds the pieces of equal weight into the int64 digits:
//   [0] m; [1 + 2a, 2 + 2a] S_a; [7 + 2a, 8 + 2a] T_a; [13 + 4k .. 16 + 4k] P_k (k = 3a + b) =
//   w0 + w24 2^24 + w48 2^48 + w72 2^72; [49, 50] D.
// The digits depend on how the entries were grouped into flushes; the integers they stand for do
// not, and only those enter the solve.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstdint>

#include "exact_refit.hpp"

namespace dlg {

constexpr int kIcpDigits = 51;
constexpr int kIcpFlush = 16;  // entries per IcpAcc between flushes (B: 2 x 16 x 2^48 = 2^53)

// pcl::registration::DefaultConvergenceCriteria::ConvergenceState
enum {
  kIcpNotConverged = 0,
  kIcpIterations = 1,
  kIcpTransform = 2,
  kIcpAbsMse = 3,
  kIcpRelMse = 4,
  kIcpNoCorrespondences = 5
};

// a point through a row-major 4x4 (float, no contraction): ((m0 x + m1 y) + m2 z) + m3
DLG_HD inline void icp_xf(const float* m, float x, float y, float z, float& ox, float& oy,
                          float& oz) {
  ox = ((m[0] * x + m[1] * y) + m[2] * z) + m[3];
  oy = ((m[4] * x + m[5] * y) + m[6] * z) + m[7];
  oz = ((m[8] * x + m[9] * y) + m[10] * z) + m[11];
}

// FLANN's L2: ((0 + dx^2) + dy^2) + dz^2 with d = query - point
DLG_HD inline float icp_d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float ex = qx - px, ey = qy - py, ez = qz - pz;
  return ((0.0f + ex * ex) + ey * ey) + ez * ez;
}

DLG_HD inline bool icp_finite(float v) { return v - v == 0.0f; }

// fast_qexp (exact_refit.hpp) for host and device: the e with f < 2^e of a finite f > 0 (a float as
// a double is normal: frexp's exponent is the biased field - 1022), else 0
DLG_HD inline int icp_qexp(float f) {
  if (!(f > 0.0f) || !(f < INFINITY)) return 0;
  const double d = (double)f;
  uint64_t bits;
  std::memcpy(&bits, &d, 8);
  return (int)((bits >> 52) & 0x7FF) - 1022;
}

// q(v) as a double, an exact integer (|v| < 2^e, scale = 2^(48 - e): the product is exact)
DLG_HD inline double icp_q(float v, double scale) { return trunc((double)v * scale); }

// partial sums between flushes: exact integers < 2^53 held in doubles (MomAcc of exact_refit.hpp
// with the nine cross products, both clouds' linear sums and D)
struct IcpAcc {
  double n, S[3], T[3], A[9], B[9], C[9], D;
};

DLG_HD inline void icp_acc_zero(IcpAcc& m) {
  m.n = 0.0;
  m.D = 0.0;
#pragma unroll
  for (int a = 0; a < 3; ++a) m.S[a] = m.T[a] = 0.0;
#pragma unroll
  for (int k = 0; k < 9; ++k) m.A[k] = m.B[k] = m.C[k] = 0.0;
}

// one correspondence: qw, qt = q of its W and target coordinates, qd = trunc(d2 2^(48 - e2))
DLG_HD inline void icp_acc_point(IcpAcc& m, const double qw[3], const double qt[3], double qd) {
  double wh[3], wl[3], th[3], tl[3];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    wh[a] = floor(qw[a] * 0x1p-24);
    wl[a] = fma(-wh[a], 0x1p24, qw[a]);  // exact: 0 <= lo < 2^24
    th[a] = floor(qt[a] * 0x1p-24);
    tl[a] = fma(-th[a], 0x1p24, qt[a]);
  }
  m.n += 1.0;
  m.D += qd;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    m.S[a] += qw[a];
    m.T[a] += qt[a];
  }
#pragma unroll
  for (int a = 0; a < 3; ++a)
#pragma unroll
    for (int b = 0; b < 3; ++b) {
      const int k = 3 * a + b;
      m.A[k] = fma(wh[a], th[b], m.A[k]);
      m.B[k] = fma(wl[a], th[b], fma(wh[a], tl[b], m.B[k]));
      m.C[k] = fma(wl[a], tl[b], m.C[k]);
    }
}

// the accumulator into the digits (split24, exact_refit.hpp: X = X0 + X1 2^24); m is zeroed
DLG_HD inline void icp_acc_flush(int64_t* dig, IcpAcc& m) {
  dig[0] += (int64_t)(int32_t)m.n;
  int64_t x0, x1;
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    split24(m.S[a], x0, x1);
    dig[1 + 2 * a] += x0;
    dig[2 + 2 * a] += x1;
    split24(m.T[a], x0, x1);
    dig[7 + 2 * a] += x0;
    dig[8 + 2 * a] += x1;
  }
#pragma unroll
  for (int k = 0; k < 9; ++k) {
    int64_t c0, c1, b0, b1, a0, a1;
    split24(m.C[k], c0, c1);
    split24(m.B[k], b0, b1);
    split24(m.A[k], a0, a1);
    dig[13 + 4 * k] += c0;
    dig[14 + 4 * k] += c1 + b0;
    dig[15 + 4 * k] += b1 + a0;
    dig[16 + 4 * k] += a1;
  }
  split24(m.D, x0, x1);
  dig[49] += x0;
  dig[50] += x1;
  icp_acc_zero(m);
}

// ---- host side: the solve and the criteria (double + - * / sqrt only) ---------------------------

struct IcpMoments {
  int64_t m;
  double M[9];          // RN(m P_ab - S_a T_b), row a = W's axis, column b = the target's
  double S[3], T[3];    // RN(S_a), RN(T_a)
  double D;             // RN(D)
};

inline IcpMoments icp_moments(const int64_t* dig) {
  IcpMoments r;
  r.m = dig[0];
  Big S[3], T[3];
  for (int a = 0; a < 3; ++a) {
    S[a] = big_lin(dig + 1 + 2 * a);
    T[a] = big_lin(dig + 7 + 2 * a);
    r.S[a] = big_to_double(S[a]);
    r.T[a] = big_to_double(T[a]);
  }
  for (int a = 0; a < 3; ++a)
    for (int b = 0; b < 3; ++b)
      r.M[3 * a + b] = big_to_double(big_add(
          big_mul(big_i64(dig[0]), big_prod(dig + 13 + 4 * (3 * a + b))), big_neg(big_mul(S[a], T[b]))));
  r.D = big_to_double(big_lin(dig + 49));
  return r;
}

// one rotation of the cyclic Jacobi on a symmetric 4x4 (row-major), annihilating A[p][q]
inline void icp_jacobi_rot(double A[16], double V[16], int p, int q) {
  const double apq = A[4 * p + q];
  if (apq == 0.0) return;
  const double app = A[4 * p + p], aqq = A[4 * q + q];
  const double theta = (aqq - app) / (2.0 * apq);
  double t;
  if (theta > 1e150 || theta < -1e150) {
    t = 0.5 / theta;
  } else {
    t = 1.0 / ((theta < 0.0 ? -theta : theta) + std::sqrt(theta * theta + 1.0));
    if (theta < 0.0) t = -t;
  }
  const double c = 1.0 / std::sqrt(t * t + 1.0), s = t * c;
  A[4 * p + p] = app - t * apq;
  A[4 * q + q] = aqq + t * apq;
  A[4 * p + q] = 0.0;
  A[4 * q + p] = 0.0;
  for (int o = 0; o < 4; ++o) {
    if (o == p || o == q) continue;
    const double aop = A[4 * o + p], aoq = A[4 * o + q];
    const double nop = c * aop - s * aoq, noq = s * aop + c * aoq;
    A[4 * o + p] = nop; A[4 * p + o] = nop;
    A[4 * o + q] = noq; A[4 * q + o] = noq;
  }
  for (int i = 0; i < 4; ++i) {
    const double vip = V[4 * i + p], viq = V[4 * i + q];
    V[4 * i + p] = c * vip - s * viq;
    V[4 * i + q] = s * vip + c * viq;
  }
}

// jacobi3 (exact_refit.hpp) extended to 4x4: sweeps of the rotations (0,1), (0,2), (0,3), (1,2),
// (1,3), (2,3), until the sum of the squared off-diagonal entries is exactly zero (at most 32)
constexpr int kIcpJacobiSweeps = 32;
inline void icp_jacobi4(double A[16], double V[16]) {
  for (int k = 0; k < 16; ++k) V[k] = (k % 5 == 0) ? 1.0 : 0.0;
  for (int sweep = 0; sweep < kIcpJacobiSweeps; ++sweep) {
    const double off = ((((A[1] * A[1] + A[2] * A[2]) + A[3] * A[3]) + A[6] * A[6]) + A[7] * A[7]) +
                       A[11] * A[11];
    if (off == 0.0) break;
    icp_jacobi_rot(A, V, 0, 1);
    icp_jacobi_rot(A, V, 0, 2);
    icp_jacobi_rot(A, V, 0, 3);
    icp_jacobi_rot(A, V, 1, 2);
    icp_jacobi_rot(A, V, 1, 3);
    icp_jacobi_rot(A, V, 2, 3);
  }
}

// Horn's closed form: the rotation R (row-major 3x3) that maximises sum (R w) . t for the
// cross-covariance M_ab = sum w_a t_b.  M is first scaled by the power of two that puts its largest
// |entry| in [1, 2) (all zero: left alone); the unit quaternion (w, x, y, z) is the eigenvector of
// N(M)'s largest eigenvalue (ties: lowest index), normalised, with the sign that makes w >= 0.
inline void icp_horn(const double Min[9], double R[9]) {
  double big = 0.0;
  for (int k = 0; k < 9; ++k) {
    const double a = Min[k] < 0.0 ? -Min[k] : Min[k];
    if (a > big) big = a;
  }
  double sc = 1.0;
  if (big > 0.0) {
    int ex = 0;
    (void)std::frexp(big, &ex);  // big = f 2^ex, f in [0.5, 1)
    sc = pow2d(1 - ex);
  }
  double S[9];
  for (int k = 0; k < 9; ++k) S[k] = Min[k] * sc;
  const double Sxx = S[0], Sxy = S[1], Sxz = S[2], Syx = S[3], Syy = S[4], Syz = S[5], Szx = S[6],
               Szy = S[7], Szz = S[8];
  double A[16];
  A[0] = (Sxx + Syy) + Szz;
  A[5] = (Sxx - Syy) - Szz;
  A[10] = (Syy - Sxx) - Szz;
  A[15] = (Szz - Sxx) - Syy;
  A[1] = A[4] = Syz - Szy;
  A[2] = A[8] = Szx - Sxz;
  A[3] = A[12] = Sxy - Syx;
  A[6] = A[9] = Sxy + Syx;
  A[7] = A[13] = Szx + Sxz;
  A[11] = A[14] = Syz + Szy;
  double V[16];
  icp_jacobi4(A, V);
  int k = 0;
  for (int i = 1; i < 4; ++i)
    if (A[5 * i] > A[5 * k]) k = i;
  double w = V[k], x = V[4 + k], y = V[8 + k], z = V[12 + k];
  const double nq = std::sqrt(((w * w + x * x) + y * y) + z * z);
  w = w / nq; x = x / nq; y = y / nq; z = z / nq;
  if (w < 0.0) {
    w = -w; x = -x; y = -y; z = -z;
  }
  R[0] = ((w * w + x * x) - y * y) - z * z;
  R[1] = 2.0 * (x * y - w * z);
  R[2] = 2.0 * (x * z + w * y);
  R[3] = 2.0 * (x * y + w * z);
  R[4] = ((w * w - x * x) + y * y) - z * z;
  R[5] = 2.0 * (y * z - w * x);
  R[6] = 2.0 * (x * z - w * y);
  R[7] = 2.0 * (y * z + w * x);
  R[8] = ((w * w - x * x) - y * y) + z * z;
}

// the iteration's transformation (row-major 4x4 float) and mse from the moments (mo.m >= 3)
inline void icp_solve(const IcpMoments& mo, int e, int e2, float T[16], double* mse) {
  double R[9];
  icp_horn(mo.M, R);
  const double md = (double)mo.m, back = pow2d(e - kFastBits);
  double cs[3], ct[3];
  for (int a = 0; a < 3; ++a) {
    cs[a] = mo.S[a] / md * back;
    ct[a] = mo.T[a] / md * back;
  }
  for (int a = 0; a < 3; ++a) {
    const double t = ct[a] - ((R[3 * a] * cs[0] + R[3 * a + 1] * cs[1]) + R[3 * a + 2] * cs[2]);
    T[4 * a] = (float)R[3 * a];
    T[4 * a + 1] = (float)R[3 * a + 1];
    T[4 * a + 2] = (float)R[3 * a + 2];
    T[4 * a + 3] = (float)t;
  }
  T[12] = T[13] = T[14] = 0.0f;
  T[15] = 1.0f;
  *mse = mo.D / md * pow2d(e2 - kFastBits);
}

// out = a b (row-major 4x4 float): each entry the four products summed left to right
inline void icp_mul4(const float a[16], const float b[16], float out[16]) {
  float r[16];
  for (int i = 0; i < 4; ++i)
    for (int j = 0; j < 4; ++j)
      r[4 * i + j] = ((a[4 * i] * b[j] + a[4 * i + 1] * b[4 + j]) + a[4 * i + 2] * b[8 + j]) +
                     a[4 * i + 3] * b[12 + j];
  for (int k = 0; k < 16; ++k) out[k] = r[k];
}

inline bool icp_is_identity(const float m[16]) {  // bit-equal to the identity
  for (int k = 0; k < 16; ++k) {
    const float want = (k % 5 == 0) ? 1.0f : 0.0f;
    uint32_t a, b;
    std::memcpy(&a, &m[k], 4);
    std::memcpy(&b, &want, 4);
    if (a != b) return false;
  }
  return true;
}

// pcl::registration::DefaultConvergenceCriteria as IterativeClosestPoint wires it (the
// similar-transform counter left out)
struct IcpCriteria {
  int max_iterations = 10;
  double rot_thr = 1.0;    // 1 - transformation_epsilon
  double trans_thr = 0.0;  // transformation_epsilon (compared with the squared norm, as PCL)
  double rel_mse = -DBL_MAX;
  double abs_mse = 1e-12;
  double prev_mse = DBL_MAX;
};

// after ++iterations: the state (kIcpNotConverged: prev_mse updated, the loop goes on)
inline int icp_criteria(IcpCriteria& c, int iterations, const float T[16], double mse) {
  if (iterations >= c.max_iterations) return kIcpIterations;
  const double cos_angle = 0.5 * ((((double)T[0] + (double)T[5]) + (double)T[10]) - 1.0);
  const double tx = (double)T[3], ty = (double)T[7], tz = (double)T[11];
  const double tsq = (tx * tx + ty * ty) + tz * tz;
  if (cos_angle >= c.rot_thr && tsq <= c.trans_thr) return kIcpTransform;
  const double diff = mse - c.prev_mse;
  const double ad = diff < 0.0 ? -diff : diff;
  if (ad < c.abs_mse) return kIcpAbsMse;
  if (ad / c.prev_mse < c.rel_mse) return kIcpRelMse;
  c.prev_mse = mse;
  return kIcpNotConverged;
}

}  // namespace dlg
