// mls_model.hpp -- the per-query arithmetic of pcl::MovingLeastSquares<PointXYZ, PointNormal>::
// computeMLSPointNormal (PCL 1.8 surface/impl/mls.hpp, upsampling NONE, restated from memory: parity
// unpinned), for the host and the device alike.  All double unless marked float;
// build with -ffp-contract=off.
//
//   centroid = (sum p) / m;  C = sum (p - centroid)(p - centroid)^T  (unnormalised)
//   (lambda, n) = pcl::eigen33(C);  d = -(n . centroid);  dist = q . n + d;  point = q - dist n
//   curvature = trace(C); non-zero: |lambda / trace|; cast to float
//   polynomial fit (m >= nr_coeff): v = n.unitOrthogonal(), u = n x v; per neighbour de = p - point,
//   sq = (float)(de . de), w = exp(-(double)sq / sqr_gauss_param), uc = de . u, vc = de . v,
//   f = de . n, t_j = uc^ui vc^vi;  A = sum (t w) t^T, b = sum (t w) f;  c = llt(A).solve(b) (Eigen's
//   unblocked Cholesky: it stops at the first pivot <= 0 and the solves run over what it left);
//   isfinite(c[0]): point += c[0] n, normal = n - c[order + 1] u - c[1] v (not normalised)
//
// The order of the sums over the neighbours is free: mls_query() below takes them
// in the source's order, k_mls (mls.hip) as wave reductions.  Plain C++ without HIP too
// (tests/cpp/mls_model_san.cpp).
#pragma once

#include <cmath>
#include <cstdint>

#include "host_math.hpp"  // DLG_HD, eigen33

namespace dlg {

constexpr int kMlsMaxOrder = 3;  // nr_coeff <= 10
// what became of a query (the branch counts of dlg_mls_stats)
enum { kMlsFit = 0, kMlsPlaneOnly = 1, kMlsFitNonfinite = 2, kMlsTooFew = 3 };

DLG_HD constexpr int mls_nr_coeff(int order) { return (order + 1) * (order + 2) / 2; }

DLG_HD inline double mls_dot3(const double a[3], const double b[3]) {
  return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
}

// the local frame of a query: plane normal and in-plane axes, the projected query, curvature
struct MlsFrame {
  double n[3], u[3], v[3];
  double point[3];
  float curvature;
};

// Eigen's Vector3d::unitOrthogonal (isMuchSmallerThan at the double precision 1e-12)
DLG_HD inline void mls_unit_orthogonal(const double s[3], double o[3]) {
  const bool small = m_fabs(s[0]) <= m_fabs(s[2]) * 1e-12 && m_fabs(s[1]) <= m_fabs(s[2]) * 1e-12;
  if (!small) {
    const double inv = 1.0 / m_sqrt(s[0] * s[0] + s[1] * s[1]);
    o[0] = -s[1] * inv; o[1] = s[0] * inv; o[2] = 0.0;
  } else {
    const double inv = 1.0 / m_sqrt(s[1] * s[1] + s[2] * s[2]);
    o[0] = 0.0; o[1] = -s[2] * inv; o[2] = s[1] * inv;
  }
}

// cov6 = (xx, xy, xz, yy, yz, zz) of the centred neighbours; q = the query
DLG_HD inline void mls_frame(const double cov6[6], const double centroid[3], const float q[3],
                             MlsFrame* F) {
  const double cov[9] = {cov6[0], cov6[1], cov6[2], cov6[1], cov6[3], cov6[4],
                         cov6[2], cov6[4], cov6[5]};
  double ev;
  eigen33<double>(cov, &ev, F->n);
  const double d = -mls_dot3(F->n, centroid);
  const double qd[3] = {(double)q[0], (double)q[1], (double)q[2]};
  const double dist = mls_dot3(qd, F->n) + d;
  for (int k = 0; k < 3; ++k) F->point[k] = qd[k] - dist * F->n[k];
  const double tr = (cov6[0] + cov6[3]) + cov6[5];
  F->curvature = (float)(tr != 0.0 ? m_fabs(ev / tr) : tr);
  mls_unit_orthogonal(F->n, F->v);
  F->u[0] = F->n[1] * F->v[2] - F->n[2] * F->v[1];
  F->u[1] = F->n[2] * F->v[0] - F->n[0] * F->v[2];
  F->u[2] = F->n[0] * F->v[1] - F->n[1] * F->v[0];
}

// one neighbour's row of the normal equations: tw[j] = t_j w, t[j], f
template <int ORDER>
DLG_HD inline void mls_terms(float px, float py, float pz, const MlsFrame& F, double sqr_gauss,
                             double (&t)[mls_nr_coeff(ORDER)], double* w, double* f) {
  const double de[3] = {(double)px - F.point[0], (double)py - F.point[1], (double)pz - F.point[2]};
  const float sq = (float)mls_dot3(de, de);
  *w = exp(-(double)sq / sqr_gauss);
  const double uc = mls_dot3(de, F.u), vc = mls_dot3(de, F.v);
  *f = mls_dot3(de, F.n);
  int j = 0;
  double u_pow = 1.0;
#pragma unroll
  for (int ui = 0; ui <= ORDER; ++ui) {
    double v_pow = 1.0;
#pragma unroll
    for (int vi = 0; vi <= ORDER - ui; ++vi) {
      t[j++] = u_pow * v_pow;
      v_pow *= vc;
    }
    u_pow *= uc;
  }
}

// Eigen's unblocked LLT on the lower triangle of A (row-major N x N) and the two triangular solves
// of b in place.  A pivot <= 0 ends the factorisation; the solves use the matrix as it stands.
template <int N>
DLG_HD inline void mls_llt_solve(double (&A)[N * N], double (&b)[N]) {
  for (int k = 0; k < N; ++k) {
    double dot = 0.0;
    for (int j = 0; j < k; ++j) dot = dot + A[k * N + j] * A[k * N + j];
    double x = A[k * N + k] - dot;
    if (x <= 0.0) break;
    x = m_sqrt(x);
    A[k * N + k] = x;
    for (int i = k + 1; i < N; ++i) {
      double d2 = 0.0;
      for (int j = 0; j < k; ++j) d2 = d2 + A[i * N + j] * A[k * N + j];
      A[i * N + k] = (A[i * N + k] - d2) / x;
    }
  }
  for (int i = 0; i < N; ++i) {
    double dot = 0.0;
    for (int j = 0; j < i; ++j) dot = dot + A[i * N + j] * b[j];
    b[i] = (b[i] - dot) / A[i * N + i];
  }
  for (int i = N - 1; i >= 0; --i) {
    double dot = 0.0;
    for (int j = i + 1; j < N; ++j) dot = dot + A[j * N + i] * b[j];
    b[i] = (b[i] - dot) / A[i * N + i];
  }
}

DLG_HD inline bool mls_finite(double x) {
  uint64_t u;
  __builtin_memcpy(&u, &x, 8);
  return (u & 0x7ff0000000000000ull) != 0x7ff0000000000000ull;
}

// the output row of a query: position, (normal, curvature), branch
struct MlsRow {
  float xyz[3];
  float nrm[4];
  int code;
};

// the three output branches: c0 / cu / cv = c[0], c[order + 1], c[1] of a fit that ran (fitted)
DLG_HD inline void mls_finish(const MlsFrame& F, bool fitted, double c0, double cu, double cv,
                              bool compute_normals, MlsRow* out) {
  double p[3] = {F.point[0], F.point[1], F.point[2]};
  double nn[3] = {F.n[0], F.n[1], F.n[2]};
  out->code = kMlsPlaneOnly;
  if (fitted) {
    out->code = kMlsFitNonfinite;
    if (mls_finite(c0)) {
      out->code = kMlsFit;
      for (int k = 0; k < 3; ++k) {
        p[k] = p[k] + c0 * F.n[k];
        nn[k] = F.n[k] - cu * F.u[k] - cv * F.v[k];
      }
    }
  }
  for (int k = 0; k < 3; ++k) {
    out->xyz[k] = (float)p[k];
    out->nrm[k] = compute_normals ? (float)nn[k] : 0.0f;
  }
  out->nrm[3] = compute_normals ? F.curvature : 0.0f;
}

// One query by one thread: src.size() neighbours (the query included), src.get(i, p) their
// coordinates, every sum in the source's order.
template <int ORDER, typename Src>
DLG_HD inline void mls_query(const Src& src, const float q[3], bool polynomial_fit,
                             bool compute_normals, double sqr_gauss, MlsRow* out) {
  constexpr int N = mls_nr_coeff(ORDER);
  const int m = src.size();
  if (m < 3) {
    out->code = kMlsTooFew;
    return;
  }
  float p[3];
  double sum[3] = {0.0, 0.0, 0.0};
  for (int i = 0; i < m; ++i) {
    src.get(i, p);
    for (int k = 0; k < 3; ++k) sum[k] = sum[k] + (double)p[k];
  }
  double cen[3];
  for (int k = 0; k < 3; ++k) cen[k] = sum[k] / (double)m;
  double cov6[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
  for (int i = 0; i < m; ++i) {
    src.get(i, p);
    const double dx = (double)p[0] - cen[0], dy = (double)p[1] - cen[1], dz = (double)p[2] - cen[2];
    cov6[0] = cov6[0] + dx * dx; cov6[1] = cov6[1] + dx * dy; cov6[2] = cov6[2] + dx * dz;
    cov6[3] = cov6[3] + dy * dy; cov6[4] = cov6[4] + dy * dz; cov6[5] = cov6[5] + dz * dz;
  }
  MlsFrame F;
  mls_frame(cov6, cen, q, &F);
  const bool fit = polynomial_fit && m >= N;
  double b[N];
  if (fit) {
    double A[N * N];
    for (int k = 0; k < N * N; ++k) A[k] = 0.0;
    for (int k = 0; k < N; ++k) b[k] = 0.0;
    for (int i = 0; i < m; ++i) {
      src.get(i, p);
      double t[N], w, f;
      mls_terms<ORDER>(p[0], p[1], p[2], F, sqr_gauss, t, &w, &f);
      for (int a = 0; a < N; ++a) {
        const double tw = t[a] * w;
        for (int c = 0; c <= a; ++c) A[a * N + c] = A[a * N + c] + tw * t[c];
        b[a] = b[a] + tw * f;
      }
    }
    mls_llt_solve<N>(A, b);
  }
  mls_finish(F, fit, fit ? b[0] : 0.0, fit ? b[ORDER + 1] : 0.0, fit ? b[1] : 0.0, compute_normals,
             out);
}

}  // namespace dlg
