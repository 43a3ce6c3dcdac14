/*
 * pcl_oracle.c -- TEST INFRASTRUCTURE ONLY (see pcl_oracle.h for provenance and the
 * pinning status).  Scalar C restatement of PCL 1.8 / Eigen 3.3 / Boost 1.64 semantics.
 *
 * Build: gcc -O2 -std=c11 -ffp-contract=off -fno-fast-math (x86-64 SSE scalar math, no FMA),
 * which matches MSVC x64 /fp:precise code generation for the PCL build used by the reference
 * (Dialog/PropertySheet-success.props:5-10: PCL 1.8, MSVC v140).
 *
 * Citations are to third-party sources ([PCL-1.8 ext], not vendored) unless they name a
 * Dialog/ file, which are the reference call sites.
 */
#include "pcl_oracle.h"

#include <float.h>
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <string.h>

/* ------------------------------------------------------------------------------------------ */
/* Boost mt19937 + variate_generator<mt19937&, uniform_int<>(0, INT_MAX)>                       */
/* pcl/sample_consensus/sac_model.h: SampleConsensusModel ctor seeds rng_alg_ with 12345u and   */
/* rnd() returns (*rng_gen_)().  generate_uniform_int: brange = 2^32-1 > range = 2^31-1,        */
/* bucket_size = 2 (brange % (range+1) == range), result = eng()/2 <= range always.             */
/* ------------------------------------------------------------------------------------------ */
void orc_mt_seed(orc_mt19937* g, uint32_t seed) {
  g->mt[0] = seed;
  for (int i = 1; i < 624; ++i)
    g->mt[i] = 1812433253u * (g->mt[i - 1] ^ (g->mt[i - 1] >> 30)) + (uint32_t)i;
  g->idx = 624;
}

static void orc_mt_twist(orc_mt19937* g) {
  for (int i = 0; i < 624; ++i) {
    uint32_t y = (g->mt[i] & 0x80000000u) | (g->mt[(i + 1) % 624] & 0x7fffffffu);
    g->mt[i] = g->mt[(i + 397) % 624] ^ (y >> 1) ^ ((y & 1u) ? 0x9908b0dfu : 0u);
  }
  g->idx = 0;
}

uint32_t orc_mt_next(orc_mt19937* g) {
  if (g->idx >= 624) orc_mt_twist(g);
  uint32_t y = g->mt[g->idx++];
  y ^= y >> 11;
  y ^= (y << 7) & 0x9d2c5680u;
  y ^= (y << 15) & 0xefc60000u;
  y ^= y >> 18;
  return y;
}

int orc_rnd(orc_mt19937* g) { return (int)(orc_mt_next(g) >> 1); }

/* ------------------------------------------------------------------------------------------ */
/* SampleConsensusModelPlane                                                                   */
/* ------------------------------------------------------------------------------------------ */
/* isSampleGood: dy1dy2 = (p1-p0)/(p2-p0) (Array4f, lanes 0..2 matter);
 * good iff (d0 != d1) || (d2 != d1)  (IEEE: NaN makes it "good"). */
int orc_plane_sample_good(const float p0[3], const float p1[3], const float p2[3]) {
  float d0 = (p1[0] - p0[0]) / (p2[0] - p0[0]);
  float d1 = (p1[1] - p0[1]) / (p2[1] - p0[1]);
  float d2 = (p1[2] - p0[2]) / (p2[2] - p0[2]);
  return (d0 != d1) || (d2 != d1);
}

/* computeModelCoefficients: cross product in source order, VectorXf::normalize() with the
 * Eigen-3.3 guard (z > 0) and SSE predux order (c0^2 + c2^2) + (c1^2 + c3^2), then
 * d = -1 * ((c0 x0 + c2 z0) + (c1 y0 + c3 * 1)) with c3 == 0. */
int orc_plane_coefficients(const float p0[3], const float p1[3], const float p2[3], float c[4]) {
  float a0 = p1[0] - p0[0], a1 = p1[1] - p0[1], a2 = p1[2] - p0[2];
  float b0 = p2[0] - p0[0], b1 = p2[1] - p0[1], b2 = p2[2] - p0[2];
  float r0 = a0 / b0, r1 = a1 / b1, r2 = a2 / b2;
  if ((r0 == r1) && (r2 == r1)) return 0; /* collinear */
  float c0 = a1 * b2 - a2 * b1;
  float c1 = a2 * b0 - a0 * b2;
  float c2 = a0 * b1 - a1 * b0;
  float c3 = 0.0f;
  float z = (c0 * c0 + c2 * c2) + (c1 * c1 + c3 * c3);
  if (z > 0.0f) {
    float s = sqrtf(z);
    c0 = c0 / s; c1 = c1 / s; c2 = c2 / s; c3 = c3 / s;
  }
  float dot = (c0 * p0[0] + c2 * p0[2]) + (c1 * p0[1] + c3 * 1.0f);
  c[0] = c0; c[1] = c1; c[2] = c2; c[3] = -1.0f * dot;
  return 1;
}

/* countWithinDistance / selectWithinDistance: fabs(model_coefficients.dot(Vector4f(x,y,z,1)))
 * with the VectorXf(4) SSE predux order (c0 x + c2 z) + (c1 y + c3 * 1). */
float orc_plane_abs_dist(const float c[4], float x, float y, float z) {
  float d = (c[0] * x + c[2] * z) + (c[1] * y + c[3] * 1.0f);
  return fabsf(d);
}

float orc_thr_ceil(double thr) {
  float f = (float)thr;                 /* round to nearest */
  if ((double)f < thr) f = nextafterf(f, INFINITY);
  return f;
}

int64_t orc_count_within(const float* xyz, int64_t stride, const int32_t* idx, int64_t n,
                         const float c[4], double thr) {
  int64_t cnt = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + (int64_t)(idx ? idx[i] : i) * stride;
    if ((double)orc_plane_abs_dist(c, p[0], p[1], p[2]) < thr) ++cnt;
  }
  return cnt;
}

/* ------------------------------------------------------------------------------------------ */
/* SampleConsensusModelNormalPlane::countWithinDistance / selectWithinDistance (PCL 1.8         */
/* sac_model_normal_plane.hpp; SACMODEL_NORMAL_PLANE, not used by the reference -- config C5):  */
/*   coeff = model with coeff[3] = 0;  p = (x, y, z, 0);  n = (nx, ny, nz, 0)                    */
/*   d_euclid = fabs(coeff.dot(p) + model[3])            float, predux (c0x + c2z) + (c1y + 0)   */
/*   d_normal = getAngle3D(n, coeff) = acos(clamp(n.normalized().dot(coeff.normalized())))       */
/*   d_normal = min(d_normal, M_PI - d_normal)                                                   */
/*   weight   = normal_distance_weight * (1.0 - curvature)                                       */
/*   inlier  <=> fabs(weight * d_normal + (1.0 - weight) * d_euclid) < threshold   (double)      */
/* Eigen normalized(): z = squaredNorm (predux order); z > 0 ? v / sqrt(z) : v.                  */
/* ------------------------------------------------------------------------------------------ */
void orc_normalized4(const float v[3], float out[3]) {
  float z = (v[0] * v[0] + v[2] * v[2]) + (v[1] * v[1] + 0.0f * 0.0f);
  if (z > 0.0f) {
    float s = sqrtf(z);
    out[0] = v[0] / s; out[1] = v[1] / s; out[2] = v[2] / s;
  } else {
    out[0] = v[0]; out[1] = v[1]; out[2] = v[2];
  }
}

double orc_normal_plane_dist(const float c[4], const float p[3], const float nrm[4],
                             double lambda) {
  float de_f = fabsf(((c[0] * p[0] + c[2] * p[2]) + (c[1] * p[1] + 0.0f * 0.0f)) + c[3]);
  double d_euclid = (double)de_f;
  float nn[3], cn[3];
  orc_normalized4(nrm, nn);
  orc_normalized4(c, cn);
  float rad_f = (nn[0] * cn[0] + nn[2] * cn[2]) + (nn[1] * cn[1] + 0.0f * 0.0f);
  double rad = (double)rad_f;
  if (rad < -1.0) rad = -1.0;
  else if (rad > 1.0) rad = 1.0;
  double d_normal = fabs(acos(rad));
  double alt = 3.14159265358979323846 - d_normal;  /* M_PI */
  if (alt < d_normal) d_normal = alt;             /* std::min(a, b) = (b < a) ? b : a */
  double weight = lambda * (1.0 - (double)nrm[3]);
  return fabs(weight * d_normal + (1.0 - weight) * d_euclid);
}

static int orc_within(const orc_sac_params* prm, const float* xyz, int64_t stride, int32_t g,
                      const float c[4], double thr) {
  const float* p = xyz + (int64_t)g * stride;
  if (prm && prm->model == ORC_SACMODEL_NORMAL_PLANE) {
    /* (exact shortcut, same verdicts: with w in [0, 1] the sum w*theta + (1-w)*d rounds to at
     * least (1-w)*d, so (1-w)*d >= thr already decides "out" without the acos) */
    const float* nrm = prm->normals + (int64_t)g * 4;
    const double w = prm->normal_distance_weight * (1.0 - (double)nrm[3]);
    if (w >= 0.0 && w <= 1.0) {
      const double de = (double)fabsf(((c[0] * p[0] + c[2] * p[2]) + (c[1] * p[1] + 0.0f * 0.0f)) + c[3]);
      if ((1.0 - w) * de >= thr) return 0;
    }
    return orc_normal_plane_dist(c, p, nrm, prm->normal_distance_weight) < thr;
  }
  return (double)orc_plane_abs_dist(c, p[0], p[1], p[2]) < thr;
}

/* countWithinDistance.  The count is an integer sum, so splitting it over threads
 * (orc_set_threads; OpenMP, default 1) gives the same value. */
static int orc_threads = 1;
void orc_set_threads(int n) { orc_threads = n > 0 ? n : 1; }
int orc_get_threads(void) { return orc_threads; }

static int64_t orc_count_model(const orc_sac_params* prm, const float* xyz, int64_t stride,
                               const int32_t* idx, int64_t n, const float c[4], double thr) {
  int64_t cnt = 0;
#pragma omp parallel for reduction(+ : cnt) num_threads(orc_threads) if (orc_threads > 1 && n > 65536) schedule(static)
  for (int64_t i = 0; i < n; ++i) cnt += orc_within(prm, xyz, stride, idx ? idx[i] : (int32_t)i, c, thr);
  return cnt;
}

int64_t orc_count_within_np(const float* xyz, int64_t stride, const float* normals,
                            const int32_t* idx, int64_t n, const float c[4], double thr,
                            double lambda) {
  orc_sac_params prm;
  memset(&prm, 0, sizeof(prm));
  prm.model = ORC_SACMODEL_NORMAL_PLANE;
  prm.normals = normals;
  prm.normal_distance_weight = lambda;
  return orc_count_model(&prm, xyz, stride, idx, n, c, thr);
}

static int64_t orc_select_within(const orc_sac_params* prm, const float* xyz, int64_t stride,
                                 const int32_t* idx, int64_t n, const float c[4], double thr,
                                 int32_t* out) {
  int64_t k = 0;
  for (int64_t i = 0; i < n; ++i) {
    int32_t g = idx[i];
    if (orc_within(prm, xyz, stride, g, c, thr)) out[k++] = g;
  }
  return k;
}

/* ------------------------------------------------------------------------------------------ */
/* pcl::computeMeanAndCovarianceMatrix (common/impl/centroid.hpp, dense branch), float.        */
/* ------------------------------------------------------------------------------------------ */
unsigned orc_mean_cov(const float* xyz, int64_t stride, const int32_t* idx, int64_t n,
                      float cov[9], float centroid[4]) {
  float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + (int64_t)idx[i] * stride;
    float x = p[0], y = p[1], z = p[2];
    a[0] += x * x; a[1] += x * y; a[2] += x * z;
    a[3] += y * y; a[4] += y * z; a[5] += z * z;
    a[6] += x;     a[7] += y;     a[8] += z;
  }
  float cntf = (float)(size_t)n;
  for (int k = 0; k < 9; ++k) a[k] = a[k] / cntf;
  centroid[0] = a[6]; centroid[1] = a[7]; centroid[2] = a[8]; centroid[3] = 1.0f;
  cov[0] = a[0] - a[6] * a[6];
  cov[1] = a[1] - a[6] * a[7];
  cov[2] = a[2] - a[6] * a[8];
  cov[4] = a[3] - a[7] * a[7];
  cov[5] = a[4] - a[7] * a[8];
  cov[8] = a[5] - a[8] * a[8];
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  return (unsigned)n;
}

/* ------------------------------------------------------------------------------------------ */
/* pcl::computeRoots2 / computeRoots / eigen33 (common/impl/eigen.hpp), float.                  */
/* ------------------------------------------------------------------------------------------ */
static void orc_compute_roots2(float b, float c, float roots[3]) {
  roots[0] = 0.0f;
  float d = (float)((double)(b * b) - 4.0 * (double)c); /* Scalar(b * b - 4.0 * c) */
  if (d < 0.0f) d = 0.0f;
  float sd = sqrtf(d);
  roots[2] = 0.5f * (b + sd);
  roots[1] = 0.5f * (b - sd);
}

#define M(r, c) m[(r) * 3 + (c)]
void orc_compute_roots(const float m[9], float roots[3]) {
  float c0 = M(0, 0) * M(1, 1) * M(2, 2) + 2.0f * M(0, 1) * M(0, 2) * M(1, 2) -
             M(0, 0) * M(1, 2) * M(1, 2) - M(1, 1) * M(0, 2) * M(0, 2) -
             M(2, 2) * M(0, 1) * M(0, 1);
  float c1 = M(0, 0) * M(1, 1) - M(0, 1) * M(0, 1) + M(0, 0) * M(2, 2) - M(0, 2) * M(0, 2) +
             M(1, 1) * M(2, 2) - M(1, 2) * M(1, 2);
  float c2 = M(0, 0) + M(1, 1) + M(2, 2);
  if (fabsf(c0) < FLT_EPSILON) {
    orc_compute_roots2(c2, c1, roots);
  } else {
    const float s_inv3 = (float)(1.0 / 3.0);
    const float s_sqrt3 = sqrtf(3.0f);
    float c2_over_3 = c2 * s_inv3;
    float a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.0f) a_over_3 = 0.0f;
    float half_b = 0.5f * (c0 + c2_over_3 * (2.0f * c2_over_3 * c2_over_3 - c1));
    float q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.0f) q = 0.0f;
    float rho = sqrtf(-a_over_3);
    /* std::atan2 / cos / sin on floats: the correctly rounded float value, evaluated as the
     * double function rounded to float (the platform's float libm is unknowable; see
     * dialog_amd/csrc/host_math.hpp m_atan2) */
    float theta = (float)atan2((double)sqrtf(-q), (double)half_b) * s_inv3;
    float cos_theta = (float)cos((double)theta);
    float sin_theta = (float)sin((double)theta);
    roots[0] = c2_over_3 + 2.0f * rho * cos_theta;
    roots[1] = c2_over_3 - rho * (cos_theta + s_sqrt3 * sin_theta);
    roots[2] = c2_over_3 - rho * (cos_theta - s_sqrt3 * sin_theta);
    float t;
    if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
    if (roots[1] >= roots[2]) {
      t = roots[1]; roots[1] = roots[2]; roots[2] = t;
      if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
    }
    if (roots[0] <= 0.0f) orc_compute_roots2(c2, c1, roots);
  }
}

/* Vector3f::squaredNorm(): Eigen's non-vectorised unroller gives x^2 + (y^2 + z^2). */
static float sqn3(const float v[3]) { return v[0] * v[0] + (v[1] * v[1] + v[2] * v[2]); }
static void cross3(const float* a, const float* b, float* o) {
  o[0] = a[1] * b[2] - a[2] * b[1];
  o[1] = a[2] * b[0] - a[0] * b[2];
  o[2] = a[0] * b[1] - a[1] * b[0];
}

void orc_eigen33(const float mat[9], float* eval, float evec[3]) {
  float scale = 0.0f;
  for (int k = 0; k < 9; ++k) { float v = fabsf(mat[k]); if (v > scale) scale = v; }
  if (scale <= FLT_MIN) scale = 1.0f;
  float m[9];
  for (int k = 0; k < 9; ++k) m[k] = mat[k] / scale;
  float roots[3];
  orc_compute_roots(m, roots);
  *eval = roots[0] * scale;
  M(0, 0) -= roots[0]; M(1, 1) -= roots[0]; M(2, 2) -= roots[0];
  float v1[3], v2[3], v3[3];
  cross3(&M(0, 0), &M(1, 0), v1);
  cross3(&M(0, 0), &M(2, 0), v2);
  cross3(&M(1, 0), &M(2, 0), v3);
  float l1 = sqn3(v1), l2 = sqn3(v2), l3 = sqn3(v3);
  const float* v; float l;
  if (l1 >= l2 && l1 >= l3) { v = v1; l = l1; }
  else if (l2 >= l1 && l2 >= l3) { v = v2; l = l2; }
  else { v = v3; l = l3; }
  float s = sqrtf(l);
  evec[0] = v[0] / s; evec[1] = v[1] / s; evec[2] = v[2] / s;
}
#undef M

/* ---- double twin (fast-mode reference) ---- */
#define M(r, c) m[(r) * 3 + (c)]
static void orc_compute_roots2_d(double b, double c, double roots[3]) {
  roots[0] = 0.0;
  double d = b * b - 4.0 * c;
  if (d < 0.0) d = 0.0;
  double sd = sqrt(d);
  roots[2] = 0.5 * (b + sd);
  roots[1] = 0.5 * (b - sd);
}
static void orc_compute_roots_d(const double m[9], double roots[3]) {
  double c0 = M(0, 0) * M(1, 1) * M(2, 2) + 2.0 * M(0, 1) * M(0, 2) * M(1, 2) -
              M(0, 0) * M(1, 2) * M(1, 2) - M(1, 1) * M(0, 2) * M(0, 2) -
              M(2, 2) * M(0, 1) * M(0, 1);
  double c1 = M(0, 0) * M(1, 1) - M(0, 1) * M(0, 1) + M(0, 0) * M(2, 2) - M(0, 2) * M(0, 2) +
              M(1, 1) * M(2, 2) - M(1, 2) * M(1, 2);
  double c2 = M(0, 0) + M(1, 1) + M(2, 2);
  if (fabs(c0) < DBL_EPSILON) {
    orc_compute_roots2_d(c2, c1, roots);
  } else {
    const double s_inv3 = 1.0 / 3.0, s_sqrt3 = sqrt(3.0);
    double c2_over_3 = c2 * s_inv3;
    double a_over_3 = (c1 - c2 * c2_over_3) * s_inv3;
    if (a_over_3 > 0.0) a_over_3 = 0.0;
    double half_b = 0.5 * (c0 + c2_over_3 * (2.0 * c2_over_3 * c2_over_3 - c1));
    double q = half_b * half_b + a_over_3 * a_over_3 * a_over_3;
    if (q > 0.0) q = 0.0;
    double rho = sqrt(-a_over_3);
    double theta = atan2(sqrt(-q), half_b) * s_inv3;
    double ct = cos(theta), st = sin(theta);
    roots[0] = c2_over_3 + 2.0 * rho * ct;
    roots[1] = c2_over_3 - rho * (ct + s_sqrt3 * st);
    roots[2] = c2_over_3 - rho * (ct - s_sqrt3 * st);
    double t;
    if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
    if (roots[1] >= roots[2]) {
      t = roots[1]; roots[1] = roots[2]; roots[2] = t;
      if (roots[0] >= roots[1]) { t = roots[0]; roots[0] = roots[1]; roots[1] = t; }
    }
    if (roots[0] <= 0.0) orc_compute_roots2_d(c2, c1, roots);
  }
}
void orc_eigen33_d(const double mat[9], double* eval, double evec[3]) {
  double scale = 0.0;
  for (int k = 0; k < 9; ++k) { double v = fabs(mat[k]); if (v > scale) scale = v; }
  if (scale <= DBL_MIN) scale = 1.0;
  double m[9];
  for (int k = 0; k < 9; ++k) m[k] = mat[k] / scale;
  double roots[3];
  orc_compute_roots_d(m, roots);
  *eval = roots[0] * scale;
  M(0, 0) -= roots[0]; M(1, 1) -= roots[0]; M(2, 2) -= roots[0];
  double v[3][3];
  const double* r0 = &M(0, 0); const double* r1 = &M(1, 0); const double* r2 = &M(2, 0);
  v[0][0] = r0[1] * r1[2] - r0[2] * r1[1]; v[0][1] = r0[2] * r1[0] - r0[0] * r1[2]; v[0][2] = r0[0] * r1[1] - r0[1] * r1[0];
  v[1][0] = r0[1] * r2[2] - r0[2] * r2[1]; v[1][1] = r0[2] * r2[0] - r0[0] * r2[2]; v[1][2] = r0[0] * r2[1] - r0[1] * r2[0];
  v[2][0] = r1[1] * r2[2] - r1[2] * r2[1]; v[2][1] = r1[2] * r2[0] - r1[0] * r2[2]; v[2][2] = r1[0] * r2[1] - r1[1] * r2[0];
  double l[3];
  for (int k = 0; k < 3; ++k) l[k] = v[k][0] * v[k][0] + (v[k][1] * v[k][1] + v[k][2] * v[k][2]);
  int b = (l[0] >= l[1] && l[0] >= l[2]) ? 0 : ((l[1] >= l[0] && l[1] >= l[2]) ? 1 : 2);
  double s = sqrt(l[b]);
  evec[0] = v[b][0] / s; evec[1] = v[b][1] / s; evec[2] = v[b][2] / s;
}
#undef M

/* Least-squares plane in double: two-pass centroid and covariance, eigen33 in double.
 * Same "< 4 inliers keeps the model" rule as optimizeModelCoefficients. */
int orc_refit_double(const float* xyz, int64_t stride, const int32_t* idx, int64_t n,
                     const float coeff_in[4], float coeff_out[4]) {
  if (n < 4) { memcpy(coeff_out, coeff_in, 4 * sizeof(float)); return 0; }
  double cx = 0, cy = 0, cz = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + (int64_t)idx[i] * stride;
    cx += p[0]; cy += p[1]; cz += p[2];
  }
  cx /= (double)n; cy /= (double)n; cz /= (double)n;
  double c[9] = {0};
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + (int64_t)idx[i] * stride;
    double dx = p[0] - cx, dy = p[1] - cy, dz = p[2] - cz;
    c[0] += dx * dx; c[1] += dx * dy; c[2] += dx * dz;
    c[4] += dy * dy; c[5] += dy * dz; c[8] += dz * dz;
  }
  for (int k = 0; k < 9; ++k) c[k] /= (double)n;
  c[3] = c[1]; c[6] = c[2]; c[7] = c[5];
  double ev, v[3];
  orc_eigen33_d(c, &ev, v);
  double d = -(v[0] * cx + v[1] * cy + v[2] * cz);
  coeff_out[0] = (float)v[0]; coeff_out[1] = (float)v[1]; coeff_out[2] = (float)v[2];
  coeff_out[3] = (float)d;
  return 1;
}

/* ------------------------------------------------------------------------------------------ */
/* The product's fast refit (DLG_REFIT_FAST), restated from its definition in                 */
/* dialog_amd/csrc/exact_refit.hpp (not PCL: the order-independent LS plane of the inlier set): */
/* exact integer moments of q(v) = trunc(v 2^(48-e)), C_ab = n P_ab - L_a L_b exactly,          */
/* correctly rounded to double, cyclic Jacobi (same rotation sequence), centre RN(L)/n 2^(e-48). */
/* Independent code: __int128 sums and 4 x 64-bit limbs here, 32-bit limbs in the product.      */
/* ------------------------------------------------------------------------------------------ */
typedef struct { uint64_t w[4]; } orc_i256; /* two's complement */

static orc_i256 orc_i256_from_i128(__int128 v) {
  orc_i256 r;
  unsigned __int128 u = (unsigned __int128)v;
  r.w[0] = (uint64_t)u; r.w[1] = (uint64_t)(u >> 64);
  uint64_t s = v < 0 ? ~0ull : 0ull;
  r.w[2] = s; r.w[3] = s;
  return r;
}
static orc_i256 orc_i256_sub(orc_i256 a, orc_i256 b) {
  orc_i256 r;
  unsigned __int128 borrow = 0;
  for (int k = 0; k < 4; ++k) {
    unsigned __int128 d = (unsigned __int128)a.w[k] - b.w[k] - borrow;
    r.w[k] = (uint64_t)d;
    borrow = (d >> 64) ? 1 : 0;
  }
  return r;
}
/* signed 128 x signed 128 -> 256 (magnitudes, then sign) */
static orc_i256 orc_i256_mul128(__int128 a, __int128 b) {
  int neg = (a < 0) != (b < 0);
  unsigned __int128 ua = a < 0 ? -(unsigned __int128)a : (unsigned __int128)a;
  unsigned __int128 ub = b < 0 ? -(unsigned __int128)b : (unsigned __int128)b;
  uint64_t x[2] = {(uint64_t)ua, (uint64_t)(ua >> 64)}, y[2] = {(uint64_t)ub, (uint64_t)(ub >> 64)};
  uint64_t r[4] = {0, 0, 0, 0};
  for (int i = 0; i < 2; ++i) {
    unsigned __int128 carry = 0;
    for (int j = 0; j < 2; ++j) {
      unsigned __int128 t = (unsigned __int128)x[i] * y[j] + r[i + j] + carry;
      r[i + j] = (uint64_t)t;
      carry = t >> 64;
    }
    r[i + 2] += (uint64_t)carry;
  }
  orc_i256 m = {{r[0], r[1], r[2], r[3]}};
  if (neg) m = orc_i256_sub(orc_i256_from_i128(0), m);
  return m;
}
/* round to nearest, ties to even */
static double orc_i256_to_double(orc_i256 a) {
  int neg = (a.w[3] >> 63) != 0;
  if (neg) a = orc_i256_sub(orc_i256_from_i128(0), a);
  int L = 0;
  for (int k = 3; k >= 0; --k)
    if (a.w[k]) { L = 64 * k + 64 - __builtin_clzll(a.w[k]); break; }
  if (L == 0) return 0.0;
  double r;
  if (L <= 53) {
    r = (double)a.w[0];
  } else {
#define ORC_BIT(i) ((a.w[(i) >> 6] >> ((i) & 63)) & 1ull)
    uint64_t mant = 0;
    for (int i = L - 1; i >= L - 53; --i) mant = (mant << 1) | ORC_BIT(i);
    uint64_t rb = ORC_BIT(L - 54);
    int sticky = 0;
    for (int i = L - 55; i >= 0; --i) if (ORC_BIT(i)) { sticky = 1; break; }
#undef ORC_BIT
    if (rb && (sticky || (mant & 1ull))) ++mant;
    r = ldexp((double)mant, L - 53);
  }
  return neg ? -r : r;
}

static void orc_jacobi3(double A[9], double V[9]) {
  for (int k = 0; k < 9; ++k) V[k] = (k % 4 == 0) ? 1.0 : 0.0;
  static const int P[3] = {0, 0, 1}, Q[3] = {1, 2, 2};
  for (int sweep = 0; sweep < 16; ++sweep) {
    double off = (A[1] * A[1] + A[2] * A[2]) + A[5] * A[5];
    if (off == 0.0) break;
    for (int r = 0; r < 3; ++r) {
      int p = P[r], q = Q[r], o = 3 - p - q;
      double apq = A[3 * p + q];
      if (apq == 0.0) continue;
      double app = A[3 * p + p], aqq = A[3 * q + q];
      double theta = (aqq - app) / (2.0 * apq), t;
      if (theta > 1e150 || theta < -1e150) {
        t = 0.5 / theta;
      } else {
        t = 1.0 / (fabs(theta) + sqrt(theta * theta + 1.0));
        if (theta < 0.0) t = -t;
      }
      double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
      A[3 * p + p] = app - t * apq;
      A[3 * q + q] = aqq + t * apq;
      A[3 * p + q] = A[3 * q + p] = 0.0;
      double aop = A[3 * o + p], aoq = A[3 * o + q];
      double nop = c * aop - sn * aoq, noq = sn * aop + c * aoq;
      A[3 * o + p] = A[3 * p + o] = nop;
      A[3 * o + q] = A[3 * q + o] = noq;
      for (int i = 0; i < 3; ++i) {
        double vip = V[3 * i + p], viq = V[3 * i + q];
        V[3 * i + p] = c * vip - sn * viq;
        V[3 * i + q] = sn * vip + c * viq;
      }
    }
  }
}

int orc_fast_qexp(const float* xyz, int64_t stride, const int32_t* idx, int64_t n) {
  float f = 0.0f;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + (int64_t)(idx ? idx[i] : (int32_t)i) * stride;
    float ax = fabsf(p[0]), ay = fabsf(p[1]), az = fabsf(p[2]);
    if (isfinite(ax) && isfinite(ay) && isfinite(az)) {
      if (ax > f) f = ax;
      if (ay > f) f = ay;
      if (az > f) f = az;
    }
  }
  if (!(f > 0.0f)) return 0;
  int e = 0;
  (void)frexp((double)f, &e);
  return e;
}

/* the product's moment digits (exact_refit.hpp layout) of the points idx[0..n) */
void orc_mom_digits(const float* xyz, int64_t stride, const int32_t* idx, int64_t n, int qexp,
                    int64_t d[25]) {
  const double scale = ldexp(1.0, 48 - qexp);
  memset(d, 0, 25 * sizeof(int64_t));
  static const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + (int64_t)idx[i] * stride;
    int64_t q[3];
    for (int a = 0; a < 3; ++a) q[a] = (int64_t)((double)p[a] * scale);
    d[0] += 1;
    for (int a = 0; a < 3; ++a) {
      d[1 + 2 * a] += q[a] & 0xFFFFFFFFll;
      d[2 + 2 * a] += q[a] >> 32;   /* arithmetic shift (gcc) */
    }
    for (int k = 0; k < 6; ++k) {
      __int128 pr = (__int128)q[ia[k]] * q[ib[k]];
      unsigned __int128 u = (unsigned __int128)pr;
      d[7 + 3 * k] += (int64_t)(uint64_t)(u & 0xFFFFFFFFull);
      d[8 + 3 * k] += (int64_t)(uint64_t)((u >> 32) & 0xFFFFFFFFull);
      d[9 + 3 * k] += (int64_t)(pr >> 64);
    }
  }
}

/* the refit from summed digits (any split of the points over ranks gives the same sums) */
int orc_refit_digits(const int64_t d[25], int qexp, const float cin[4], float cout[4]) {
  const int64_t n = d[0];
  if (n < 4) { memcpy(cout, cin, 4 * sizeof(float)); return 0; }
  __int128 L[3], P[6];
  const __int128 two32 = (__int128)1 << 32, two64 = (__int128)1 << 64;  /* (no shifts of
                                                                          negatives: UB in C) */
  for (int a = 0; a < 3; ++a) L[a] = (__int128)d[2 + 2 * a] * two32 + d[1 + 2 * a];
  for (int k = 0; k < 6; ++k)
    P[k] = (__int128)d[9 + 3 * k] * two64 + (__int128)d[8 + 3 * k] * two32 + d[7 + 3 * k];
  static const int ia[6] = {0, 0, 0, 1, 1, 2}, ib[6] = {0, 1, 2, 1, 2, 2};
  double m6[6];
  for (int k = 0; k < 6; ++k) {
    orc_i256 c = orc_i256_sub(orc_i256_mul128((__int128)n, P[k]), orc_i256_mul128(L[ia[k]], L[ib[k]]));
    m6[k] = orc_i256_to_double(c);
  }
  double A[9] = {m6[0], m6[1], m6[2], m6[1], m6[3], m6[4], m6[2], m6[4], m6[5]}, V[9];
  orc_jacobi3(A, V);
  int k = 0;
  if (A[4] < A[0]) k = 1;
  if (A[8] < A[4 * k]) k = 2;
  double v0 = V[k], v1 = V[3 + k], v2 = V[6 + k];
  double nv = sqrt((v0 * v0 + v1 * v1) + v2 * v2);
  v0 = v0 / nv; v1 = v1 / nv; v2 = v2 / nv;
  if ((v0 * (double)cin[0] + v1 * (double)cin[1]) + v2 * (double)cin[2] < 0.0) { v0 = -v0; v1 = -v1; v2 = -v2; }
  double nd = (double)n, back = ldexp(1.0, qexp - 48);
  double c0 = orc_i256_to_double(orc_i256_from_i128(L[0])) / nd * back;
  double c1 = orc_i256_to_double(orc_i256_from_i128(L[1])) / nd * back;
  double c2 = orc_i256_to_double(orc_i256_from_i128(L[2])) / nd * back;
  double dd = -((v0 * c0 + v1 * c1) + v2 * c2);
  cout[0] = (float)v0; cout[1] = (float)v1; cout[2] = (float)v2; cout[3] = (float)dd;
  return 1;
}

int orc_refit_exact(const float* xyz, int64_t stride, const int32_t* idx, int64_t n, int qexp,
                    const float cin[4], float cout[4]) {
  int64_t d[25];
  orc_mom_digits(xyz, stride, idx, n, qexp, d);
  return orc_refit_digits(d, qexp, cin, cout);
}

/* optimizeModelCoefficients (sac_model_plane.hpp): < 4 inliers keep the coefficients; else
 * float mean/cov, eigen33, coeff = (v, 0), coeff[3] = -1 * coeff.dot(centroid). */
static void orc_optimize_plane(const float* xyz, int64_t stride, const int32_t* inl, int64_t n,
                               const float cin[4], float cout[4]) {
  if (n < 4) { memcpy(cout, cin, 4 * sizeof(float)); return; }
  float cov[9], cen[4], ev, v[3];
  orc_mean_cov(xyz, stride, inl, n, cov, cen);
  orc_eigen33(cov, &ev, v);
  float c3 = 0.0f;
  float dot = (v[0] * cen[0] + v[2] * cen[2]) + (v[1] * cen[1] + c3 * cen[3]);
  cout[0] = v[0]; cout[1] = v[1]; cout[2] = v[2]; cout[3] = -1.0f * dot;
}

/* ------------------------------------------------------------------------------------------ */
/* SACSegmentation::segment -> RandomSampleConsensus::computeModel (sac_segmentation.hpp,      */
/* ransac.hpp), SampleConsensusModel::getSamples / drawIndexSample (sac_model.h/.hpp).          */
/* ------------------------------------------------------------------------------------------ */
int orc_sac_segment(const float* xyz, int64_t n_points, int64_t stride,
                    const int32_t* indices, int64_t n_idx, const orc_sac_params* prm,
                    float coeff[4], int32_t* inliers_out, int64_t* n_inliers, orc_sac_stats* st) {
  orc_sac_stats dummy;
  if (!st) st = &dummy;
  memset(st, 0, sizeof(*st));
  memset(coeff, 0, 4 * sizeof(float));
  *n_inliers = 0;
  if (!indices) n_idx = n_points;
  int32_t* idx = (int32_t*)malloc((size_t)(n_idx > 0 ? n_idx : 1) * sizeof(int32_t));
  int32_t* shuf = (int32_t*)malloc((size_t)(n_idx > 0 ? n_idx : 1) * sizeof(int32_t));
  for (int64_t i = 0; i < n_idx; ++i) idx[i] = indices ? indices[i] : (int32_t)i;
  memcpy(shuf, idx, (size_t)n_idx * sizeof(int32_t));

  orc_mt19937 g;
  orc_mt_seed(&g, prm->seed);
  const double thr = prm->threshold;
  int iterations = 0;
  int best = -INT_MAX;
  double k = 1.0;
  double log_probability = log(1.0 - prm->probability);
  double one_over_indices = 1.0 / (double)n_idx;
  unsigned skipped = 0;
  const unsigned max_skip = (unsigned)prm->max_iterations * 10u;
  int have = 0;
  float best_c[4] = {0, 0, 0, 0};
  int32_t best_s[3] = {0, 0, 0};

  if (thr == DBL_MAX) goto done; /* "No threshold set!" */
  while (iterations < k && skipped < max_skip) {
    int32_t s[3];
    int found = 0;
    if (n_idx < 3) { iterations = INT_MAX - 1; break; } /* getSamples: cannot select 3 points */
    for (unsigned t = 0; t < 1000u; ++t) {                 /* max_sample_checks_ */
      for (int i = 0; i < 3; ++i) {
        size_t j = (size_t)i + ((size_t)orc_rnd(&g) % (size_t)(n_idx - i));
        int32_t tmp = shuf[i]; shuf[i] = shuf[j]; shuf[j] = tmp;
      }
      st->draws++;
      s[0] = shuf[0]; s[1] = shuf[1]; s[2] = shuf[2];
      if (orc_plane_sample_good(xyz + (int64_t)s[0] * stride, xyz + (int64_t)s[1] * stride,
                                xyz + (int64_t)s[2] * stride)) { found = 1; break; }
    }
    if (!found) break; /* "No samples could be selected!" */
    float c[4];
    if (!orc_plane_coefficients(xyz + (int64_t)s[0] * stride, xyz + (int64_t)s[1] * stride,
                                xyz + (int64_t)s[2] * stride, c)) { ++skipped; continue; }
    int n = (int)orc_count_model(prm, xyz, stride, idx, n_idx, c, thr);
    if (n > best) {
      best = n;
      have = 1;
      memcpy(best_c, c, sizeof(best_c));
      memcpy(best_s, s, sizeof(best_s));
      double w = (double)best * one_over_indices;
      double p_no_outliers = 1.0 - pow(w, 3.0);
      if (p_no_outliers < DBL_EPSILON) p_no_outliers = DBL_EPSILON;
      if (p_no_outliers > 1.0 - DBL_EPSILON) p_no_outliers = 1.0 - DBL_EPSILON;
      k = log_probability / log(p_no_outliers);
    }
    ++iterations;
    if (iterations > prm->max_iterations) break;
  }
done:
  st->iterations = iterations;
  st->skipped = (int)skipped;
  if (have) {
    st->has_model = 1;
    memcpy(st->best_sample, best_s, sizeof(best_s));
    memcpy(st->coeff_unrefined, best_c, sizeof(best_c));
    int64_t nin = orc_select_within(prm, xyz, stride, idx, n_idx, best_c, thr, inliers_out);
    st->n_unrefined = nin;
    if (prm->optimize) {
      float rc[4];
      if (prm->refit_double == 2) {
        const int qe = prm->fast_qexp != ORC_QEXP_AUTO ? prm->fast_qexp
                                                        : orc_fast_qexp(xyz, stride, idx, n_idx);
        orc_refit_exact(xyz, stride, inliers_out, nin, qe, best_c, rc);
      } else if (prm->refit_double) {
        orc_refit_double(xyz, stride, inliers_out, nin, best_c, rc);
      } else {
        orc_optimize_plane(xyz, stride, inliers_out, nin, best_c, rc);
      }
      memcpy(coeff, rc, sizeof(rc));
      nin = orc_select_within(prm, xyz, stride, idx, n_idx, rc, thr, inliers_out);
    } else {
      memcpy(coeff, best_c, sizeof(best_c));
    }
    *n_inliers = nin;
  }
  free(idx);
  free(shuf);
  return have;
}

int orc_extract_planes(const float* xyz, int64_t n_points, int64_t stride,
                       const orc_sac_params* prm, int max_planes, int64_t min_inliers,
                       float* coeffs, int64_t* offsets, int32_t* inliers, int* n_planes) {
  int32_t* rem = (int32_t*)malloc((size_t)(n_points > 0 ? n_points : 1) * sizeof(int32_t));
  int32_t* buf = (int32_t*)malloc((size_t)(n_points > 0 ? n_points : 1) * sizeof(int32_t));
  int64_t n_rem = n_points;
  for (int64_t i = 0; i < n_points; ++i) rem[i] = (int32_t)i;
  int64_t total = 0;
  int np = 0;
  offsets[0] = 0;
  int64_t floor_n = min_inliers > 3 ? min_inliers : 3;
  orc_sac_params p2 = *prm;  /* the fast refit's quantum: the whole cloud's, fixed for all rounds */
  if (p2.refit_double == 2 && p2.fast_qexp == ORC_QEXP_AUTO)
    p2.fast_qexp = orc_fast_qexp(xyz, stride, NULL, n_points);
  prm = &p2;
  while (np < max_planes && n_rem >= floor_n) {
    float c[4];
    int64_t nin = 0;
    int ok = orc_sac_segment(xyz, n_points, stride, rem, n_rem, prm, c, buf, &nin, NULL);
    if (!ok || nin == 0 || nin < min_inliers) break;
    memcpy(coeffs + 4 * np, c, sizeof(c));
    memcpy(inliers + total, buf, (size_t)nin * sizeof(int32_t));
    /* remove (both lists ascending) */
    int64_t w = 0, j = 0;
    for (int64_t i = 0; i < n_rem; ++i) {
      if (j < nin && rem[i] == buf[j]) { ++j; continue; }
      rem[w++] = rem[i];
    }
    n_rem = w;
    total += nin;
    ++np;
    offsets[np] = total;
  }
  *n_planes = np;
  free(rem);
  free(buf);
  return np;
}

/* ------------------------------------------------------------------------------------------ */
/* Normals: NormalEstimation(OMP)::computeFeature with radius search (features/impl/normal_3d) */
/* called at Dialog/PlaneDetect.h:529-535.  Neighbour search = KdTreeFLANN::radiusSearch:       */
/* dist2 = ((0 + dx^2) + dy^2) + dz^2 with d = query - point, kept iff dist2 < (float)(r*r),     */
/* results sorted by (dist2, index).  A uniform grid (cell = r) finds the same set exactly.     */
/* ------------------------------------------------------------------------------------------ */
typedef struct { float d; int32_t j; } orc_nb;
static int orc_nb_cmp(const void* a, const void* b) {
  const orc_nb* x = (const orc_nb*)a; const orc_nb* y = (const orc_nb*)b;
  if (x->d < y->d) return -1;
  if (x->d > y->d) return 1;
  return (x->j > y->j) - (x->j < y->j);
}

typedef struct {
  float minx, miny, minz, cell;
  int64_t gx, gy, gz;
  int64_t* start;   /* gx*gy*gz + 1 */
  int32_t* order;   /* point ids sorted by cell */
} orc_grid;

static int64_t orc_cell_of(const orc_grid* G, float v, float lo, int64_t gdim) {
  int64_t c = (int64_t)floor(((double)v - (double)lo) / (double)G->cell);
  if (c < 0) c = 0;
  if (c >= gdim) c = gdim - 1;
  return c;
}

static void orc_grid_build(orc_grid* G, const float* xyz, int64_t n, int64_t stride, float r) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      float v = xyz[i * stride + k];
      if (v < mn[k]) mn[k] = v;
      if (v > mx[k]) mx[k] = v;
    }
  G->minx = mn[0]; G->miny = mn[1]; G->minz = mn[2];
  G->cell = r;
  int64_t dims[3];
  for (int k = 0; k < 3; ++k) {
    double ext = n > 0 ? ((double)mx[k] - (double)mn[k]) / (double)r : 0.0;
    dims[k] = (int64_t)floor(ext) + 1;
    if (dims[k] < 1) dims[k] = 1;
    if (dims[k] > 1024) dims[k] = 1024;
  }
  /* clamp total cells */
  while (dims[0] * dims[1] * dims[2] > (int64_t)1 << 24) {
    G->cell *= 2.0f;
    for (int k = 0; k < 3; ++k) dims[k] = (dims[k] + 1) / 2;
  }
  G->gx = dims[0]; G->gy = dims[1]; G->gz = dims[2];
  int64_t nc = G->gx * G->gy * G->gz;
  G->start = (int64_t*)calloc((size_t)nc + 1, sizeof(int64_t));
  G->order = (int32_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int32_t));
  int64_t* cid = (int64_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int64_t));
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + i * stride;
    int64_t cx = orc_cell_of(G, p[0], G->minx, G->gx), cy = orc_cell_of(G, p[1], G->miny, G->gy),
            cz = orc_cell_of(G, p[2], G->minz, G->gz);
    cid[i] = (cz * G->gy + cy) * G->gx + cx;
    G->start[cid[i] + 1]++;
  }
  for (int64_t c = 0; c < nc; ++c) G->start[c + 1] += G->start[c];
  int64_t* fill = (int64_t*)malloc((size_t)nc * sizeof(int64_t));
  memcpy(fill, G->start, (size_t)nc * sizeof(int64_t));
  for (int64_t i = 0; i < n; ++i) G->order[fill[cid[i]]++] = (int32_t)i;
  free(fill);
  free(cid);
}

static void orc_grid_free(orc_grid* G) { free(G->start); free(G->order); }

/* exact radius neighbours of query q, sorted by (dist2, index); returns count */
static int64_t orc_radius(const orc_grid* G, const float* xyz, int64_t stride, const float q[3],
                          float r2, orc_nb** buf, int64_t* cap) {
  int64_t cx = orc_cell_of(G, q[0], G->minx, G->gx), cy = orc_cell_of(G, q[1], G->miny, G->gy),
          cz = orc_cell_of(G, q[2], G->minz, G->gz);
  int64_t k = 0;
  /* cell >= r, so the 27-neighbourhood covers the ball except for points clamped into the
   * border cells; clamping only merges cells, never drops a point within r. */
  for (int64_t dz = -1; dz <= 1; ++dz)
    for (int64_t dy = -1; dy <= 1; ++dy)
      for (int64_t dx = -1; dx <= 1; ++dx) {
        int64_t x = cx + dx, y = cy + dy, z = cz + dz;
        if (x < 0 || y < 0 || z < 0 || x >= G->gx || y >= G->gy || z >= G->gz) continue;
        int64_t c = (z * G->gy + y) * G->gx + x;
        for (int64_t t = G->start[c]; t < G->start[c + 1]; ++t) {
          int32_t j = G->order[t];
          const float* p = xyz + (int64_t)j * stride;
          float ex = q[0] - p[0], ey = q[1] - p[1], ez = q[2] - p[2];
          float d = ((0.0f + ex * ex) + ey * ey) + ez * ez;
          if (d < r2) {
            if (k == *cap) { *cap = *cap * 2 + 64; *buf = (orc_nb*)realloc(*buf, (size_t)*cap * sizeof(orc_nb)); }
            (*buf)[k].d = d; (*buf)[k].j = j; ++k;
          }
        }
      }
  qsort(*buf, (size_t)k, sizeof(orc_nb), orc_nb_cmp);
  return k;
}

void orc_estimate_normals(const float* xyz, int64_t n, int64_t stride, float radius,
                          const float vp[3], float* out) {
  orc_grid G;
  orc_grid_build(&G, xyz, n, stride, radius);
  float r2 = (float)((double)radius * (double)radius);
  orc_nb* nb = NULL; int64_t cap = 0;
  int32_t* ids = NULL; int64_t idcap = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + i * stride;
    int64_t k = orc_radius(&G, xyz, stride, p, r2, &nb, &cap);
    float* o = out + 4 * i;
    if (k < 3) { o[0] = o[1] = o[2] = o[3] = NAN; continue; }
    if (k > idcap) { idcap = k; ids = (int32_t*)realloc(ids, (size_t)idcap * sizeof(int32_t)); }
    for (int64_t t = 0; t < k; ++t) ids[t] = nb[t].j;
    float cov[9], cen[4], ev, v[3];
    orc_mean_cov(xyz, stride, ids, k, cov, cen);
    orc_eigen33(cov, &ev, v);
    float eig_sum = cov[0] + cov[4] + cov[8];
    float curv = eig_sum != 0.0f ? fabsf(ev / eig_sum) : 0.0f;
    float vx = vp[0] - p[0], vy = vp[1] - p[1], vz = vp[2] - p[2];
    float cos_theta = vx * v[0] + vy * v[1] + vz * v[2];
    if (cos_theta < 0.0f) { v[0] *= -1.0f; v[1] *= -1.0f; v[2] *= -1.0f; }
    o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = curv;
  }
  free(nb); free(ids);
  orc_grid_free(&G);
}

/* k-nearest-neighbour variant: NormalEstimation with setKSearch(k) (PCLViewer.cpp:507-522,
 * TriangularMeshing.h:28-35, k = 20).  Neighbours = the k smallest (dist2, index) pairs, FLANN's
 * sorted kNN result (the query itself has dist2 0), rows with a NaN or infinite coordinate never
 * taken and NaN as queries (pcl::isFinite, see orc_estimate_normals_knn_brute).  The brute-force
 * form is the definition; the grid form below finds the same pairs (checked against it on
 * tie-heavy clouds, tests/test_oracle.py) and is what clouds of any size use when every
 * coordinate is finite. */
static void orc_normal_from_ids(const float* xyz, int64_t stride, const float* p, const int32_t* ids,
                                int64_t k, const float vp[3], float* o) {
  float cov[9], cen[4], ev, v[3];
  orc_mean_cov(xyz, stride, ids, k, cov, cen);
  orc_eigen33(cov, &ev, v);
  float eig_sum = cov[0] + cov[4] + cov[8];
  float curv = eig_sum != 0.0f ? fabsf(ev / eig_sum) : 0.0f;
  float vx = vp[0] - p[0], vy = vp[1] - p[1], vz = vp[2] - p[2];
  float cos_theta = vx * v[0] + vy * v[1] + vz * v[2];
  if (cos_theta < 0.0f) { v[0] *= -1.0f; v[1] *= -1.0f; v[2] *= -1.0f; }
  o[0] = v[0]; o[1] = v[1]; o[2] = v[2]; o[3] = curv;
}

void orc_estimate_normals_knn_brute(const float* xyz, int64_t n, int64_t stride, int k_nn,
                                    const float vp[3], float* out) {
  orc_nb* all = (orc_nb*)malloc((size_t)(n > 0 ? n : 1) * sizeof(orc_nb));
  int32_t* ids = (int32_t*)malloc((size_t)(k_nn > 0 ? k_nn : 1) * sizeof(int32_t));
  /* PCL's rule for a non-dense cloud (PCL 1.8, restated from memory like the rest of this file):
   * pcl::isFinite(point) -- every coordinate finite, so +-inf as well as NaN -- decides both
   * sides.  NormalEstimation::computeFeature gives a query that fails
   * it a NaN normal (normal_3d.hpp), and KdTreeFLANN::convertCloudToArray leaves such points out of
   * the tree (kdtree_flann.hpp), so they are nobody's neighbour.  The test is on the row's
   * coordinates, not on d: a d2 that overflows to +inf between two finite points stays a
   * candidate. */
  uint8_t* fin = (uint8_t*)malloc((size_t)(n > 0 ? n : 1));
  for (int64_t j = 0; j < n; ++j) {
    const float* q = xyz + j * stride;
    fin[j] = (uint8_t)(isfinite(q[0]) && isfinite(q[1]) && isfinite(q[2]));
  }
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + i * stride;
    float* o = out + 4 * i;
    if (!fin[i]) {
      o[0] = o[1] = o[2] = o[3] = NAN;
      continue;
    }
    int64_t m = 0;
    for (int64_t j = 0; j < n; ++j) {
      if (!fin[j]) continue;
      const float* q = xyz + j * stride;
      float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
      float d = ((0.0f + ex * ex) + ey * ey) + ez * ez;
      all[m].d = d; all[m].j = (int32_t)j; ++m;
    }
    qsort(all, (size_t)m, sizeof(orc_nb), orc_nb_cmp);
    int64_t k = m < k_nn ? m : k_nn;
    if (k < 3) {
      o[0] = o[1] = o[2] = o[3] = NAN;
      continue;
    }
    for (int64_t t = 0; t < k; ++t) ids[t] = all[t].j;
    orc_normal_from_ids(xyz, stride, p, ids, k, vp, o);
  }
  free(all); free(ids); free(fin);
}

/* (d, j) lexicographic: a before b */
static int orc_nb_less(orc_nb a, orc_nb b) { return a.d < b.d || (a.d == b.d && a.j < b.j); }
/* max-heap on (d, j) of at most K entries: the K best so far, worst on top */
static void orc_heap_push(orc_nb* h, int* sz, int K, orc_nb v) {
  if (*sz < K) {
    int i = (*sz)++;
    h[i] = v;
    while (i > 0) {
      int p = (i - 1) / 2;
      if (!orc_nb_less(h[p], h[i])) break;
      orc_nb t = h[p]; h[p] = h[i]; h[i] = t;
      i = p;
    }
    return;
  }
  if (!orc_nb_less(v, h[0])) return;
  h[0] = v;
  int i = 0;
  for (;;) {
    int l = 2 * i + 1, r = l + 1, m = i;
    if (l < K && orc_nb_less(h[m], h[l])) m = l;
    if (r < K && orc_nb_less(h[m], h[r])) m = r;
    if (m == i) break;
    orc_nb t = h[m]; h[m] = h[i]; h[i] = t;
    i = m;
  }
}

/* Grid form: cells of about 16 points per occupied cell layer, searched in Chebyshev shells
 * around the query's cell; after shell R every point not yet seen lies outside the box of
 * shells 0..R, so its distance is at least the distance lb from the query to that box's nearest
 * open face.  The search stops once the K-th best dist2 is below lb^2 with a relative margin of
 * 1e-5 (the float dist2 of a farther point is within a few ulps of its true value, far inside
 * the margin), so neither a nearer point nor an equally near point of lower index can be
 * missing. */
static void orc_knn_grid(const float* xyz, int64_t n, int64_t stride, int k_nn, const float vp[3],
                         float* out) {
  float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
  for (int64_t i = 0; i < n; ++i)
    for (int k = 0; k < 3; ++k) {
      float v = xyz[i * stride + k];
      if (v < mn[k]) mn[k] = v;
      if (v > mx[k]) mx[k] = v;
    }
  double ext = 0.0;
  for (int k = 0; k < 3; ++k) ext = fmax(ext, (double)mx[k] - (double)mn[k]);
  /* cell edge: the cube root of the volume per 8 points if the cloud filled its box (a lower
   * bound of the spacing on surfaces), at least ext / 255 */
  double vol = 1.0;
  for (int k = 0; k < 3; ++k) vol *= fmax((double)mx[k] - (double)mn[k], ext * 1e-3 + 1e-30);
  double h = cbrt(vol * 8.0 / (double)(n > 0 ? n : 1));
  if (h < ext / 255.0) h = ext / 255.0;
  if (!(h > 0.0)) h = 1.0;
  orc_grid G;
  orc_grid_build(&G, xyz, n, stride, (float)h);
  const double cell = (double)G.cell;
  const int K = k_nn;
#pragma omp parallel num_threads(orc_threads)
  {
    orc_nb* heap = (orc_nb*)malloc((size_t)(K > 0 ? K : 1) * sizeof(orc_nb));
    int32_t* ids = (int32_t*)malloc((size_t)(K > 0 ? K : 1) * sizeof(int32_t));
#pragma omp for schedule(dynamic, 4096)
    for (int64_t i = 0; i < n; ++i) {
      const float* p = xyz + i * stride;
      float* o = out + 4 * i;
      const int64_t c[3] = {orc_cell_of(&G, p[0], G.minx, G.gx), orc_cell_of(&G, p[1], G.miny, G.gy),
                            orc_cell_of(&G, p[2], G.minz, G.gz)};
      const int64_t dim[3] = {G.gx, G.gy, G.gz};
      const double lo[3] = {G.minx, G.miny, G.minz};
      int sz = 0;
      for (int64_t R = 0;; ++R) {
        for (int64_t z = c[2] - R; z <= c[2] + R; ++z) {
          if (z < 0 || z >= G.gz) continue;
          for (int64_t y = c[1] - R; y <= c[1] + R; ++y) {
            if (y < 0 || y >= G.gy) continue;
            const int shell_zy = (z == c[2] - R || z == c[2] + R || y == c[1] - R || y == c[1] + R);
            for (int64_t x = c[0] - R; x <= c[0] + R; x += (shell_zy || R == 0) ? 1 : 2 * R) {
              if (x < 0 || x >= G.gx) continue;
              int64_t cc = (z * G.gy + y) * G.gx + x;
              for (int64_t t = G.start[cc]; t < G.start[cc + 1]; ++t) {
                int32_t j = G.order[t];
                const float* q = xyz + (int64_t)j * stride;
                float ex = p[0] - q[0], ey = p[1] - q[1], ez = p[2] - q[2];
                orc_nb v;
                v.d = ((0.0f + ex * ex) + ey * ey) + ez * ez;
                v.j = j;
                orc_heap_push(heap, &sz, K, v);
              }
            }
          }
        }
        /* the nearest face of the searched box that still has cells beyond it */
        double lb = INFINITY;
        int open = 0;
        for (int k = 0; k < 3; ++k) {
          if (c[k] - R > 0) { lb = fmin(lb, (double)p[k] - (lo[k] + (double)(c[k] - R) * cell)); open = 1; }
          if (c[k] + R < dim[k] - 1) { lb = fmin(lb, (lo[k] + (double)(c[k] + R + 1) * cell) - (double)p[k]); open = 1; }
        }
        if (!open) break;                                 /* every cell searched */
        if (sz == K && lb > 0.0 && (double)heap[0].d < lb * lb * (1.0 - 1e-5)) break;
      }
      int k = sz;
      if (k < 3) { o[0] = o[1] = o[2] = o[3] = NAN; continue; }
      qsort(heap, (size_t)k, sizeof(orc_nb), orc_nb_cmp);
      for (int t = 0; t < k; ++t) ids[t] = heap[t].j;
      orc_normal_from_ids(xyz, stride, p, ids, k, vp, o);
    }
    free(heap); free(ids);
  }
  orc_grid_free(&G);
}

void orc_estimate_normals_knn(const float* xyz, int64_t n, int64_t stride, int k_nn,
                              const float vp[3], float* out) {
  int finite = 1;
  for (int64_t i = 0; i < n && finite; ++i)
    for (int k = 0; k < 3; ++k)
      if (!isfinite(xyz[i * stride + k])) { finite = 0; break; }
  if (finite && k_nn > 0) orc_knn_grid(xyz, n, stride, k_nn, vp, out);
  else orc_estimate_normals_knn_brute(xyz, n, stride, k_nn, vp, out);
}

/* Dialog/PlaneDetect.h:547-665 (first-round branch; the second-round 1-NN branch at :553-584
 * is not part of this oracle). normals: 4 floats per point. Returns #processed points. */
int64_t orc_regulate_normals(const float* xyz, int64_t n, int64_t stride, float* normals,
                             int64_t seed_idx, int seed_is_outward, float radius,
                             uint8_t* processed) {
  if (seed_idx < 0 || seed_idx >= n) return 0;   /* "invalid point index" */
  memset(processed, 0, (size_t)n);
  orc_grid G;
  orc_grid_build(&G, xyz, n, stride, radius);
  float r2 = (float)((double)radius * (double)radius);
  if (!seed_is_outward) {
    float* s = normals + 4 * seed_idx;
    s[0] *= -1.0f; s[1] *= -1.0f; s[2] *= -1.0f;
  }
  processed[seed_idx] = 1;
  int32_t* Q = (int32_t*)malloc((size_t)n * sizeof(int32_t));
  int64_t qh = 0, qt = 0, cnt = 1;
  Q[qt++] = (int32_t)seed_idx;
  orc_nb* nb = NULL; int64_t cap = 0;
  while (qh < qt) {
    int32_t cur = Q[qh++];
    int64_t k = orc_radius(&G, xyz, stride, xyz + (int64_t)cur * stride, r2, &nb, &cap);
    for (int64_t t = 0; t < k; ++t) {
      int32_t j = nb[t].j;
      if (processed[j]) continue;
      const float* pc = normals + 4 * (int64_t)cur;
      float* pn = normals + 4 * (int64_t)j;
      float dp = pc[0] * pn[0] + pc[1] * pn[1] + pc[2] * pn[2];
      if (dp < 0.0f) { pn[0] *= -1.0f; pn[1] *= -1.0f; pn[2] *= -1.0f; }
      processed[j] = 1;
      ++cnt;
      Q[qt++] = j;
    }
  }
  free(Q); free(nb);
  orc_grid_free(&G);
  return cnt;
}

/* Dialog/PlaneDetect.h:553-584 (later-round branch of regulateNormal): nearest neighbour of each
 * point in the backup cloud (FLANN L2 dist2, k = 1; equidistant -> lowest index), flip when the
 * Vector3f dot (a0 b0 + a1 b1) + a2 b2 is negative.  Brute force: test-sized clouds only. */
void orc_orient_normals_nn(const float* xyz, int64_t n, int64_t stride, float* normals,
                           const float* ref_xyz, int64_t m, int64_t ref_stride,
                           const float* ref_normals) {
  for (int64_t i = 0; i < n; ++i) {
    const float* q = xyz + i * stride;
    float bd = INFINITY;
    int64_t bj = -1;
    for (int64_t j = 0; j < m; ++j) {
      const float* p = ref_xyz + j * ref_stride;
      float ex = q[0] - p[0], ey = q[1] - p[1], ez = q[2] - p[2];
      float d = ((0.0f + ex * ex) + ey * ey) + ez * ez;
      if (d < bd) { bd = d; bj = j; }
    }
    if (bj < 0) continue;
    float* a = normals + 4 * i;
    const float* b = ref_normals + 4 * bj;
    float dd = (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2];
    if (dd < 0.0f) { a[0] *= -1.0f; a[1] *= -1.0f; a[2] *= -1.0f; }
  }
}

/* Dialog/PlaneDetect.h:448-512 preProcess(), restated literally: removeNaNFromPointCloud (drop
 * points with a non-finite coordinate), optional translation to the centroid (pcl::PointXYZ p:
 * float sums in index order, then /= float(n), then every point -= p), then the redundancy loop
 * with radiusSearch results sorted by (dist2, index) and indices[0] skipped.  out_xyz: 3 floats
 * per kept point; out_index: input index.  Returns the number kept. */
int64_t orc_preprocess(const float* xyz, int64_t n, int64_t stride, int translate, float min_dist,
                       float* out_xyz, int32_t* out_index, float translation[3]) {
  float* pts = (float*)malloc((size_t)(n > 0 ? n : 1) * 3 * sizeof(float));
  int32_t* src = (int32_t*)malloc((size_t)(n > 0 ? n : 1) * sizeof(int32_t));
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + i * stride;
    if (!isfinite(p[0]) || !isfinite(p[1]) || !isfinite(p[2])) continue;
    pts[3 * m] = p[0]; pts[3 * m + 1] = p[1]; pts[3 * m + 2] = p[2];
    src[m++] = (int32_t)i;
  }
  translation[0] = translation[1] = translation[2] = 0.0f;
  if (translate && m > 0) {
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    for (int64_t i = 0; i < m; ++i) { px += pts[3 * i]; py += pts[3 * i + 1]; pz += pts[3 * i + 2]; }
    px /= (float)m; py /= (float)m; pz /= (float)m;
    for (int64_t i = 0; i < m; ++i) { pts[3 * i] -= px; pts[3 * i + 1] -= py; pts[3 * i + 2] -= pz; }
    translation[0] = px; translation[1] = py; translation[2] = pz;
  }
  int64_t kept = 0;
  if (m > 0) {
    uint8_t* processed = (uint8_t*)calloc((size_t)m, 1);
    float radius = min_dist;
    orc_grid G;
    orc_grid_build(&G, pts, m, 3, radius > 0.0f ? radius : 1.0f);
    float r2 = (float)((double)radius * (double)radius);
    orc_nb* nb = NULL; int64_t cap = 0;
    for (int64_t i = 0; i < m; ++i) {
      if (processed[i]) continue;
      processed[i] = 1;
      out_xyz[3 * kept] = pts[3 * i]; out_xyz[3 * kept + 1] = pts[3 * i + 1];
      out_xyz[3 * kept + 2] = pts[3 * i + 2];
      out_index[kept++] = src[i];
      int64_t k = radius > 0.0f ? orc_radius(&G, pts, 3, pts + 3 * i, r2, &nb, &cap) : 0;
      for (int64_t j = 1; j < k; ++j) processed[nb[j].j] = 1;
    }
    free(nb);
    orc_grid_free(&G);
    free(processed);
  }
  free(pts);
  free(src);
  return kept;
}


/* ------------------------------------------------------------------------------------------ */
/* postProcessPlanes (Dialog/PlaneDetect.h:1454-1579), isPointInPoly (:1891-1964) with its     */
/* helpers isBothLineSegsIntersect (:1966-2015), getInfoBetPointAndPlane (:2018-2022),          */
/* projPoint2Plane (:1437-1443), distP2P (:203-207), and clusterFilt (:1582-1655).             */
/* Vector3f arithmetic as Eigen 3.3 evaluates it (no SSE for 3-vectors):                       */
/*   dot / squaredNorm = a0*b0 + (a1*b1 + a2*b2); normalize: if (z > 0) v /= sqrt(z).          */
/* pow(a, 0.5f) in distP2P is taken as the correctly rounded square root (sqrtf).              */
/* rand(): MSVC CRT LCG; srand(time(0)) runs at every isPointInPoly call, so one call's ten    */
/* edge draws depend on the seed only -- `seed` stands for that time(0) value.                 */
/* ------------------------------------------------------------------------------------------ */
typedef struct { float x, y, z; } orc_v3;

static orc_v3 v3_at(const float* p) { orc_v3 v = {p[0], p[1], p[2]}; return v; }
static orc_v3 v3_sub(orc_v3 a, orc_v3 b) { orc_v3 v = {a.x - b.x, a.y - b.y, a.z - b.z}; return v; }
static float v3_dot(orc_v3 a, orc_v3 b) { return a.x * b.x + (a.y * b.y + a.z * b.z); }
static orc_v3 v3_normalized(orc_v3 v) {
  float z = v.x * v.x + (v.y * v.y + v.z * v.z);
  if (z > 0.0f) { float s = sqrtf(z); v.x /= s; v.y /= s; v.z /= s; }
  return v;
}
static orc_v3 v3_cross(orc_v3 a, orc_v3 b) {
  orc_v3 o = {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x};
  return o;
}
/* distP2P: pow(((dx*dx + dy*dy) + dz*dz), 0.5f) */
static float orc_dist_p2p(orc_v3 a, orc_v3 b) {
  float dx = a.x - b.x, dy = a.y - b.y, dz = a.z - b.z;
  return sqrtf((dx * dx + dy * dy) + dz * dz);
}

/* projPoint2Plane: lambda in float from 2.0 * (float expression), the update in double */
static orc_v3 orc_proj_to_plane(orc_v3 p, const float c[4]) {
  float lam = (float)(2.0 * (double)(((c[0] * p.x + c[1] * p.y) + c[2] * p.z) + c[3]));
  orc_v3 o;
  o.x = (float)((double)p.x - (double)lam / 2.0 * (double)c[0]);
  o.y = (float)((double)p.y - (double)lam / 2.0 * (double)c[1]);
  o.z = (float)((double)p.z - (double)lam / 2.0 * (double)c[2]);
  return o;
}

/* isBothLineSegsIntersect(a, b, c, d), literally: the one statement of the crossing test */
int orc_segs_intersect(const float a[3], const float b[3], const float c[3], const float e[3]) {
  orc_v3 pa = v3_at(a), pb = v3_at(b), pc = v3_at(c), pd = v3_at(e);
  orc_v3 nab = v3_normalized(v3_sub(pb, pa));
  orc_v3 ncd = v3_normalized(v3_sub(pd, pc));
  orc_v3 pa_pc = v3_sub(pc, pa);
  float l1, l2;
  float d = v3_dot(nab, ncd);
  if (fabsf(d) <= 0.001f) {
    l1 = v3_dot(nab, pa_pc);
    l2 = -1.0f * v3_dot(ncd, pa_pc);
  } else if (d >= 0.9999f) {
    return 0;
  } else {
    float c1 = 1.0f - d * d;
    float c2 = v3_dot(nab, pa_pc) * d - v3_dot(ncd, pa_pc);
    l2 = c2 / c1;
    l1 = (l2 + v3_dot(ncd, pa_pc)) / d;
  }
  orc_v3 p1 = {pa.x + l1 * nab.x, pa.y + l1 * nab.y, pa.z + l1 * nab.z};
  orc_v3 p2 = {pc.x + l2 * ncd.x, pc.y + l2 * ncd.y, pc.z + l2 * ncd.z};
  orc_v3 pi = {(p1.x + p2.x) / 2.0f, (p1.y + p2.y) / 2.0f, (p1.z + p2.z) / 2.0f};
  float dpa = orc_dist_p2p(pi, pa), dpb = orc_dist_p2p(pi, pb), dab = orc_dist_p2p(pa, pb);
  float dpc = orc_dist_p2p(pi, pc), dpd = orc_dist_p2p(pi, pd), dcd = orc_dist_p2p(pc, pd);
  return fabsf(dpa + dpb - dab) < 0.001f && fabsf(dpc + dpd - dcd) < 0.001f;
}

uint32_t orc_msvc_rand(uint32_t* state) {
  *state = *state * 214013u + 2531011u;
  return (*state >> 16) & 0x7fffu;
}

/* isPointInPoly up to its vote: returns whether the point is a candidate (dist <= t_dist and a
 * border to test against); *mask bit i = parity of ray i's crossings with the border */
int orc_pip_parities(const float p[3], const float coeff[4], const float* border, int64_t nb,
                     int64_t border_stride, float t_dist, uint32_t seed, uint32_t* mask) {
  *mask = 0;
  orc_v3 q = v3_at(p);
  orc_v3 pp = orc_proj_to_plane(q, coeff);
  float dist = orc_dist_p2p(q, pp);
  if (dist > t_dist) return 0;
  if (nb <= 0) return 0;
  uint32_t st = seed;
  orc_v3 pn = {coeff[0], coeff[1], coeff[2]};
  const float lambda = 10000.0f;
  const float c[3] = {pp.x, pp.y, pp.z};
  for (int i = 0; i < 10; ++i) {
    int64_t index = (int64_t)((uint64_t)orc_msvc_rand(&st) % (uint64_t)nb);
    orc_v3 s = v3_at(border + index * border_stride);
    orc_v3 e = v3_at(border + (index == nb - 1 ? 0 : index + 1) * border_stride);
    orc_v3 dir = v3_normalized(v3_sub(e, s));
    orc_v3 dp = v3_normalized(v3_cross(dir, pn));
    const float pl[3] = {pp.x + lambda * dp.x, pp.y + lambda * dp.y, pp.z + lambda * dp.z};
    int count = 0;
    for (int64_t j = 0; j < nb; ++j) {
      const float* a = border + j * border_stride;
      const float* b = border + (j == nb - 1 ? 0 : j + 1) * border_stride;
      if (orc_segs_intersect(a, b, c, pl)) ++count;
    }
    *mask |= (uint32_t)(count % 2) << i;
  }
  return 1;
}

int orc_is_point_in_poly(const float p[3], const float coeff[4], const float* border, int64_t nb,
                         int64_t border_stride, float t_dist, uint32_t seed) {
  uint32_t mask;
  if (!orc_pip_parities(p, coeff, border, nb, border_stride, t_dist, seed, &mask)) return 0;
  return __builtin_popcount(mask) >= 10 / 2;
}

int orc_compute_point_normal(const float* xyz, int64_t n, int64_t stride, float plane[4],
                             float* curvature) {
  if (n < 3) {
    plane[0] = plane[1] = plane[2] = plane[3] = NAN;
    *curvature = NAN;
    return 0;
  }
  float a[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = 0; i < n; ++i) {
    const float* p = xyz + i * stride;
    float x = p[0], y = p[1], z = p[2];
    a[0] += x * x; a[1] += x * y; a[2] += x * z;
    a[3] += y * y; a[4] += y * z; a[5] += z * z;
    a[6] += x;     a[7] += y;     a[8] += z;
  }
  float cntf = (float)(size_t)n;
  for (int k = 0; k < 9; ++k) a[k] = a[k] / cntf;
  float cov[9];
  cov[0] = a[0] - a[6] * a[6];
  cov[1] = a[1] - a[6] * a[7];
  cov[2] = a[2] - a[6] * a[8];
  cov[4] = a[3] - a[7] * a[7];
  cov[5] = a[4] - a[7] * a[8];
  cov[8] = a[5] - a[8] * a[8];
  cov[3] = cov[1]; cov[6] = cov[2]; cov[7] = cov[5];
  float ev, v[3];
  orc_eigen33(cov, &ev, v);
  float eig_sum = cov[0] + cov[4] + cov[8];
  *curvature = eig_sum != 0.0f ? fabsf(ev / eig_sum) : 0.0f;
  plane[0] = v[0]; plane[1] = v[1]; plane[2] = v[2];
  /* -1 * plane.dot(centroid), Vector4f SSE predux: (p0 c0 + p2 c2) + (p1 c1 + p3 c3), p3 = 0 */
  plane[3] = -1.0f * ((v[0] * a[6] + v[2] * a[8]) + (v[1] * a[7] + 0.0f * 1.0f));
  return 1;
}

/* PlaneDetect.h:1477-1498: refit + orientation by the previous coefficients' normal */
void orc_refit_planes(int n_planes, const float* coeffs_in, const float* pts, int64_t stride,
                      const int64_t* offs, float* coeffs_out) {
  for (int i = 0; i < n_planes; ++i) {
    float prm[4], curv;
    orc_compute_point_normal(pts + offs[i] * stride, offs[i + 1] - offs[i], stride, prm, &curv);
    const float* v = coeffs_in + 4 * i;
    float d = (v[0] * prm[0] + v[2] * prm[2]) + (v[1] * prm[1] + 0.0f * prm[3]);
    if (d < 0.0f)
      for (int k = 0; k < 4; ++k) prm[k] = -1.0f * prm[k];
    memcpy(coeffs_out + 4 * i, prm, sizeof(prm));
  }
}

/* clusterFilt: BFS over radiusSearch(radius) results (sorted, first skipped); clusters with
 * size <= t_cluster_num are dropped.  valid[i] = 1 for the points kept. */
void orc_cluster_filter(const float* xyz, int64_t n, int64_t stride, float radius,
                        int t_cluster_num, uint8_t* valid) {
  if (n <= 0) return;
  uint8_t* proc = (uint8_t*)calloc((size_t)n, 1);
  int32_t* queue = (int32_t*)malloc((size_t)n * sizeof(int32_t));
  int32_t* members = (int32_t*)malloc((size_t)n * sizeof(int32_t));
  memset(valid, 1, (size_t)n);
  orc_grid G;
  orc_grid_build(&G, xyz, n, stride, radius > 0.0f ? radius : 1.0f);
  float r2 = (float)((double)radius * (double)radius);
  orc_nb* nb = NULL; int64_t cap = 0;
  int64_t scan = 0;
  for (;;) {
    while (scan < n && proc[scan]) ++scan;  /* getSeedIndex: first unprocessed */
    if (scan == n) break;
    int64_t qh = 0, qt = 0, nm = 0;
    queue[qt++] = (int32_t)scan;
    members[nm++] = (int32_t)scan;
    while (qh < qt) {
      int32_t cur = queue[qh++];
      proc[cur] = 1;
      float q[3] = {xyz[cur * stride], xyz[cur * stride + 1], xyz[cur * stride + 2]};
      int64_t k = radius > 0.0f ? orc_radius(&G, xyz, stride, q, r2, &nb, &cap) : 0;
      for (int64_t j = 1; j < k; ++j) {
        int32_t v = nb[j].j;
        if (proc[v]) continue;
        queue[qt++] = v;
        members[nm++] = v;
        proc[v] = 1;
      }
    }
    if ((uint64_t)nm <= (uint64_t)(int64_t)t_cluster_num)
      for (int64_t i = 0; i < nm; ++i) valid[members[i]] = 0;
  }
  free(nb);
  orc_grid_free(&G);
  free(members);
  free(queue);
  free(proc);
}

/* postProcessPlanes: refit (all planes), isProcessed from the 1-NN of every plane point in the
 * cloud (ties -> lowest index), absorption of the unprocessed points into planes
 * [plane_start, n_planes) (every plane whose polygon contains the point), clusterFilt of the
 * rest.  absorbed: n_planes x n flags; remaining: n flags (1 = stays in source_cloud). */
void orc_post_process_planes(const float* cloud, int64_t n, int64_t stride, int n_planes,
                             const float* coeffs_in, const float* pts, int64_t pts_stride,
                             const int64_t* pts_off, const float* border, int64_t border_stride,
                             const int64_t* border_off, float t_dist, int plane_start,
                             uint32_t seed, float radius_local, int t_cluster_num,
                             float* coeffs_out, uint8_t* absorbed, uint8_t* remaining) {
  orc_refit_planes(n_planes, coeffs_in, pts, pts_stride, pts_off, coeffs_out);
  uint8_t* proc = (uint8_t*)calloc((size_t)(n > 0 ? n : 1), 1);
  memset(absorbed, 0, (size_t)n_planes * (size_t)n);
  if (n > 0)
    for (int64_t t = 0; t < pts_off[n_planes]; ++t) {
      const float* q = pts + t * pts_stride;
      float bd = INFINITY;
      int64_t bj = -1;
      for (int64_t j = 0; j < n; ++j) {
        const float* p = cloud + j * stride;
        float ex = q[0] - p[0], ey = q[1] - p[1], ez = q[2] - p[2];
        float d = ((0.0f + ex * ex) + ey * ey) + ez * ez;
        if (d < bd) { bd = d; bj = j; }
      }
      if (bj >= 0) proc[bj] = 1;
    }
  for (int64_t i = 0; i < n; ++i) {
    if (proc[i]) continue;
    for (int ii = plane_start; ii < n_planes; ++ii) {
      if (orc_is_point_in_poly(cloud + i * stride, coeffs_out + 4 * ii,
                               border + border_off[ii] * border_stride,
                               border_off[ii + 1] - border_off[ii], border_stride, t_dist, seed)) {
        proc[i] = 1;
        absorbed[(int64_t)ii * n + i] = 1;
      }
    }
  }
  int64_t m = 0;
  for (int64_t i = 0; i < n; ++i) m += !proc[i];
  float* rest = (float*)malloc((size_t)(m > 0 ? m : 1) * 3 * sizeof(float));
  int64_t* rid = (int64_t*)malloc((size_t)(m > 0 ? m : 1) * sizeof(int64_t));
  uint8_t* ok = (uint8_t*)malloc((size_t)(m > 0 ? m : 1));
  m = 0;
  for (int64_t i = 0; i < n; ++i)
    if (!proc[i]) {
      memcpy(rest + 3 * m, cloud + i * stride, 3 * sizeof(float));
      rid[m++] = i;
    }
  memset(remaining, 0, (size_t)n);
  orc_cluster_filter(rest, m, 3, radius_local, t_cluster_num, ok);
  for (int64_t t = 0; t < m; ++t) remaining[rid[t]] = ok[t];
  free(ok);
  free(rid);
  free(rest);
  free(proc);
}
