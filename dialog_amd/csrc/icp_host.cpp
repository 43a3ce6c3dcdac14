// icp_host.cpp -- host driver of the rigid registration: dlg_icp_align and dlg_icp_correspondences
// (include/dialog_ransac.h; pcl::IterativeClosestPoint<PointXYZ, PointXYZ> as
// Dialog/PCLViewer.cpp:581-636 calls it).
//
// Once per call: the target's finite points are compacted into the shared nw.x/y/z and their whole
// grid hierarchy is built (build_target, cloud_call.hpp); the listed source points become the
// working cloud W, which stays on the device.  Per iteration: the level passes (the previous
// iteration's transformation applied at level 0, deferrals counted on the device), the moments pass
// and the publish kernel, then ONE stream synchronisation; the host runs the solve and the criteria
// (icp_model.hpp) and the next level-0 pass takes the 16 floats as its argument.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "cloud_call.hpp"
#include "grid_host.hpp"
#include "icp.hpp"
#include "normals.hpp"
#include "segment.hpp"  // event_ms

namespace dlg {
namespace {

// max_dist^2 as the pairs are tested against it
double squared_limit(double max_dist) {
  if (std::isnan(max_dist) || !(max_dist > 0.0))
    throw DlgError(DLG_ERR_INVALID, "max_correspondence_distance must be > 0");
  const double md2 = max_dist * max_dist;
  return md2 > DBL_MAX ? DBL_MAX : md2;
}

struct IcpCall {
  dlg_ctx* c;
  int m = 0;    // list entries = W's size
  int64_t n_src_finite = 0;
  float guess[16];  // the checked guess (the identity when none is given)
  Target T;         // the finite target points and their hierarchy
  IcpState* st = nullptr;
  IcpState* pub = nullptr;
  int levels_used = 0;
  int64_t syncs = 0;

  explicit IcpCall(dlg_ctx* ctx) : c(ctx) {}

  // the target's hierarchy and W (moved by xf when given); ev[0] is recorded behind the build
  void setup(const dlg_points* src, const int32_t* indices, int64_t n_indices,
             const dlg_points* tgt, const float* xf16) {
    check_whole_cloud(c->comm->world(), "registration");
    check_points(src, "source");
    check_points(tgt, "target");
    m = check_list(indices, n_indices, src->n);
    const int64_t sf = src->stride_bytes / 4;
    for (int i = 0; i < m; ++i) {
      const float* p = src->xyz + (indices ? indices[i] : i) * sf;
      n_src_finite += std::isfinite(p[0]) && std::isfinite(p[1]) && std::isfinite(p[2]);
    }
    check_guess(xf16, guess);
    IcpXf xf{};
    std::memcpy(xf.m, guess, 64);
    const int apply = !icp_is_identity(guess);
    IcpWork& v = c->iw;
    // 1. the target: its finite points and their hierarchy (every level)
    T = build_target(c, tgt,
                     [&](const float* X, const float* Y, const float* Z, int rows, uint8_t* flags) {
                       launch_finite_flags(X, Y, Z, rows, flags, c->stream);
                     },
                     1, "the target has no finite point");
    // 2. W
    const float* raw = upload_raw(c, src);
    const int32_t* didx = stage_list(c, indices, m);
    mark(c, 0);
    const size_t mm = (size_t)std::max(m, 1);
    v.wx.ensure(mm); v.wy.ensure(mm); v.wz.ensure(mm);
    v.qa.ensure(mm); v.qb.ensure(mm); v.nn.ensure(mm); v.d2.ensure(mm);
    v.state.ensure(sizeof(IcpState));
    v.pub.ensure(sizeof(IcpState));
    st = reinterpret_cast<IcpState*>(v.state.p);
    pub = reinterpret_cast<IcpState*>(v.pub.p);
    HIPCHK(hipMemsetAsync(st, 0, sizeof(IcpState), c->stream));
    launch_icp_gather(raw, sf, didx, m, xf, apply, v.wx.p, v.wy.p, v.wz.p, c->opt.icp_max_blocks,
                      c->stream);
    HIPCHK(hipGetLastError());
  }

  // one correspondence pass of W (first moved by xf when apply != 0) and its published sums: one
  // stream synchronisation
  const IcpState& pass(const IcpXf& xf, int apply, double md2) {
    NormalsWork& w = c->nw;  // (the target as build_target left it: ax/ay/az, fin_pos)
    IcpWork& v = c->iw;
    for (int l = 0; l < T.L.levels; ++l)
      launch_icp_level(T.L, l, xf, apply, c->opt.icp_reversed, v.wx.p, v.wy.p, v.wz.p, m,
                       (l & 1) ? v.qa.p : v.qb.p, (l & 1) ? v.qb.p : v.qa.p, st, w.fin_pos.p, md2,
                       v.nn.p, v.d2.p, c->num_cus, c->opt.icp_max_blocks, c->stream);
    launch_icp_finish(v.wx.p, v.wy.p, v.wz.p, m, v.nn.p, v.d2.p, w.ax.p, w.ay.p, w.az.p, T.tmax, st,
                      c->num_cus, c->opt.icp_max_blocks, c->stream);
    launch_icp_publish(st, pub, c->stream);
    HIPCHK(hipGetLastError());
    sync(c);
    ++syncs;
    levels_used = std::max(levels_used, 1);
    for (int l = 1; l < T.L.levels; ++l)
      if (pub->qn[l] > 0) levels_used = std::max(levels_used, l + 1);
    return *pub;
  }
};

int64_t to_digits(const IcpState& s, int64_t* dig) {
  for (int k = 0; k < kIcpDigits; ++k) dig[k] = (int64_t)s.dig[k];
  return dig[0];
}

// getFitnessScore from a pass that kept d2 <= max_range: DBL_MAX when nothing was kept
double fitness_of(const IcpState& s) {
  int64_t dig[kIcpDigits];
  const int64_t k = to_digits(s, dig);
  if (k <= 0) return DBL_MAX;
  const IcpMoments mo = icp_moments(dig);
  return mo.D / (double)k * pow2d(icp_qexp(bits_float(s.d2max)) - kFastBits);
}

}  // namespace

double icp_fitness(dlg_ctx* c, const dlg_points* src, const dlg_points* tgt, const float* xf16,
                   double max_range) {
  IcpCall ic(c);
  ic.setup(src, nullptr, 0, tgt, xf16);
  return fitness_of(ic.pass(IcpXf{}, 0, std::isnan(max_range) ? -1.0 : max_range));
}

}  // namespace dlg

extern "C" {

void dlg_icp_params_default(dlg_icp_params* p) {
  if (!p) return;
  p->max_iterations = 10;
  p->compute_fitness = 0;
  p->max_correspondence_distance = std::sqrt(DBL_MAX);
  p->transformation_epsilon = 0.0;
  p->euclidean_fitness_epsilon = -DBL_MAX;
  p->fitness_max_range = DBL_MAX;
}

dlg_status dlg_icp_align(dlg_ctx* c, const dlg_points* src, const int32_t* indices,
                         int64_t n_indices, const dlg_points* tgt, const dlg_icp_params* prm,
                         const float* guess, float* final_out, float* aligned_out,
                         int64_t out_stride_bytes, dlg_icp_iteration* history_out,
                         int64_t history_cap, dlg_icp_stats* stats) {
  if (!c || !prm || !final_out) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    if (prm->max_iterations < 1) throw DlgError(DLG_ERR_INVALID, "max_iterations must be >= 1");
    const double md2 = squared_limit(prm->max_correspondence_distance);
    if (aligned_out) check_out_stride(out_stride_bytes);
    if (history_out && history_cap < 0) throw DlgError(DLG_ERR_INVALID, "negative history_cap");
    IcpCall ic(c);
    ic.setup(src, indices, n_indices, tgt, guess);
    IcpWork& v = c->iw;
    float fin[16];
    std::memcpy(fin, ic.guess, 64);
    IcpCriteria crit;
    crit.max_iterations = prm->max_iterations;
    crit.rot_thr = 1.0 - prm->transformation_epsilon;
    crit.trans_thr = prm->transformation_epsilon;
    crit.rel_mse = prm->euclidean_fitness_epsilon;
    IcpXf xf{};       // the transformation W has not taken yet
    int pending = 0;
    int iterations = 0, state = kIcpNotConverged;
    int64_t n_corr = 0;
    double mse = 0.0;
    int64_t dig[kIcpDigits];
    for (;;) {
      const IcpState& s = ic.pass(xf, pending, md2);
      pending = 0;
      n_corr = to_digits(s, dig);
      if (n_corr < 3) {
        state = kIcpNoCorrespondences;
        break;
      }
      const int e = icp_qexp(std::fmax(ic.T.tmax, bits_float(s.wmax)));
      const int e2 = icp_qexp(bits_float(s.d2max));
      const IcpMoments mo = icp_moments(dig);
      icp_solve(mo, e, e2, xf.m, &mse);
      pending = 1;
      icp_mul4(xf.m, fin, fin);
      if (history_out && iterations < history_cap) {
        dlg_icp_iteration& h = history_out[iterations];
        h.n_corr = n_corr;
        h.mse = mse;
        h.e = e;
        h.e2 = e2;
        std::memcpy(h.T, xf.m, 64);
      }
      ++iterations;
      state = icp_criteria(crit, iterations, xf.m, mse);
      if (state != kIcpNotConverged) break;
    }
    const int64_t loop_syncs = ic.syncs;
    double fitness = 0.0;
    if (prm->compute_fitness) {
      const double mr = prm->fitness_max_range;
      // (d2 <= max_range is "not d2 > max_range": the pass's own test)
      const IcpState& s = ic.pass(xf, pending, std::isnan(mr) ? -1.0 : mr);
      pending = 0;
      fitness = fitness_of(s);
    }
    if (pending)
      launch_icp_apply(xf, v.wx.p, v.wy.p, v.wz.p, ic.m, c->opt.icp_max_blocks, c->stream);
    if (aligned_out && ic.m > 0) {
      const size_t obytes = (size_t)ic.m * (size_t)out_stride_bytes;
      c->nw.out.ensure(obytes);
      launch_icp_pack(v.wx.p, v.wy.p, v.wz.p, ic.m, reinterpret_cast<float*>(c->nw.out.p),
                      (int)(out_stride_bytes / 4), c->opt.icp_max_blocks, c->stream);
      HIPCHK(hipGetLastError());
      mark(c, 1);
      HIPCHK(hipMemcpyAsync(aligned_out, c->nw.out.p, obytes, hipMemcpyDeviceToHost, c->stream));
    } else {
      mark(c, 1);
    }
    HIPCHK(hipGetLastError());
    sync(c);
    std::memcpy(final_out, fin, 64);
    if (stats) {
      stats->iterations = iterations;
      stats->converged = state != kIcpNotConverged && state != kIcpNoCorrespondences;
      stats->state = state;
      stats->levels = ic.levels_used;
      stats->n_corr = n_corr;
      stats->n_src_finite = ic.n_src_finite;
      stats->n_tgt_finite = ic.T.nf;
      stats->host_syncs = loop_syncs;
      stats->mse = state == kIcpNoCorrespondences && iterations == 0 ? 0.0 : mse;
      stats->fitness = fitness;
      stats->build_ms = ic.T.build_ms;
      if (c->profiling) stats->device_ms = event_ms(c, 0, 1);
    }
  });
}

dlg_status dlg_icp_correspondences(dlg_ctx* c, const dlg_points* src, const int32_t* indices,
                                   int64_t n_indices, const dlg_points* tgt, const float* transform,
                                   double max_dist, int32_t* nn_out, float* d2_out,
                                   int64_t* n_corr) {
  if (!c || !n_corr) return DLG_ERR_INVALID;
  *n_corr = 0;
  return guarded(c, [&] {
    const double md2 = squared_limit(max_dist);
    IcpCall ic(c);
    ic.setup(src, indices, n_indices, tgt, transform);
    const IcpState& s = ic.pass(IcpXf{}, 0, md2);
    *n_corr = (int64_t)s.dig[0];
    IcpWork& v = c->iw;
    if (ic.m > 0 && nn_out)
      HIPCHK(hipMemcpyAsync(nn_out, v.nn.p, 4 * (size_t)ic.m, hipMemcpyDeviceToHost, c->stream));
    if (ic.m > 0 && d2_out)
      HIPCHK(hipMemcpyAsync(d2_out, v.d2.p, 4 * (size_t)ic.m, hipMemcpyDeviceToHost, c->stream));
    sync(c);
  });
}

}  // extern "C"
