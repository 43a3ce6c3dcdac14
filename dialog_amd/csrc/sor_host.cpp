// sor_host.cpp -- host driver of the statistical outlier filter: dlg_statistical_outlier_removal
// and dlg_statistical_outlier_removal_cloud (include/dialog_ransac.h;
// pcl::StatisticalOutlierRemoval<PointXYZ> as Dialog/PCLViewer.cpp:334-358 calls it).
//
// The caller's records go up as they are; the finite points are compacted into the shared nw.x/y/z
// (flag_points / keep_flagged, cloud_call.hpp) and searched through its grid hierarchy (a level is built only once a query is sent to
// it).  k_sor_knn leaves one mean distance per finite point that the list names, the entries take
// theirs, one reduction certifies the two statistics sums (else the host runs the literal loops
// over a copy of the distances), the host derives the threshold (sor_model.hpp) and the device
// classifies and compacts.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "cloud_call.hpp"
#include "grid_host.hpp"
#include "normals.hpp"
#include "segment.hpp"  // event_ms
#include "sor.hpp"

namespace dlg {
namespace {

struct SorCall {
  dlg_ctx* c;
  int n = 0;   // points of the cloud
  int m = 0;   // list entries
  int nf = 0;  // finite points
  const int32_t* didx = nullptr;  // the list on the device (null: 0..n-1)
  int64_t n_valid = 0, n_keep = 0, n_rem = 0, literal = 0;
  double sum = 0.0, sq_sum = 0.0;
  SorThreshold th{};
  int exact = 0;

  explicit SorCall(dlg_ctx* ctx) : c(ctx) {}

  // everything up to the compacted kept / removed index values in sw.out_keep / sw.out_rem
  void run(const dlg_points* pts, const int32_t* indices, int64_t n_indices,
           const dlg_sor_params* prm) {
    check_whole_cloud(c->comm->world(), "statistical outlier removal");
    check_points(pts);
    n = (int)pts->n;
    m = check_list(indices, n_indices, n);
    if (prm->mean_k < 1 || prm->mean_k > kSorMaxMeanK)
      throw DlgError(DLG_ERR_INVALID, "mean_k must be in 1..255");
    if (!std::isfinite(prm->stddev_mul))
      throw DlgError(DLG_ERR_INVALID, "stddev_mul must be finite");
    const int K = prm->mean_k + 1;
    const auto too_few = [&](int finite) {
      return DlgError(DLG_ERR_INVALID, "fewer than mean_k + 1 finite points (" +
                                           std::to_string(finite) + "): PCL would read past the "
                                           "neighbours FLANN returned");
    };
    if (n == 0) throw too_few(0);  // (whatever the list: an empty one too)
    NormalsWork& w = c->nw;
    SorWork& v = c->sw;
    // 1. upload, de-interleave, the finite points and their ranks
    upload_raw(c, pts);
    didx = stage_list(c, indices, m);
    mark(c, 0);
    w.sort_tmp.ensure(select_tmp_bytes(std::max(n, m)));
    nf = flag_points(c, pts, [&](const float* X, const float* Y, const float* Z, int rows,
                                 uint8_t* flags) {
      launch_finite_flags(X, Y, Z, rows, flags, c->stream);
    });
    if (nf < K) throw too_few(nf);
    if (m == 0) return;  // an empty list: nothing kept, nothing removed
    v.rank.ensure(n);
    HIPCHK(hipMemsetAsync(v.rank.p, 0xff, 4 * (size_t)n, c->stream));
    launch_sor_rank(w.fin_pos.p, nf, v.rank.p, c->stream);
    const BBox b = keep_flagged(c, nf);
    const uint8_t* need = nullptr;
    if (indices) {  // (a list: only the finite points it names are queries; the structure holds them all)
      v.need.ensure(nf);
      HIPCHK(hipMemsetAsync(v.need.p, 0, (size_t)nf, c->stream));
      launch_sor_need(didx, m, v.rank.p, v.need.p, c->stream);
      need = v.need.p;
    }
    // 2. the search, level by level; a level is built once a query is deferred to it
    KnnPlan plan;
    KnnLevels L = build_hierarchy_plan(c, nf, b, K, &plan, 1);
    w.queue.ensure(nf);
    w.processed.ensure(nf);
    w.dflags.ensure((size_t)nf * L.levels);
    if (L.levels > 1)
      HIPCHK(hipMemsetAsync(w.dflags.p + nf, 0, (size_t)nf * (L.levels - 1), c->stream));
    v.dist_pt.ensure(nf);
    v.acc.ensure(kSorAccWords);
    HIPCHK(hipMemsetAsync(v.acc.p, 0, 8 * (size_t)kSorAccWords, c->stream));
    const int force = c->opt.sor_literal & 1;
    for (int l = 0; l < L.levels; ++l) {
      const int32_t* qpos = nullptr;  // level 0: every point
      int nq = nf;
      if (l > 0) {
        const uint8_t* f = w.dflags.p + (size_t)l * nf;
        if (count_flagged(c, f, nf, w.queue.p) == 0) break;  // (deferrals go one level up: nothing above either)
        build_level(c, plan, L, l, nullptr);
        // the flagged queries in this level's cell order
        launch_gather_flags(f, L.idx[l], nf, w.processed.p, c->stream);
        nq = count_flagged(c, w.processed.p, nf, w.queue.p);
        qpos = w.queue.p;
      }
      launch_sor_knn(L, l, qpos, nq, l == 0 ? need : nullptr, prm->mean_k, force, v.dist_pt.p,
                     w.dflags.p, (int64_t)nf, std::min(l + 1, L.levels - 1), v.acc.p + kSorLiteral,
                     c->stream);
      HIPCHK(hipGetLastError());
    }
    // 3. the entries' distances and the statistics
    v.dist.ensure(m);
    launch_sor_entries(didx, m, v.rank.p, v.dist_pt.p, v.dist.p, c->stream);
    launch_sor_stats(didx, m, v.rank.p, v.dist.p, v.acc.p, c->stream);
    HIPCHK(hipGetLastError());
    unsigned long long acc[kSorAccWords];
    HIPCHK(hipMemcpyAsync(acc, v.acc.p, sizeof(acc), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    n_valid = (int64_t)acc[kSorValid];
    literal = (int64_t)acc[kSorLiteral];
    const unsigned __int128 ud = ((unsigned __int128)acc[kSorDHi] << 32) + acc[kSorDLo];
    const unsigned __int128 us = ((unsigned __int128)acc[kSorSHi] << 32) + acc[kSorSLo];
    exact = !(c->opt.sor_literal & 2) && acc[kSorFail] == 0 && (ud >> 53) == 0 && (us >> 53) == 0;
    if (exact) {
      // (all-zero distances leave the unit unset; their sums are 0)
      const int qd = (int)acc[kSorQd] - kSorQBias, qs = (int)acc[kSorQs] - kSorQBias;
      sum = ud ? sor_from_units((uint64_t)ud, qd) : 0.0;
      sq_sum = us ? sor_from_units((uint64_t)us, qs) : 0.0;
    } else {
      std::vector<float> h((size_t)m);
      HIPCHK(hipMemcpyAsync(h.data(), v.dist.p, 4 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
      sync(c);
      sum = sq_sum = 0.0;
      for (int e = 0; e < m; ++e) {
        sum = sor_chain(sum, h[e]);
        sq_sum = sor_chain(sq_sum, sor_square(h[e]));
      }
    }
    th = sor_threshold(sum, sq_sum, n_valid, prm->stddev_mul);
    // 4. classify, compact, the list's index values
    v.keep.ensure(m); v.rem.ensure(m);
    v.sel_keep.ensure(m); v.sel_rem.ensure(m); v.out_keep.ensure(m); v.out_rem.ensure(m);
    launch_sor_classify(v.dist.p, m, th.threshold, prm->negative, v.keep.p, v.rem.p, c->stream);
    HIPCHK(select_flagged(w.sort_tmp.p, w.sort_tmp.cap, v.keep.p, m, v.sel_keep.p,
                          w.counters.p + 4, c->stream));
    HIPCHK(select_flagged(w.sort_tmp.p, w.sort_tmp.cap, v.rem.p, m, v.sel_rem.p, w.counters.p + 5,
                          c->stream));
    launch_sor_emit(v.sel_keep.p, w.counters.p + 4, m, didx, v.out_keep.p, c->stream);
    launch_sor_emit(v.sel_rem.p, w.counters.p + 5, m, didx, v.out_rem.p, c->stream);
    HIPCHK(hipGetLastError());
    mark(c, 1);
    HIPCHK(hipMemcpyAsync(w.h_cnt.p + 4, w.counters.p + 4, 8, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    n_keep = w.h_cnt.p[4];
    n_rem = w.h_cnt.p[5];
  }

  // (after the stream has been synchronised)
  void stats(dlg_sor_stats* st) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->n_finite = nf;
    if (m == 0) return;
    st->n_valid = n_valid;
    st->sum = sum;
    st->sq_sum = sq_sum;
    st->mean = th.mean;
    st->stddev = th.stddev;
    st->threshold = th.threshold;
    st->literal_queries = literal;
    st->exact_sums = exact;
    if (c->profiling) st->device_ms = event_ms(c, 0, 1);
  }
};

}  // namespace
}  // namespace dlg

extern "C" {

dlg_status dlg_statistical_outlier_removal(dlg_ctx* c, const dlg_points* pts,
                                           const int32_t* indices, int64_t n_indices,
                                           const dlg_sor_params* prm, int32_t* kept_out,
                                           int64_t cap, int64_t* n_kept, int32_t* removed_out,
                                           int64_t cap_removed, int64_t* n_removed,
                                           float* distances_out, dlg_sor_stats* stats) {
  if (!c || !prm || !n_kept) return DLG_ERR_INVALID;
  *n_kept = 0;
  if (n_removed) *n_removed = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    SorCall sc(c);
    sc.run(pts, indices, n_indices, prm);
    *n_kept = sc.n_keep;
    if (n_removed) *n_removed = sc.n_rem;
    sc.stats(stats);
    if (sc.n_keep > cap)
      throw DlgError(DLG_ERR_CAPACITY, "kept_out too small: need " + std::to_string(sc.n_keep));
    if (removed_out && sc.n_rem > cap_removed)
      throw DlgError(DLG_ERR_CAPACITY, "removed_out too small: need " + std::to_string(sc.n_rem));
    if (sc.n_keep > 0 && !kept_out) throw DlgError(DLG_ERR_INVALID, "kept_out is null");
    if (sc.m == 0) return;
    SorWork& v = c->sw;
    if (sc.n_keep > 0)
      HIPCHK(hipMemcpyAsync(kept_out, v.out_keep.p, 4 * (size_t)sc.n_keep, hipMemcpyDeviceToHost,
                            c->stream));
    if (removed_out && sc.n_rem > 0)
      HIPCHK(hipMemcpyAsync(removed_out, v.out_rem.p, 4 * (size_t)sc.n_rem, hipMemcpyDeviceToHost,
                            c->stream));
    if (distances_out)
      HIPCHK(hipMemcpyAsync(distances_out, v.dist.p, 4 * (size_t)sc.m, hipMemcpyDeviceToHost,
                            c->stream));
    sync(c);
  });
}

dlg_status dlg_statistical_outlier_removal_cloud(dlg_ctx* c, const dlg_points* pts,
                                                 const int32_t* indices, int64_t n_indices,
                                                 const dlg_sor_params* prm, int32_t id_base,
                                                 dlg_cloud** out, int64_t* n_kept,
                                                 int32_t* kept_out, dlg_sor_stats* stats) {
  if (!c || !prm || !out || !n_kept) return DLG_ERR_INVALID;
  *n_kept = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  SorCall sc(c);
  return make_cloud(
      c, id_base, out,
      [&](dlg_cloud& cl) {
        sc.run(pts, indices, n_indices, prm);
        const int64_t k = *n_kept = sc.n_keep;
        SoA& rows = cloud_rows(cl, k);
        if (k > 0) {
          // the kept points and their ids straight into the cloud's pristine list
          NormalsWork& w = c->nw;
          SorWork& v = c->sw;
          launch_gather3(v.out_keep.p, (int)k, w.ax.p, w.ay.p, w.az.p, rows.x.p, rows.y.p, rows.z.p,
                         c->stream);
          launch_sor_ids(rows.gid.p, (int)k, id_base, c->stream);
          HIPCHK(hipGetLastError());
          mark(c, 1);
          if (kept_out)
            HIPCHK(hipMemcpyAsync(kept_out, v.out_keep.p, 4 * (size_t)k, hipMemcpyDeviceToHost,
                                  c->stream));
        }
        return k;
      },
      [&](dlg_cloud&) { sc.stats(stats); });
}

}  // extern "C"
