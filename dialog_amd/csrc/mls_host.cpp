// mls_host.cpp -- host driver of the moving-least-squares filter: dlg_moving_least_squares and
// dlg_moving_least_squares_cloud (include/dialog_ransac.h; pcl::MovingLeastSquares<PointXYZ,
// PointNormal> as Dialog/PCLViewer.cpp:387-423 calls it).
//
// The caller's records go up as they are and are de-interleaved into the normals path's nw.x/y/z;
// one grid with cell edge >= the radius is built over all of them (non-finite points sort last and
// are in no cell), k_mls leaves one result per point the list names, the entries take theirs, the
// valid ones are compacted in list order and emitted as rows.  The host waits for the bounding box,
// the grid build and the row count (the existing helpers read back a word each), then for the copy
// out.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>

#include "cloud_call.hpp"
#include "grid_host.hpp"
#include "mls.hpp"
#include "normals.hpp"
#include "segment.hpp"  // event_ms

namespace dlg {
namespace {

struct MlsCall {
  dlg_ctx* c;
  int n = 0;  // points of the cloud
  int m = 0;  // list entries
  const int32_t* didx = nullptr;  // the list on the device (null: 0..n-1)
  int64_t n_out = 0;
  unsigned long long acc[kMlsAccWords] = {};

  explicit MlsCall(dlg_ctx* ctx) : c(ctx) {}

  void check(const dlg_points* pts, const int32_t* indices, int64_t n_indices,
             const dlg_mls_params* prm) {
    check_whole_cloud(c->comm->world(), "moving least squares");
    check_points(pts);
    n = (int)pts->n;
    m = check_list(indices, n_indices, n);
    if (prm->polynomial_order < 1 || prm->polynomial_order > kMlsMaxOrder)
      throw DlgError(DLG_ERR_INVALID, "polynomial_order must be in 1..3");
    if (!std::isfinite(prm->search_radius) || !(prm->search_radius > 0.0f))
      throw DlgError(DLG_ERR_INVALID, "search_radius must be finite and > 0");
    if (std::isnan(prm->sqr_gauss_param))
      throw DlgError(DLG_ERR_INVALID, "sqr_gauss_param is NaN");
  }

  // everything up to the compacted list positions of the rows in mw.sel (count: nw.counters[4]);
  // n_out is read back, and the caller emits the rows once it has sized their destination
  void run(const dlg_points* pts, const int32_t* indices, int64_t n_indices,
           const dlg_mls_params* prm) {
    check(pts, indices, n_indices, prm);
    if (n == 0 || m == 0) {
      if (n > 0) count_finite_only(pts);
      return;
    }
    NormalsWork& w = c->nw;
    MlsWork& v = c->mw;
    const BBox b = upload_points(c, pts);  // (nw.raw, nw.x/y/z; synchronises)
    didx = stage_list(c, indices, m);
    v.acc.ensure(kMlsAccWords);
    v.cnt.ensure(n); v.res_p.ensure(n); v.res_n.ensure(n);
    v.valid.ensure(m); v.sel.ensure(m); v.o_nb.ensure(m);
    GridBufs B;
    const GridDesc G = make_grid(b, (double)prm->search_radius);
    build_grid(c, n, G, 0, &B);  // (synchronises)
    mark(c, 0);
    HIPCHK(hipMemsetAsync(v.acc.p, 0, 8 * (size_t)kMlsAccWords, c->stream));
    launch_count_finite(w.x.p, w.y.p, w.z.p, n, v.acc.p + kMlsFinite, c->stream);
    const uint8_t* need = nullptr;
    if (indices) {  // (a list: only the points it names are queries; the grid holds them all)
      v.need.ensure(n);
      HIPCHK(hipMemsetAsync(v.need.p, 0, (size_t)n, c->stream));
      launch_mls_need(didx, m, v.need.p, c->stream);
      need = v.need.p;
    }
    const double r = (double)prm->search_radius;
    const float r2 = (float)(r * r);  // KdTreeFLANN: radius * radius
    const double sqr_gauss = prm->sqr_gauss_param > 0.0 ? prm->sqr_gauss_param : r * r;
    launch_mls(G, B, n, need, r2, prm->polynomial_order, prm->polynomial_fit != 0,
               prm->compute_normals != 0, sqr_gauss, v.res_p.p, v.res_n.p, v.cnt.p, c->num_cus,
               c->stream);
    launch_mls_entries(didx, m, w.x.p, w.y.p, w.z.p, v.cnt.p, v.res_p.p, v.o_nb.p, v.valid.p,
                       v.acc.p, c->stream);
    HIPCHK(hipGetLastError());
    w.sort_tmp.ensure(select_tmp_bytes(m));
    w.counters.ensure(8);
    w.h_cnt.ensure(8);
    HIPCHK(select_flagged(w.sort_tmp.p, w.sort_tmp.cap, v.valid.p, m, v.sel.p, w.counters.p + 4,
                          c->stream));
    HIPCHK(hipMemcpyAsync(w.h_cnt.p + 4, w.counters.p + 4, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(acc, v.acc.p, sizeof(acc), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    n_out = w.h_cnt.p[4];
  }

  // (an empty list over a cloud: n_finite alone)
  void count_finite_only(const dlg_points* pts) {
    NormalsWork& w = c->nw;
    MlsWork& v = c->mw;
    (void)upload_points(c, pts);
    v.acc.ensure(kMlsAccWords);
    HIPCHK(hipMemsetAsync(v.acc.p, 0, 8 * (size_t)kMlsAccWords, c->stream));
    launch_count_finite(w.x.p, w.y.p, w.z.p, n, v.acc.p + kMlsFinite, c->stream);
    HIPCHK(hipMemcpyAsync(acc, v.acc.p, sizeof(acc), hipMemcpyDeviceToHost, c->stream));
    sync(c);
  }

  bool ran() const { return n > 0 && m > 0; }

  // (after the stream has been synchronised)
  void stats(dlg_mls_stats* st) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->n_finite = (int64_t)acc[kMlsFinite];
    st->n_out = n_out;
    st->n_too_few = (int64_t)acc[kMlsNTooFew];
    st->n_plane_only = (int64_t)acc[kMlsNPlane];
    st->n_fit_nonfinite = (int64_t)acc[kMlsNNonfinite];
    st->max_neighbours = (int64_t)acc[kMlsMaxNb];
    st->n_lds_overflow = (int64_t)acc[kMlsNOverflow];
    if (c->profiling && ran()) st->device_ms = event_ms(c, 0, 1);
  }
};

}  // namespace
}  // namespace dlg

extern "C" {

dlg_status dlg_moving_least_squares(dlg_ctx* c, const dlg_points* pts, const int32_t* indices,
                                    int64_t n_indices, const dlg_mls_params* prm, float* out_xyz,
                                    int64_t out_stride_bytes, float* out_normals, int64_t cap,
                                    int64_t* n_out, int32_t* src_index, int32_t* neighbours,
                                    dlg_mls_stats* stats) {
  if (!c || !prm || !n_out) return DLG_ERR_INVALID;
  *n_out = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_out_stride(out_stride_bytes);
    if (cap < 0) throw DlgError(DLG_ERR_INVALID, "negative cap");
    MlsCall mc(c);
    mc.run(pts, indices, n_indices, prm);
    const int64_t k = mc.n_out;
    *n_out = k;
    if (!mc.ran()) {
      mc.stats(stats);
      return;
    }
    NormalsWork& w = c->nw;
    MlsWork& v = c->mw;
    if (k <= cap && k > 0 && !out_xyz) throw DlgError(DLG_ERR_INVALID, "out_xyz is null");
    if (k <= cap && k > 0) {
      const int64_t sf = out_stride_bytes / 4;
      v.o_xyz.ensure((size_t)k * (size_t)sf);
      v.o_nrm.ensure((size_t)k);
      v.o_src.ensure((size_t)k);
      launch_mls_emit(v.sel.p, w.counters.p + 4, mc.m, mc.didx, v.res_p.p, v.res_n.p, v.o_xyz.p, sf,
                      v.o_nrm.p, v.o_src.p, c->stream);
      HIPCHK(hipGetLastError());
    }
    mark(c, 1);
    if (k > cap) {
      sync(c);
      mc.stats(stats);
      throw DlgError(DLG_ERR_CAPACITY, "output too small: need " + std::to_string(k));
    }
    if (k > 0) {
      HIPCHK(hipMemcpyAsync(out_xyz, v.o_xyz.p, (size_t)k * (size_t)out_stride_bytes,
                            hipMemcpyDeviceToHost, c->stream));
      if (out_normals)
        HIPCHK(hipMemcpyAsync(out_normals, v.o_nrm.p, 16 * (size_t)k, hipMemcpyDeviceToHost,
                              c->stream));
      if (src_index)
        HIPCHK(hipMemcpyAsync(src_index, v.o_src.p, 4 * (size_t)k, hipMemcpyDeviceToHost,
                              c->stream));
    }
    if (neighbours)
      HIPCHK(hipMemcpyAsync(neighbours, v.o_nb.p, 4 * (size_t)mc.m, hipMemcpyDeviceToHost,
                            c->stream));
    sync(c);
    mc.stats(stats);
  });
}

dlg_status dlg_moving_least_squares_cloud(dlg_ctx* c, const dlg_points* pts,
                                          const int32_t* indices, int64_t n_indices,
                                          const dlg_mls_params* prm, int32_t id_base,
                                          dlg_cloud** out, int64_t* n_out, int32_t* src_index,
                                          dlg_mls_stats* stats) {
  if (!c || !prm || !out || !n_out) return DLG_ERR_INVALID;
  *n_out = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  MlsCall mc(c);
  MlsWork& v = c->mw;
  return make_cloud(
      c, id_base, out,
      [&](dlg_cloud& cl) {
        mc.run(pts, indices, n_indices, prm);
        const int64_t k = *n_out = mc.n_out;
        SoA& rows = cloud_rows(cl, k);
        if (k > 0) {
          // the rows and their ids straight into the cloud's pristine list
          v.o_nrm.ensure((size_t)k);
          v.o_src.ensure((size_t)k);
          launch_mls_emit_cloud(v.sel.p, c->nw.counters.p + 4, mc.m, mc.didx, v.res_p.p, v.res_n.p,
                                rows.x.p, rows.y.p, rows.z.p, rows.gid.p, id_base, v.o_nrm.p,
                                v.o_src.p, c->stream);
          HIPCHK(hipGetLastError());
          if (src_index)
            HIPCHK(hipMemcpyAsync(src_index, v.o_src.p, 4 * (size_t)k, hipMemcpyDeviceToHost,
                                  c->stream));
        }
        if (mc.ran()) mark(c, 1);
        return k;
      },
      [&](dlg_cloud& cl) {
        if (prm->compute_normals)
          attach_normals(c, &cl, cl.n_total > 0 ? reinterpret_cast<const float*>(v.o_nrm.p) : nullptr,
                         4, 3, true);
        mc.stats(stats);
      });
}

}  // extern "C"
