// fpfh_host.cpp -- host driver of the FPFH descriptors: dlg_fpfh_estimate and dlg_cloud_fpfh
// (include/dialog_ransac.h; pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33> as
// Dialog/PCLViewer.cpp:524-543 calls it).
//
// The points are the normals path's nw.x/y/z (the caller's records de-interleaved, or the cloud's
// device copy), the normals float4 rows in nw.nrm.  One grid with cell edge >= the radius is built
// over all points, the normals are gathered into its sorted order, k_fpfh_spfh fills the n x 33
// table of every finite point and k_fpfh_weight one row per list entry.
// The host waits for the bounding box and the grid build (the existing helpers read back a word
// each), then for the copy out.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>

#include "cloud_call.hpp"
#include "fpfh.hpp"
#include "grid_host.hpp"
#include "normals.hpp"
#include "segment.hpp"  // event_ms

namespace dlg {
namespace {

// (the checks of both entry points but the points' and the list's)
void check_call(dlg_ctx* c, const dlg_fpfh_params* prm, int64_t hist_stride) {
  check_whole_cloud(c->comm->world(), "FPFH");
  if (!std::isfinite(prm->search_radius) || !(prm->search_radius > 0.0f))
    throw DlgError(DLG_ERR_INVALID, "search_radius must be finite and > 0");
  if (hist_stride < 4 * kFpfhDim || hist_stride % 4)
    throw DlgError(DLG_ERR_INVALID, "hist_stride_bytes must be >= 132 and a multiple of 4");
}

// the points in nw.x/y/z (bounding box b), the normals in nw.nrm; everything from the grid build to
// the copies out
void fpfh_core(dlg_ctx* c, int n, const BBox& b, const int32_t* indices, int m,
               const dlg_fpfh_params* prm, float* hist_out, int64_t hist_stride,
               int32_t* neighbours, int32_t* spfh_counts, dlg_fpfh_stats* stats) {
  NormalsWork& w = c->nw;
  FpfhWork& v = c->fw;
  unsigned long long acc[kFpfhAccWords] = {};
  v.acc.ensure(kFpfhAccWords);
  HIPCHK(hipMemsetAsync(v.acc.p, 0, 8 * (size_t)kFpfhAccWords, c->stream));
  launch_count_finite(w.x.p, w.y.p, w.z.p, n, v.acc.p + kFpfhFinite, c->stream);
  const bool run = n > 0 && m > 0;
  if (run) {
    if (!hist_out) throw DlgError(DLG_ERR_INVALID, "hist_out is null");
    const int32_t* didx = stage_list(c, indices, m);
    const size_t table = (size_t)n * kFpfhDim;
    v.snrm.ensure(n); v.spfh.ensure(table); v.cnt.ensure(n); v.pairs.ensure(n);
    v.hist.ensure((size_t)m * kFpfhDim); v.o_nb.ensure(m);
    if (spfh_counts) v.counts.ensure(table);
    mark(c, 0);
    GridBufs B;
    const GridDesc G = make_grid(b, (double)prm->search_radius);
    build_grid(c, n, G, 0, &B);  // (synchronises)
    mark(c, 1);
    const double r = (double)prm->search_radius;
    const float r2 = (float)(r * r);  // KdTreeFLANN: radius * radius
    launch_fpfh_sort_normals(B, n, w.nrm.p, v.snrm.p, c->stream);
    if (spfh_counts) HIPCHK(hipMemsetAsync(v.counts.p, 0, 4 * table, c->stream));
    launch_fpfh_spfh(G, B, n, r2, v.snrm.p, v.spfh.p, spfh_counts ? v.counts.p : nullptr, v.cnt.p,
                     v.pairs.p, c->num_cus, c->stream);
    mark(c, 2);
    launch_fpfh_weight(G, B, n, r2, didx, m, w.x.p, w.y.p, w.z.p, v.spfh.p, v.pairs.p,
                       v.hist.p, v.o_nb.p, v.acc.p, c->num_cus, c->stream);
    HIPCHK(hipGetLastError());
    mark(c, 3);
    HIPCHK(hipMemcpy2DAsync(hist_out, (size_t)hist_stride, v.hist.p, 4 * (size_t)kFpfhDim,
                            4 * (size_t)kFpfhDim, (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (neighbours)
      HIPCHK(hipMemcpyAsync(neighbours, v.o_nb.p, 4 * (size_t)m, hipMemcpyDeviceToHost, c->stream));
    if (spfh_counts)
      HIPCHK(hipMemcpyAsync(spfh_counts, v.counts.p, 4 * table, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(hipMemcpyAsync(acc, v.acc.p, sizeof(acc), hipMemcpyDeviceToHost, c->stream));
  sync(c);
  if (!stats) return;
  stats->n_finite = (int64_t)acc[kFpfhFinite];
  stats->n_nan_rows = (int64_t)acc[kFpfhNanRows];
  stats->n_zero_rows = (int64_t)acc[kFpfhZeroRows];
  stats->max_neighbours = (int64_t)acc[kFpfhMaxNb];
  stats->n_lds_overflow = (int64_t)acc[kFpfhNOverflow];
  stats->n_pairs = (int64_t)acc[kFpfhPairs];
  stats->n_pairs_failed = (int64_t)acc[kFpfhPairsFailed];
  stats->n_sum_literal = (int64_t)acc[kFpfhLiteral];
  if (c->profiling && run) {
    stats->device_ms = event_ms(c, 0, 3);
    stats->build_ms = event_ms(c, 0, 1);
    stats->spfh_ms = event_ms(c, 1, 2);
    stats->weight_ms = event_ms(c, 2, 3);
  }
}

}  // namespace
}  // namespace dlg

extern "C" {

dlg_status dlg_fpfh_estimate(dlg_ctx* c, const dlg_points* pts, const float* normals,
                             int64_t normals_stride_bytes, const int32_t* indices,
                             int64_t n_indices, const dlg_fpfh_params* prm, float* hist_out,
                             int64_t hist_stride_bytes, int32_t* neighbours, int32_t* spfh_counts,
                             dlg_fpfh_stats* stats) {
  if (!c || !prm) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_points(pts);
    if (!normals) throw DlgError(DLG_ERR_INVALID, "normals is null");
    if (normals_stride_bytes < 12 || normals_stride_bytes % 4)
      throw DlgError(DLG_ERR_INVALID, "normals_stride_bytes must be >= 12 and a multiple of 4");
    check_call(c, prm, hist_stride_bytes);
    const int n = (int)pts->n;
    const int m = check_list(indices, n_indices, n);
    NormalsWork& w = c->nw;
    BBox b = {};
    if (n > 0) {
      b = upload_points(c, pts);  // (nw.raw, nw.x/y/z; synchronises)
      const size_t nbytes = (size_t)n * (size_t)normals_stride_bytes;
      w.out.ensure(nbytes);
      w.nrm.ensure(n);
      HIPCHK(hipMemcpyAsync(w.out.p, normals, nbytes, hipMemcpyHostToDevice, c->stream));
      launch_unpack_normals(reinterpret_cast<const float*>(w.out.p), n, normals_stride_bytes / 4,
                            w.nrm.p, c->stream);
    }
    fpfh_core(c, n, b, indices, m, prm, hist_out, hist_stride_bytes, neighbours, spfh_counts,
              stats);
  });
}

dlg_status dlg_cloud_fpfh(dlg_ctx* c, dlg_cloud* cl, const dlg_fpfh_params* prm, float* hist_out,
                          int64_t hist_stride_bytes, int32_t* neighbours, dlg_fpfh_stats* stats) {
  if (!c || !cl || cl->ctx != c || !prm) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    if (!cl->has_normals) throw DlgError(DLG_ERR_INVALID, "the cloud has no normals attached");
    check_call(c, prm, hist_stride_bytes);
    const int n = (int)cl->n_total;
    NormalsWork& w = c->nw;
    BBox b = {};
    if (n > 0) {
      // the cloud's own device copy (upload order) and its attached normals
      w.x.ensure(n); w.y.ensure(n); w.z.ensure(n); w.nrm.ensure(n);
      const size_t nb = 4 * (size_t)n;
      HIPCHK(hipMemcpyAsync(w.x.p, cl->pristine.x.p, nb, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(w.y.p, cl->pristine.y.p, nb, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(w.z.p, cl->pristine.z.p, nb, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(w.nrm.p, cl->raw_nrm.p, 4 * nb, hipMemcpyDeviceToDevice, c->stream));
      b = bbox_of(c, w.x.p, w.y.p, w.z.p, n);
    }
    fpfh_core(c, n, b, nullptr, n, prm, hist_out, hist_stride_bytes, neighbours, nullptr, stats);
  });
}

}  // extern "C"
