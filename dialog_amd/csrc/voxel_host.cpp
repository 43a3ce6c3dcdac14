// voxel_host.cpp -- host driver of the voxel-grid filter: dlg_voxel_grid and dlg_voxel_grid_cloud
// (include/dialog_ransac.h; pcl::VoxelGrid<PointXYZ> as Dialog/PCLViewer.cpp:245-253, 283-300 and
// 313-332 call it).
//
// The caller's records go up as they are (one DMA); the de-interleave, the gather by the index
// list, the finite flags and the bounds run on the device.  The host takes the six bounds, derives
// the grid (voxel_model.hpp: the same functions the key kernel calls) and returns the verdicts
// "leaf too small" / "outside the int range"; keys, the stable sort, the voxel runs and the output
// rows follow on the device, the host reads the counts once, and the centroid kernels write either
// SoA scratch that is packed for one D2H copy (dlg_voxel_grid) or straight into a new cloud's
// pristine list (dlg_voxel_grid_cloud).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

#include "cloud_call.hpp"
#include "normals.hpp"
#include "segment.hpp"  // event_ms
#include "voxel.hpp"

namespace dlg {
namespace {

// one call's state between its phases
struct VoxelCall {
  dlg_ctx* c;
  int n = 0;   // list entries
  int nf = 0;  // finite ones
  int64_t n_voxels = 0, n_out = 0, n_long = 0;
  VoxelDesc g{};
  VoxelRuns R{};

  explicit VoxelCall(dlg_ctx* ctx) : c(ctx) {}

  // validation, upload, bounds, keys, sort, runs and counts (two host synchronisations)
  void prepare(const dlg_points* pts, const int32_t* indices, int64_t n_indices,
               const dlg_voxel_params* prm) {
    check_whole_cloud(c->comm->world(), "voxel grid");
    check_points(pts);
    n = check_list(indices, n_indices, pts->n);
    for (int a = 0; a < 3; ++a)
      if (!(std::isfinite(prm->leaf[a]) && prm->leaf[a] > 0.0f))
        throw DlgError(DLG_ERR_INVALID, "leaf sizes must be finite and > 0");
    if (prm->min_points_per_voxel < 0)
      throw DlgError(DLG_ERR_INVALID, "min_points_per_voxel must be >= 0");
    if (n == 0) return;
    NormalsWork& w = c->nw;
    VoxelWork& v = c->vw;
    // 1. upload, de-interleave + gather, finite flags
    const float* raw = upload_raw(c, pts);
    const int32_t* didx = stage_list(c, indices, n);
    mark(c, 0);
    w.x.ensure(n); w.y.ensure(n); w.z.ensure(n);
    v.flags.ensure(n);
    w.rec.ensure(n);
    launch_voxel_gather(raw, pts->stride_bytes / 4, didx, n,
                        w.x.p, w.y.p, w.z.p, w.rec.p, v.flags.p, c->stream);
    // 2. the finite list positions (ascending) and the bounds of the finite entries
    v.fin_pos.ensure(n);
    w.sort_tmp.ensure(voxel_tmp_bytes(n));
    w.counters.ensure(8);
    w.h_cnt.ensure(8);
    HIPCHK(select_flagged(w.sort_tmp.p, w.sort_tmp.cap, v.flags.p, n, v.fin_pos.p, w.counters.p,
                          c->stream));
    const int nb = bbox_blocks(n);
    w.partial.ensure(6 * (size_t)nb);
    launch_bbox(w.x.p, w.y.p, w.z.p, n, w.partial.p, c->stream);
    HIPCHK(hipGetLastError());
    std::vector<float> part(6 * (size_t)nb);
    HIPCHK(hipMemcpyAsync(w.h_cnt.p, w.counters.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(part.data(), w.partial.p, part.size() * 4, hipMemcpyDeviceToHost,
                          c->stream));
    sync(c);
    nf = (int)w.h_cnt.p[0];
    if (nf == 0) return;  // (before any check: PCL's own arithmetic is undefined there)
    float mn[3] = {INFINITY, INFINITY, INFINITY}, mx[3] = {-INFINITY, -INFINITY, -INFINITY};
    for (int i = 0; i < nb; ++i)
      for (int k = 0; k < 3; ++k) {
        mn[k] = std::fmin(mn[k], part[6 * i + k]);
        mx[k] = std::fmax(mx[k], part[6 * i + 3 + k]);
      }
    // 3. the grid (steps 4-6 of the restatement, on the host)
    const int verdict = voxel_make_desc(prm->leaf, mn, mx, &g);
    if (verdict == kVoxelTooSmall)
      throw DlgError(DLG_ERR_INVALID, "leaf size too small: voxel indices would overflow");
    if (verdict == kVoxelOutOfInt)
      throw DlgError(DLG_ERR_INVALID, "leaf size too small for the cloud's coordinates: "
                                      "floorf(coordinate / leaf) is outside the int range");
    // 4. keys, 5. stable sort by key over the bits div0 * div1 * div2 needs
    v.keys_in.ensure(nf); v.keys_out.ensure(nf); v.pos_in.ensure(nf); v.pos_out.ensure(nf);
    w.sort_tmp.ensure(sort_tmp_bytes(nf, voxel_key_bits(g)));  // (never above the 32-bit figure)
    launch_voxel_keys(g, v.fin_pos.p, nf, w.x.p, w.y.p, w.z.p, v.keys_in.p, v.pos_in.p, c->stream);
    HIPCHK(voxel_sort(w.sort_tmp.p, w.sort_tmp.cap, v.keys_in.p, v.keys_out.p, v.pos_in.p,
                      v.pos_out.p, nf, voxel_key_bits(g), c->stream));
    // 6. voxel runs, the min_points filter, output rows, the wave kernel's voxels
    v.head.ensure(nf); v.vid.ensure(nf); v.vstart.ensure((size_t)nf + 1);
    v.keep.ensure(nf); v.row.ensure(nf); v.lflag.ensure(nf); v.long_list.ensure(nf);
    R = VoxelRuns{v.head.p, v.vid.p, v.vstart.p, v.keep.p, v.row.p, v.lflag.p, v.long_list.p,
                  w.counters.p + 4, w.sort_tmp.p, w.sort_tmp.cap};
    HIPCHK(voxel_runs(v.keys_out.p, nf, prm->min_points_per_voxel, c->opt.voxel_long_run, R,
                      c->stream));
    HIPCHK(hipMemcpyAsync(w.h_cnt.p + 4, R.cnt, 4 * kVoxCounts, hipMemcpyDeviceToHost, c->stream));
    sync(c);
    n_voxels = w.h_cnt.p[4 + kVoxN];
    n_out = w.h_cnt.p[4 + kVoxKept];
    n_long = w.h_cnt.p[4 + kVoxLong];
  }

  // 7. the coordinates in sorted order, 8. the centroids into O's rows
  void centroids(const VoxelOut& O) {
    if (n_out == 0) return;
    NormalsWork& w = c->nw;
    VoxelWork& v = c->vw;
    v.sx.ensure(nf); v.sy.ensure(nf); v.sz.ensure(nf);
    launch_voxel_sorted(v.pos_out.p, nf, w.rec.p, v.sx.p, v.sy.p, v.sz.p, c->stream);
    launch_voxel_centroids(R, (int)n_voxels, (int)n_long, c->opt.voxel_long_run, v.sx.p, v.sy.p,
                           v.sz.p, O, c->stream);
    HIPCHK(hipGetLastError());
  }

  // voxel_of_entry on the device (when the caller asks for it); the last kernel of a call, so the
  // timing's end event follows it, ahead of every copy to the host
  void entries(bool wanted) {
    if (wanted && nf > 0) {
      VoxelWork& v = c->vw;
      v.voe.ensure(n);
      HIPCHK(hipMemsetAsync(v.voe.p, 0xff, 4 * (size_t)n, c->stream));
      launch_voxel_scatter(R, v.pos_out.p, nf, v.voe.p, c->stream);
      HIPCHK(hipGetLastError());
    }
    if (n > 0) mark(c, 1);
  }

  // voxel_of_entry -> the caller (enqueued; the caller synchronises)
  void copy_entries(int32_t* voe_host) {
    if (!voe_host || n == 0) return;
    if (nf == 0) {
      std::memset(voe_host, 0xff, 4 * (size_t)n);
      return;
    }
    HIPCHK(hipMemcpyAsync(voe_host, c->vw.voe.p, 4 * (size_t)n, hipMemcpyDeviceToHost, c->stream));
  }

  // (after the stream has been synchronised)
  void stats(dlg_voxel_stats* st) {
    if (!st) return;
    std::memset(st, 0, sizeof(*st));
    st->n_finite = nf;
    st->n_voxels = n_voxels;
    if (nf > 0) {
      std::memcpy(st->div, g.div, sizeof(g.div));
      std::memcpy(st->min_b, g.min_b, sizeof(g.min_b));
    }
    if (c->profiling && n > 0) st->device_ms = event_ms(c, 0, 1);
  }
};

}  // namespace
}  // namespace dlg

extern "C" {

dlg_status dlg_voxel_grid(dlg_ctx* c, const dlg_points* pts, const int32_t* indices,
                          int64_t n_indices, const dlg_voxel_params* prm, float* out_xyz,
                          int64_t out_stride_bytes, int64_t cap, int64_t* n_out,
                          int32_t* counts_out, int32_t* voxel_of_entry, dlg_voxel_stats* stats) {
  if (!c || !prm || !n_out) return DLG_ERR_INVALID;
  *n_out = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_out_stride(out_stride_bytes);
    VoxelCall vc(c);
    vc.prepare(pts, indices, n_indices, prm);
    *n_out = vc.n_out;
    if (vc.n_out > cap)
      throw DlgError(DLG_ERR_CAPACITY, "output too small: need " + std::to_string(vc.n_out));
    if (vc.n_out > 0 && !out_xyz) throw DlgError(DLG_ERR_INVALID, "out_xyz is null");
    VoxelWork& v = c->vw;
    const size_t k = (size_t)vc.n_out;
    const size_t obytes = k * (size_t)out_stride_bytes;
    if (k > 0) {
      v.ox.ensure(k); v.oy.ensure(k); v.oz.ensure(k); v.ocnt.ensure(k);
      vc.centroids(VoxelOut{v.ox.p, v.oy.p, v.oz.p, v.ocnt.p, nullptr, 0});
      c->nw.out.ensure(obytes);
      launch_voxel_pack(v.ox.p, v.oy.p, v.oz.p, (int)k, reinterpret_cast<float*>(c->nw.out.p),
                        out_stride_bytes / 4, c->stream);
      HIPCHK(hipGetLastError());
    }
    vc.entries(voxel_of_entry != nullptr);
    if (k > 0) {
      HIPCHK(hipMemcpyAsync(out_xyz, c->nw.out.p, obytes, hipMemcpyDeviceToHost, c->stream));
      if (counts_out)
        HIPCHK(hipMemcpyAsync(counts_out, v.ocnt.p, 4 * k, hipMemcpyDeviceToHost, c->stream));
    }
    vc.copy_entries(voxel_of_entry);
    sync(c);
    vc.stats(stats);
  });
}

dlg_status dlg_voxel_grid_cloud(dlg_ctx* c, const dlg_points* pts, const int32_t* indices,
                                int64_t n_indices, const dlg_voxel_params* prm, int32_t id_base,
                                dlg_cloud** out, int64_t* n_out, int32_t* voxel_of_entry,
                                dlg_voxel_stats* stats) {
  if (!c || !prm || !out || !n_out) return DLG_ERR_INVALID;
  *n_out = 0;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  VoxelCall vc(c);
  return make_cloud(
      c, id_base, out,
      [&](dlg_cloud& cl) {
        vc.prepare(pts, indices, n_indices, prm);
        *n_out = vc.n_out;
        // the centroids and the ids straight into the cloud's pristine list (no host copy of them)
        SoA& rows = cloud_rows(cl, vc.n_out);
        vc.centroids(VoxelOut{rows.x.p, rows.y.p, rows.z.p, nullptr, rows.gid.p, id_base});
        vc.entries(voxel_of_entry != nullptr);
        vc.copy_entries(voxel_of_entry);
        return vc.n_out;
      },
      [&](dlg_cloud&) { vc.stats(stats); });
}

}  // extern "C"
