// gsphere_host.cpp -- host driver of the Gaussian-sphere plane seeds: dlg_gs_space, dlg_gs_vote,
// dlg_gs_segment and dlg_cloud_gs_segment (include/dialog_ransac.h; Dialog/PlaneDetect.h:667-1015
// as PCLViewer.cpp:887-960 and :1133-1151 call it).
//
// The parameter space of the last num_res stays in the context (gw.space, with its dense lattice
// table, and their device copies): building it is a walk over size^3 lattice cubes.  The points are
// the normals path's nw.x/y/z (the caller's records de-interleaved, or the cloud's device copy),
// the normals float4 rows in nw.nrm.  Vote and filter run on the device; the raw and filtered
// votes are read back once; the gradient field and the sink rectification (gsphere_model.hpp) run
// here; the per-cell sinks go back up and the seed planes are labelled, joined and ordered on the
// device.  The host waits four times: the votes, the bounding box and grid build of the points,
// the kept-point count, the plane count with the copies out.
#include <hip/hip_runtime.h>

#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstring>

#include "cloud_call.hpp"
#include "grid_host.hpp"
#include "gsphere.hpp"
#include "gsphere_model.hpp"
#include "normals.hpp"
#include "segment.hpp"  // event_ms

namespace dlg {
namespace {

double now_ms() {
  using namespace std::chrono;
  return duration<double, std::milli>(steady_clock::now().time_since_epoch()).count();
}

bool pos_finite(float v) { return std::isfinite(v) && v > 0.0f; }

// the vote reads num_res alone; the rest only when `all`
void check_params(const dlg_gs_params* p, bool all) {
  if (!gs::valid_res(p->num_res))
    throw DlgError(DLG_ERR_INVALID, "num_res must be finite, > 0 and give at most 512 lattice "
                                    "cells per axis");
  if (!all) return;
  if (!pos_finite(p->std_dev_gaussian) || !pos_finite(p->search_radius_create_gradient) ||
      !pos_finite(p->search_radius_for_plane_seg))
    throw DlgError(DLG_ERR_INVALID, "std_dev_gaussian and the search radii must be finite and > 0");
  if (!std::isfinite(p->radius_base) || !std::isfinite(p->s_threshold) ||
      !std::isfinite(p->dev_threshold))
    throw DlgError(DLG_ERR_INVALID, "radius_base, s_threshold and dev_threshold must be finite");
  const float rmax = gs::rectify_radius_max(p->dev_threshold);
  if (!(p->delta_radius > 0.0f) ||
      (rmax >= p->radius_base &&
       ((double)rmax - (double)p->radius_base) / (double)p->delta_radius > 1e5))
    throw DlgError(DLG_ERR_INVALID, "delta_radius must be > 0 and end the rectification within "
                                    "100000 steps");
  if (p->t_vote_num < 0 || p->t_num_of_single_plane < 0)
    throw DlgError(DLG_ERR_INVALID, "negative threshold");
}

// the parameter space of num_res on the host and the device (kept between calls)
GsSpaceDev space_of(dlg_ctx* c, float num_res, dlg_gs_stats* st) {
  GsWork& g = c->gw;
  if (g.space.size == 0 || std::memcmp(&g.space.num_res, &num_res, 4) != 0) {
    const double t0 = now_ms();
    g.space = gs::Space();  // (a failure below leaves no half-uploaded space behind)
    gs::Space S = gs::build_space(num_res);
    const size_t m = (size_t)S.cells();
    g.table.ensure(S.table.size());
    g.coord.ensure(m); g.px.ensure(m); g.py.ensure(m); g.pz.ensure(m);
    HIPCHK(hipMemcpyAsync(g.table.p, S.table.data(), 4 * S.table.size(), hipMemcpyHostToDevice,
                          c->stream));
    if (m) {
      HIPCHK(hipMemcpyAsync(g.coord.p, S.coord.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(g.px.p, S.px.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(g.py.p, S.py.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(g.pz.p, S.pz.data(), 4 * m, hipMemcpyHostToDevice, c->stream));
    }
    sync(c);
    g.space = std::move(S);
    if (st) st->space_ms = now_ms() - t0;
  }
  return GsSpaceDev{g.table.p, g.coord.p, g.px.p, g.py.p, g.pz.p, g.space.cells(), g.space.size,
                    num_res};
}

// voteForPS of nw.nrm[0..n): gw.cell_of, gw.votes (enqueued; gw.cnt zeroed first)
void enqueue_vote(dlg_ctx* c, const GsSpaceDev& S, int n) {
  GsWork& g = c->gw;
  g.cnt.ensure(kGsCounters);
  g.cell_of.ensure(n); g.queue.ensure(n); g.votes.ensure(S.cells);
  HIPCHK(hipMemsetAsync(g.cnt.p, 0, 8 * (size_t)kGsCounters, c->stream));
  if (S.cells > 0) HIPCHK(hipMemsetAsync(g.votes.p, 0, 4 * (size_t)S.cells, c->stream));
  if (n <= 0) return;
  if (S.cells == 0) {  // (no cell to vote for)
    HIPCHK(hipMemsetAsync(g.cell_of.p, 0xff, 4 * (size_t)n, c->stream));
    return;
  }
  launch_gs_vote(S, c->nw.nrm.p, n, g.cell_of.p, g.votes.p, g.queue.p, g.cnt.p, c->stream);
  launch_gs_vote_all(S, c->nw.nrm.p, g.queue.p, g.cnt.p, g.cell_of.p, g.votes.p, c->num_cus,
                     c->stream);
  HIPCHK(hipGetLastError());
}

// the caller's normal records -> nw.nrm
void upload_normals(dlg_ctx* c, const float* normals, int64_t stride_bytes, int n) {
  if (stride_bytes < 12 || stride_bytes % 4)
    throw DlgError(DLG_ERR_INVALID, "the normals' stride must be >= 12 and a multiple of 4");
  if (n <= 0) return;
  if (!normals) throw DlgError(DLG_ERR_INVALID, "normals is null");
  NormalsWork& w = c->nw;
  const size_t nbytes = (size_t)n * (size_t)stride_bytes;
  w.out.ensure(nbytes);
  w.nrm.ensure(n);
  HIPCHK(hipMemcpyAsync(w.out.p, normals, nbytes, hipMemcpyHostToDevice, c->stream));
  launch_unpack_normals(reinterpret_cast<const float*>(w.out.p), n, stride_bytes / 4, w.nrm.p,
                        c->stream);
}

void check_result(const dlg_gs_result* r) {
  if (!r) throw DlgError(DLG_ERR_INVALID, "result is null");
  if (r->planes_cap < 0 || r->ids_cap < 0 || r->sinks_cap < 0 || r->cells_cap < 0)
    throw DlgError(DLG_ERR_INVALID, "negative capacity");
  if (!r->plane_offsets) throw DlgError(DLG_ERR_INVALID, "plane_offsets is null");
  if ((r->ids_cap > 0 && !r->plane_ids) || (r->sinks_cap > 0 && (!r->sink_cells || !r->sink_votes)))
    throw DlgError(DLG_ERR_INVALID, "a buffer with a capacity is null");
}

// the points in nw.x/y/z, the normals in nw.nrm; everything from the vote to the copies out
void gs_core(dlg_ctx* c, int n, const dlg_gs_params* prm, dlg_gs_result* res, dlg_gs_stats* st) {
  GsWork& g = c->gw;
  NormalsWork& w = c->nw;
  dlg_gs_stats local = {};
  if (!st) st = &local;
  const GsSpaceDev S = space_of(c, prm->num_res, st);
  const gs::Space& H = g.space;
  const int32_t cells = S.cells;
  const size_t cb = 4 * (size_t)cells;
  res->n_cells = cells;
  st->n_cells = cells;
  const bool dbg = res->raw_vote || res->filtered_vote || res->sink_init || res->sink;
  if (dbg && res->cells_cap < cells)
    throw DlgError(DLG_ERR_CAPACITY, "cells_cap too small: need " + std::to_string(cells));

  // ---- vote, filter
  mark(c, 0);
  enqueue_vote(c, S, n);
  mark(c, 1);
  const float radius = (float)(3.0 * prm->std_dev_gaussian);
  const float r2 = gs::radius2(radius);
  const int steps = gs::reach_steps(radius, prm->num_res, S.size);
  std::vector<int32_t> raw((size_t)cells), filt((size_t)cells, 0);
  unsigned long long cnt[kGsCounters] = {};
  if (cells > 0) {
    g.reach.ensure(cells); g.off.ensure(cells); g.cur.ensure(cells); g.filt.ensure(cells);
    g.tmp.ensure(gs_scan_tmp_bytes(cells));
    HIPCHK(hipMemsetAsync(g.reach.p, 0, cb, c->stream));
    HIPCHK(hipMemsetAsync(g.cur.p, 0, cb, c->stream));
    launch_gs_reach(S, g.votes.p, steps, r2, g.reach.p, nullptr, nullptr, nullptr, g.cnt.p,
                    c->stream);
    HIPCHK(launch_gs_scan(g.reach.p, g.off.p, cells, g.tmp.p, g.tmp.cap, c->stream));
    HIPCHK(hipMemcpyAsync(raw.data(), g.votes.p, cb, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(cnt, g.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    const uint64_t pairs = cnt[kGsPairs];  // (the scan's offsets are 32-bit)
    if (pairs > (uint64_t)INT32_MAX)
      throw DlgError(DLG_ERR_INVALID, "the filter's neighbour lists exceed 2^31 entries");
    st->n_filter_pairs = (int64_t)pairs;
    g.keys.ensure(pairs); g.terms.ensure(pairs);
    launch_gs_reach(S, g.votes.p, steps, r2, g.reach.p, g.off.p, g.cur.p, g.keys.p, g.cnt.p,
                    c->stream);
    launch_gs_filter(S, g.votes.p, g.reach.p, g.off.p, g.keys.p, g.terms.p,
                     prm->std_dev_gaussian, g.filt.p, c->stream);
    HIPCHK(hipGetLastError());
    mark(c, 2);
    HIPCHK(hipMemcpyAsync(filt.data(), g.filt.p, cb, hipMemcpyDeviceToHost, c->stream));
  } else {
    mark(c, 2);
    HIPCHK(hipMemcpyAsync(cnt, g.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
  }
  sync(c);
  if (c->profiling) {
    st->vote_ms = event_ms(c, 0, 1);
    st->filter_ms = event_ms(c, 1, 2);
  }
  st->n_occupied = (int64_t)cnt[kGsOccupied];
  st->n_fallback_votes = (int64_t)cnt[kGsQueued];
  for (int32_t v : raw) st->n_voters += v;

  // ---- host: gradient field, sinks
  const double t0 = now_ms();
  std::vector<int32_t> sink_init, sink;
  const std::vector<gs::Sink> sinks =
      gs::gradient_field(H, filt.data(), raw.data(), prm->search_radius_create_gradient,
                         prm->t_vote_num, sink_init);
  gs::rectify_sinks(H, sinks, sink_init, prm->radius_base, prm->delta_radius, prm->s_threshold,
                    prm->dev_threshold, sink);
  st->host_ms = now_ms() - t0;
  const int32_t ns = (int32_t)sinks.size();
  st->n_sinks = ns;
  res->n_sinks = ns;
  res->n_planes = 0;
  res->n_ids = 0;

  // ---- seed planes
  int64_t nk = 0;
  int32_t np = 0;
  bool timed = false;
  if (n > 0 && ns > 0) {
    std::vector<int32_t> rank((size_t)cells, 0);
    for (int32_t k = 0; k < ns; ++k) rank[(size_t)sinks[k].index] = k;
    g.sink.ensure(cells); g.sink_rank.ensure(cells); g.total.ensure(cells);
    g.label.ensure(n); g.lab_s.ensure(n); g.parent.ensure(n); g.size.ensure(n);
    g.root_of.ensure(n); g.ids.ensure(n); g.ids_a.ensure(n); g.ids_b.ensure(n); g.first.ensure(n);
    g.key1.ensure(n); g.key1_out.ensure(n); g.key2.ensure(n); g.key2_out.ensure(n);
    g.heads.ensure(n); g.offs.ensure(n); g.n_planes.ensure(1);
    g.tmp.ensure(gs_sort_tmp_bytes(n));
    HIPCHK(hipMemcpyAsync(g.sink.p, sink.data(), cb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(g.sink_rank.p, rank.data(), cb, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(g.total.p, 0, cb, c->stream));
    const BBox b = bbox_of(c, w.x.p, w.y.p, w.z.p, n);  // (synchronises)
    const double r = (double)prm->search_radius_for_plane_seg;
    const GridDesc G = make_grid(b, r);
    GridBufs B;
    build_grid(c, n, G, 0, &B);  // (synchronises)
    mark(c, 0);
    launch_gs_label(w.x.p, w.y.p, w.z.p, n, g.cell_of.p, g.sink.p, g.label.p, g.total.p, c->stream);
    launch_gs_cc(G, B, n, (float)(r * r), g.label.p, g.lab_s.p, g.parent.p, g.size.p, c->stream);
    launch_gs_keys(B, n, g.lab_s.p, g.parent.p, g.size.p, g.total.p, g.cell_of.p, g.sink_rank.p, ns,
                   (int64_t)prm->t_num_of_single_plane, g.root_of.p, g.key1.p, g.ids.p, g.cnt.p,
                   c->stream);
    int rank_bits = 1;  // (the rank of a point that is not kept is ns)
    while ((1ll << rank_bits) <= (long long)ns) ++rank_bits;
    HIPCHK(launch_gs_sort_list(g.key1.p, g.key1_out.p, g.ids.p, g.ids_a.p, n, 32 + rank_bits,
                               g.tmp.p, g.tmp.cap, c->stream));
    HIPCHK(hipMemcpyAsync(cnt, g.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    nk = (int64_t)cnt[kGsKept];
    if (nk > 0) {
      HIPCHK(launch_gs_order(g.ids_a.p, (int)nk, n, g.root_of.p, g.first.p, g.key2.p, g.key2_out.p,
                             g.ids_b.p, g.heads.p, g.offs.p, g.n_planes.p, g.tmp.p, g.tmp.cap,
                             c->stream));
      HIPCHK(hipMemcpyAsync(&np, g.n_planes.p, 4, hipMemcpyDeviceToHost, c->stream));
    }
    mark(c, 1);
    sync(c);
    timed = true;
  }
  if (c->profiling && timed) st->segment_ms = event_ms(c, 0, 1);
  st->device_ms = st->vote_ms + st->filter_ms + st->segment_ms;
  st->n_planes = np;
  st->n_plane_points = nk;
  res->n_planes = np;
  res->n_ids = nk;
  if (ns > res->sinks_cap)
    throw DlgError(DLG_ERR_CAPACITY, "sinks_cap too small: need " + std::to_string(ns));
  if (np > res->planes_cap)
    throw DlgError(DLG_ERR_CAPACITY, "planes_cap too small: need " + std::to_string(np));
  if (nk > res->ids_cap)
    throw DlgError(DLG_ERR_CAPACITY, "ids_cap too small: need " + std::to_string(nk));

  // ---- out
  for (int32_t k = 0; k < ns; ++k) {
    res->sink_cells[k] = sinks[k].index;
    res->sink_votes[k] = sinks[k].vote_num;
  }
  std::vector<int32_t> offs((size_t)np);
  if (np > 0) {
    HIPCHK(hipMemcpyAsync(offs.data(), g.offs.p, 4 * (size_t)np, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(res->plane_ids, g.ids_b.p, 4 * (size_t)nk, hipMemcpyDeviceToHost,
                          c->stream));
  }
  if (res->cell_of_point && n > 0)
    HIPCHK(hipMemcpyAsync(res->cell_of_point, g.cell_of.p, 4 * (size_t)n, hipMemcpyDeviceToHost,
                          c->stream));
  sync(c);
  for (int32_t k = 0; k < np; ++k) res->plane_offsets[k] = offs[(size_t)k];
  res->plane_offsets[np] = nk;
  if (cells > 0) {
    if (res->raw_vote) std::memcpy(res->raw_vote, raw.data(), cb);
    if (res->filtered_vote) std::memcpy(res->filtered_vote, filt.data(), cb);
    if (res->sink_init) std::memcpy(res->sink_init, sink_init.data(), cb);
    if (res->sink) std::memcpy(res->sink, sink.data(), cb);
  }
}

}  // namespace
}  // namespace dlg

extern "C" {

void dlg_gs_params_default(dlg_gs_params* p) {
  if (!p) return;
  p->num_res = 0.01f;
  p->std_dev_gaussian = 0.05f;
  p->search_radius_create_gradient = 0.03f;
  p->t_vote_num = 500;
  p->radius_base = 0.03f;
  p->delta_radius = 0.01f;
  p->s_threshold = 0.9f;
  p->dev_threshold = 15.0f;
  p->search_radius_for_plane_seg = 0.1f;
  p->t_num_of_single_plane = 500;
}

dlg_status dlg_gs_space(const dlg_gs_params* prm, float* corners_out, int64_t cap,
                        int64_t* n_cells) {
  if (!prm || !n_cells || cap < 0 || !gs::valid_res(prm->num_res)) return DLG_ERR_INVALID;
  try {
    const gs::Space S = gs::build_space(prm->num_res, false);
    *n_cells = S.cells();
    if (!corners_out) return DLG_OK;
    if (cap < S.cells()) return DLG_ERR_CAPACITY;
    for (int32_t k = 0; k < S.cells(); ++k) {
      corners_out[3 * (size_t)k] = S.px[(size_t)k];
      corners_out[3 * (size_t)k + 1] = S.py[(size_t)k];
      corners_out[3 * (size_t)k + 2] = S.pz[(size_t)k];
    }
    return DLG_OK;
  } catch (...) {
    return DLG_ERR_INTERNAL;
  }
}

dlg_status dlg_gs_vote(dlg_ctx* c, const float* normals, int64_t n64, int64_t stride_bytes,
                       const dlg_gs_params* prm, int32_t* cell_of_point, int32_t* votes,
                       int64_t votes_cap, dlg_gs_stats* stats) {
  if (!c || !prm) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_whole_cloud(c->comm->world(), "Gaussian-sphere vote");
    check_params(prm, false);
    if (n64 < 0 || n64 > kMaxGridPoints) throw DlgError(DLG_ERR_INVALID, "n out of range");
    if (n64 > 0 && !cell_of_point) throw DlgError(DLG_ERR_INVALID, "cell_of_point is null");
    const int n = (int)n64;
    upload_normals(c, normals, stride_bytes, n);
    dlg_gs_stats local = {};
    dlg_gs_stats* st = stats ? stats : &local;
    const GsSpaceDev S = space_of(c, prm->num_res, st);
    st->n_cells = S.cells;
    if (votes && votes_cap < S.cells)
      throw DlgError(DLG_ERR_CAPACITY, "votes_cap too small: need " + std::to_string(S.cells));
    mark(c, 0);
    enqueue_vote(c, S, n);
    mark(c, 1);
    GsWork& g = c->gw;
    std::vector<int32_t> raw((size_t)S.cells);
    unsigned long long cnt[kGsCounters] = {};
    if (S.cells > 0)
      HIPCHK(hipMemcpyAsync(raw.data(), g.votes.p, 4 * (size_t)S.cells, hipMemcpyDeviceToHost,
                            c->stream));
    if (n > 0)
      HIPCHK(hipMemcpyAsync(cell_of_point, g.cell_of.p, 4 * (size_t)n, hipMemcpyDeviceToHost,
                            c->stream));
    HIPCHK(hipMemcpyAsync(cnt, g.cnt.p, sizeof(cnt), hipMemcpyDeviceToHost, c->stream));
    sync(c);
    for (int32_t v : raw) {
      st->n_voters += v;
      st->n_occupied += v != 0;
    }
    st->n_fallback_votes = (int64_t)cnt[kGsQueued];
    if (c->profiling) st->device_ms = st->vote_ms = event_ms(c, 0, 1);
    if (votes && S.cells > 0) std::memcpy(votes, raw.data(), 4 * (size_t)S.cells);
  });
}

dlg_status dlg_gs_segment(dlg_ctx* c, const dlg_points* pts, const float* normals,
                          int64_t normals_stride_bytes, const dlg_gs_params* prm,
                          dlg_gs_result* res, dlg_gs_stats* stats) {
  if (!c || !prm) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_whole_cloud(c->comm->world(), "Gaussian-sphere segmentation");
    check_points(pts, "points", kMaxGridPoints);
    check_params(prm, true);
    check_result(res);
    const int n = (int)pts->n;
    if (n > 0) (void)upload_points(c, pts);  // (nw.x/y/z; synchronises)
    upload_normals(c, normals, normals_stride_bytes, n);
    gs_core(c, n, prm, res, stats);
  });
}

dlg_status dlg_cloud_gs_segment(dlg_ctx* c, dlg_cloud* cl, const dlg_gs_params* prm,
                                dlg_gs_result* res, dlg_gs_stats* stats) {
  if (!c || !cl || cl->ctx != c || !prm) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_whole_cloud(c->comm->world(), "Gaussian-sphere segmentation");
    if (!cl->has_normals) throw DlgError(DLG_ERR_INVALID, "the cloud has no normals attached");
    if (cl->n_total > kMaxGridPoints) throw DlgError(DLG_ERR_INVALID, "too many points");
    check_params(prm, true);
    check_result(res);
    const int n = (int)cl->n_total;
    NormalsWork& w = c->nw;
    if (n > 0) {
      // the cloud's own device copy (upload order) and its attached normals
      w.x.ensure(n); w.y.ensure(n); w.z.ensure(n); w.nrm.ensure(n);
      const size_t nb = 4 * (size_t)n;
      HIPCHK(hipMemcpyAsync(w.x.p, cl->pristine.x.p, nb, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(w.y.p, cl->pristine.y.p, nb, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(w.z.p, cl->pristine.z.p, nb, hipMemcpyDeviceToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(w.nrm.p, cl->raw_nrm.p, 4 * nb, hipMemcpyDeviceToDevice, c->stream));
    }
    gs_core(c, n, prm, res, stats);
  });
}

}  // extern "C"
