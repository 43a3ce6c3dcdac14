// segment.cpp -- one RANSAC round of the MI355X plane path: the host side of segment().
//
// One RANSAC segment() (PCL 1.8 SACSegmentation<PointXYZ>::segment, SACMODEL_PLANE, SAC_RANSAC;
// reference call pattern Dialog/SimplifyVerticesSize.cpp:62-67) runs as:
//
//   host   : replay SampleConsensusModel::drawIndexSample over list *positions* for a batch of D
//            draws (mt19937(seed) >> 1, swaps kept in a sparse overlay of the shuffled list; the
//            positions do not depend on the data, only on N_active)
//   device : k_gather_samples (positions -> points, per shard) [+ allreduce over ranks]
//            k_build_hyps     (isSampleGood + computeModelCoefficients, PCL op order)
//            k_score          (countWithinDistance for all D draws)    [+ allreduce of counts]
//   host   : replay RandomSampleConsensus::computeModel over the D counts in draw order
//            (strict '>' keeps the first best, k = log(1-p)/log(1-w^3), iteration cap, 1000-bad-
//            draw getSamples limit); next batch only if the loop has not terminated
//   device : refit (PCL float parity mode on the host from the gathered inlier xyz, or fast
//            double moments on the device) and the final selectWithinDistance, which in
//            extract-and-remove mode also compacts the survivors into the ping-pong buffers.
//
// The data-independent part of getSamples (which list positions are swapped) is what lets the
// whole hypothesis batch be scored in one launch while still reproducing PCL's sequential RNG
// use bit-for-bit.
//
// SegmentRound below is that round: RoundPlan holds every path decision (made once, up front),
// the member functions are its phases in stream order (DESIGN.md §3 lists their collectives).
#include "segment.hpp"

#include <algorithm>
#include <cfloat>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "fsum.hpp"
#include "host_math.hpp"
#include "np_limit_host.hpp"
#include "sac_control.hpp"

namespace dlg {

static_assert(DLG_SACMODEL_PERPENDICULAR_PLANE == kModelPerpendicularPlane &&
                  DLG_SACMODEL_PARALLEL_PLANE == kModelParallelPlane,
              "axis_model.hpp's model values");

bool trace_on() {
  static const bool on = [] {
    const char* e = std::getenv("DLG_TRACE");
    return e && e[0] == '1';
  }();
  return on;
}
double now_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

namespace {

// part of the staged ids to the caller, once the copy has landed (called while the host spins
// on a round's results, so the copy costs the rounds nothing)
void pump_pending(dlg_ctx* c, int64_t ids) {
  if (!c->pending_dst) return;
  if (!c->stage_ready) {
    const hipError_t e = hipEventQuery(c->ev_stage);
    if (e == hipErrorNotReady) return;
    HIPCHK(e);
    c->stage_ready = true;
  }
  const int64_t n = std::min<int64_t>(ids, c->pending_n - c->pending_off);
  std::memcpy(c->pending_dst + c->pending_off, c->h_stage.p + c->pending_off, (size_t)n * 4);
  c->pending_off += n;
  if (c->pending_off == c->pending_n) {
    c->pending_dst = nullptr;
    c->pending_n = c->pending_off = 0;
  }
}

// spin until k_publish has released `seq` into c->pub.p[0] (the round's results are then in
// c->pub).  A stream query backs it up (no event marker on the stream: each one costs the GPU
// a few microseconds between kernels): once the stream has drained the word must be visible; an
// error of the stream surfaces through the query.
void wait_published(dlg_ctx* c, int32_t seq) {
  Comm* g = c->group();
  const bool poll = g->world() > 1;
  const auto t0 = std::chrono::steady_clock::now();
  for (uint32_t k = 1;; ++k) {
    if (__atomic_load_n(c->pub.p, __ATOMIC_ACQUIRE) == seq) return;
    // (several ranks: a failed peer's poison, or no progress within the group's timeout, ends
    // the wait -- the round's collectives may be waiting for that peer on the device)
    if (poll && (k & 255u) == 0) {
      g->check();
      if (g->timeout_ms > 0 && (k & 65535u) == 0) {
        const auto ms = std::chrono::duration_cast<std::chrono::milliseconds>(
                            std::chrono::steady_clock::now() - t0).count();
        if (ms > g->timeout_ms) {
          g->abort("rank " + std::to_string(g->rank()) + ": round not published after " +
                   std::to_string(ms) + " ms (DLG_OPT_COMM_TIMEOUT_MS)");
          g->check();
        }
      }
    }
    // the staged ids go to the caller while we wait; until their copy has landed, its event is
    // queried only every 16th spin (a HIP API call takes the runtime lock)
    if (c->stage_ready || (k & 15u) == 0) pump_pending(c, 16384);
    if ((k & 1023u) == 0) {
      const hipError_t e = hipStreamQuery(c->stream);
      if (e == hipSuccess) {
        if (__atomic_load_n(c->pub.p, __ATOMIC_ACQUIRE) == seq) return;
        throw DlgError(DLG_ERR_INTERNAL, "round results not visible after the round completed");
      }
      if (e != hipErrorNotReady) HIPCHK(e);
    }
#if defined(__x86_64__)
    __builtin_ia32_pause();
#endif
  }
}

// a single-pass select's look-back failed (sticky word set): clear it and fail the call
[[noreturn]] void sel1_failed(dlg_ctx* c) {
  (void)hipMemsetAsync(c->sel1_err.p, 0, sizeof(int32_t), c->stream);
  if (c->sel1_tk.p) {  // (a failed launch may have left tickets untaken)
    (void)hipMemsetAsync(c->sel1_tk.p, 0, sizeof(uint64_t), c->stream);
    c->sel1.issued = 0;
  }
  (void)hipStreamSynchronize(c->stream);
  throw DlgError(DLG_ERR_INTERNAL, "single-pass select did not complete (look-back gave up)");
}

// the previous compaction's Morton-copy totals (in, out) against what the list copy predicted
void check_sp_totals(dlg_ctx* c, const int32_t* sp_tot) {
  if (!c->sp_check) return;
  c->sp_check = false;
  if (c->sp_expect_in != 0 || c->sp_expect_out != 0) {
    if (sp_tot[0] != c->sp_expect_in || sp_tot[1] != c->sp_expect_out)
      throw DlgError(DLG_ERR_INTERNAL, "spatial copy out of step with the active list");
  }
}

// the PCL refit walk's share of a round's select phase (its events ride k_fs_walk's dispatch)
void add_walk_ms(dlg_ctx* c, int k) {
  if (!c->walk_rec[k]) return;
  float ms = 0.f;
  if (c->mid_rec[k]) {
    // several ranks, rank > 0: the two walks apart from the exchange and rebase between them
    float a = 0.f, b = 0.f;
    HIPCHK(hipEventElapsedTime(&a, c->ev_walk[k][0], c->ev_walk[k][4]));
    HIPCHK(hipEventElapsedTime(&b, c->ev_walk[k][5], c->ev_walk[k][1]));
    HIPCHK(hipEventElapsedTime(&ms, c->ev_walk[k][4], c->ev_walk[k][5]));
    c->sel_pending->refit_rebase_ms += ms;
    ms = a + b;
    c->mid_rec[k] = false;
  } else {
    HIPCHK(hipEventElapsedTime(&ms, c->ev_walk[k][0], c->ev_walk[k][1]));
  }
  c->sel_pending->refit_walk_ms += ms;
  c->walk_rec[k] = false;
  if (c->rep_rec[k]) {
    HIPCHK(hipEventElapsedTime(&ms, c->ev_walk[k][2], c->ev_walk[k][3]));
    c->sel_pending->refit_repair_ms += ms;
    c->rep_rec[k] = false;
  }
}

// the select timing of round pair k (the pair whose events have completed), into its stats
void add_select_ms(dlg_ctx* c, int k) {
  if (!c->sel_pending) return;
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev_sel[k][0], c->ev_sel[k][1]));
  c->sel_pending->select_ms += ms;
  add_walk_ms(c, k);
  c->sel_pending = nullptr;
}

}  // namespace

// after a stream synchronisation: the last compaction's Morton-copy totals and select timing
void settle_round(dlg_ctx* c) {
  if (c->sel1_err.p) {
    int32_t e = 0;
    HIPCHK(hipMemcpy(&e, c->sel1_err.p, 4, hipMemcpyDeviceToHost));
    if (e) sel1_failed(c);
  }
  if (c->sp_check) {
    int32_t t[2] = {0, 0};
    HIPCHK(hipMemcpy(t, c->totals.p + 2, 8, hipMemcpyDeviceToHost));
    check_sp_totals(c, t);
  }
  add_select_ms(c, c->sel_k ^ 1);  // the last round's pair
}

int64_t allgather_i64(dlg_ctx* c, int64_t v, std::vector<int64_t>* all) {
  const int W = c->comm->world();
  all->assign(W, 0);
  if (W == 1) {
    (*all)[0] = v;
    return v;
  }
  c->gath64.ensure(W + 1);
  c->h_g64.ensure(W + 1);
  c->h_g64.p[0] = v;
  HIPCHK(hipMemcpyAsync(c->gath64.p + W, c->h_g64.p, 8, hipMemcpyHostToDevice, c->stream));
  c->comm->allgather(c->gath64.p + W, c->gath64.p, 1, DType::I64, c->stream);
  HIPCHK(hipMemcpyAsync(c->h_g64.p, c->gath64.p, 8 * W, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  int64_t s = 0;
  for (int r = 0; r < W; ++r) {
    (*all)[r] = c->h_g64.p[r];
    s += c->h_g64.p[r];
  }
  return s;
}

namespace {
// gather every rank's device list (count_r items of `width` int32 each) into host `out`, rank order
void gather_lists(dlg_ctx* c, const int32_t* dev_local, int64_t n_local, int width,
                  std::vector<int32_t>* out) {
  const int W = c->comm->world();
  std::vector<int64_t> cnt;
  int64_t total = allgather_i64(c, n_local, &cnt);
  out->resize((size_t)(total * width));
  if (W == 1) {
    if (total)
      HIPCHK(hipMemcpyAsync(out->data(), dev_local, (size_t)total * width * 4, hipMemcpyDeviceToHost,
                            c->stream));
    sync(c);
    return;
  }
  int64_t mx = *std::max_element(cnt.begin(), cnt.end());
  if (mx == 0) return;
  const size_t per = (size_t)mx * width;
  c->gath32.ensure(per * (W + 1));
  int32_t* send = c->gath32.p + per * W;
  if (n_local)
    HIPCHK(hipMemcpyAsync(send, dev_local, (size_t)n_local * width * 4, hipMemcpyDeviceToDevice,
                          c->stream));
  c->comm->allgather(send, c->gath32.p, per, DType::I32, c->stream);
  std::vector<int32_t> tmp(per * W);
  HIPCHK(hipMemcpyAsync(tmp.data(), c->gath32.p, per * W * 4, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  size_t w = 0;
  for (int r = 0; r < W; ++r) {
    std::memcpy(out->data() + w, tmp.data() + per * r, (size_t)cnt[r] * width * 4);
    w += (size_t)cnt[r] * width;
  }
}
}  // namespace

float event_ms(dlg_ctx* c, int a, int b) {
  float ms = 0.f;
  HIPCHK(hipEventElapsedTime(&ms, c->ev[a], c->ev[b]));
  return ms;
}

void drain_pending(dlg_ctx* c) {
  if (!c->pending_dst) return;
  if (!c->stage_ready) HIPCHK(hipEventSynchronize(c->ev_stage));
  std::memcpy(c->pending_dst + c->pending_off, c->h_stage.p + c->pending_off,
              (size_t)(c->pending_n - c->pending_off) * 4);
  c->pending_dst = nullptr;
  c->pending_n = c->pending_off = 0;
}

// the requested inlier copy: device -> pinned stage on the copy stream, behind the select that
// wrote inl_gid (ev_inl); enqueued after the next round's launches, off the host's critical path
void flush_emit(dlg_ctx* c) {
  if (!c->emit_dst) return;
  drain_pending(c);  // (the stage is reused)
  c->h_stage.ensure((size_t)c->emit_n);
  if (!c->ev_stage) HIPCHK(hipEventCreateWithFlags(&c->ev_stage, hipEventDisableTiming));
  HIPCHK(hipStreamWaitEvent(c->cstream, c->ev_inl_cur, 0));
  HIPCHK(hipMemcpyAsync(c->h_stage.p, c->inl_gid.p, (size_t)c->emit_n * 4, hipMemcpyDeviceToHost,
                        c->cstream));
  HIPCHK(hipEventRecord(c->ev_stage, c->cstream));
  c->stage_inflight = true;  // inl_gid is read until ev_stage
  c->pending_dst = c->emit_dst;
  c->pending_n = c->emit_n;
  c->pending_off = 0;
  c->stage_ready = false;
  c->emit_dst = nullptr;
  c->emit_n = 0;
}

// the pruned kernel's work counters (DLG_OPT_PRUNE_STATS), accumulated over its launches
// the list lengths + the scorers' work area (spatial.hpp); a new allocation starts with zeroed
// counters (afterwards the scorer's last workgroup leaves them zero)
void ensure_prune_work(dlg_ctx* c, int64_t ns) {
  int32_t* old = c->lp_n.p;
  c->lp_n.ensure((size_t)prune_work_words(ns));
  if (c->lp_n.p != old) HIPCHK(hipMemsetAsync(c->lp_n.p, 0, sizeof(int32_t) * c->lp_n.cap, c->stream));
}

unsigned long long* prune_stats_ptr(dlg_ctx* c) {
  return c->opt.prune_stats ? c->pstats.p : nullptr;
}

CullBufs ensure_cull(dlg_ctx* c) {
  if (!c->cull_i.p) {
    c->cull_i.ensure(cull_int_words());
    c->cull_h.ensure(2 * (size_t)kMaxHypPerLaunch);
    HIPCHK(hipMemsetAsync(c->cull_i.p, 0, sizeof(int32_t) * c->cull_i.cap, c->stream));
  }
  return cull_bufs(c->cull_i.p, c->cull_h.p);
}

namespace {
// a count as a buffer size: never 0
size_t at_least_1(int64_t n) { return (size_t)std::max<int64_t>(n, 1); }

// the sphere-bound arrays of ping-pong buffer b, sized for the working copy's count
void ensure_bound_bufs(dlg_cloud* cl, int b) {
  cl->sp_tb[b].ensure(at_least_1(sp_tiles(cl->sp_n)));
  cl->sp_sb[b].ensure(at_least_1(sp_supers(cl->sp_n)));
}
}  // namespace

void build_spatial(dlg_ctx* c, dlg_cloud* cl) {
  const int64_t n = cl->n_total;
  auto &k0 = c->mk0, &k1 = c->mk1;
  auto &i0 = c->mi0, &i1 = c->mi1;
  auto& tmp = c->msort;
  k0.ensure(n); k1.ensure(n); i0.ensure(n); i1.ensure(n);
  const size_t tb = morton_sort_temp_bytes(n);
  tmp.ensure(std::max<size_t>(tb, 16));
  c->totals.ensure(8);
  HIPCHK(hipMemsetAsync(c->totals.p, 0, 4, c->stream));
  c->mxyz.ensure(at_least_1(n));
  launch_morton_keys(cl->pristine.view(n), cl->amax[0], cl->amax[1], cl->amax[2], k0.p, i0.p,
                     c->totals.p, c->mxyz.p, c->stream, c->opt.spatial_curve == 1);
  HIPCHK(morton_sort(tmp.p, tb, k0.p, k1.p, i0.p, i1.p, n, c->stream));
  int32_t nonfinite = 0;
  HIPCHK(hipMemcpyAsync(&nonfinite, c->totals.p, 4, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  const int64_t m = n - nonfinite;
  cl->sp_pristine.ensure(at_least_1(m));
  launch_gather_order(c->mxyz.p, i1.p, m, cl->sp_pristine.out(), c->stream);
  cl->sp_order.ensure(at_least_1(m));
  if (m > 0)
    HIPCHK(hipMemcpyAsync(cl->sp_order.p, i1.p, (size_t)m * 4, hipMemcpyDeviceToDevice, c->stream));
  if (cl->has_normals) {
    cl->sp_pristine.ensure_nrm(at_least_1(m));
    launch_gather_nrm(cl->pristine.nrm.p, cl->sp_order.p, m, cl->sp_pristine.nrm.p, c->stream);
  }
  cl->sp_tiles_pr.ensure(at_least_1(sp_tiles(m)));
  cl->sp_supers_pr.ensure(at_least_1(sp_supers(m)));
  launch_sphere_bounds(cl->sp_pristine.x.p, cl->sp_pristine.y.p, cl->sp_pristine.z.p, m, nullptr,
                       cl->sp_tiles_pr.p, cl->sp_supers_pr.p, c->stream);
  HIPCHK(hipGetLastError());
  // (no synchronisation: everything that reads the copy is queued behind it on the stream;
  // the scratch above is only rewritten by the next build, on the same stream)
  cl->sp_n_pristine = cl->sp_n = m;
  cl->sp_built = cl->sp_valid = true;
  cl->sp_cur = -1;
  cl->sp_dirty = false;
}

SpatialView spatial_view(const dlg_cloud* cl) {
  const SoA& s = cl->sp_soa();
  const bool pr = cl->sp_cur < 0;
  return SpatialView{s.x.p, s.y.p, s.z.p, cl->sp_n, pr ? cl->sp_tiles_pr.p : cl->sp_tb[cl->sp_cur].p,
                     pr ? cl->sp_supers_pr.p : cl->sp_sb[cl->sp_cur].p};
}

// (re)compute the sphere bounds of the working spatial copy when they are stale
void ensure_sphere_bounds(dlg_ctx* c, dlg_cloud* cl) {
  if (cl->sp_dirty && cl->sp_cur >= 0 && cl->sp_n > 0) {
    const int b = cl->sp_cur;
    ensure_bound_bufs(cl, b);
    const SoA& s = cl->sp_soa();
    launch_sphere_bounds(s.x.p, s.y.p, s.z.p, cl->sp_n, nullptr, cl->sp_tb[b].p, cl->sp_sb[b].p,
                         c->stream);
  }
  cl->sp_dirty = false;
}

// a lean list's coordinates (and ids, normals) from the pristine copy, before any path that
// reads them
void ensure_list_xyz(dlg_ctx* c, dlg_cloud* cl) {
  if (!cl->list_lean()) return;
  SoA& b = cl->buf[cl->cur];
  if (cl->pristine.with_nrm) b.ensure_nrm(at_least_1(cl->n_active));
  PointsOut io = b.out();
  if (!cl->pristine.with_nrm) io.nrm = nullptr;
  launch_list_materialize(cl->pristine.view(cl->n_total), cl->n_active, io, c->stream);
  HIPCHK(hipGetLastError());
  cl->buf_lean[cl->cur] = false;
}

namespace {

void ensure_sel1(dlg_ctx* c, int64_t n, int64_t min_tiles = 0) {
  const size_t nt = (size_t)std::max<int64_t>(sel1_tiles(n), min_tiles) + 1;
  if (nt > c->sel1_status.cap) {
    c->sel1_status.ensure(nt);
    HIPCHK(hipMemsetAsync(c->sel1_status.p, 0, sizeof(uint64_t) * c->sel1_status.cap, c->stream));
  }
  if (!c->sel1_err.p) {
    c->sel1_err.ensure(1);
    HIPCHK(hipMemsetAsync(c->sel1_err.p, 0, sizeof(int32_t), c->stream));
  }
  if (!c->sel1_tk.p) {
    c->sel1_tk.ensure(1);
    HIPCHK(hipMemsetAsync(c->sel1_tk.p, 0, sizeof(uint64_t), c->stream));
    c->sel1.issued = 0;
  }
  c->sel1.status = c->sel1_status.p;
  c->sel1.err = c->sel1_err.p;
  // (tickets whenever another context of this process may run its selects on the same device
  // at once: with the device to itself a launch's tiles complete in workgroup-index order)
  const bool tk = c->opt.sel1_ticket == 1 || (c->opt.sel1_ticket == -1 && ctx_shared(c->device));
  c->sel1.ticket = tk ? reinterpret_cast<unsigned long long*>(c->sel1_tk.p) : nullptr;
}

// a last-workgroup counter of one word: allocated once, zero between launches
void ensure_zeroed(dlg_ctx* c, DevBuf<unsigned>& w) {
  if (w.p) return;
  w.ensure(1);
  HIPCHK(hipMemsetAsync(w.p, 0, sizeof(unsigned), c->stream));
}

// every path decision of a round, made once from (context options, cloud state, parameters,
// compact) before anything is enqueued; the phases only read it
struct RoundPlan {
  bool np, pcl_refit, pcl_dev, pruned, pruned_np, pruned_any, lean, spec, sp_compact, fuse_pick,
      ext_ev, fused_pub, cull;
  int cap_h;  // draws per scoring launch
  float np_lim = INFINITY, pmargin, cthr;
  ModelTest mt;
};

RoundPlan make_plan(const dlg_ctx* c, const dlg_cloud* cl, const dlg_sac_params& prm, bool compact) {
  const PathOptions& o = c->opt;
  RoundPlan p{};
  const bool np = p.np = prm.model == DLG_SACMODEL_NORMAL_PLANE;
  p.cap_h = prm.hypotheses_per_launch > 0 ? std::min(prm.hypotheses_per_launch, kMaxHypPerLaunch)
                                          : kMaxHypPerLaunch;
  p.pcl_refit = prm.optimize && prm.refit_mode != DLG_REFIT_FAST;
  // PCL's float sums on the device (fsum.hip; several ranks: each walks its segment of the list
  // from the previous rank's end values); lean rounds take the unrefined inliers in list order
  // from a bitmap over pristine indices instead of list coordinates
  p.pcl_dev = p.pcl_refit && o.pcl_dev != 0;
  // NORMAL_PLANE over the Morton copy: the prefilter d_euclid < lim(w) holds for the cloud's
  // largest w = lambda (1 - min curvature) when every w lies in [0, 1) (then lim is finite and
  // monotone in w); NaN curvatures never pass PCL's test.  Otherwise the exhaustive kernel.
  if (np && cl->curv_known) {
    const double w_max = prm.normal_distance_weight * (1.0 - (double)cl->curv_min);
    const double w_min = prm.normal_distance_weight * (1.0 - (double)cl->curv_max);
    if (w_min >= 0.0 && w_max < 1.0) p.np_lim = np_lim_max(w_max, prm.threshold);
  }
  // pruned scoring over the spatial copy (plane model, default kernel, spatial copy in step)
  p.pruned = !np && cl->sp_valid && o.prune != 0;
  // (NORMAL_PLANE: only with the pruned NP scorer -- every w in [0, 1), the copy carrying normals)
  p.pruned_np = np && cl->sp_valid && cl->sp_soa().with_nrm && o.prune != 0 && o.prune_np &&
                p.np_lim < INFINITY;
  p.pruned_any = p.pruned || p.pruned_np;
  p.cthr = thr_ceil(prm.threshold);
  p.pmargin = p.pruned ? prune_margin(p.cthr, cl->amax)
                       : p.pruned_np ? prune_margin(p.np_lim, cl->amax) : 0.0f;
  // lean-list round: plane model over the Morton copy, device refit, a list that is pristine or
  // already lean (a list compacted with coordinates stays on the full path); any rank count
  // (any rank count: the fast refit's moments are exact integers, so summing them over the
  // Morton copies of the shards gives the list's bits.  Every rank decides alike: whether all
  // ranks hold a spatial copy is agreed once per extraction (c->sp_all), and the other inputs
  // -- the list lean, NORMAL_PLANE rounds dropping the copy -- evolve identically on every rank)
  p.lean = compact && (!np || p.pruned_np) && (!p.pcl_refit || p.pcl_dev) && o.lean &&
           cl->sp_valid && c->sp_all && cl->n_total < (int64_t(1) << 30) && o.prune != 0 &&
           (cl->cur < 0 || cl->buf_lean[cl->cur]);
  // Speculative pick (probability 1): the first batch holds all max_iterations + 1 draws, so
  // k_pick_p1 can take computeModel's decision on the device and the refit + select follow
  // without a host round trip (one sync per round in fast-refit mode, one less in PCL mode).
  // The counts still come back with the round's sync and the host replays them
  // (RansacControl::consume); on any disagreement, or when the loop needs more draws (bad
  // samples), the round continues on the exact host path and the refit + select are redone.
  p.spec = o.spec_pick && prm.probability == 1.0 && prm.max_iterations >= 0 &&
           (int64_t)prm.max_iterations + 1 <= p.cap_h;
  p.sp_compact = compact && cl->sp_valid && (!np || cl->sp_soa().with_nrm);
  const bool one = c->comm->world() == 1;
  // the speculative pick: fused into the pruned scoring's last workgroup on one rank (at N > 1
  // it needs the allreduced counts: its own launch after the collective)
  p.fuse_pick = p.spec && p.pruned_any && one && !c->hcomm;
  // culled scoring (DLG_OPT_CULL; spatial.hpp): the speculative batch of a plane-model round on
  // one rank, exact tile scorer; off for the rest of a call once a round scored most of its batch
  p.cull = p.fuse_pick && p.pruned && o.cull != 0 && o.tile_scorer == DLG_TILE_EXACT &&
           !c->cull_off && cl->sp_n > 0;
  // the pruned scorer records its timing events on its own dispatches (no marker packets)
  p.ext_ev = c->profiling && p.pruned_any;
  p.fused_pub = p.lean && one;  // (the Morton select's last tile publishes the round)
  p.mt.cthr = p.cthr;
  p.mt.normal_plane = np ? 1 : 0;
  p.mt.thr = prm.threshold;
  p.mt.lambda = prm.normal_distance_weight;
  // the axis-constrained plane models: SACMODEL_PLANE on every path, plus isModelValid as float
  // thresholds (axis_model.hpp) in the hypothesis build and in every kernel that selects with a
  // plane; kAxisNone for the other models and for eps <= 0
  p.mt.axis = make_axis_test(prm.model, c->axis, c->eps_angle);
  return p;
}

// computeModelCoefficients of three kept samples (k_build_hyps' arithmetic, on the host)
void sample_coefficients(const SampleRec* s, float c[4]) {
  const float p0[3] = {s[0].x, s[0].y, s[0].z}, p1[3] = {s[1].x, s[1].y, s[1].z},
              p2[3] = {s[2].x, s[2].y, s[2].z};
  sample_plane(p0, p1, p2, c);
}

bool model_known(int model) {
  return model == DLG_SACMODEL_PLANE || model == DLG_SACMODEL_NORMAL_PLANE ||
         model == DLG_SACMODEL_PERPENDICULAR_PLANE || model == DLG_SACMODEL_PARALLEL_PLANE;
}

// one batch of draws on its way through the scoring
struct Batch {
  int D = 0, Dp = 0;  // draws; D rounded up to the 64-hypothesis groups of k_score
  double t_draw0 = 0.0, t_draw1 = 0.0;
  PickArgs pk;
};

struct SegmentRound {
  SegmentRound(dlg_ctx* c_, dlg_cloud* cl_, const dlg_sac_params& prm_, bool compact_,
               const RoundPlan& plan, int64_t N_, std::vector<int64_t> per_rank_,
               dlg_sac_stats* st_, dlg_extract_stats* xs_)
      : c(c_), cl(cl_), prm(prm_), compact(compact_), P(plan), N(N_), per_rank(std::move(per_rank_)),
        st(st_), xs(xs_), W(c->comm->world()), src(cl->view()), n1(at_least_1(src.n)),
        lidx(P.lean && cl->cur >= 0 ? cl->buf[cl->cur].gid.p : nullptr),
        t_ctl0(trace_on() ? now_ms() : 0.0), ctl(prm, N, P.cap_h, &c->replay) {
    for (int r = 0; r < c->comm->rank(); ++r) offset += per_rank[r];
    if (trace_on()) std::fprintf(stderr, "[dlg] segment start %.3fms ctl %.3fms\n", t_ctl0 - c->t_tot, now_ms() - t_ctl0);
  }
  dlg_ctx* const c;
  dlg_cloud* const cl;
  const dlg_sac_params& prm;
  const bool compact;
  const RoundPlan P;
  const int64_t N;                      // active points over all ranks
  const std::vector<int64_t> per_rank;  // ... and of each rank
  dlg_sac_stats* const st;
  dlg_extract_stats* const xs;
  const int W;  // ranks of c->comm (1 under hypothesis sharding)
  const PointsView src;
  const size_t n1;  // src.n as a buffer size (never 0)
  // the lean list's pristine indices (null while the list is the pristine one)
  const int32_t* const lidx;
  const double t_ctl0;
  RansacControl ctl;
  int64_t offset = 0;  // this rank's first position in the global list
  // device slots: winning HypRec (its first float4 is the plane), its 3 samples, refined plane
  HypRec* best_dev = nullptr;
  SampleRec* best_smp_dev = nullptr;
  float4* rc_dev = nullptr;
  const float4* bc_dev = nullptr;
  PointsOut dst{};  // the spare list buffer (compact)
  int launches = 0;
  int spec_D = 0, spec_Dp = 0;  // the speculative batch, its counts not yet replayed
  bool spec_pending = false;
  bool spec_culled = false;  // ... scored culled: res[Dp + D] = the hypotheses scored exactly
  double t_ref0 = 0.0;
  SegOut out;

  // everything a round needs before its first batch: stale sphere bounds, the scratch of the
  // refit + final select (+ compaction of both copies, sphere bounds of the survivors), the
  // cloud's fast-refit quantum
  void prepare() {
    if (P.pruned_any) ensure_sphere_bounds(c, cl);
    c->small.ensure(16);
    c->h_small.ensure(16);
    best_dev = reinterpret_cast<HypRec*>(c->small.p);
    best_smp_dev = reinterpret_cast<SampleRec*>(c->small.p + 2);
    rc_dev = c->small.p + 5;
    bc_dev = c->small.p;
    c->pick.ensure(4);
    c->h_pick.ensure(4);
    t_ref0 = trace_on() ? now_ms() : 0.0;
    const int nt = select_tiles(src.n);
    c->tile_in.ensure(nt + 1);
    c->tile_off_in.ensure(nt + 1);
    c->tile_off_out.ensure(nt + 1);
    c->totals.ensure(8);
    c->h_tot.ensure(4);
    c->h_small.ensure(8);
    c->inl_gid.ensure(n1);
    c->moments.ensure(kMomDigits);
    if (!cl->qexp_known && prm.optimize && !P.pcl_refit) {
      // the fast refit's quantum comes from the largest finite |coordinate| of the whole cloud
      // (all ranks: one max-allreduce per cloud)
      double f = (double)cl->fmax;
      if (W > 1) {
        c->scratch_f64.ensure(1);
        HIPCHK(hipMemcpyAsync(c->scratch_f64.p, &f, 8, hipMemcpyHostToDevice, c->stream));
        c->comm->allreduce_max_f64(c->scratch_f64.p, 1, c->stream);
        HIPCHK(hipMemcpyAsync(&f, c->scratch_f64.p, 8, hipMemcpyDeviceToHost, c->stream));
        sync(c);
      }
      cl->qexp = fast_qexp((float)f);
      cl->qexp_known = true;
    }
    if (compact) {
      SoA& sp = cl->buf[cl->spare()];
      sp.ensure(n1);
      if (src.nrm) sp.ensure_nrm(n1);
      dst = sp.out();
    }
    if (P.lean && cl->tag.cap < (size_t)cl->n_total) {
      cl->tag.ensure(at_least_1(cl->n_total));
      HIPCHK(hipMemsetAsync(cl->tag.p, 0, cl->tag.cap, c->stream));
      cl->tagv = 0;
    }
  }

  // one batch of draws: replay, gather, build, score; then either the host replay (sync) or,
  // for the first batch of a speculative round, the device pick
  void batch(bool speculate) {
    Batch b = draw_and_build();
    score(b, speculate);
    if (speculate) enqueue_pick(b);
    else replay_batch(b);
  }

  Batch draw_and_build() {
    const int D = ctl.next_size();
    // ---- host: drawIndexSample over positions
    const double t_draw0 = trace_on() ? now_ms() : 0.0;
    c->h_pos.ensure(3 * (size_t)D);
    ctl.next_batch(c->h_pos.p);
    Batch b = build(D);
    b.t_draw0 = t_draw0;
    return b;
  }

  // the D draws whose list positions are in c->h_pos: samples, hypotheses, good flags
  Batch build(int D) {
    Batch b;
    b.D = D;
    int32_t* hp = c->h_pos.p;
    b.t_draw0 = b.t_draw1 = trace_on() ? now_ms() : 0.0;
    // ---- device: gather, build, score
    c->pos.ensure(3 * (size_t)D);
    c->samples.ensure(3 * (size_t)D);
    c->hyps.ensure(kHypScratchBytes / sizeof(HypRec) + 1);
    c->res.ensure(2 * (size_t)kMaxHypPerLaunch + 64);
    // res = counts[Dp] | good[D]  (Dp = D rounded up to the 64-hypothesis groups of k_score)
    const int Dp = b.Dp = (D + 63) / 64 * 64;
    const float* am = cl->amax;
    // (a lean list holds indices into the pristine copy; a list with coordinates is read
    // directly, lidx null, and the list length the launches take is its own n either way)
    const PointsView pts = P.lean ? cl->pristine.view(cl->n_total) : src;
    if (W == 1) {
      // one launch: positions read from the pinned host buffer (the next round's draw rewrites
      // it only after this round's results were published, i.e. after this kernel ran)
      launch_gather_build(hp, D, pts, c->samples.p, P.cthr, am[0], am[1], am[2], c->hyps.p,
                          c->res.p, c->stream, lidx, src.n, &P.mt.axis);
    } else {
      HIPCHK(hipMemcpyAsync(c->pos.p, hp, 12 * (size_t)D, hipMemcpyHostToDevice, c->stream));
      launch_gather_samples(c->pos.p, 3 * D, offset, pts, c->samples.p, c->stream, lidx, src.n);
      c->comm->allreduce_sum(c->samples.p, 12 * (size_t)D, DType::I32, c->stream);
      launch_build_hyps(c->samples.p, D, P.cthr, am[0], am[1], am[2], c->hyps.p, c->res.p + Dp,
                        c->stream, &P.mt.axis);
      HIPCHK(hipMemsetAsync(c->res.p, 0, 4 * (size_t)Dp, c->stream));
    }
    return b;
  }

  void score(Batch& b, bool speculate) {
    const int D = b.D, Dp = b.Dp;
    // hypothesis sharding: this rank scores hypotheses [h_lo, h_hi) only (slices in whole
    // 64-hypothesis groups, so an exhaustive kernel's padded group never reaches into another
    // rank's slice), the other counts stay zero until the allreduce below
    int h_lo = 0, h_hi = D;
    if (c->hcomm) {
      const int64_t U = Dp / 64, R = c->hcomm->world(), r = c->hcomm->rank();
      h_lo = (int)std::min<int64_t>(D, 64 * (U * r / R));
      h_hi = (int)std::min<int64_t>(D, 64 * (U * (r + 1) / R));
    }
    const int Ds = h_hi - h_lo;
    const HypRec* hyps_s = c->hyps.p + h_lo;
    int32_t* counts_s = c->res.p + h_lo;
    if (c->profiling && !P.ext_ev) HIPCHK(hipEventRecord(c->ev[0], c->stream));
    PickArgs& pk = b.pk;
    if (speculate) {
      pk.res = c->res.p;
      pk.Dp = Dp;
      pk.D = D;
      pk.need_good = prm.max_iterations + 1;
      pk.hyps = c->hyps.p;
      pk.samples = c->samples.p;
      pk.best = best_dev;
      pk.best_smp = best_smp_dev;
      pk.out = c->pick.p;
    }
    const bool fuse_pick = speculate && P.fuse_pick;
    if (fuse_pick) {
      ensure_zeroed(c, c->pick_done);
      pk.done = c->pick_done.p;
    }
    if (P.pruned_any) {
      c->lp.ensure((size_t)sp_supers(cl->sp_n) * prune_list_stride(D) + 1);
      ensure_prune_work(c, sp_supers(cl->sp_n));
      if (P.pruned_np) c->np_cn.ensure(kMaxHypPerLaunch);
      const PrunedNp npp{cl->sp_soa().nrm.p, prm.normal_distance_weight, prm.threshold, c->np_cn.p};
      // (the speculative batch of one rank: Ds == D, the whole of res)
      spec_culled = fuse_pick && P.cull && Ds > 0;
      if (spec_culled) {
        const int K = cull_k(c->opt.cull);
        launch_score_culled(spatial_view(cl), hyps_s, Ds, Dp, K, P.cthr, P.pmargin, counts_s, c->lp.p,
                            c->lp_n.p + kPwHeader, c->num_cus, c->stream, prune_stats_ptr(c),
                            ensure_cull(c), &pk, P.ext_ev ? c->ev[0] : nullptr,
                            P.ext_ev ? c->ev[1] : nullptr, kCullRound, c->opt.cull_fuse != 0);
      } else {
        launch_score_pruned(spatial_view(cl), hyps_s, Ds, P.cthr, P.pmargin, cl->amax, counts_s,
                            c->lp.p, c->lp_n.p + kPwHeader, c->num_cus, c->stream, prune_stats_ptr(c),
                            P.pruned_np ? &npp : nullptr, fuse_pick ? &pk : nullptr,
                            P.ext_ev ? c->ev[0] : nullptr, P.ext_ev ? c->ev[1] : nullptr,
                            c->opt.tile_scorer);
      }
    } else if (P.np) {
      if (Ds > 0) launch_score_np(src, hyps_s, Ds, P.mt, counts_s, c->num_cus, c->stream);
    } else if (Ds > 0) {
      launch_score(src, hyps_s, Ds, P.cthr, counts_s, c->opt.score_kernel, c->num_cus, c->stream);
    }
    HIPCHK(hipGetLastError());
    if (c->profiling && !P.ext_ev) HIPCHK(hipEventRecord(c->ev[1], c->stream));
    if (W > 1) c->comm->allreduce_sum(c->res.p, D, DType::I32, c->stream);
    if (c->hcomm) c->hcomm->allreduce_sum(c->res.p, D, DType::I32, c->stream);
    c->h_res.ensure((size_t)Dp + D + 1);
    ++launches;
    st->tests_scored += (int64_t)D * N;
  }

  void enqueue_pick(const Batch& b) {
    // (the counts and the pick come back with the round's totals: a copy here would sit
    // between the scoring and the pick on the stream)
    if (!P.fuse_pick) launch_pick_p1(b.pk, c->stream);
    HIPCHK(hipGetLastError());
    spec_pending = true;
    spec_D = b.D;
    spec_Dp = b.Dp;
    flush_emit(c);  // the previous round's inlier copy, behind this round's launches
    if (trace_on())
      std::fprintf(stderr, "[dlg] N=%lld D=%d totals->draw=%.3fms draw=%.3fms enqueue=%.3fms (speculative pick)\n",
                   (long long)N, b.D, c->t_tot > 0 ? b.t_draw0 - c->t_tot : 0.0, b.t_draw1 - b.t_draw0,
                   now_ms() - b.t_draw1);
  }

  void replay_batch(const Batch& b) {
    const int D = b.D, Dp = b.Dp;
    HIPCHK(hipMemcpyAsync(c->h_res.p, c->res.p, 4 * ((size_t)Dp + D), hipMemcpyDeviceToHost, c->stream));
    const double t_launch = trace_on() ? now_ms() : 0.0;
    flush_emit(c);  // the previous round's inlier copy, behind this round's launches
    sync(c);
    if (trace_on())
      std::fprintf(stderr, "[dlg] N=%lld D=%d totals->draw=%.3fms draw=%.3fms launch=%.3fms score+wait=%.3fms\n",
                   (long long)N, D, c->t_tot > 0 ? b.t_draw0 - c->t_tot : 0.0, b.t_draw1 - b.t_draw0,
                   t_launch - b.t_draw1, now_ms() - t_launch);
    if (c->profiling) st->score_ms += event_ms(c, 0, 1);
    // ---- host: computeModel replay over the batch
    keep_winner(ctl.consume(c->h_res.p, c->h_res.p + Dp, D));
  }

  // keep the winner on the device (the next batch overwrites hyps)
  void keep_winner(int best_d) {
    if (best_d < 0) return;
    HIPCHK(hipMemcpyAsync(best_dev, c->hyps.p + best_d, sizeof(HypRec), hipMemcpyDeviceToDevice,
                          c->stream));
    HIPCHK(hipMemcpyAsync(best_smp_dev, c->samples.p + 3 * best_d, 3 * sizeof(SampleRec),
                          hipMemcpyDeviceToDevice, c->stream));
  }

  // the exact host replay of the counts the device picked from; false: the pick is overturned
  bool replay_speculative() {
    if (c->profiling) {
      float ms = 0.f;
      HIPCHK(hipEventElapsedTime(&ms, c->ev[0], c->ev_score_end));
      st->score_ms += ms;
    }
    // a culled round that scored more than D / kCullFallbackDiv: the bound does not separate on this
    // cloud, the rest of the call scores unculled (the bound pass is then paid once)
    if (spec_culled && cull_falls_back(c->h_res.p[spec_Dp + spec_D], spec_D)) c->cull_off = true;
    const int best_d = ctl.consume(c->h_res.p, c->h_res.p + spec_Dp, spec_D);
    if (ctl.done() && best_d == c->h_pick.p[0] && c->h_pick.p[1] == 1) return true;
    ++c->spec_misses;
    if (xs) xs->spec_misses++;
    if (trace_on())
      std::fprintf(stderr, "[dlg] speculative pick overturned: host %d done %d, device %d complete %d\n",
                   best_d, ctl.done() ? 1 : 0, c->h_pick.p[0], c->h_pick.p[1]);
    keep_winner(best_d);
    return false;
  }

  // before the first launch of a round that writes inl_gid: the previous round's inlier copy
  // (copy stream) may still read it.  A stream wait only when the copy is still running (it
  // has almost always landed by then); placed at the writer, not at the round's start, so a
  // wait never sits between the scoring and the refit on the critical path.
  void stage_wait() {
    if (!c->stage_inflight) return;
    const hipError_t q = hipEventQuery(c->ev_stage);
    if (q == hipErrorNotReady) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_stage, 0));
    else HIPCHK(q);
    c->stage_inflight = false;
  }

  PointsView sp_cur_view() const {
    const SoA& ss = cl->sp_soa();
    return PointsView{ss.x.p, ss.y.p, ss.z.p, ss.gid.p, cl->sp_n,
                      P.np && ss.with_nrm ? ss.nrm.p : nullptr};
  }

  // refit + final select (+ compaction of both copies, sphere bounds of the survivors); ends
  // with the round's sync
  void refit_select() {
    // Fast mode (and no optimisation) never leave the device: moments of the unrefined plane's
    // inliers (k_moments, centred on the winning sample), the double eigen33 refit in a
    // one-thread kernel, then the select with the refined plane read from device memory.  PCL
    // mode needs the host's sequential float sums in between.
    // (tests: DLG_OPT_FAULT_INJECT -- this rank fails here, after the round's scoring
    // collectives, while its peers go on into the refit's and the select's)
    if (xs && c->opt.fault_round > 0 && xs->rounds == c->opt.fault_round - 1)
      throw DlgError(DLG_ERR_INTERNAL, "injected fault (DLG_OPT_FAULT_INJECT) in extract round " +
                                           std::to_string(xs->rounds));
    const int sk = c->sel_k;  // this round's pair of select timing events
    begin_select_phase(sk);
    if (!P.pcl_refit) refit_fast();
    else if (P.pcl_dev) refit_pcl_device();
    else refit_pcl_host();
    select_round(sk, c->profiling);
    if (P.pcl_dev) recheck_pcl_tail();
  }

  void begin_select_phase(int sk) {
    c->walk_rec[sk] = false;
    // the PCL refit walk's timing events (profiling only)
    // (e = 2, 3: k_fs_repair's, which runs on ranks > 0 of a group only)
    c->rep_rec[sk] = false;
    c->mid_rec[sk] = false;
    if (!c->profiling) return;
    for (auto& ev : c->ev_sel[sk])
      if (!ev) HIPCHK(hipEventCreate(&ev));
    if (spec_pending) {
      // the scoring's end event (just recorded) opens the select phase: no second marker
      std::swap(c->ev[1], c->ev_sel[sk][0]);
      c->ev_score_end = c->ev_sel[sk][0];
    } else {
      HIPCHK(hipEventRecord(c->ev_sel[sk][0], c->stream));
    }
  }

  // timing event e of this round's PCL refit walk (null: not recorded)
  // (e = 4, 5: the first walk's end and the second's start, ranks > 0 under protocols 0, 2)
  hipEvent_t walk_ev(int e) {
    const int sk = c->sel_k;
    if (!c->profiling || !c->walk_events) return nullptr;
    if (e >= 2 && (W == 1 || c->comm->rank() == 0)) return nullptr;
    if (e >= 4 && c->opt.fs_protocol == 1) return nullptr;
    if (!c->ev_walk[sk][e]) HIPCHK(hipEventCreate(&c->ev_walk[sk][e]));
    (e >= 4 ? c->mid_rec : e >= 2 ? c->rep_rec : c->walk_rec)[sk] = true;
    return c->ev_walk[sk][e];
  }

  void refit_fast() {
    const bool one = W == 1;
    if (prm.optimize) {
      // (lean: the moments of the Morton copy -- the same finite inliers -- over the tiles
      // whose sphere may hold one; one rank: the refit in the same launch)
      const PointsView mv = P.lean ? sp_cur_view() : src;
      const int nb = P.lean ? moments_sp_blocks(mv.n) : moments_blocks(mv.n);
      c->partials.ensure((size_t)nb * kMomDigits);
      ensure_zeroed(c, c->mom_done);
      if (P.lean) {
        const SpatialView sv = spatial_view(cl);
        launch_moments_sp(mv, sv.tiles, sv.supers, P.pmargin, bc_dev, P.mt, cl->qexp, c->partials.p,
                          c->mom_done.p, nb, c->moments.p, one ? rc_dev : nullptr, c->stream);
      } else if (one) {
        launch_moments_refit(mv, bc_dev, P.mt, cl->qexp, c->partials.p, c->mom_done.p, nb,
                             c->moments.p, rc_dev, c->stream);
      } else {
        launch_moments(mv, bc_dev, P.mt, cl->qexp, c->partials.p, c->mom_done.p, nb,
                       c->moments.p, c->stream);
      }
    }
    if (!(prm.optimize && one)) {
      // exact integers: the rank sum is the one-rank result, whatever the sharding
      if (prm.optimize) c->comm->allreduce_sum(c->moments.p, kMomDigits, DType::I64, c->stream);
      launch_refit_moments(c->moments.p, cl->qexp, bc_dev, prm.optimize, rc_dev, c->stream);
    }
  }

  // PCL float refit on the device: the unrefined plane's inliers in list order, PCL's nine
  // sequential float sums evaluated exactly in parallel (fsum.hip), the float eigen33; the
  // refined plane stays on the device (no host round trip)
  void refit_pcl_device() {
    if (c->fs_cap < src.n) {
      const int64_t cap = (int64_t)n1;
      c->fs_scr.ensure(fs_scratch_bytes(cap, W));
      c->fs_b = fs_carve(c->fs_scr.p, cap, W);
      HIPCHK(fs_reset(c->fs_b, c->stream, c->opt.fs_poison));
      c->fs_cap = cap;
    }
    if (P.lean) {
      unrefined_inliers_lean();
      fs_refit(c->fs_x.p, c->fs_y.p, c->fs_z.p, 1, c->fs_n.p);
    } else {
      select_unrefined();
      fs_refit(c->inl_xyz.p, c->inl_xyz.p + 1, c->inl_xyz.p + 2, 3, c->totals.p);
    }
  }

  // the unrefined plane's inliers over the list with coordinates: xyz into inl_xyz, count in totals[0]
  void select_unrefined() {
    c->inl_xyz.ensure(3 * n1);
    stage_wait();
    launch_select(src, bc_dev, P.mt, c->tile_in.p, c->tile_off_in.p, c->tile_off_out.p,
                  c->totals.p, c->inl_gid.p, c->inl_xyz.p, nullptr, c->stream);
  }

  // the unrefined plane's inliers' x, y, z in list order (= ascending pristine order):
  // one pass over the active list (k_ulist), or (DLG_OPT_UNREFINED_LIST 0) stamped into a
  // bitmap over pristine indices from the Morton copy's near tiles and compacted from it
  void unrefined_inliers_lean() {
    const int64_t nw = (cl->n_total + 31) / 32;
    c->fs_x.ensure(n1);
    c->fs_y.ensure(n1);
    c->fs_z.ensure(n1);
    c->fs_n.ensure(1);
    if (c->opt.unrefined_list) {
      ensure_sel1(c, std::max<int64_t>(src.n, cl->sp_n));
      launch_ulist(lidx, src.n, cl->pristine.view(cl->n_total), bc_dev, P.mt, c->sel1,
                   c->fs_x.p, c->fs_y.p, c->fs_z.p, c->fs_n.p, c->stream);
      HIPCHK(hipGetLastError());
      return;
    }
    if (cl->ubits.cap < (size_t)nw + 16 || cl->ubits_dirty) {
      // (new, or left stamped by an extraction that failed between the stamp and the
      // compaction, which clears every word it reads)
      cl->ubits.ensure((size_t)nw + 16);
      HIPCHK(hipMemsetAsync(cl->ubits.p, 0, cl->ubits.cap * sizeof(uint32_t), c->stream));
      cl->ubits_dirty = false;
    }
    ensure_sel1(c, std::max<int64_t>(src.n, cl->sp_n), ucompact_tiles(nw));
    const SpatialView sv = spatial_view(cl);
    cl->ubits_dirty = true;
    launch_ustamp(sp_cur_view(), sv.tiles, sv.supers, P.pmargin, bc_dev, P.mt, cl->ubits.p,
                  c->stream);
    launch_ucompact(cl->ubits.p, nw, cl->pristine.view(cl->n_total), c->sel1, c->fs_x.p,
                    c->fs_y.p, c->fs_z.p, c->fs_n.p, c->stream);
    HIPCHK(hipGetLastError());
    cl->ubits_dirty = false;
  }

  // fsum.hip's refit over n_dev[0] inliers at px, py, pz (stride floats apart)
  void fs_refit(const float* px, const float* py, const float* pz, int stride, const int32_t* n_dev) {
    int32_t* fs_res = reinterpret_cast<int32_t*>(c->small.p + 8);
    int repairs = 0;
    launch_fs_refit(px, py, pz, stride, n_dev, src.n, c->fs_b, bc_dev, rc_dev, fs_res, c->num_cus,
                    c->stream, c->comm.get(), walk_ev(0), walk_ev(1), walk_ev(2), walk_ev(3),
                    c->opt.fs_protocol, &repairs, c->opt.fs_segments, walk_ev(4), walk_ev(5),
                    c->opt.fs_join);
    HIPCHK(hipGetLastError());
    if (xs) xs->refit_repairs += repairs;
  }

  // PCL float refit: inlier xyz in global list order -> sequential float sums on the host
  void refit_pcl_host() {
    select_unrefined();
    HIPCHK(hipMemcpyAsync(c->h_tot.p, c->totals.p, 8, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(hipMemcpyAsync(c->h_small.p, c->small.p, 5 * sizeof(float4), hipMemcpyDeviceToHost,
                          c->stream));
    sync(c);
    const HypRec* bh = reinterpret_cast<const HypRec*>(c->h_small.p);
    const float bc[4] = {bh->a, bh->b, bh->c, bh->d};
    std::vector<int32_t> xyz_bits;
    gather_lists(c, reinterpret_cast<const int32_t*>(c->inl_xyz.p), c->h_tot.p[0], 3, &xyz_bits);
    float rc[4];
    refit_pcl_float(reinterpret_cast<const float*>(xyz_bits.data()), (int64_t)xyz_bits.size() / 3,
                    bc, rc);
    c->h_small.p[5] = make_float4(rc[0], rc[1], rc[2], rc[3]);
    HIPCHK(hipMemcpyAsync(rc_dev, c->h_small.p + 5, sizeof(float4), hipMemcpyHostToDevice,
                          c->stream));
  }

  // an eigen33 transcendental the device could not round for certain (a double result within
  // 2^-46 of a float rounding boundary): the host's value from the published sums decides,
  // and the select is redone when it differs (DLG_OPT_PCL_REFIT_DEVICE 2 / 3: every round)
  void recheck_pcl_tail() {
    const int32_t* fr = reinterpret_cast<const int32_t*>(c->h_small.p + 8);
    if (fr[0] == 0 && c->opt.pcl_dev < 2) return;
    ++c->fs_checks;
    if (xs) xs->pcl_host_checks++;
    float a9[9], rh[4];
    std::memcpy(a9, fr + 2, sizeof(a9));
    const HypRec* bh = reinterpret_cast<const HypRec*>(c->h_small.p);
    const float cin[4] = {bh->a, bh->b, bh->c, bh->d};
    fs_refit_tail_plain(a9, fr[1], cin, rh);
    const float4 rd = c->h_small.p[5];
    if (std::memcmp(rh, &rd, sizeof(rh)) == 0 && c->opt.pcl_dev != 3) return;
    ++c->fs_fixes;
    c->h_small.p[15] = make_float4(rh[0], rh[1], rh[2], rh[3]);
    HIPCHK(hipMemcpyAsync(rc_dev, c->h_small.p + 15, sizeof(float4), hipMemcpyHostToDevice,
                          c->stream));
    // (the first select wrote only spare buffers and stamps under its own tag: redone
    // outright; its timing is not kept)
    select_round(c->sel_k, /*timed=*/false);
  }

  // timed: the round's end marker is its select timing pair's, read at the next publish
  void select_round(int sk, bool timed) {
    // final selectWithinDistance with the refined plane at rc_dev (+ compaction, publish, wait):
    // the head (counts + scan) makes the
    // round's totals final, they are published right away, and the scatters (inlier ids,
    // survivors of both copies) and the sphere bounds run while the host reads them and draws
    // the next round
    // (lean: the Morton copy's single-pass select makes the totals final and stamps the inliers;
    // on one rank its last tile publishes the round too)
    PubArgs pa = make_pub_args();
    if (P.lean) {
      select_lean(pa);
    } else {
      select_full(pa);
      if (P.sp_compact) compact_spatial_copy();
    }
    HIPCHK(hipGetLastError());
    // one marker at the end of the round's work: inl_gid is final there (flush_emit's copy waits
    // for it) and, when profiling, it closes the select phase.  (The GPU then waits for the
    // host's next draw anyway.)
    c->ev_inl_cur = timed ? c->ev_sel[sk][1] : c->ev_inl;
    HIPCHK(hipEventRecord(c->ev_inl_cur, c->stream));
    const double t_wait0 = trace_on() ? now_ms() : 0.0;
    wait_published(c, pa.seq);
    if (trace_on())
      std::fprintf(stderr, "[dlg] select enqueue=%.3fms wait=%.3fms\n", t_wait0 - t_ref0, now_ms() - t_wait0);
    read_published(pa, sk, timed);
  }

  // the round's results into the coherent pinned buffer + a sequence number the host spins on
  // (totals[2..3] still hold the previous compaction's Morton-copy totals: checked below)
  PubArgs make_pub_args() {
    const bool with_counts = spec_pending;
    const int nres = with_counts ? spec_Dp + spec_D + (spec_culled ? 1 : 0) : 0;
    const size_t need = (size_t)kPubRk + (W > 1 ? 2 * (size_t)W : 0) + (size_t)nres;
    if (need > c->pub.cap) {
      c->pub.ensure(std::max<size_t>(need, 16384));
      c->pub.p[0] = 0;
    }
    if (W > 1) {
      c->rk.ensure(2 * (size_t)W + 2);
      c->h_rk.ensure(2 * (size_t)W + 2);
    }
    PubArgs pa;
    pa.totals = c->totals.p;
    pa.ntot = 4;
    pa.small = c->small.p;
    pa.nsmall = P.pcl_dev ? 12 : 6;  // (+ the device PCL refit's flag, count and sums: small[8..11])
    pa.rk = W > 1 ? c->rk.p : nullptr;
    pa.nrk = W > 1 ? 2 * W : 0;
    pa.pick = with_counts ? c->pick.p : nullptr;
    pa.npick = with_counts ? 2 : 0;
    pa.res = with_counts ? c->res.p : nullptr;
    pa.nres = nres;
    pa.err = c->sel1_err.p;
    pa.pub = c->pub.p;
    pa.seq = ++c->pub_seq == 0 ? ++c->pub_seq : c->pub_seq;
    return pa;
  }

  void publish_totals(const PubArgs& pa) {
    HIPCHK(hipGetLastError());
    if (W > 1)  // every rank's (in, out): the extract loop needs no host-synced allgather
      c->comm->allgather(c->totals.p, c->rk.p, 2, DType::I32, c->stream);
    if (!P.fused_pub) launch_publish(pa, c->stream);
    HIPCHK(hipGetLastError());
    spec_pending = false;
  }

  // the Morton copy's spare buffer (sized for the current count, an upper bound) and the current
  // copy as a select's source
  PointsOut spare_spatial(PointsView* spv) {
    SoA& sd = cl->sp_buf[cl->sp_spare()];
    sd.ensure(at_least_1(cl->sp_n));
    const SoA& ss = cl->sp_soa();
    if (ss.with_nrm) sd.ensure_nrm(at_least_1(cl->sp_n));
    PointsOut spo = sd.out();
    *spv = sp_cur_view();
    if (ss.with_nrm) spv->nrm = ss.nrm.p;  // (a later NORMAL_PLANE round reads them)
    else spo.nrm = nullptr;                // (normals travel only when the source has them)
    return spo;
  }

  void select_lean(PubArgs& pa) {
    if (++cl->tagv > 255) {
      HIPCHK(hipMemsetAsync(cl->tag.p, 0, (size_t)cl->n_total, c->stream));
      cl->tagv = 1;
    }
    ensure_sel1(c, std::max<int64_t>(src.n, cl->sp_n));
    pa.err = c->sel1_err.p;
    PointsView spv;
    const PointsOut spo = spare_spatial(&spv);
    launch_sel1_morton(spv, rc_dev, P.mt, c->sel1, cl->tag.p, (uint8_t)cl->tagv, spo, src.n,
                       c->totals.p, c->stream, P.fused_pub ? &pa : nullptr, c->opt.sel1_tile);
    publish_totals(pa);
    // the list from the stamps (ids in list order; survivors' pristine indices), then the
    // sphere bounds of the Morton survivors (count in totals[4]).  DLG_OPT_BOUNDS_STREAM: the
    // bounds on a second stream beside the list pass (independent passes over different
    // buffers; forked after the Morton select, joined before anything later on the stream).
    // (Round 5 dropped it after an 8-context loopback run hung; the cause was the single-pass
    // selects' look-back, not the stream: DESIGN.md §6.)
    const int b = cl->sp_spare();
    SoA& sd = cl->sp_buf[b];
    ensure_bound_bufs(cl, b);
    const bool side = c->opt.bounds_stream;
    if (side) {
      if (!c->sstream) {
        HIPCHK(hipStreamCreateWithFlags(&c->sstream, hipStreamNonBlocking));
        HIPCHK(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming));
        HIPCHK(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming));
      }
      HIPCHK(hipEventRecord(c->ev_fork, c->stream));
      HIPCHK(hipStreamWaitEvent(c->sstream, c->ev_fork, 0));
      launch_sphere_bounds(sd.x.p, sd.y.p, sd.z.p, cl->sp_n, c->totals.p + 4, cl->sp_tb[b].p,
                           cl->sp_sb[b].p, c->sstream);
      HIPCHK(hipEventRecord(c->ev_join, c->sstream));
    }
    stage_wait();
    launch_sel1_list(lidx, src.n, cl->tag.p, (uint8_t)cl->tagv,
                     cl->gid_ident ? nullptr : cl->pristine.gid.p, cl->id_base, c->sel1,
                     c->inl_gid.p, dst.gid, c->totals.p + 2, c->stream, c->opt.sel1_tile);
    if (side) HIPCHK(hipStreamWaitEvent(c->stream, c->ev_join, 0));
    else
      launch_sphere_bounds(sd.x.p, sd.y.p, sd.z.p, cl->sp_n, c->totals.p + 4, cl->sp_tb[b].p,
                           cl->sp_sb[b].p, c->stream);
  }

  void select_full(const PubArgs& pa) {
    launch_select_head(src, rc_dev, P.mt, c->tile_in.p, c->tile_off_in.p, c->tile_off_out.p,
                       c->totals.p, c->stream);
    publish_totals(pa);
    stage_wait();
    launch_select_tail(src, rc_dev, P.mt, c->tile_off_in.p, c->tile_off_out.p, c->inl_gid.p,
                       nullptr, compact ? &dst : nullptr, c->stream);
  }

  // the Morton copy loses the same points (same predicate, same float inputs): its totals
  // land in totals[2..3], checked at the next publish / the end of the extraction
  void compact_spatial_copy() {
    PointsView spv;
    PointsOut spo = spare_spatial(&spv);
    launch_select(spv, rc_dev, P.mt, c->tile_in.p, c->tile_off_in.p, c->tile_off_out.p,
                  c->totals.p + 2, nullptr, nullptr, &spo, c->stream);
    // sphere bounds of the survivors, into the spare buffer's own bound arrays (sized for
    // the current count, an upper bound; the kernel reads the survivor count from
    // totals[3]), so a round whose plane is rejected leaves the current bounds intact
    const int b = cl->sp_spare();
    ensure_bound_bufs(cl, b);
    launch_sphere_bounds(spo.x, spo.y, spo.z, cl->sp_n, c->totals.p + 3, cl->sp_tb[b].p,
                         cl->sp_sb[b].p, c->stream);
  }

  void read_published(const PubArgs& pa, int sk, bool timed) {
    if (trace_on()) c->t_tot = now_ms();
    std::memcpy(c->h_tot.p, c->pub.p + kPubTot, 16);
    if (c->pub.p[kPubErr] != 0) sel1_failed(c);  // (this round's or the last list pass's look-back)
    std::memcpy(c->h_small.p, c->pub.p + kPubSmall, (size_t)pa.nsmall * sizeof(float4));
    if (W > 1) std::memcpy(c->h_rk.p, c->pub.p + kPubRk, 8 * (size_t)W);
    check_sp_totals(c, c->h_tot.p + 2);
    if (pa.pick) {  // (with the speculative batch's counts)
      std::memcpy(c->h_pick.p, c->pub.p + kPubPick, 8);
      std::memcpy(c->h_res.p, c->pub.p + kPubRk + (W > 1 ? 2 * W : 0), 4 * (size_t)pa.nres);
    }
    // the previous round's select events precede this publish on the stream: complete now
    add_select_ms(c, sk ^ 1);
    if (timed && xs) c->sel_pending = xs;  // this round's: read at the next publish / end
    c->sel_k = sk ^ 1;
  }

  SegOut run() {
    prepare();
    bool selected = false;
    if (P.spec && !ctl.done()) {
      batch(true);
      refit_select();  // on the device's pick
      selected = replay_speculative();
    }
    while (!ctl.done()) batch(false);
    st->draws = ctl.draws();
    st->tests = ctl.tests();
    st->iterations = ctl.iterations();
    st->launches = launches;
    if (xs) {
      xs->tests += st->tests;
      xs->tests_scored += st->tests_scored;
      xs->score_launches += launches;
      xs->score_ms += st->score_ms;
    }
    if (!ctl.have_model()) return out;
    st->has_model = 1;
    st->n_unrefined = ctl.best_count();
    if (!selected) refit_select();
    finish();
    return out;
  }

  // the round's results (published by the last select) into the caller's stats and SegOut
  void finish() {
    const HypRec* bh = reinterpret_cast<const HypRec*>(c->h_small.p);
    const SampleRec* bs = reinterpret_cast<const SampleRec*>(c->h_small.p + 2);
    const float4 rc = c->h_small.p[5];
    st->coeff_unrefined[0] = bh->a; st->coeff_unrefined[1] = bh->b;
    st->coeff_unrefined[2] = bh->c; st->coeff_unrefined[3] = bh->d;
    for (int i = 0; i < 3; ++i) st->best_sample[i] = bs[i].gid;
    out.coeff[0] = rc.x; out.coeff[1] = rc.y; out.coeff[2] = rc.z; out.coeff[3] = rc.w;
    if (bh->good & kHypInvalid) {
      // an axis-constrained model whose every hypothesis was invalid: the first good draw won
      // with 0 inliers.  The device carried it as a NaN plane (no inliers, and the refit of
      // fewer than 4 inliers keeps its input), so its real coefficients -- PCL reports them --
      // are rebuilt from its samples with the arithmetic that built the hypothesis
      sample_coefficients(bs, st->coeff_unrefined);
      std::memcpy(out.coeff, st->coeff_unrefined, sizeof(out.coeff));
    }
    out.has_model = true;
    out.n_in_local = c->h_tot.p[0];
    out.n_out_local = src.n == 0 ? 0 : c->h_tot.p[1];
    out.in_ranks.assign(W, 0);
    out.out_ranks.assign(W, 0);
    for (int r = 0; r < W; ++r) {
      // (a rank with no active points skips its select kernels: its totals are zero)
      const bool empty = per_rank[r] == 0;
      out.in_ranks[r] = W == 1 ? out.n_in_local : (empty ? 0 : c->h_rk.p[2 * r]);
      out.out_ranks[r] = W == 1 ? out.n_out_local : (empty ? 0 : c->h_rk.p[2 * r + 1]);
    }
    out.n_in_global = 0;
    for (int64_t v : out.in_ranks) out.n_in_global += v;
    if (P.lean) {
      // the Morton copy decided the inliers; the list pass's own totals (totals[2..3]) must agree
      // with them (checked at the next publish, check_sp_totals)
      out.lean = true;
      out.sp_compacted = true;
      out.sp_n_out = cl->sp_n - out.n_in_local;
      c->sp_expect_in = out.n_in_local;
      c->sp_expect_out = out.n_out_local;
      c->sp_check = out.n_in_local != 0 || out.n_out_local != 0;
    } else if (P.sp_compact) {
      // non-finite points are never inliers: the Morton copy loses exactly the list's inliers
      // (its own totals are checked at the next publish, check_sp_totals)
      out.sp_compacted = true;
      out.sp_n_out = cl->sp_n - out.n_in_local;
      c->sp_expect_in = cl->sp_n == 0 ? 0 : out.n_in_local;
      c->sp_expect_out = out.sp_n_out;
      c->sp_check = true;
    }
    if (trace_on())
      std::fprintf(stderr, "[dlg] refit+select=%.3fms n_in=%lld\n", now_ms() - t_ref0,
                   (long long)out.n_in_local);
  }
};

}  // namespace

// one SACSegmentation::segment() over the cloud's active list (all ranks)
// active_ranks: every rank's active count when the caller already knows it (the extract loop
// carries it from the previous round's survivors), else allgathered here
SegOut segment_round(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params& prm, bool compact,
                     dlg_sac_stats* st, dlg_extract_stats* xs,
                     const std::vector<int64_t>* active_ranks) {
  std::memset(st, 0, sizeof(*st));
  if (!model_known(prm.model))
    throw DlgError(DLG_ERR_INVALID, "model must be SACMODEL_PLANE, SACMODEL_NORMAL_PLANE, "
                                    "SACMODEL_PERPENDICULAR_PLANE or SACMODEL_PARALLEL_PLANE");
  if (prm.model == DLG_SACMODEL_NORMAL_PLANE && !cl->has_normals)  // PCL: "No input dataset containing normals was given!"
    throw DlgError(DLG_ERR_INVALID, "SACMODEL_NORMAL_PLANE needs normals (dlg_cloud_set_normals)");
  if (!(prm.threshold == prm.threshold)) throw DlgError(DLG_ERR_INVALID, "threshold is NaN");
  std::vector<int64_t> per_rank;
  int64_t N = 0;
  if (active_ranks && (int)active_ranks->size() == c->comm->world() &&
      (*active_ranks)[c->comm->rank()] == cl->n_active) {
    per_rank = *active_ranks;
    for (int64_t v : per_rank) N += v;
  } else {
    N = allgather_i64(c, cl->n_active, &per_rank);
  }
  st->n_active = N;
  if (N > INT32_MAX) throw DlgError(DLG_ERR_INVALID, "more than 2^31-1 active points");
  if (prm.threshold == DBL_MAX) return SegOut{};  // PCL: "No threshold set!" -> computeModel false
  if (N < 3) return SegOut{};                      // getSamples: cannot select 3 unique points
  const RoundPlan plan = make_plan(c, cl, prm, compact);
  if (!plan.lean) ensure_list_xyz(c, cl);
  return SegmentRound(c, cl, prm, compact, plan, N, std::move(per_rank), st, xs).run();
}

// dlg_score_samples: the round's own draw_and_build and score phases over the caller's draws
// (3 list positions each), on the path make_plan chooses for this cloud -- every scorer, the
// gather and count collectives of several ranks, the hypothesis slices -- with every draw's
// verdicts and coefficients handed back instead of a decision.  The list is not changed.
void score_samples(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params& prm, const int32_t* positions,
                   int D, int32_t* counts_out, int32_t* good_out, int32_t* valid_out,
                   float* coeffs_out) {
  if (!model_known(prm.model)) throw DlgError(DLG_ERR_INVALID, "unknown model");
  if (prm.model == DLG_SACMODEL_NORMAL_PLANE && !cl->has_normals)
    throw DlgError(DLG_ERR_INVALID, "SACMODEL_NORMAL_PLANE needs normals (dlg_cloud_set_normals)");
  if (!(prm.threshold == prm.threshold)) throw DlgError(DLG_ERR_INVALID, "threshold is NaN");
  std::vector<int64_t> per_rank;
  const int64_t N = allgather_i64(c, cl->n_active, &per_rank);
  if (N > INT32_MAX) throw DlgError(DLG_ERR_INVALID, "more than 2^31-1 active points");
  if (N < 3) throw DlgError(DLG_ERR_INVALID, "need >= 3 active points");
  for (int i = 0; i < 3 * D; ++i)
    if (positions[i] < 0 || positions[i] >= N)
      throw DlgError(DLG_ERR_INVALID, "position outside the active list");
  const RoundPlan plan = make_plan(c, cl, prm, /*compact=*/false);
  ensure_list_xyz(c, cl);
  dlg_sac_stats st;
  std::memset(&st, 0, sizeof(st));
  SegmentRound r(c, cl, prm, false, plan, N, std::move(per_rank), &st, nullptr);
  if (plan.pruned_any) ensure_sphere_bounds(c, cl);
  c->h_pos.ensure(3 * (size_t)D);
  std::memcpy(c->h_pos.p, positions, 12 * (size_t)D);
  Batch b = r.build(D);
  r.score(b, /*speculate=*/false);
  std::vector<HypRec> hyps((size_t)D);
  std::vector<SampleRec> smp(3 * (size_t)D);
  HIPCHK(hipMemcpyAsync(c->h_res.p, c->res.p, 4 * ((size_t)b.Dp + D), hipMemcpyDeviceToHost, c->stream));
  HIPCHK(hipMemcpyAsync(hyps.data(), c->hyps.p, sizeof(HypRec) * (size_t)D, hipMemcpyDeviceToHost,
                        c->stream));
  HIPCHK(hipMemcpyAsync(smp.data(), c->samples.p, sizeof(SampleRec) * 3 * (size_t)D,
                        hipMemcpyDeviceToHost, c->stream));
  sync(c);
  for (int d = 0; d < D; ++d) {
    const int32_t g = c->h_res.p[b.Dp + d];
    const bool invalid = (g & kHypInvalid) != 0;
    counts_out[d] = c->h_res.p[d];
    good_out[d] = g != 0;
    if (valid_out) valid_out[d] = invalid ? 0 : 1;
    if (!coeffs_out) continue;
    float* co = coeffs_out + 4 * (size_t)d;
    co[0] = hyps[d].a; co[1] = hyps[d].b; co[2] = hyps[d].c; co[3] = hyps[d].d;
    if (invalid) sample_coefficients(&smp[3 * (size_t)d], co);  // (the device's plane is NaN)
  }
}

// an accepted extract round's removal: the spare buffers `so` was compacted into become current
void commit_round(dlg_cloud* cl, const SegOut& so) {
  cl->buf_lean[cl->spare()] = so.lean;
  cl->cur = cl->spare();  // commit the removal
  cl->n_active = so.n_out_local;
  if (so.sp_compacted) {
    cl->sp_cur = cl->sp_spare();
    cl->sp_n = so.sp_n_out;
    cl->sp_dirty = false;  // bounds queued by the round behind the compaction
  } else {
    cl->sp_valid = false;  // (SACMODEL_NORMAL_PLANE rounds do not carry the spatial copy)
  }
}

// DLG_OPT_SYNC_CHECK: every rank's view of the round just run -- (round, model, global inliers,
// coefficient bits, collectives issued so far, the axis and eps_angle of dlg_ctx_set_axis) --
// allgathered and compared; the first rank that differs from rank 0 fails the call on every rank
// (and, through guarded_group, nothing waits)
void check_in_step(dlg_ctx* c, int round, const SegOut& so) {
  Comm* g = c->group();
  const int W = g->world();
  if (W == 1) return;
  constexpr int K = 8;
  int64_t mine[K];
  uint32_t cb[4];
  std::memcpy(cb, so.coeff, sizeof(cb));
  mine[0] = round;
  mine[1] = so.has_model ? so.n_in_global : -1;
  mine[2] = (int64_t)(((uint64_t)cb[0] << 32) | cb[1]);
  mine[3] = (int64_t)(((uint64_t)cb[2] << 32) | cb[3]);
  mine[4] = (int64_t)g->ops();
  // (the axis-constrained models' context state: every rank must have set the same values)
  uint32_t ab[3];
  std::memcpy(ab, c->axis, sizeof(ab));
  mine[5] = (int64_t)(((uint64_t)ab[0] << 32) | ab[1]);
  mine[6] = (int64_t)ab[2];
  std::memcpy(&mine[7], &c->eps_angle, 8);
  c->gath64.ensure((size_t)K * (W + 1));
  c->h_g64.ensure((size_t)K * W);
  HIPCHK(hipMemcpyAsync(c->gath64.p + (size_t)K * W, mine, sizeof(mine), hipMemcpyHostToDevice,
                        c->stream));
  g->allgather(c->gath64.p + (size_t)K * W, c->gath64.p, K, DType::I64, c->stream);
  HIPCHK(hipMemcpyAsync(c->h_g64.p, c->gath64.p, sizeof(mine) * W, hipMemcpyDeviceToHost,
                        c->stream));
  sync(c);
  static const char* what[K] = {"round", "inliers", "coefficients", "coefficients", "collectives",
                                "axis", "axis", "eps_angle"};
  for (int r = 1; r < W; ++r)
    for (int k = 0; k < K; ++k)
      if (c->h_g64.p[(size_t)K * r + k] != c->h_g64.p[k])
        throw DlgError(DLG_ERR_INTERNAL,
                       "ranks diverged in extract round " + std::to_string(round) + ": rank " +
                           std::to_string(r) + "'s " + what[k] + " " +
                           std::to_string(c->h_g64.p[(size_t)K * r + k]) + " vs rank 0's " +
                           std::to_string(c->h_g64.p[k]));
}

// copy this rank's (or every rank's) refined inliers to the caller buffer
int64_t emit_inliers(dlg_ctx* c, const SegOut& so, bool gather, int32_t* dst, int64_t cap,
                     int64_t* global_count, bool deferred, bool counts_known) {
  if (gather && c->comm->world() > 1) {
    gather_lists(c, c->inl_gid.p, so.n_in_local, 1, &c->h_inl);
    int64_t n = (int64_t)c->h_inl.size();
    *global_count = n;
    if (n > cap) throw DlgError(DLG_ERR_CAPACITY, "inlier buffer too small: need " + std::to_string(n));
    if (n) std::memcpy(dst, c->h_inl.data(), (size_t)n * 4);
    return n;
  }
  if (counts_known) {
    *global_count = so.n_in_global;
  } else {
    std::vector<int64_t> all;
    *global_count = allgather_i64(c, so.n_in_local, &all);
  }
  if (so.n_in_local > cap)
    throw DlgError(DLG_ERR_CAPACITY, "inlier buffer too small: need " + std::to_string(so.n_in_local));
  if (so.n_in_local) {
    if (deferred) {
      // (copied by flush_emit after the next round's launches, or at the end of the loop)
      flush_emit(c);
      c->emit_dst = dst;
      c->emit_n = so.n_in_local;
    } else {
      HIPCHK(hipMemcpyAsync(dst, c->inl_gid.p, (size_t)so.n_in_local * 4, hipMemcpyDeviceToHost,
                            c->stream));
      sync(c);
    }
  }
  return so.n_in_local;
}

}  // namespace dlg
