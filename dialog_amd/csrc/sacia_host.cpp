// sacia_host.cpp -- host driver of the SAC-IA initial alignment: dlg_sac_ia_align, dlg_sac_ia_score
// and dlg_fpfh_knn (include/dialog_ransac.h; pcl::SampleConsensusInitialAlignment as
// Dialog/PCLViewer.cpp:546-558 calls it).
//
// The draws of every iteration depend on the source coordinates alone, so the host replays them all
// first (sacia_model.hpp).  Then: the valid target points' hierarchy (ICP's builder), the sampled
// source rows -- deduplicated, gathered on the host, the only source descriptors uploaded --
// searched against the target table in one batched launch, ONE read-back of the matches, the ranks
// picked and the transformations solved on the host, the hypotheses scored in batches that are all
// queued behind each other, ONE read-back of their sums, and the winner picked from the records.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "cloud_call.hpp"
#include "grid_host.hpp"
#include "normals.hpp"
#include "sacia.hpp"
#include "segment.hpp"  // event_ms

namespace dlg {
namespace {

static_assert(sizeof(IcpXf) == 64, "transformations are uploaded as packed 16-float records");
static_assert(sizeof(SaciaAcc) == 24, "the sums are read back as three words a hypothesis");

constexpr int64_t kQueueCap = 1 << 24;  // deferred pairs a queue holds: bounds the batch
constexpr int kMaxBatch = 256;
constexpr int64_t kPartCap = 1 << 26;   // entries of the search's per-slab lists (query chunks)
constexpr int64_t kFeatBytes = 4 * kSaciaDim;

void check_feat_stride(int64_t stride) {
  if (stride < kFeatBytes || stride % 4)
    throw DlgError(DLG_ERR_INVALID, "a descriptor stride must be >= 132 and a multiple of 4");
}

float checked_threshold(double mcd) {
  if (std::isnan(mcd) || !(mcd > 0.0))
    throw DlgError(DLG_ERR_INVALID, "max_correspondence_distance must be > 0");
  return sacia_threshold(mcd);
}

bool point_finite(const float* p) {
  return sacia_finite(p[0]) && sacia_finite(p[1]) && sacia_finite(p[2]);
}

// The k nearest flagged rows of nq packed queries; every pointer is device memory, so a caller
// whose descriptors already live on the device can use it as it is.
void knn_device(dlg_ctx* c, const float* queries, int nq, const float* rows, int64_t row_stride_f,
                int n_rows, const uint8_t* flags, int k, float* d_out, int32_t* i_out) {
  if (nq <= 0) return;
  SaciaWork& a = c->aw;
  const int64_t per_q = (int64_t)sacia_slabs(n_rows) * k;
  const int chunk = (int)std::min<int64_t>(nq, std::max<int64_t>(64, kPartCap / per_q / 64 * 64));
  a.part_d.ensure((size_t)(chunk * per_q));
  a.part_i.ensure((size_t)(chunk * per_q));
  for (int q0 = 0; q0 < nq; q0 += chunk)
    launch_sacia_knn(queries + (int64_t)q0 * kSaciaDim, std::min(chunk, nq - q0), rows, row_stride_f,
                     n_rows, flags, k, a.part_d.p, a.part_i.p, d_out + (int64_t)q0 * k,
                     i_out + (int64_t)q0 * k, c->stream);
  HIPCHK(hipGetLastError());
}

// host records (33 floats first, stride bytes apart) -> the packed device table
void upload_rows(dlg_ctx* c, const float* rows, int64_t stride, int n, DevBuf<float>& dst) {
  dst.ensure((size_t)std::max(n, 1) * kSaciaDim);
  if (n > 0)
    HIPCHK(hipMemcpy2DAsync(dst.p, (size_t)kFeatBytes, rows, (size_t)stride, (size_t)kFeatBytes,
                            (size_t)n, hipMemcpyHostToDevice, c->stream));
}

// The target (build_target, cloud_call.hpp): its packed descriptor table in aw.rows (feats null:
// none), nw.flags = the valid rows, and the hierarchy of the valid points (nw.x/y/z, nw.lv[]).
Target sacia_target(dlg_ctx* c, const dlg_points* tgt, const float* feats, int64_t feat_stride,
                    int k) {
  SaciaWork& a = c->aw;
  return build_target(c, tgt,
                      [&](const float* X, const float* Y, const float* Z, int rows, uint8_t* flags) {
                        if (feats) upload_rows(c, feats, feat_stride, rows, a.rows);
                        launch_sacia_row_flags(feats ? a.rows.p : nullptr, kSaciaDim, X, Y, Z, rows,
                                               flags, nullptr, c->stream);
                      },
                      k, "the target has fewer valid rows than k");
}

// computeErrorMetric of H transformations over the source in aw.sx/sy/sz: every batch is queued
// behind the last, the sums are read back once.
struct Scorer {
  dlg_ctx* c;
  const Target& T;
  int n_src = 0;
  int batches = 0, levels = 0;

  Scorer(dlg_ctx* ctx, const Target& t) : c(ctx), T(t) {}

  void upload_source(const dlg_points* src) {
    SaciaWork& a = c->aw;
    n_src = (int)src->n;
    const size_t mm = (size_t)std::max(n_src, 1);
    a.sx.ensure(mm); a.sy.ensure(mm); a.sz.ensure(mm);
    if (n_src == 0) return;
    launch_deinterleave(upload_raw(c, src), n_src, src->stride_bytes / 4, a.sx.p, a.sy.p, a.sz.p,
                        c->stream);
  }

  // queues the batches; sums[h] is valid after the caller's next synchronisation
  void run(const float* xfs, int H, float thr, int batch, int max_blocks,
           std::vector<SaciaAcc>& sums, SaciaState* state_out) {
    SaciaWork& a = c->aw;
    sums.assign((size_t)std::max(H, 1), SaciaAcc{0, 0, 0});
    std::memset(state_out, 0, sizeof(*state_out));
    if (H == 0) return;
    const float cell0 = T.L.G[0].cell;
    const bool never_defers = T.L.levels == 1 || (thr < INFINITY && cell0 * cell0 > thr);
    const int64_t fit = std::max<int64_t>(1, kQueueCap / std::max(n_src, 1));
    int b = batch > 0 ? batch : kMaxBatch;
    b = (int)std::min<int64_t>(std::min(b, kMaxBatch), never_defers ? kMaxBatch : fit);
    b = std::min(b, H);
    const size_t cap = never_defers ? 16 : (size_t)b * (size_t)std::max(n_src, 1);
    a.qa.ensure(cap); a.qb.ensure(cap);
    a.xfs.ensure((size_t)H * 16);
    a.acc.ensure((size_t)H * 3);
    a.state.ensure(sizeof(SaciaState));
    SaciaState* st = reinterpret_cast<SaciaState*>(a.state.p);
    const IcpXf* dx = reinterpret_cast<const IcpXf*>(a.xfs.p);
    SaciaAcc* dacc = reinterpret_cast<SaciaAcc*>(a.acc.p);
    HIPCHK(hipMemcpyAsync(a.xfs.p, xfs, 64 * (size_t)H, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemsetAsync(a.acc.p, 0, sizeof(SaciaAcc) * (size_t)H, c->stream));
    HIPCHK(hipMemsetAsync(st, 0, sizeof(SaciaState), c->stream));
    for (int h0 = 0; h0 < H; h0 += b) {
      const int nb = std::min(b, H - h0);
      HIPCHK(hipMemsetAsync(st->qn, 0, sizeof(st->qn), c->stream));
      launch_sacia_score0(T.L, a.sx.p, a.sy.p, a.sz.p, n_src, dx + h0, nb, thr, T.tmax, a.qa.p, st,
                          dacc + h0, c->num_cus, max_blocks, c->stream);
      if (!never_defers)
        for (int l = 1; l < T.L.levels; ++l)
          launch_sacia_score_level(T.L, l, a.sx.p, a.sy.p, a.sz.p, dx + h0, thr,
                                   (l & 1) ? a.qa.p : a.qb.p, (l & 1) ? a.qb.p : a.qa.p,
                                   (uint32_t)std::min<size_t>(cap, UINT32_MAX), st, dacc + h0,
                                   c->num_cus, max_blocks, c->stream);
      ++batches;
    }
    HIPCHK(hipGetLastError());
    HIPCHK(hipMemcpyAsync(sums.data(), a.acc.p, sizeof(SaciaAcc) * (size_t)H, hipMemcpyDeviceToHost,
                          c->stream));
    HIPCHK(hipMemcpyAsync(state_out, st, sizeof(SaciaState), hipMemcpyDeviceToHost, c->stream));
  }
};

void fill_scores(dlg_sac_ia_hypothesis& r, const SaciaAcc& s) {
  uint64_t hi, lo;
  sacia_error_words(s.lo, s.hi, &hi, &lo);
  r.err_hi = hi;
  r.err_lo = lo;
  r.n_far = (int64_t)(s.cnt & 0xFFFFFFFFull);
  r.n_used = (int64_t)(s.cnt >> 32);
}

void blank_record(dlg_sac_ia_hypothesis& r) {
  std::memset(&r, 0, sizeof(r));
  for (int j = 0; j < kSaciaMaxSamples; ++j) r.sample[j] = r.match[j] = r.rank[j] = -1;
}

}  // namespace
}  // namespace dlg

extern "C" {

void dlg_sac_ia_params_default(dlg_sac_ia_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->max_iterations = 1000;
  p->nr_samples = 3;
  p->k_correspondences = 10;
  p->rng = kSaciaRngGlibc;
  p->seed = 1;
  p->min_sample_distance = 0.0f;
  p->max_correspondence_distance = std::sqrt(DBL_MAX);
  p->fitness_max_range = DBL_MAX;
}

dlg_status dlg_fpfh_knn(dlg_ctx* c, const float* queries, int64_t q_stride_bytes, int64_t n_queries,
                        const float* rows, int64_t row_stride_bytes, int64_t n_rows, int32_t k,
                        int32_t* idx_out, float* d_out) {
  if (!c) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    if (n_queries < 0 || n_rows < 0 || n_queries > INT32_MAX || n_rows > INT32_MAX)
      throw DlgError(DLG_ERR_INVALID, "a count is negative or above 2^31-1");
    if ((n_queries > 0 && !queries) || (n_rows > 0 && !rows))
      throw DlgError(DLG_ERR_INVALID, "null descriptors");
    check_feat_stride(q_stride_bytes);
    check_feat_stride(row_stride_bytes);
    if (k < 1 || k > kSaciaMaxK) throw DlgError(DLG_ERR_INVALID, "k must be in 1..32");
    if (n_queries > 0 && (!idx_out || !d_out)) throw DlgError(DLG_ERR_INVALID, "null output");
    if (n_rows < k) throw DlgError(DLG_ERR_INVALID, "fewer valid rows than k");
    NormalsWork& w = c->nw;
    SaciaWork& a = c->aw;
    const int nq = (int)n_queries, nr = (int)n_rows;
    upload_rows(c, rows, row_stride_bytes, nr, a.rows);
    upload_rows(c, queries, q_stride_bytes, nq, a.queries);
    w.flags.ensure(nr);
    w.counters.ensure(8);
    w.h_cnt.ensure(8);
    HIPCHK(hipMemsetAsync(w.counters.p, 0, 4, c->stream));
    launch_sacia_row_flags(a.rows.p, kSaciaDim, nullptr, nullptr, nullptr, nr, w.flags.p,
                           w.counters.p, c->stream);
    HIPCHK(hipMemcpyAsync(w.h_cnt.p, w.counters.p, 4, hipMemcpyDeviceToHost, c->stream));
    const size_t no = (size_t)std::max(nq, 1) * (size_t)k;
    a.knn_d.ensure(no);
    a.knn_i.ensure(no);
    knn_device(c, a.queries.p, nq, a.rows.p, kSaciaDim, nr, w.flags.p, k, a.knn_d.p, a.knn_i.p);
    if (nq > 0) {
      HIPCHK(hipMemcpyAsync(idx_out, a.knn_i.p, 4 * (size_t)nq * k, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipMemcpyAsync(d_out, a.knn_d.p, 4 * (size_t)nq * k, hipMemcpyDeviceToHost, c->stream));
    }
    sync(c);
    if ((int64_t)w.h_cnt.p[0] < k) throw DlgError(DLG_ERR_INVALID, "fewer valid rows than k");
  });
}

dlg_status dlg_sac_ia_score(dlg_ctx* c, const dlg_points* src, const dlg_points* tgt,
                            const float* transforms, int64_t n_transforms,
                            double max_correspondence_distance, int32_t batch, int32_t max_blocks,
                            dlg_sac_ia_hypothesis* hyp_out) {
  if (!c) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    check_whole_cloud(c->comm->world(), "SAC-IA");
    check_points(src, "source");
    check_points(tgt, "target");
    if (n_transforms < 0 || n_transforms > INT32_MAX || (n_transforms > 0 && (!transforms || !hyp_out)))
      throw DlgError(DLG_ERR_INVALID, "transforms: null, negative or above 2^31-1");
    if (batch < 0 || max_blocks < 0) throw DlgError(DLG_ERR_INVALID, "negative batch or max_blocks");
    const float thr = checked_threshold(max_correspondence_distance);
    const int H = (int)n_transforms;
    for (int64_t k = 0; k < 16 * (int64_t)H; ++k)
      if (!std::isfinite(transforms[k])) throw DlgError(DLG_ERR_INVALID, "a transform is not finite");
    const Target T = sacia_target(c, tgt, nullptr, 0, 1);
    Scorer sc(c, T);
    sc.upload_source(src);
    std::vector<SaciaAcc> sums;
    SaciaState st;
    sc.run(transforms, H, thr, batch, max_blocks, sums, &st);
    sync(c);
    for (int h = 0; h < H; ++h) {
      blank_record(hyp_out[h]);
      hyp_out[h].valid = 1;
      std::memcpy(hyp_out[h].T, transforms + 16 * (size_t)h, 64);
      fill_scores(hyp_out[h], sums[h]);
    }
  });
}

dlg_status dlg_sac_ia_align(dlg_ctx* c, const dlg_points* src, const float* src_features,
                            int64_t src_feat_stride, const dlg_points* tgt,
                            const float* tgt_features, int64_t tgt_feat_stride,
                            const dlg_sac_ia_params* prm, const float* guess, float* final_out,
                            float* aligned_out, int64_t out_stride_bytes,
                            dlg_sac_ia_hypothesis* hyp_out, int64_t hyp_cap,
                            dlg_sac_ia_stats* stats) {
  if (!c || !prm || !final_out) return DLG_ERR_INVALID;
  if (stats) std::memset(stats, 0, sizeof(*stats));
  return guarded(c, [&] {
    check_whole_cloud(c->comm->world(), "SAC-IA");
    check_points(src, "source");
    check_points(tgt, "target");
    if (!src_features || !tgt_features) throw DlgError(DLG_ERR_INVALID, "null features");
    check_feat_stride(src_feat_stride);
    check_feat_stride(tgt_feat_stride);
    const int nr = prm->nr_samples, k = prm->k_correspondences;
    if (prm->max_iterations < 0) throw DlgError(DLG_ERR_INVALID, "max_iterations must be >= 0");
    if (nr < 3 || nr > kSaciaMaxSamples) throw DlgError(DLG_ERR_INVALID, "nr_samples must be in 3..8");
    if (k < 1 || k > kSaciaMaxK) throw DlgError(DLG_ERR_INVALID, "k_correspondences must be in 1..32");
    if (prm->rng != kSaciaRngGlibc && prm->rng != kSaciaRngMsvc)
      throw DlgError(DLG_ERR_INVALID, "rng must be 0 (glibc) or 1 (MSVC)");
    if (prm->batch < 0 || prm->max_blocks < 0)
      throw DlgError(DLG_ERR_INVALID, "negative batch or max_blocks");
    if (std::isnan(prm->min_sample_distance))
      throw DlgError(DLG_ERR_INVALID, "min_sample_distance is NaN");
    if ((int64_t)nr > src->n) throw DlgError(DLG_ERR_INVALID, "nr_samples exceeds the source's size");
    const float thr = checked_threshold(prm->max_correspondence_distance);
    if (aligned_out) check_out_stride(out_stride_bytes);
    if (hyp_out && hyp_cap < 0) throw DlgError(DLG_ERR_INVALID, "negative hyp_cap");
    float fin[16];
    check_guess(guess, fin);
    const bool score_guess = !sacia_guess_is_identity(fin);
    const int n_src = (int)src->n;
    const int64_t sf = src->stride_bytes / 4, ff = src_feat_stride / 4;
    const int n_rec = score_guess ? std::max(prm->max_iterations, 1) : prm->max_iterations;

    // 1. every iteration's draws
    std::vector<dlg_sac_ia_hypothesis> rec((size_t)n_rec);
    SaciaRng rng;
    rng.seed(prm->rng, prm->seed);
    std::vector<int32_t> uniq;
    int64_t draws = 0, relaxations = 0;
    int n_valid = 0, n_invalid = 0;
    for (int it = 0; it < n_rec; ++it) {
      dlg_sac_ia_hypothesis& r = rec[(size_t)it];
      blank_record(r);
      if (it == 0 && score_guess) {
        r.valid = 1;
        std::memcpy(r.T, fin, 64);
        continue;
      }
      sacia_select(rng, src->xyz, sf, n_src, nr, prm->min_sample_distance, r.sample, &r.draws,
                   &r.relaxations);
      bool ok = true;
      for (int j = 0; j < nr; ++j) {
        r.rank[j] = rng.index(k);
        ++r.draws;
        ok = ok && point_finite(src->xyz + (int64_t)r.sample[j] * sf) &&
             sacia_row_finite(src_features + (int64_t)r.sample[j] * ff);
      }
      r.valid = ok ? 1 : 0;
      draws += r.draws;
      relaxations += r.relaxations;
      if (ok) {
        ++n_valid;
        for (int j = 0; j < nr; ++j) uniq.push_back(r.sample[j]);
      } else {
        ++n_invalid;
      }
    }
    std::sort(uniq.begin(), uniq.end());
    uniq.erase(std::unique(uniq.begin(), uniq.end()), uniq.end());
    const int nq = (int)uniq.size();

    // 2. the target's valid rows, their hierarchy; the sampled source rows searched
    const Target T = sacia_target(c, tgt, tgt_features, tgt_feat_stride, k);
    SaciaWork& a = c->aw;
    int64_t syncs = 0;
    std::vector<int32_t> knn((size_t)nq * (size_t)k);
    mark(c, 0);
    if (nq > 0) {
      std::vector<float> q((size_t)nq * kSaciaDim);
      for (int u = 0; u < nq; ++u)
        std::memcpy(&q[(size_t)u * kSaciaDim], src_features + (int64_t)uniq[(size_t)u] * ff, kFeatBytes);
      a.queries.ensure(q.size());
      HIPCHK(hipMemcpyAsync(a.queries.p, q.data(), 4 * q.size(), hipMemcpyHostToDevice, c->stream));
      a.knn_d.ensure(knn.size());
      a.knn_i.ensure(knn.size());
      knn_device(c, a.queries.p, nq, a.rows.p, kSaciaDim, T.nt, c->nw.flags.p, k, a.knn_d.p,
                 a.knn_i.p);
      mark(c, 1);
      HIPCHK(hipMemcpyAsync(knn.data(), a.knn_i.p, 4 * knn.size(), hipMemcpyDeviceToHost, c->stream));
      sync(c);
      ++syncs;
    } else {
      mark(c, 1);
    }

    // 3. the ranks picked, the transformations solved
    std::vector<float> xfs;
    std::vector<int> slot((size_t)n_rec, -1);
    for (int it = 0; it < n_rec; ++it) {
      dlg_sac_ia_hypothesis& r = rec[(size_t)it];
      if (!r.valid) continue;
      if (r.draws != 0) {
        float w3[kSaciaMaxSamples][3], t3[kSaciaMaxSamples][3];
        for (int j = 0; j < nr; ++j) {
          const int u = (int)(std::lower_bound(uniq.begin(), uniq.end(), r.sample[j]) - uniq.begin());
          const int32_t mrow = knn[(size_t)u * (size_t)k + (size_t)r.rank[j]];
          if (mrow < 0 || mrow >= T.nt) throw DlgError(DLG_ERR_INTERNAL, "SAC-IA: a match is missing");
          r.match[j] = mrow;
          std::memcpy(w3[j], src->xyz + (int64_t)r.sample[j] * sf, 12);
          std::memcpy(t3[j], tgt->xyz + (int64_t)mrow * (tgt->stride_bytes / 4), 12);
        }
        sacia_estimate(w3, t3, nr, r.T);
      }
      slot[(size_t)it] = (int)(xfs.size() / 16);
      xfs.insert(xfs.end(), r.T, r.T + 16);
    }

    // 4. the scores, 5. the winner
    const int H = (int)(xfs.size() / 16);
    Scorer sc(c, T);
    sc.upload_source(src);
    std::vector<SaciaAcc> sums;
    SaciaState st;
    mark(c, 2);
    sc.run(xfs.data(), H, thr, prm->batch, prm->max_blocks, sums, &st);
    mark(c, 3);
    sync(c);
    ++syncs;
    SaciaBest best;
    for (int it = 0; it < n_rec; ++it) {
      dlg_sac_ia_hypothesis& r = rec[(size_t)it];
      if (slot[(size_t)it] < 0) continue;
      fill_scores(r, sums[(size_t)slot[(size_t)it]]);
      if (best.offer(it, r.err_hi, r.err_lo, r.draws != 0)) std::memcpy(fin, r.T, 64);
    }
    std::memcpy(final_out, fin, 64);
    if (aligned_out) {
      const int64_t of = out_stride_bytes / 4;
      for (int i = 0; i < n_src; ++i) {
        const float* p = src->xyz + (int64_t)i * sf;
        float* o = aligned_out + (int64_t)i * of;
        icp_xf(fin, p[0], p[1], p[2], o[0], o[1], o[2]);
        if (of > 3) o[3] = 1.0f;
      }
    }
    double knn_ms = 0.0, score_ms = 0.0;
    if (c->profiling) {
      knn_ms = event_ms(c, 0, 1);
      score_ms = event_ms(c, 2, 3);
    }
    // (icp_fitness builds its own target over the shared staging: the de-interleaved target, nw.flags
    // and nw.fin_pos of this call are overwritten.  Their last readers, the descriptor search and the
    // scoring batches, were synchronised above, and nothing below reads them.)
    double fitness = 0.0;
    if (prm->compute_fitness) fitness = icp_fitness(c, src, tgt, fin, prm->fitness_max_range);
    if (hyp_out)
      for (int64_t it = 0; it < std::min<int64_t>(n_rec, hyp_cap); ++it) hyp_out[it] = rec[(size_t)it];
    if (stats) {
      stats->iterations = n_rec;
      stats->converged = best.best_iteration >= 0;
      stats->best_iteration = best.best_iteration;
      stats->n_valid = n_valid;
      stats->n_invalid = n_invalid;
      stats->batches = sc.batches;
      stats->levels = std::max(1, (int)st.levels);
      stats->draws = draws;
      stats->relaxations = relaxations;
      stats->n_queries = nq;
      stats->host_syncs = syncs;
      stats->error = best.scored ? sacia_error_double(best.hi, best.lo) : 0.0;
      stats->fitness = fitness;
      stats->build_ms = T.build_ms;
      stats->knn_ms = knn_ms;
      stats->score_ms = score_ms;
      stats->device_ms = knn_ms + score_ms;
    }
  });
}

}  // extern "C"
