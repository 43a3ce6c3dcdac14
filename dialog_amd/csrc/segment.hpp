// segment.hpp -- what driver.cpp calls of segment.cpp (each function is described where it is
// defined).  The round's interface is the first group; the second is exported only because the
// two benchmark entry points and the cloud upload stayed with the C ABI in driver.cpp.
#pragma once

#include "driver.hpp"
#include "spatial.hpp"

namespace dlg {

struct SegOut {
  bool has_model = false;
  float coeff[4] = {0, 0, 0, 0};
  int64_t n_in_local = 0;   // refined inliers on this rank (ids in ctx->inl_gid)
  int64_t n_out_local = 0;  // survivors on this rank (compacted into the spare buffer if remove)
  int64_t n_in_global = 0;
  bool sp_compacted = false;  // the spatial copy's survivors are in its spare buffer
  int64_t sp_n_out = 0;
  bool lean = false;  // lean-list round: the spare list buffer holds pristine indices only
  // every rank's refined inliers / survivors (device allgather folded into the round's sync)
  std::vector<int64_t> in_ranks, out_ranks;
};

// ---- the round
SegOut segment_round(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params& prm, bool compact,
                     dlg_sac_stats* st, dlg_extract_stats* xs,
                     const std::vector<int64_t>* active_ranks = nullptr);
void score_samples(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params& prm, const int32_t* positions,
                   int D, int32_t* counts_out, int32_t* good_out, int32_t* valid_out,
                   float* coeffs_out);
void commit_round(dlg_cloud* cl, const SegOut& so);
void check_in_step(dlg_ctx* c, int round, const SegOut& so);
int64_t emit_inliers(dlg_ctx* c, const SegOut& so, bool gather, int32_t* dst, int64_t cap,
                     int64_t* global_count, bool deferred = false, bool counts_known = false);
void flush_emit(dlg_ctx* c);
void drain_pending(dlg_ctx* c);
void settle_round(dlg_ctx* c);
int64_t allgather_i64(dlg_ctx* c, int64_t v, std::vector<int64_t>* all);
bool trace_on();  // DLG_TRACE=1: per-round host timing breakdown on stderr (diagnostics only)
double now_ms();

// ---- shared with dlg_cloud_upload, dlg_cloud_build_spatial and dlg_score_benchmark
// pruned scoring (spatial.hpp): by default clouds of >= kPruneMinPoints points get a Morton copy
constexpr int64_t kPruneMinPoints = 131072;
void build_spatial(dlg_ctx* c, dlg_cloud* cl);
SpatialView spatial_view(const dlg_cloud* cl);
void ensure_sphere_bounds(dlg_ctx* c, dlg_cloud* cl);
void ensure_list_xyz(dlg_ctx* c, dlg_cloud* cl);
void ensure_prune_work(dlg_ctx* c, int64_t ns);
unsigned long long* prune_stats_ptr(dlg_ctx* c);
// the culled scoring's device scratch (allocated and zeroed on first use)
CullBufs ensure_cull(dlg_ctx* c);
float event_ms(dlg_ctx* c, int a, int b);

}  // namespace dlg
