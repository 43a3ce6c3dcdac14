// driver.hpp -- host-side state shared by every host driver (the RANSAC rounds in driver.cpp and
// segment.cpp, the normals path, postProcessPlanes and the six cloud filters / registration calls):
// the owning device and pinned buffers, each driver's scratch, the context and cloud objects.
// (The error type and the argument checks: call_args.hpp.)
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <atomic>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/dialog_ransac.h"
#include "call_args.hpp"
#include "comm.hpp"
#include "gsphere_model.hpp"
#include "kernels.hpp"
#include "sac_control.hpp"
#include "postprocess.hpp"

namespace dlg {

#define HIPCHK(expr)                                                                          \
  do {                                                                                        \
    hipError_t e_ = (expr);                                                                   \
    if (e_ != hipSuccess)                                                                     \
      throw DlgError(DLG_ERR_HIP, std::string(#expr) + " -> " + hipGetErrorString(e_));       \
  } while (0)

// bytes this process holds in DevBuf ([0]) and PinBuf ([1]) allocations (dlg_debug_live_bytes)
inline std::atomic<int64_t> g_live_bytes[2];

// Device memory of one owner: grown by ensure() (never shrunk, contents not kept), freed by
// release() or the destructor.  The device it was allocated on must be current when it dies
// (dlg_ctx_destroy, dlg_cloud_destroy and a failed cloud call see to that).
template <typename T>
struct DevBuf {
  T* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) HIPCHK(hipFree(p));
    forget();
    size_t want = std::max<size_t>(n, 16);
    HIPCHK(hipMalloc(reinterpret_cast<void**>(&p), want * sizeof(T)));
    cap = want;
    g_live_bytes[0] += (int64_t)(cap * sizeof(T));
  }
  void release() {
    if (p) (void)hipFree(p);
    forget();
  }

 private:
  void forget() {
    g_live_bytes[0] -= (int64_t)(cap * sizeof(T));
    p = nullptr;
    cap = 0;
  }
};

// pinned host memory, the same way (Flags: hipHostMallocCoherent for what a kernel publishes)
template <typename T, unsigned Flags = hipHostMallocDefault>
struct PinBuf {
  T* p = nullptr;
  size_t cap = 0;
  PinBuf() = default;
  PinBuf(const PinBuf&) = delete;
  PinBuf& operator=(const PinBuf&) = delete;
  ~PinBuf() { release(); }
  void ensure(size_t n) {
    if (n <= cap) return;
    if (p) HIPCHK(hipHostFree(p));
    forget();
    size_t want = std::max<size_t>(n, 16);
    HIPCHK(hipHostMalloc(reinterpret_cast<void**>(&p), want * sizeof(T), Flags));
    cap = want;
    g_live_bytes[1] += (int64_t)(cap * sizeof(T));
  }
  void release() {
    if (p) (void)hipHostFree(p);
    forget();
  }

 private:
  void forget() {
    g_live_bytes[1] -= (int64_t)(cap * sizeof(T));
    p = nullptr;
    cap = 0;
  }
};

// (an owner is never copied or moved: the aggregates below are built in place)
static_assert(!std::is_copy_constructible<DevBuf<float>>::value &&
                  !std::is_copy_assignable<DevBuf<float>>::value &&
                  !std::is_move_constructible<DevBuf<float>>::value,
              "DevBuf owns its allocation");
static_assert(!std::is_copy_constructible<PinBuf<float>>::value &&
                  !std::is_copy_assignable<PinBuf<float>>::value &&
                  !std::is_move_constructible<PinBuf<float>>::value,
              "PinBuf owns its allocation");

struct SoA {
  DevBuf<float> x, y, z;
  DevBuf<int32_t> gid;
  DevBuf<float4> nrm;  // SACMODEL_NORMAL_PLANE only (normalized normal, curvature)
  bool with_nrm = false;
  void ensure(size_t n) { x.ensure(n); y.ensure(n); z.ensure(n); gid.ensure(n); }
  void ensure_nrm(size_t n) { nrm.ensure(n); with_nrm = true; }
  PointsView view(int64_t n) const {
    return PointsView{x.p, y.p, z.p, gid.p, n, with_nrm ? nrm.p : nullptr};
  }
  PointsOut out() { return PointsOut{x.p, y.p, z.p, gid.p, with_nrm ? nrm.p : nullptr}; }
};

// one sorted grid of the normals path (normals.hip): points in cell order + occupied-cell table
struct GridLevelBufs {
  DevBuf<float> sx, sy, sz;
  DevBuf<int32_t> idx, pos;
  DevBuf<uint32_t> tkeys;
  DevBuf<int2> trange;
};

// scratch of the normals / RegulateNormal path (normals_host.cpp), and what the cloud calls share
// (cloud_call.cpp): the raw upload, the staged index list, the de-interleaved cloud with its flags
// and kept positions, the kept points and their grids
struct NormalsWork {
  static constexpr int kLevels = 12;
  GridLevelBufs lv[kLevels];
  DevBuf<uint8_t> raw, out, processed, processed_s, sort_tmp, dflags, fs_scr;
  DevBuf<float> x, y, z, qx, qy, qz, partial;
  DevBuf<uint32_t> keys_in, keys_out, counters;
  DevBuf<int32_t> idx_in, queue, cand, ids, ids_alt, pos_of, nn;
  DevBuf<float4> nrm, nrm_s;
  DevBuf<float4> rec;  // grid builds: the points as (x, y, z, 0) records for the sorted gather
  DevBuf<uint32_t> claim, ccnt, coffs, ccur, ctile, cslot, cdone;
  DevBuf<float> sd2;
  DevBuf<int32_t> ncnt;   // PCL-float radius normals: neighbours per query (chunk)
  DevBuf<int64_t> noff;   //   their offsets
  DevBuf<uint64_t> nkeys; //   (d2, index) keys
  DevBuf<int32_t> ovfa, ovfb;  // fused radius normals: queries with too many neighbours
  DevBuf<uint32_t> ovfc;       //   their counts
  DevBuf<long long> bst;
  PinBuf<long long> h_bst;
  DevBuf<unsigned long long> keys64, keys_alt;
  PinBuf<uint32_t> h_cnt;
  DevBuf<int32_t> lst;         // a call's index list (stage_list)
  DevBuf<float> ax, ay, az;    // flag_points: the uploaded cloud de-interleaved, original order
  DevBuf<uint8_t> flags;       //   its flagged rows
  DevBuf<int32_t> fin_pos;     //   their positions, ascending
};

// scratch of postProcessPlanes (postprocess_host.cpp)
struct PostWork {
  DevBuf<uint8_t> processed, flags, absorbed, keep;
  DevBuf<uint32_t> bcnt, boff, offs, abs_cnt, mask, csize;
  DevBuf<int32_t> cand, cand2, ids, parent, sel, rids, out, table, rest;
  DevBuf<PipTask> tasks;
  DevBuf<float4> planes, rays;
  DevBuf<PipEdge> edges;
  DevBuf<int64_t> edge_off;
};

// scratch of the voxel-grid filter (voxel_host.cpp; the list-order coordinates and records, the raw
// upload, the staged list and the hipcub temporaries are the shared nw.x/y/z, nw.rec, nw.raw,
// nw.lst, nw.sort_tmp)
struct VoxelWork {
  DevBuf<uint8_t> flags, lflag;
  DevBuf<uint32_t> keys_in, keys_out;
  DevBuf<int32_t> fin_pos, pos_in, pos_out, head, vid, vstart, keep, row, long_list, ocnt, voe;
  DevBuf<float> sx, sy, sz, ox, oy, oz;
};

// scratch of the statistical outlier filter (sor_host.cpp; the cloud, its finite points and their
// hierarchy are the shared nw.ax/ay/az, nw.x/y/z and nw.lv[])
struct SorWork {
  DevBuf<uint8_t> need, keep, rem;
  DevBuf<float> dist_pt, dist;
  DevBuf<int32_t> rank, sel_keep, sel_rem, out_keep, out_rem;
  DevBuf<unsigned long long> acc;
};

// scratch of the moving-least-squares filter (mls_host.cpp; the points, the grid and the staged
// list are the shared nw.x/y/z, nw.lv[0] and nw.lst)
struct MlsWork {
  DevBuf<uint8_t> need, valid;
  DevBuf<float4> res_p, res_n, o_nrm;  // per point: (x, y, z, branch), (nx, ny, nz, curvature)
  DevBuf<int32_t> cnt, sel, o_src, o_nb;
  DevBuf<float> o_xyz;
  DevBuf<unsigned long long> acc;
};

// scratch of the FPFH descriptors (fpfh_host.cpp; the points, the grid and the staged list are the
// shared nw.x/y/z, nw.lv[0] and nw.lst, the normals nw.nrm)
struct FpfhWork {
  DevBuf<float4> snrm;             // the normals in the grid's sorted order
  DevBuf<float> spfh, hist;        // n x 33 SPFH table; one 33-float row per list entry
  DevBuf<int32_t> cnt, pairs, counts, o_nb;
  DevBuf<unsigned long long> acc;
};

// scratch of the rigid registration (icp_host.cpp; the target, its finite points and their
// hierarchy are the shared nw.ax/ay/az, nw.x/y/z and nw.lv[])
struct IcpWork {
  DevBuf<uint8_t> state;             // one IcpState (icp.hpp)
  DevBuf<float> wx, wy, wz, d2;
  DevBuf<int32_t> qa, qb, nn;
  PinBuf<uint8_t, hipHostMallocCoherent> pub;  // k_icp_publish's copy of the state
};

// scratch of the SAC-IA initial alignment (sacia_host.cpp; the target, its valid rows and points
// and their hierarchy are the shared nw.ax/ay/az, nw.flags, nw.x/y/z and nw.lv[])
struct SaciaWork {
  DevBuf<uint8_t> state;             // one SaciaState (sacia.hpp)
  DevBuf<float> sx, sy, sz;          // the source's points, de-interleaved
  DevBuf<float> rows, queries, part_d, knn_d, xfs;
  DevBuf<int32_t> part_i, knn_i;
  DevBuf<unsigned long long> qa, qb, acc;
};

// scratch of the Gaussian-sphere plane seeds (gsphere_host.cpp; the points and their grid are the
// shared nw.x/y/z and nw.lv[0], the normals nw.nrm).  The parameter space of the last num_res is
// kept, on the host and on the device.
struct GsWork {
  gs::Space space;
  DevBuf<int32_t> table, coord;
  DevBuf<float> px, py, pz;
  DevBuf<int32_t> cell_of, votes, filt, queue, sink, sink_rank, label, lab_s, parent, root_of;
  DevBuf<int32_t> ids, ids_a, ids_b, first, offs, n_planes;
  DevBuf<uint32_t> reach, off, cur, size, total, key2, key2_out;
  DevBuf<uint64_t> keys, key1, key1_out;
  DevBuf<float> terms;
  DevBuf<uint8_t> heads, tmp;
  DevBuf<unsigned long long> cnt;
};

}  // namespace dlg

using namespace dlg;

// execution-path options of a context (dlg_ctx_set_option).  Every combination gives the same
// results: they only select among equivalent paths (tests run each against the oracle).
// (All ints, booleans as 0 / 1: one member type for the option table in driver.cpp.)
struct PathOptions {
  int prune = -1;       // Morton copy + pruned scoring: -1 clouds >= 131072 points, 0 never, 1 always
  int lean = 1;      // lean-list rounds (single-pass selects driven by the Morton copy)
  int spec_pick = 1;   // device pick for probability-1 rounds
  int prune_np = 1;    // pruned NORMAL_PLANE scoring
  int score_kernel = kScoreBf16;  // exhaustive scorer: kScoreBf16 or kScoreExact
  int prune_stats = 0;         // accumulate the pruned kernel's work counters (dlg_prune_stats)
  int sel1_tile = 16384;          // points per single-pass select tile (kSel1Points)
  int tile_scorer = DLG_TILE_EXACT;  // pruned plane scorer (spatial.hpp kTileScorer*)
  int nbr_fused = 1;           // PCL-float radius normals in one fused pass (else chunked)
  int bfs_wave = 1;            // RegulateNormal's claim pass: one wave per frontier node
  // PCL float refit (DLG_REFIT_PCL, any rank count): 1 = the nine sums on the device (fsum.hip,
  // exact), 0 = gathered to the host and summed there, 2 = device, and the host recomputes the
  // refit's tail from the published sums every round, 3 = as 2 and the round's select is always
  // redone with the host's plane (exercises the path an uncertain transcendental takes)
  int pcl_dev = 1;
  int hyp_shard = -1;  // every rank holds the whole cloud; rank r scores its slice of each
                       // batch's hypotheses, the counts are allreduced (DLG_OPT_HYP_SHARD: 1 on,
                       // 0 off, -1 = on when every rank holds the same cloud, ids included)
  int fs_protocol = 0;  // several ranks: the PCL refit's protocol (DLG_OPT_FS_ONE_WALK, 0..2)
  int fs_segments = 8;  // one rank: walkers per float chain (DLG_OPT_FS_SEGMENTS)
  int fs_poison = 0;    // tests only: fill the float-sum walk's window tables with garbage
                           // entries stamped for the next launch before the clear (fs_reset)
  int fault_round = 0;     // tests only (DLG_OPT_FAULT_INJECT): > 0 = this rank throws in the
                           // middle of extract round fault_round - 1 (after the round's scoring)
  int sync_check = 0;   // DLG_OPT_SYNC_CHECK: per-round allgather of (round, inliers,
                           // coefficient bits, collectives issued), mismatch fails the call
  int sel1_ticket = -1;    // DLG_OPT_SEL1_TICKET: single-pass select tiles numbered by an atomic
                           // ticket (dispatch order) instead of the workgroup index: 1 always,
                           // 0 never, -1 while another context of this process shares the device
  int bounds_stream = 0;    // DLG_OPT_BOUNDS_STREAM: lean rounds' survivor sphere bounds on a
                               // second stream beside the list pass (event-ordered)
  int spatial_curve = 1;  // DLG_OPT_SPATIAL_CURVE: 1 Hilbert, 0 Morton order of the spatial copy
  int fs_join = 1;     // DLG_OPT_FS_JOIN: segmented walk's joins by each chain's last walker
  int unrefined_list = 1;   // DLG_OPT_UNREFINED_LIST: lean PCL refit's inliers by one list pass
  int voxel_long_run = 32;  // DLG_OPT_VOXEL_LONG_RUN: voxels of this many points or more are summed
                            // by one wave each (voxel.hip), smaller ones by one thread each
  int sor_literal = 0;      // DLG_OPT_SOR_LITERAL (tests only): bit 0 every query's literal sum,
                            // bit 1 the literal statistics loop (sor_host.cpp)
  int icp_reversed = 0;     // DLG_OPT_ICP_REVERSED: the registration's level-0 pass visits W from
                            // the last entry to the first (icp.hip)
  int icp_max_blocks = 0;   // DLG_OPT_ICP_MAX_BLOCKS (tests only): n >= 1 caps the workgroups of
                            // every launch of the registration (icp.hip); 0 the default shapes
  int cull = 1;             // DLG_OPT_CULL: probability-1 rounds score only the hypotheses whose
                            // tile bound can still win (spatial.hpp): 0 off, 1 = the 64 largest
                            // bounds first, n >= 2 = the n largest first
  int cull_fuse = 1;        // DLG_OPT_CULL_FUSE (A/B): a culled round's selections run in the last
                            // workgroup of the launch before them (spatial.hpp); 0 = one launch each
};

struct dlg_ctx {
  int device = 0;
  bool counted = false;  // registered in the per-device context count (ctx_shared)
  PathOptions opt;
  int num_cus = 256;
  hipStream_t stream = nullptr;
  std::unique_ptr<Comm> comm;
  // hypothesis sharding (DLG_OPT_HYP_SHARD, SURVEY 8(e)'s small-N fallback): while a call on a
  // replicated cloud runs, `comm` is a one-rank communicator (every rank computes the whole
  // round), `solo` holds the real one and `hcomm` points at it for the scoring's split
  std::unique_ptr<Comm> solo;
  Comm* hcomm = nullptr;
  // the real communicator of the group (the one a failure must abort)
  Comm* group() const { return hcomm ? hcomm : comm.get(); }
  std::string err;
  bool profiling = false;
  bool walk_events = false;  // (profiling level 1: the PCL refit walk's events too)
  bool sp_all = true;  // every rank holds a valid spatial copy (agreed per extraction)
  // dlg_ctx_set_axis: setAxis / setEpsAngle of the axis-constrained plane models (read whenever
  // the model is SACMODEL_PERPENDICULAR_PLANE or SACMODEL_PARALLEL_PLANE; axis_model.hpp)
  float axis[3] = {0.0f, 0.0f, 0.0f};
  double eps_angle = 0.0;
  // scratch
  DevBuf<int32_t> pos;
  DevBuf<SampleRec> samples;
  DevBuf<HypRec> hyps;
  DevBuf<int32_t> res;  // counts[D] | good[D]
  DevBuf<int32_t> tile_in, tile_off_in, tile_off_out, totals;
  dlg::Sel1State sel1;  // single-pass selects: tile status words + launch epoch
  DevBuf<uint64_t> sel1_status;
  DevBuf<int32_t> sel1_err;  // sticky look-back failure word of the single-pass selects
  DevBuf<uint64_t> sel1_tk;  // their tile ticket counter (DLG_OPT_SEL1_TICKET; never reset:
                             // each launch's tickets start at the count issued before it)
  DevBuf<int64_t> partials, moments;  // fast refit: exact moment digits (exact_refit.hpp)
  DevBuf<unsigned> pick_done;          // the fused pick's workgroup ticket (zero between launches)
  DevBuf<unsigned> mom_done;           // k_moments' last-workgroup counter (zero between launches)
  DevBuf<double> scratch_f64;          // max-allreduce of host doubles
  DevBuf<uint64_t> sig;                // dlg_cloud_signature's result word
  DevBuf<int32_t> inl_gid;
  DevBuf<float> inl_xyz;
  DevBuf<int64_t> gath64;
  DevBuf<int32_t> gath32;
  PinBuf<int32_t> h_pos, h_res, h_tot;
  PinBuf<double> h_mom;
  PinBuf<int64_t> h_g64;
  DevBuf<float4> small;    // winning plane + samples + refined plane (segment.cpp)
  DevBuf<float4> np_cn;    // NORMAL_PLANE pruned scoring: the hypotheses' normalized normals
  DevBuf<uint16_t> lp;     // pruned scoring: per super-tile lists of near planes
  DevBuf<int32_t> lp_n;
  DevBuf<unsigned long long> pstats;  // pruned-kernel work counters (DLG_OPT_PRUNE_STATS)
  // culled scoring (DLG_OPT_CULL; spatial.hpp CullBufs): the bound pass's tile counts, the two
  // compacted candidate sets and the counters of dlg_cull_stats; zeroed when allocated
  DevBuf<int32_t> cull_i;
  DevBuf<HypRec> cull_h;
  bool cull_off = false;  // a round of this call scored more than D / 16 hypotheses: the rest
                          // of the call scores unculled
  PinBuf<float4> h_small;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  std::vector<int32_t> h_inl;
  std::vector<float> h_xyz;
  // inlier ids of the previous extract round: D2H into pinned staging is enqueued behind the
  // round's select, the memcpy into the caller's buffer runs while the next round's scoring
  // kernel executes (the host would otherwise only wait for it)
  PinBuf<int32_t> h_stage;
  hipEvent_t ev_stage = nullptr;
  // the deferred inlier copy runs on its own stream, off the rounds' critical path: it waits for
  // ev_inl (the round's select on the main stream); the next select waits for ev_stage
  hipStream_t cstream = nullptr;
  // DLG_OPT_BOUNDS_STREAM: the lean rounds' survivor sphere bounds on sstream beside the list
  // pass (forked by ev_fork, joined by ev_join on the main stream); created on first use
  hipStream_t sstream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr;
  hipEvent_t ev_inl = nullptr;
  hipEvent_t ev_inl_cur = nullptr;    // the marker the copy waits for (ev_inl, or the round's
                                      // end-of-select timing event when profiling)
  hipEvent_t ev_score_end = nullptr;  // (profiling) the last speculative round's scoring end
  bool stage_inflight = false;
  DevBuf<int32_t> pick;   // k_pick_p1 result
  PinBuf<int32_t, hipHostMallocCoherent> pub;  // k_publish's round results (pub[0] = sequence)
  int32_t pub_seq = 0;
  // the last compaction's predicted Morton-copy totals, checked at the next publish
  bool sp_check = false;
  int64_t sp_expect_in = 0, sp_expect_out = 0;
  dlg_extract_stats* sel_pending = nullptr;  // select_ms of the last round, not yet read
  hipEvent_t ev_sel[2][2] = {{nullptr, nullptr}, {nullptr, nullptr}};  // per-round pairs
  hipEvent_t ev_walk[2][6] = {};  // [pair][walk start, walk end, repair start, repair end]:   // the PCL refit's walk
  bool walk_rec[2] = {false, false};  // the pair's walk events were recorded this round
  bool rep_rec[2] = {false, false};   // ... and its repair events (several ranks, rank > 0)
  bool mid_rec[2] = {false, false};   // ... and the two walks' inner events (protocols 0, 2)
  int sel_k = 0;
  DevBuf<int32_t> rk;     // every rank's (inliers, survivors) of a round
  PinBuf<int32_t> h_rk;
  PinBuf<int32_t> h_pick;
  int64_t spec_misses = 0;  // speculative picks the host replay overturned
  double t_tot = 0.0;    // (DLG_TRACE) host time the last round's totals arrived
  ShuffleReplay replay;  // drawIndexSample replay table, reused by every segment on this context  // end of a round's totals D2H (work queued after it may still run)
  int32_t* pending_dst = nullptr;
  int64_t pending_n = 0;
  int64_t pending_off = 0;   // ids already copied to the caller (pumped while waiting)
  bool stage_ready = false;  // ev_stage has completed
  int32_t* emit_dst = nullptr;  // a round's inliers to copy (enqueued after the next launches)
  int64_t emit_n = 0;
  NormalsWork nw;
  dlg_knn_record knn_rec = {};  // dlg_knn_stats: the levels the last k-NN normals call used
  PostWork pw;
  VoxelWork vw;
  SorWork sw;
  MlsWork mw;
  IcpWork iw;
  FpfhWork fw;
  SaciaWork aw;
  GsWork gw;
  // PCL float refit on the device (fsum.hip): scratch sized for fs_cap inliers
  DevBuf<uint8_t> fs_scr;
  // the spatial index build's sort scratch (Morton keys and orders, ping-pong; radix-sort
  // temporaries), kept across builds: no allocation per build
  DevBuf<uint32_t> mk0, mk1;
  DevBuf<int32_t> mi0, mi1;
  DevBuf<uint8_t> msort;
  DevBuf<float4> mxyz;  // the points as (x, y, z, 0) records: k_gather_order's source
  int64_t fs_cap = -1;
  FsBuffers fs_b;
  DevBuf<float> fs_x, fs_y, fs_z;  // lean rounds: the unrefined plane's inliers in list order
  DevBuf<int32_t> fs_n;
  int64_t fs_checks = 0, fs_fixes = 0;  // host recomputations of the refit tail, and redone selects
};

struct dlg_cloud {
  dlg_ctx* ctx = nullptr;
  int64_t n_points = 0;  // records of the uploaded dlg_points (normals must match)
  int32_t id_base = 0;
  bool gid_ident = false;  // pristine gid[i] == id_base + i (uploaded without setIndices)
  bool repl_known = false, repl = false;  // several ranks: every rank holds this same cloud
                                          // (decided at the first call, hyp_shard_on)
  // content signature of the pristine list (k_signature), computed at the first
  // dlg_cloud_signature and kept (the pristine list never changes)
  bool sig_known = false;
  uint64_t sig = 0;
  bool has_normals = false;
  // the attached normals as given (PCL's normal_x/y/z and curvature, pristine order): RegulateNormal
  // on the device copy (dlg_cloud_regulate_normals) flips these and re-derives the normalised ones
  DevBuf<float4> raw_nrm;
  int64_t n_total = 0;
  int64_t n_active = 0;
  int cur = -1;  // -1 pristine, 0 = A, 1 = B
  SoA pristine, buf[2];
  float amax[3] = {0, 0, 0};
  float fmax = 0.0f;         // largest |coordinate| of the finite points (this rank's)
  bool qexp_known = false;   // fast refit quantum exponent (global over ranks), set lazily
  int qexp = 0;
  // Morton-ordered copy of the finite active points for the pruned scoring kernel (spatial.hpp):
  // built at upload (large clouds), compacted with the list in every SACMODEL_PLANE extract round
  bool sp_built = false;   // the pristine spatial copy exists
  bool sp_valid = false;   // the current spatial copy holds exactly the finite active points
  bool sp_dirty = false;   // sphere bounds of the working copy need recomputing
  int sp_cur = -1;         // -1 pristine, 0 / 1 ping-pong
  int64_t sp_n_pristine = 0, sp_n = 0;
  DevBuf<int32_t> sp_order;  // pristine index of each Morton-copy point (normals gathered by it)
  // curvature range of the uploaded normals (NaN ignored): bounds w = lambda (1 - curvature)
  bool curv_known = false;
  float curv_min = 0.0f, curv_max = 0.0f;
  SoA sp_pristine, sp_buf[2];
  // sphere bounds of the pristine copy and of each ping-pong buffer sp_buf[i]
  DevBuf<float4> sp_tiles_pr, sp_supers_pr, sp_tb[2], sp_sb[2];
  const SoA& sp_soa() const { return sp_cur < 0 ? sp_pristine : sp_buf[sp_cur]; }
  int sp_spare() const { return sp_cur == 0 ? 1 : 0; }
  PointsView view() const {
    const SoA& s = cur < 0 ? pristine : buf[cur];
    return s.view(n_active);
  }
  int spare() const { return cur == 0 ? 1 : 0; }
  // lean-list rounds (segment.cpp): the list buffer holds only pristine indices (in its gid
  // field; x, y, z, normals stale) until a path that reads coordinates materialises it
  bool buf_lean[2] = {false, false};
  bool list_lean() const { return cur >= 0 && buf_lean[cur]; }
  DevBuf<uint32_t> ubits;  // PCL refit in lean rounds: unrefined inliers by pristine index (zero between rounds)
  bool ubits_dirty = false;  // stamped but not (known to be) compacted: cleared before next use
  DevBuf<uint8_t> tag;  // per pristine point: the stamp of the select that took it
  int tagv = 0;         // last stamp used (tag[] is zeroed when the byte wraps)
};

namespace dlg {

inline void set_device(dlg_ctx* c) { HIPCHK(hipSetDevice(c->device)); }
// live contexts of this process per device (the look-back selects' tile numbering: ctx_shared)
void ctx_count_add(int device, int delta);
bool ctx_shared(int device);
// (several ranks over RCCL: a polling wait that ends when the group is aborted, comm.hpp)
inline void sync(dlg_ctx* c) { c->group()->sync_stream(c->stream); }

inline dlg_status fail(dlg_ctx* c, dlg_status code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}

// runs f with the context's device current; exceptions become status codes + dlg_last_error text
template <typename F>
dlg_status guarded(dlg_ctx* c, F&& f) {
  try {
    if (c) set_device(c);
    f();
    if (c) c->err.clear();
    return DLG_OK;
  } catch (const CommAborted& e) {
    return fail(c, DLG_ERR_COMM, e.what());
  } catch (const DlgError& e) {
    return fail(c, e.code, e.what());
  } catch (const std::exception& e) {
    return fail(c, DLG_ERR_INTERNAL, e.what());
  } catch (...) {
    return fail(c, DLG_ERR_INTERNAL, "unknown error");
  }
}

// guarded for the entry points whose ranks run collectives together: a rank that fails aborts
// its group, so every peer returns DLG_ERR_COMM (naming this rank and its error) instead of
// waiting in the next collective forever (the reference's convention: every caller gets a
// status back, PlaneDetect.h:371-375, 592-596).  A failed group stays aborted.
template <typename F>
dlg_status guarded_group(dlg_ctx* c, F&& f) {
  const dlg_status s = guarded(c, f);
  if (s != DLG_OK && s != DLG_ERR_COMM && c && c->group()->world() > 1)
    c->group()->abort("rank " + std::to_string(c->group()->rank()) + " failed: " + c->err);
  return s;
}

// the tail of an upload (make_cloud, cloud_call.hpp): the cloud's n points and ids are in its
// pristine list on the device; computes amax / fmax and builds the spatial copy under
// DLG_OPT_PRUNE's rule
void finish_upload(dlg_ctx* c, dlg_cloud* cl, int64_t n);

// normals on the device -> the cloud (dlg_cloud_set_normals, dlg_cloud_estimate_normals)
void attach_normals(dlg_ctx* c, dlg_cloud* cl, const float* raw_dev, int64_t stride_f,
                    int curv_off, bool by_pos);

// getFitnessScore(max_range) of src moved through the row-major 4x4 xf16 against tgt, by
// dlg_icp_align's own pass (icp_host.cpp; it builds the target's hierarchy again)
double icp_fitness(dlg_ctx* c, const dlg_points* src, const dlg_points* tgt, const float* xf16,
                   double max_range);

}  // namespace dlg
