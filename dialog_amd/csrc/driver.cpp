// driver.cpp -- the C ABI of the MI355X RANSAC plane path (include/dialog_ransac.h): context and
// cloud lifetime, options, the extract loop and the benchmark entry points.  A round itself --
// draw, gather, score, pick, refit, select, compact, publish -- is segment.cpp.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <climits>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/dialog_ransac.h"
#include "cloud_call.hpp"
#include "comm.hpp"
#include "driver.hpp"
#include "fsum.hpp"  // (dlg_float_sums)
#include "kernels.hpp"
#include "segment.hpp"
#include "spatial.hpp"

using namespace dlg;

namespace {

std::string g_last_create_error;

std::mutex g_ctx_mu;
std::map<int, int> g_ctx_count;  // live contexts per device

dlg_status init_ctx(dlg_ctx* c, int device) {
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess || n <= 0)
    return fail(c, DLG_ERR_NO_DEVICE, std::string("no HIP device: ") + hipGetErrorString(e));
  if (device < 0 || device >= n) return fail(c, DLG_ERR_NO_DEVICE, "device index out of range");
  hipDeviceProp_t p;
  if (hipGetDeviceProperties(&p, device) != hipSuccess)
    return fail(c, DLG_ERR_NO_DEVICE, "hipGetDeviceProperties failed");
  if (std::strncmp(p.gcnArchName, "gfx950", 6) != 0)
    return fail(c, DLG_ERR_NO_DEVICE, std::string("built for gfx950, device is ") + p.gcnArchName);
  c->device = device;
  c->num_cus = p.multiProcessorCount;
  return guarded(c, [&] {
    HIPCHK(hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking));
    HIPCHK(hipStreamCreateWithFlags(&c->cstream, hipStreamNonBlocking));
    HIPCHK(hipEventCreateWithFlags(&c->ev_inl, hipEventDisableTiming));
    for (auto& ev : c->ev) HIPCHK(hipEventCreate(&ev));
    ctx_count_add(device, 1);  // (last: a failed init is not counted)
    c->counted = true;
  });
}

}  // namespace

void dlg::ctx_count_add(int device, int delta) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  g_ctx_count[device] += delta;
}
bool dlg::ctx_shared(int device) {
  std::lock_guard<std::mutex> lk(g_ctx_mu);
  auto it = g_ctx_count.find(device);
  return it != g_ctx_count.end() && it->second > 1;
}

// normals records on the device (raw_dev: stride_f floats per record, curvature at curv_off,
// indexed by uploaded point (by_pos false) or by pristine position) -> the cloud's normal
// buffers (normalized, + curvature), the Morton copy's, the curvature range; the cloud is reset
void dlg::attach_normals(dlg_ctx* c, dlg_cloud* cl, const float* raw_dev, int64_t stride_f,
                    int curv_off, bool by_pos) {
  {
    cl->cur = -1;  // normals attach to the pristine list: the cloud is reset
    cl->n_active = cl->n_total;
    cl->pristine.ensure_nrm((size_t)std::max<int64_t>(cl->n_total, 1));
    cl->raw_nrm.ensure((size_t)std::max<int64_t>(cl->n_total, 1));
    if (raw_dev && cl->n_total > 0) {
      PointsView pv = cl->pristine.view(cl->n_total);
      if (by_pos) pv.gid = nullptr;
      // the records as given, in pristine order (unless they are that buffer already), then the
      // normalised copy the NORMAL_PLANE model reads
      if (raw_dev != reinterpret_cast<const float*>(cl->raw_nrm.p))
        launch_pack_point_normals(raw_dev, stride_f, curv_off, pv, cl->id_base, cl->raw_nrm.p,
                                  c->stream, false);
      pv.gid = nullptr;
      launch_pack_point_normals(reinterpret_cast<const float*>(cl->raw_nrm.p), 4, 3, pv,
                                cl->id_base, cl->pristine.nrm.p, c->stream, true);
      HIPCHK(hipGetLastError());
      // the Morton copy carries the normals too (pruned NORMAL_PLANE scoring)
      if (cl->sp_built) {
        cl->sp_pristine.ensure_nrm((size_t)std::max<int64_t>(cl->sp_n_pristine, 1));
        launch_gather_nrm(cl->pristine.nrm.p, cl->sp_order.p, cl->sp_n_pristine,
                          cl->sp_pristine.nrm.p, c->stream);
      }
      // curvature range -> the largest w = lambda (1 - curvature) of the cloud
      c->small.ensure(8);
      uint32_t* cr = reinterpret_cast<uint32_t*>(c->small.p + 7);
      launch_curv_range(cl->pristine.nrm.p, cl->n_total, cr, c->stream);
      uint32_t h[2] = {0u, 0u};
      HIPCHK(hipMemcpyAsync(h, cr, 8, hipMemcpyDeviceToHost, c->stream));
      HIPCHK(hipGetLastError());
      sync(c);
      auto ord2f = [](uint32_t o) {
        const uint32_t u = (o & 0x80000000u) ? (o & 0x7FFFFFFFu) : ~o;
        float f;
        std::memcpy(&f, &u, 4);
        return f;
      };
      cl->curv_known = h[0] <= h[1];  // (all NaN: no finite curvature)
      if (cl->curv_known) {
        cl->curv_min = ord2f(h[0]);
        cl->curv_max = ord2f(h[1]);
      }
    }
    cl->has_normals = true;
    cl->sp_cur = -1;  // (the reset above also resets the Morton copy)
    cl->sp_n = cl->sp_n_pristine;
    cl->sp_valid = cl->sp_built;
    cl->sp_dirty = false;
  }
}

void dlg::finish_upload(dlg_ctx* c, dlg_cloud* cl, int64_t n) {
  c->totals.ensure(8);
  launch_absmax(cl->pristine.view(n), reinterpret_cast<uint32_t*>(c->totals.p), c->stream);
  uint32_t bits[4];
  HIPCHK(hipMemcpyAsync(bits, c->totals.p, 16, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  for (int k = 0; k < 3; ++k) std::memcpy(&cl->amax[k], &bits[k], 4);
  std::memcpy(&cl->fmax, &bits[3], 4);
  if (c->opt.prune != 0 && n >= 3 && (n >= kPruneMinPoints || c->opt.prune == 1))
    build_spatial(c, cl);
}

// ================================================================================================
// C ABI
// ================================================================================================
extern "C" {

int dlg_abi_version(void) { return DLG_ABI_VERSION; }

int64_t dlg_abi_struct_size(int which) {
  switch (which) {
    case 0: return (int64_t)sizeof(dlg_points);
    case 1: return (int64_t)sizeof(dlg_sac_params);
    case 2: return (int64_t)sizeof(dlg_sac_stats);
    case 3: return (int64_t)sizeof(dlg_extract_stats);
    case 4: return (int64_t)sizeof(dlg_planes);
    case 5: return (int64_t)sizeof(dlg_postprocess_params);
    case 6: return (int64_t)sizeof(dlg_voxel_params);
    case 7: return (int64_t)sizeof(dlg_voxel_stats);
    case 8: return (int64_t)sizeof(dlg_sor_params);
    case 9: return (int64_t)sizeof(dlg_sor_stats);
    case 10: return (int64_t)sizeof(dlg_mls_params);
    case 11: return (int64_t)sizeof(dlg_mls_stats);
    // (12 is left unassigned)
    case 13: return (int64_t)sizeof(dlg_icp_params);
    case 14: return (int64_t)sizeof(dlg_icp_stats);
    case 15: return (int64_t)sizeof(dlg_icp_iteration);
    // (16 is left unassigned)
    case 17: return (int64_t)sizeof(dlg_fpfh_params);
    case 18: return (int64_t)sizeof(dlg_fpfh_stats);
    case 19: return (int64_t)sizeof(dlg_sac_ia_params);
    case 20: return (int64_t)sizeof(dlg_sac_ia_hypothesis);
    case 21: return (int64_t)sizeof(dlg_sac_ia_stats);
    // (22 is left unassigned)
    case 23: return (int64_t)sizeof(dlg_gs_params);
    case 24: return (int64_t)sizeof(dlg_gs_stats);
    case 25: return (int64_t)sizeof(dlg_gs_result);
    case 26: return (int64_t)sizeof(dlg_knn_record);
  }
  return -1;
}

const char* dlg_status_string(dlg_status s) {
  switch (s) {
    case DLG_OK: return "ok";
    case DLG_ERR_INVALID: return "invalid argument";
    case DLG_ERR_HIP: return "HIP error";
    case DLG_ERR_NO_DEVICE: return "no usable gfx950 device";
    case DLG_ERR_COMM: return "communicator error";
    case DLG_ERR_CAPACITY: return "output buffer too small";
    case DLG_ERR_INTERNAL: return "internal error";
  }
  return "unknown status";
}

void dlg_sac_params_default(dlg_sac_params* p) {
  if (!p) return;
  std::memset(p, 0, sizeof(*p));
  p->threshold = 0.0;  // SACSegmentation::threshold_ default
  p->max_iterations = 50;
  p->probability = 0.99;
  p->optimize = 1;
  p->seed = 12345u;
  p->model = DLG_SACMODEL_PLANE;
  p->normal_distance_weight = 0.1;
  p->refit_mode = DLG_REFIT_PCL;
  p->hypotheses_per_launch = 0;
  p->gather_inliers = 1;
}

dlg_status dlg_ctx_create(dlg_ctx** out, int device) {
  if (!out) return DLG_ERR_INVALID;
  *out = nullptr;
  auto c = std::make_unique<dlg_ctx>();
  dlg_status s = init_ctx(c.get(), device);
  if (s != DLG_OK) {
    g_last_create_error = c->err;
    return s;
  }
  c->comm = make_single_comm();
  *out = c.release();
  return DLG_OK;
}

dlg_status dlg_get_unique_id(void* uid) {
  if (!uid) return DLG_ERR_INVALID;
  std::string err;
  if (!rccl_get_unique_id(uid, &err)) {
    g_last_create_error = err;
    return DLG_ERR_COMM;
  }
  return DLG_OK;
}

dlg_status dlg_ctx_create_dist(dlg_ctx** out, int device, int rank, int world, const void* uid) {
  if (!out || world < 1 || rank < 0 || rank >= world || (world > 1 && !uid)) return DLG_ERR_INVALID;
  *out = nullptr;
  auto c = std::make_unique<dlg_ctx>();
  dlg_status s = init_ctx(c.get(), device);
  if (s != DLG_OK) {
    g_last_create_error = c->err;
    return s;
  }
  if (world == 1 && !uid) {  // (world 1 with an id: a 1-rank RCCL communicator)
    c->comm = make_single_comm();
  } else {
    std::string err;
    (void)hipSetDevice(device);
    c->comm = make_rccl_comm(rank, world, uid, &err);
    if (!c->comm) {
      g_last_create_error = err;
      dlg_ctx_destroy(c.release());  // (its streams, events and device count)
      return DLG_ERR_COMM;
    }
  }
  *out = c.release();
  return DLG_OK;
}

dlg_status dlg_ctx_create_loopback_group(dlg_ctx** out_array, int world, int device) {
  if (!out_array || world < 1) return DLG_ERR_INVALID;
  auto g = make_loopback_group(world);
  std::vector<dlg_ctx*> made;
  for (int r = 0; r < world; ++r) {
    auto c = std::make_unique<dlg_ctx>();
    dlg_status s = init_ctx(c.get(), device);
    if (s != DLG_OK) {
      g_last_create_error = c->err;
      for (auto* m : made) dlg_ctx_destroy(m);
      return s;
    }
    c->comm = make_loopback_comm(g, r);
    made.push_back(c.release());
  }
  for (int r = 0; r < world; ++r) out_array[r] = made[r];
  return DLG_OK;
}

dlg_status dlg_ctx_destroy(dlg_ctx* c) {
  if (!c) return DLG_OK;
  if (c->counted) ctx_count_add(c->device, -1);
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  c->comm.reset();
  if (c->ev_stage) (void)hipEventDestroy(c->ev_stage);
  if (c->ev_inl) (void)hipEventDestroy(c->ev_inl);
  if (c->cstream) {
    (void)hipStreamSynchronize(c->cstream);
    (void)hipStreamDestroy(c->cstream);
  }
  if (c->sstream) {
    (void)hipStreamSynchronize(c->sstream);
    (void)hipStreamDestroy(c->sstream);
  }
  if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
  if (c->ev_join) (void)hipEventDestroy(c->ev_join);
  for (auto& pr : c->ev_sel)
    for (auto& ev : pr)
      if (ev) (void)hipEventDestroy(ev);
  for (auto& pr : c->ev_walk)
    for (auto& ev : pr)
      if (ev) (void)hipEventDestroy(ev);
  for (auto& ev : c->ev)
    if (ev) (void)hipEventDestroy(ev);
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;  // (frees every buffer the context owns)
  return DLG_OK;
}

int64_t dlg_debug_live_bytes(int pinned) { return g_live_bytes[pinned ? 1 : 0].load(); }

const char* dlg_last_error(const dlg_ctx* c) {
  return c ? c->err.c_str() : g_last_create_error.c_str();
}

dlg_status dlg_ctx_info(const dlg_ctx* c, int* rank, int* world, int* device) {
  if (!c) return DLG_ERR_INVALID;
  if (rank) *rank = c->comm->rank();
  if (world) *world = c->comm->world();
  if (device) *device = c->device;
  return DLG_OK;
}

dlg_status dlg_cloud_upload(dlg_ctx* c, const dlg_points* pts, const int32_t* indices,
                            int64_t n_indices, int32_t id_base, dlg_cloud** out) {
  if (!c || !out) return DLG_ERR_INVALID;
  return make_cloud(c, id_base, out, [&](dlg_cloud& cl) {
    check_points(pts, "points", indices ? INT64_MAX : kMaxPoints);  // (a list may pick from more)
    const int64_t n = check_list(indices, n_indices, pts->n);
    const int64_t sf = pts->stride_bytes / 4;
    SoA& rows = cloud_rows(cl, n);
    cl.n_points = pts->n;
    cl.gid_ident = indices == nullptr;
    if (n && (!indices || 4 * n >= pts->n)) {
      // the caller's records go up as they are (one DMA), the SoA split and ids on the device
      const float* raw = upload_raw(c, pts);
      launch_upload_gather(raw, sf, stage_list(c, indices, (int)n), n, id_base, rows.out(),
                           c->stream);
      HIPCHK(hipGetLastError());
    } else if (n) {
      // a small subset of a large cloud: gather on the host
      std::vector<float> x(n), y(n), z(n);
      std::vector<int32_t> g(n);
      for (int64_t i = 0; i < n; ++i) {
        const int64_t k = indices[i];
        const float* p = pts->xyz + k * sf;
        x[i] = p[0]; y[i] = p[1]; z[i] = p[2];
        g[i] = (int32_t)(id_base + k);
      }
      HIPCHK(hipMemcpyAsync(rows.x.p, x.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(rows.y.p, y.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(rows.z.p, z.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
      HIPCHK(hipMemcpyAsync(rows.gid.p, g.data(), 4 * n, hipMemcpyHostToDevice, c->stream));
      sync(c);  // the host vectors go out of scope
    }
    return n;
  });
}

dlg_status dlg_cloud_destroy(dlg_cloud* cl) {
  if (!cl) return DLG_OK;
  if (cl->ctx) (void)hipSetDevice(cl->ctx->device);
  if (cl->ctx && cl->ctx->stream) (void)hipStreamSynchronize(cl->ctx->stream);
  delete cl;  // (frees every buffer the cloud owns)
  return DLG_OK;
}

dlg_status dlg_cloud_build_spatial(dlg_ctx* c, dlg_cloud* cl) {
  if (!c || !cl || cl->ctx != c) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    if (cl->n_total < 3 || cl->sp_built) return;
    if (cl->cur >= 0) throw DlgError(DLG_ERR_INVALID, "build the spatial copy before extracting (or after dlg_cloud_reset)");
    build_spatial(c, cl);
  });
}

dlg_status dlg_cloud_drop_spatial(dlg_cloud* cl) {
  if (!cl) return DLG_ERR_INVALID;
  // (the copy's device buffers stay allocated for the next build -- hipFree synchronises the
  // device and a rebuild would allocate them again; dlg_cloud_destroy frees them)
  cl->sp_built = cl->sp_valid = false;
  cl->sp_n = cl->sp_n_pristine = 0;
  cl->cur = -1;  // (a lean list needs the Morton copy: back to the pristine list)
  cl->n_active = cl->n_total;
  cl->sp_cur = -1;
  cl->sp_dirty = false;
  return DLG_OK;
}

dlg_status dlg_cloud_reset(dlg_cloud* cl) {
  if (!cl) return DLG_ERR_INVALID;
  cl->cur = -1;
  cl->n_active = cl->n_total;
  cl->sp_cur = -1;
  cl->sp_n = cl->sp_n_pristine;
  cl->sp_valid = cl->sp_built;
  cl->sp_dirty = false;
  return DLG_OK;
}

dlg_status dlg_cloud_active(const dlg_cloud* cl, int64_t* n) {
  if (!cl || !n) return DLG_ERR_INVALID;
  *n = cl->n_active;
  return DLG_OK;
}

dlg_status dlg_cloud_signature(dlg_ctx* c, dlg_cloud* cl, uint64_t* out) {
  if (!c || !cl || !out || cl->ctx != c) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    if (!cl->sig_known) {  // one reduction per cloud, on demand: no upload pays for it
      c->sig.ensure(1);
      launch_signature(cl->pristine.view(cl->n_total), c->sig.p, c->stream);
      HIPCHK(hipGetLastError());
      uint64_t h = 0;
      HIPCHK(hipMemcpyAsync(&h, c->sig.p, 8, hipMemcpyDeviceToHost, c->stream));
      sync(c);
      cl->sig = h;
      cl->sig_known = true;
    }
    *out = cl->sig;
  });
}

dlg_status dlg_cloud_set_normals(dlg_ctx* c, dlg_cloud* cl, const float* normals, int64_t n,
                                 int64_t stride_bytes) {
  if (!c || !cl || cl->ctx != c || (n > 0 && !normals)) return DLG_ERR_INVALID;
  if (n != cl->n_points)
    return fail(c, DLG_ERR_INVALID, "normals must have one record per uploaded point");
  if (stride_bytes != 16 && (stride_bytes < 32 || stride_bytes % 4))
    return fail(c, DLG_ERR_INVALID, "stride_bytes must be 16 (nx, ny, nz, curvature) or >= 32 (pcl::Normal)");
  return guarded(c, [&] {
    const float* raw_dev = nullptr;
    if (n > 0) {
      DevBuf<uint8_t>& raw = c->nw.raw;  // scratch shared with the normals path
      raw.ensure((size_t)n * (size_t)stride_bytes);
      HIPCHK(hipMemcpyAsync(raw.p, normals, (size_t)n * (size_t)stride_bytes,
                            hipMemcpyHostToDevice, c->stream));
      raw_dev = reinterpret_cast<const float*>(raw.p);
    }
    attach_normals(c, cl, raw_dev, stride_bytes / 4, stride_bytes == 16 ? 3 : 4, false);
  });
}

namespace {
// DLG_OPT_HYP_SHARD on a multi-rank context: for the call, the context runs as one rank (every
// rank holds the whole cloud and computes the same round) and only the scoring is split by
// hypotheses over the real communicator (SegmentRound::score: slices + an allreduce of the counts)
struct HypShardScope {
  dlg_ctx* c;
  bool on;
  HypShardScope(dlg_ctx* ctx, bool enable) : c(ctx), on(enable) {
    if (!on) return;
    if (!c->solo) c->solo = make_single_comm();
    std::swap(c->comm, c->solo);
    c->hcomm = c->solo.get();
  }
  ~HypShardScope() {
    if (!on) return;
    std::swap(c->comm, c->solo);
    c->hcomm = nullptr;
  }
};

// whether a call on this cloud runs hypothesis-sharded.  DLG_OPT_HYP_SHARD -1 (default): when
// every rank holds the same cloud -- the same ids (id_base, count, identity) and the same extent --
// which is how SURVEY 8(e)'s small-N fallback is set up (dlg_shard_range hands every rank the
// whole cloud when point shards would fall below the Morton-copy cut-off); point-sharding such a
// replicated cloud would count every point once per rank.  Decided once per cloud (one allgather
// of a signature; every rank decides alike).
bool hyp_shard_on(dlg_ctx* c, dlg_cloud* cl) {
  if (c->comm->world() == 1) return false;
  if (c->opt.hyp_shard >= 0) return c->opt.hyp_shard == 1;
  if (!cl->repl_known) {
    uint64_t h = 1469598103934665603ull;
    auto mix = [&](uint64_t v) {
      for (int k = 0; k < 8; ++k) h = (h ^ ((v >> (8 * k)) & 0xFFu)) * 1099511628211ull;
    };
    mix((uint64_t)cl->n_points);
    mix((uint64_t)cl->n_total);
    mix((uint64_t)(uint32_t)cl->id_base);
    mix(cl->gid_ident ? 1u : 0u);
    uint32_t b[4];
    std::memcpy(b, cl->amax, 12);
    std::memcpy(b + 3, &cl->fmax, 4);
    for (uint32_t v : b) mix(v);
    std::vector<int64_t> all;
    allgather_i64(c, (int64_t)(h >> 1), &all);
    cl->repl = std::all_of(all.begin(), all.end(), [&](int64_t v) { return v == all[0]; });
    cl->repl_known = true;
  }
  return cl->repl;
}
}  // namespace

dlg_status dlg_sac_segment(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params* prm, float coeff_out[4],
                           int32_t* inliers_out, int64_t cap, int64_t* n_inliers,
                           dlg_sac_stats* stats) {
  if (!c || !cl || !prm || !coeff_out || !n_inliers || cl->ctx != c) return DLG_ERR_INVALID;
  if (!inliers_out && cap > 0) return DLG_ERR_INVALID;
  dlg_sac_stats local;
  dlg_sac_stats* st = stats ? stats : &local;
  return guarded_group(c, [&] {
    HypShardScope hs(c, hyp_shard_on(c, cl));
    c->cull_off = false;
    std::memset(coeff_out, 0, 4 * sizeof(float));
    *n_inliers = 0;
    SegOut so = segment_round(c, cl, *prm, false, st, nullptr);
    if (!so.has_model) return;
    std::memcpy(coeff_out, so.coeff, sizeof(so.coeff));
    int64_t g = 0;
    *n_inliers = emit_inliers(c, so, prm->gather_inliers != 0, inliers_out, cap, &g);
  });
}

dlg_status dlg_sac_segment_host(dlg_ctx* c, const dlg_points* pts, const int32_t* indices,
                                int64_t n_indices, const dlg_sac_params* prm, float coeff_out[4],
                                int32_t* inliers_out, int64_t cap, int64_t* n_inliers,
                                dlg_sac_stats* stats) {
  dlg_cloud* cl = nullptr;
  dlg_status s = dlg_cloud_upload(c, pts, indices, n_indices, 0, &cl);
  if (s != DLG_OK) return s;
  s = dlg_sac_segment(c, cl, prm, coeff_out, inliers_out, cap, n_inliers, stats);
  dlg_cloud_destroy(cl);
  return s;
}

dlg_status dlg_extract_planes(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params* prm, int max_planes,
                              int64_t min_inliers, float* coeffs_out, int64_t* offsets_out,
                              int32_t* inliers_out, int64_t cap, int* n_planes,
                              dlg_extract_stats* stats) {
  if (!c || !cl || !prm || max_planes < 0 || !n_planes || cl->ctx != c) return DLG_ERR_INVALID;
  if (max_planes > 0 && (!coeffs_out || !offsets_out)) return DLG_ERR_INVALID;
  if (!inliers_out && cap > 0) return DLG_ERR_INVALID;
  dlg_extract_stats local;
  dlg_extract_stats* xs = stats ? stats : &local;
  std::memset(xs, 0, sizeof(*xs));
  auto t0 = std::chrono::steady_clock::now();
  dlg_status s = guarded_group(c, [&] {
    HypShardScope hs(c, hyp_shard_on(c, cl));
    c->cull_off = false;  // (DLG_OPT_CULL's fallback lasts one call)
    *n_planes = 0;
    if (max_planes > 0) offsets_out[0] = 0;
    int64_t written = 0;
    const int64_t floor_n = std::max<int64_t>(3, min_inliers);
    // every rank's active count: gathered once, then carried from each round's survivors
    std::vector<int64_t> active;
    // (bit 40: this rank holds a valid spatial copy.  Lean rounds change the round's collective
    // sequence, so they run only when every rank can take them: one agreed decision per call)
    constexpr int64_t kSpBit = int64_t(1) << 40;
    int64_t N = allgather_i64(c, cl->n_active | (cl->sp_valid ? kSpBit : 0), &active);
    c->sp_all = true;
    N = 0;
    for (int64_t& v : active) {
      c->sp_all = c->sp_all && (v & kSpBit) != 0;
      v &= kSpBit - 1;
      N += v;
    }
    for (int p = 0; p < max_planes; ++p) {
      if (N < floor_n) break;
      dlg_sac_stats st;
      SegOut so = segment_round(c, cl, *prm, true, &st, xs, &active);
      if (c->opt.sync_check) check_in_step(c, p, so);
      xs->rounds++;
      if (!so.has_model) break;
      if (so.lean) xs->lean_rounds++;
      const int64_t n_in = so.n_in_global;
      if (n_in == 0 || n_in < min_inliers) break;  // plane rejected: active list unchanged
      int64_t g = 0;
      const double t_e0 = trace_on() ? now_ms() : 0.0;
      int64_t n = emit_inliers(c, so, prm->gather_inliers != 0, inliers_out + written,
                               cap - written, &g, /*deferred=*/true, /*counts_known=*/true);
      if (trace_on())
        std::fprintf(stderr, "[dlg] after-round: segment-return %.3fms emit %.3fms\n",
                     t_e0 - c->t_tot, now_ms() - t_e0);
      std::memcpy(coeffs_out + 4 * p, so.coeff, sizeof(so.coeff));
      written += n;
      offsets_out[p + 1] = written;
      *n_planes = p + 1;
      commit_round(cl, so);
      active = so.out_ranks;
      N = 0;
      for (int64_t v : active) N += v;
    }
    flush_emit(c);
    drain_pending(c);
    // A stream synchronisation lets the HIP runtime reclaim the per-command resources of the
    // rounds: with event waits alone they pile up until a D2H copy blocks the host for ~10 ms
    // (measured: every ~55 rounds).  The stream only holds the last round's tails here.
    sync(c);
    settle_round(c);
  });
  c->pending_dst = nullptr;  // (error path: never write into the caller's buffer later)
  c->pending_n = c->pending_off = 0;
  c->emit_dst = nullptr;
  c->emit_n = 0;
  c->sel_pending = nullptr;  // (never read into the caller's stats after the call)
  c->sp_check = false;
  xs->wall_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  return s;
}

dlg_status dlg_ctx_set_axis(dlg_ctx* c, const float axis[3], double eps_angle) {
  if (!c || !axis) return DLG_ERR_INVALID;
  for (int k = 0; k < 3; ++k)
    if (!std::isfinite(axis[k])) return fail(c, DLG_ERR_INVALID, "axis component is NaN or infinite");
  if (eps_angle != eps_angle) return fail(c, DLG_ERR_INVALID, "eps_angle is NaN");
  std::memcpy(c->axis, axis, sizeof(c->axis));
  c->eps_angle = eps_angle;
  return DLG_OK;
}

dlg_status dlg_ctx_get_axis(const dlg_ctx* c, float axis[3], double* eps_angle) {
  if (!c || !axis || !eps_angle) return DLG_ERR_INVALID;
  std::memcpy(axis, c->axis, sizeof(c->axis));
  *eps_angle = c->eps_angle;
  return DLG_OK;
}

dlg_status dlg_score_samples(dlg_ctx* c, dlg_cloud* cl, const dlg_sac_params* prm,
                             const int32_t* positions, int n_draws, int32_t* counts_out,
                             int32_t* good_out, int32_t* valid_out, float* coeffs_out) {
  if (!c || !cl || !prm || !positions || !counts_out || !good_out || cl->ctx != c)
    return DLG_ERR_INVALID;
  if (n_draws < 1 || n_draws > kMaxHypPerLaunch) return fail(c, DLG_ERR_INVALID, "n_draws: 1..4096");
  return guarded_group(c, [&] {
    HypShardScope hs(c, hyp_shard_on(c, cl));
    score_samples(c, cl, *prm, positions, n_draws, counts_out, good_out, valid_out, coeffs_out);
  });
}

dlg_status dlg_axis_verdicts(int model, double eps_angle, const float* f, int64_t n,
                             int32_t* by_threshold, int32_t* by_formula, float thresholds[2]) {
  if ((model != DLG_SACMODEL_PERPENDICULAR_PLANE && model != DLG_SACMODEL_PARALLEL_PLANE) ||
      n < 0 || (n > 0 && (!f || !by_threshold || !by_formula)) || eps_angle != eps_angle)
    return DLG_ERR_INVALID;
  const float unit[3] = {0.0f, 0.0f, 1.0f};
  const AxisTest t = make_axis_test(model, unit, eps_angle);
  if (thresholds) {
    thresholds[0] = t.t_lo;
    thresholds[1] = t.t_hi;
  }
  for (int64_t i = 0; i < n; ++i) {
    by_threshold[i] = t.mode == kAxisNone || axis_verdict(t, f[i]) ? 1 : 0;
    by_formula[i] = !(eps_angle > 0.0) ? 1
                    : model == DLG_SACMODEL_PERPENDICULAR_PLANE
                        ? (perpendicular_valid_direct(f[i], eps_angle) ? 1 : 0)
                        : (parallel_valid_direct(f[i], eps_angle) ? 1 : 0);
  }
  return DLG_OK;
}

dlg_status dlg_float_sums(dlg_ctx* c, const float* xyz, int64_t n, const float cin[4], int reps,
                          float sums_out[9], float coeff_out[4], int* uncertain,
                          double* ms_per_call, int64_t* walk_stats) {
  if (!c || n < 0 || n > INT32_MAX || (n > 0 && !xyz) || !cin || reps < 1 || !sums_out ||
      !coeff_out || !uncertain || !ms_per_call)
    return DLG_ERR_INVALID;
  return guarded(c, [&] {
    DevBuf<float> dx;
    DevBuf<float4> dc;
    DevBuf<int32_t> dn, dres;
    DevBuf<uint8_t> scr;
    dx.ensure(3 * (size_t)std::max<int64_t>(n, 1));
    dc.ensure(2);
    dn.ensure(1);
    dres.ensure(16);
    scr.ensure(fs_scratch_bytes(std::max<int64_t>(n, 1), 1));
    FsBuffers b = fs_carve(scr.p, std::max<int64_t>(n, 1), 1);
    DevBuf<int64_t> wst;
    if (walk_stats) {
      wst.ensure(72);
      HIPCHK(hipMemsetAsync(wst.p, 0, 72 * 8, c->stream));
      b.wst = wst.p;
    }
    HIPCHK(fs_reset(b, c->stream, c->opt.fs_poison));
    if (n) HIPCHK(hipMemcpyAsync(dx.p, xyz, 12 * (size_t)n, hipMemcpyHostToDevice, c->stream));
    const int32_t n32 = (int32_t)n;
    const float4 ci = make_float4(cin[0], cin[1], cin[2], cin[3]);
    HIPCHK(hipMemcpyAsync(dn.p, &n32, 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(hipMemcpyAsync(dc.p, &ci, 16, hipMemcpyHostToDevice, c->stream));
    double total = 0.0;
    for (int r = 0; r < reps; ++r) {
      if (walk_stats) HIPCHK(hipMemsetAsync(wst.p, 0, 72 * 8, c->stream));  // (the last call's)
      HIPCHK(hipEventRecord(c->ev[0], c->stream));
      launch_fs_refit(dx.p, dx.p + 1, dx.p + 2, 3, dn.p, std::max<int64_t>(n, 1), b, dc.p,
                      dc.p + 1, dres.p, c->num_cus, c->stream, nullptr, nullptr, nullptr, nullptr,
                      nullptr, 0, nullptr, c->opt.fs_segments, nullptr, nullptr,
                      c->opt.fs_join);
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[1], c->stream));
      sync(c);
      total += event_ms(c, 0, 1);
    }
    int32_t h[16];
    float4 co;
    HIPCHK(hipMemcpy(h, dres.p, sizeof(h), hipMemcpyDeviceToHost));
    HIPCHK(hipMemcpy(&co, dc.p + 1, 16, hipMemcpyDeviceToHost));
    std::memcpy(sums_out, h + 2, 9 * sizeof(float));
    coeff_out[0] = co.x; coeff_out[1] = co.y; coeff_out[2] = co.z; coeff_out[3] = co.w;
    *uncertain = h[0];
    *ms_per_call = total / reps;
    if (walk_stats) HIPCHK(hipMemcpy(walk_stats, wst.p, 72 * 8, hipMemcpyDeviceToHost));
  });
}

dlg_status dlg_score_benchmark(dlg_ctx* c, dlg_cloud* cl, int D, int kernel, int reps,
                               double threshold, double* ms_per_launch, int32_t* counts_out) {
  if (!c || !cl || D < 1 || D > kMaxHypPerLaunch || reps < 1 || !ms_per_launch) return DLG_ERR_INVALID;
  if (kernel != kScoreExact && kernel != kScoreBf16 && kernel != kScorePruned &&
      kernel != DLG_SCORE_BOUND && kernel != DLG_SCORE_CULLED)
    return DLG_ERR_INVALID;
  const int variant = kernel;
  const bool culled = kernel == DLG_SCORE_BOUND || kernel == DLG_SCORE_CULLED;
  return guarded(c, [&] {
    ensure_list_xyz(c, cl);
    const PointsView src = cl->view();
    if (src.n < 3) throw DlgError(DLG_ERR_INVALID, "need >= 3 active points");
    Mt19937 rng(777u);
    c->h_pos.ensure(3 * (size_t)D);
    for (int i = 0; i < 3 * D; ++i) c->h_pos.p[i] = (int32_t)((uint32_t)rng.rnd() % (uint64_t)src.n);
    c->pos.ensure(3 * (size_t)D);
    c->samples.ensure(3 * (size_t)D);
    c->hyps.ensure(kHypScratchBytes / sizeof(HypRec) + 1);
    c->res.ensure(2 * (size_t)kMaxHypPerLaunch + 64);
    const float cthr = thr_ceil(threshold);
    if ((variant == kScorePruned || culled) && cl->sp_valid) ensure_sphere_bounds(c, cl);
    HIPCHK(hipMemcpyAsync(c->pos.p, c->h_pos.p, 12 * (size_t)D, hipMemcpyHostToDevice, c->stream));
    launch_gather_samples(c->pos.p, 3 * D, 0, src, c->samples.p, c->stream);
    const int Dp = (D + 63) / 64 * 64;
    launch_build_hyps(c->samples.p, D, cthr, cl->amax[0], cl->amax[1], cl->amax[2], c->hyps.p,
                      c->res.p + Dp, c->stream);
    double total = 0.0;
    for (int r = 0; r < reps; ++r) {
      // (DLG_SCORE_CULLED: a hypothesis no pass scores keeps the fill, -1)
      HIPCHK(hipMemsetAsync(c->res.p, kernel == DLG_SCORE_CULLED ? 0xFF : 0, 4 * (size_t)Dp, c->stream));
      HIPCHK(hipEventRecord(c->ev[0], c->stream));
      if (culled) {
        // the culled round's launches (spatial.hpp) with DLG_OPT_CULL's K, without the pick
        if (!cl->sp_valid || cl->sp_n <= 0) throw DlgError(DLG_ERR_INVALID, "cloud has no spatial copy");
        c->lp.ensure((size_t)sp_supers(cl->sp_n) * prune_list_stride(D) + 1);
        ensure_prune_work(c, sp_supers(cl->sp_n));
        const int K = cull_k(c->opt.cull);
        launch_score_culled(spatial_view(cl), c->hyps.p, D, Dp, K, cthr, prune_margin(cthr, cl->amax),
                            c->res.p, c->lp.p, c->lp_n.p + kPwHeader, c->num_cus, c->stream,
                            prune_stats_ptr(c), ensure_cull(c), nullptr, nullptr, nullptr,
                            kernel == DLG_SCORE_BOUND ? kCullBenchBound : kCullBenchCounts,
                            c->opt.cull_fuse != 0);
      } else if (variant == kScorePruned) {
        if (!cl->sp_valid) throw DlgError(DLG_ERR_INVALID, "cloud has no spatial copy");
        c->lp.ensure((size_t)sp_supers(cl->sp_n) * prune_list_stride(D) + 1);
        ensure_prune_work(c, sp_supers(cl->sp_n));
        unsigned long long* stp = prune_stats_ptr(c);
        launch_score_pruned(spatial_view(cl), c->hyps.p, D, cthr, prune_margin(cthr, cl->amax),
                            cl->amax, c->res.p, c->lp.p, c->lp_n.p + kPwHeader, c->num_cus, c->stream, stp,
                            nullptr, nullptr, nullptr, nullptr, c->opt.tile_scorer);
      } else {
        launch_score(src, c->hyps.p, D, cthr, c->res.p, variant, c->num_cus, c->stream);
      }
      HIPCHK(hipGetLastError());
      HIPCHK(hipEventRecord(c->ev[1], c->stream));
      sync(c);
      total += event_ms(c, 0, 1);
    }
    *ms_per_launch = total / reps;
    if (counts_out) {
      HIPCHK(hipMemcpyAsync(counts_out, c->res.p, 4 * (size_t)D, hipMemcpyDeviceToHost, c->stream));
      sync(c);
    }
  });
}

namespace {
// one row per DLG_OPT_* held in PathOptions: values in [lo, hi] are accepted (`range` is the text
// of the error for any other); a null `range` marks a boolean: any value, non-zero is true
struct OptRow {
  int id;
  const char* name;
  int PathOptions::*member;
  int64_t lo, hi;
  const char* range;
};
#define OPT(ID, MEMBER, ...) {ID, #ID, &PathOptions::MEMBER, __VA_ARGS__}
#define OPT_BOOL(ID, MEMBER) OPT(ID, MEMBER, 0, 1, nullptr)
static_assert(DLG_SCORE_EXACT == 0 && DLG_SCORE_BF16 == 1, "DLG_OPT_SCORE_KERNEL's range below");
const OptRow kOptions[] = {
    OPT(DLG_OPT_PRUNE, prune, -1, 1, "-1, 0 or 1"),
    OPT_BOOL(DLG_OPT_LEAN_ROUNDS, lean),
    OPT_BOOL(DLG_OPT_SPEC_PICK, spec_pick),
    OPT_BOOL(DLG_OPT_PRUNE_NP, prune_np),
    OPT(DLG_OPT_SCORE_KERNEL, score_kernel, 0, 1, "DLG_SCORE_BF16 or DLG_SCORE_EXACT"),  // (stored as kScore*)
    OPT_BOOL(DLG_OPT_PRUNE_STATS, prune_stats),  // (setting it clears the counters)
    // (within the range only kSel1Points)
    OPT(DLG_OPT_SELECT_TILE, sel1_tile, kSel1Points[0], kSel1Points[2], "4096, 8192 or 16384"),
    OPT(DLG_OPT_PCL_REFIT_DEVICE, pcl_dev, 0, 3, "0..3"),
    // (within the range only the DLG_TILE_* values, and the A/B-only kernel variants
    // kTileScorerExK1/ExK4/ExPk and claim variants 15..17: tile_scorer_ok)
    OPT(DLG_OPT_PRUNE_TILE_SCORER, tile_scorer, 0, kTileScorerMfmaW, "DLG_TILE_EXACT or DLG_TILE_BF16"),
    OPT_BOOL(DLG_OPT_NORMALS_FUSED, nbr_fused),
    OPT_BOOL(DLG_OPT_REGULATE_WAVE, bfs_wave),
    OPT_BOOL(DLG_OPT_FS_POISON, fs_poison),
    OPT(DLG_OPT_HYP_SHARD, hyp_shard, -1, 1, "-1, 0 or 1"),
    OPT(DLG_OPT_FS_ONE_WALK, fs_protocol, 0, 2, "0..2"),
    OPT(DLG_OPT_FS_SEGMENTS, fs_segments, 1, kFsSegMax, "1..16"),
    OPT(DLG_OPT_FAULT_INJECT, fault_round, 0, INT64_MAX, ">= 0"),
    OPT_BOOL(DLG_OPT_SYNC_CHECK, sync_check),
    OPT(DLG_OPT_SEL1_TICKET, sel1_ticket, -1, 1, "-1, 0 or 1"),
    OPT_BOOL(DLG_OPT_BOUNDS_STREAM, bounds_stream),
    OPT(DLG_OPT_SPATIAL_CURVE, spatial_curve, 0, 1, "0 or 1"),
    OPT_BOOL(DLG_OPT_FS_JOIN, fs_join),
    OPT_BOOL(DLG_OPT_UNREFINED_LIST, unrefined_list),
    OPT(DLG_OPT_VOXEL_LONG_RUN, voxel_long_run, 1, INT32_MAX, "1..2147483647"),
    OPT(DLG_OPT_SOR_LITERAL, sor_literal, 0, 3, "0..3"),
    OPT_BOOL(DLG_OPT_ICP_REVERSED, icp_reversed),
    OPT(DLG_OPT_ICP_MAX_BLOCKS, icp_max_blocks, 0, 65536, "0..65536"),
    OPT(DLG_OPT_CULL, cull, 0, kMaxHypPerLaunch, "0..4096"),
    OPT_BOOL(DLG_OPT_CULL_FUSE, cull_fuse),
};
#undef OPT_BOOL
#undef OPT

const OptRow* find_option(int id) {
  for (const OptRow& r : kOptions)
    if (r.id == id) return &r;
  return nullptr;
}

bool tile_scorer_ok(int64_t v) {
  return v == DLG_TILE_EXACT || v == DLG_TILE_BF16 || v == DLG_TILE_MFMA || v == kTileScorerExK1 ||
         v == kTileScorerMfmaX || v == kTileScorerMfmaW || v == kTileScorerExK4 ||
         v == kTileScorerExPk || (v >= kTileScorerClaimR4 && v <= kTileScorerClaimTail);
}
}  // namespace

dlg_status dlg_ctx_set_option(dlg_ctx* c, int option, int64_t value) {
  if (!c) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    if (option == DLG_OPT_COMM_TIMEOUT_MS) {  // (lives on the communicators)
      if (value < 0) throw DlgError(DLG_ERR_INVALID, "DLG_OPT_COMM_TIMEOUT_MS: >= 0");
      c->comm->timeout_ms = value;
      if (c->solo) c->solo->timeout_ms = value;
      return;
    }
    const OptRow* r = find_option(option);
    if (!r) throw DlgError(DLG_ERR_INVALID, "unknown option");
    if (!r->range) value = value != 0;
    bool ok = value >= r->lo && value <= r->hi;
    if (option == DLG_OPT_SELECT_TILE) ok = ok && (value == kSel1Points[1] || value == r->lo || value == r->hi);
    if (option == DLG_OPT_PRUNE_TILE_SCORER) ok = ok && tile_scorer_ok(value);
    if (!ok) throw DlgError(DLG_ERR_INVALID, std::string(r->name) + ": " + r->range);
    if (option == DLG_OPT_SCORE_KERNEL) value = value == DLG_SCORE_EXACT ? kScoreExact : kScoreBf16;
    c->opt.*r->member = (int)value;
    if (option == DLG_OPT_PRUNE_STATS && value) {
      c->pstats.ensure(8);
      HIPCHK(hipMemsetAsync(c->pstats.p, 0, 8 * sizeof(unsigned long long), c->stream));
    }
  });
}

dlg_status dlg_ctx_get_option(const dlg_ctx* c, int option, int64_t* value) {
  if (!c || !value) return DLG_ERR_INVALID;
  const OptRow* r = find_option(option);
  if (option == DLG_OPT_COMM_TIMEOUT_MS) *value = c->comm->timeout_ms;
  else if (!r) return DLG_ERR_INVALID;
  else if (option == DLG_OPT_SCORE_KERNEL)
    *value = c->opt.score_kernel == kScoreExact ? DLG_SCORE_EXACT : DLG_SCORE_BF16;
  else *value = c->opt.*r->member;
  return DLG_OK;
}

dlg_status dlg_prune_stats(dlg_ctx* c, uint64_t out[8], int reset) {
  if (!c || !out) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    std::memset(out, 0, 8 * sizeof(uint64_t));
    if (!c->opt.prune_stats) return;
    HIPCHK(hipMemcpyAsync(out, c->pstats.p, 8 * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(hipMemsetAsync(c->pstats.p, 0, 8 * sizeof(unsigned long long), c->stream));
    sync(c);
  });
}

dlg_status dlg_cull_stats(dlg_ctx* c, uint64_t out[8], int reset) {
  if (!c || !out) return DLG_ERR_INVALID;
  return guarded(c, [&] {
    std::memset(out, 0, kCullStats * sizeof(uint64_t));
    if (!c->cull_i.p) return;  // (no culled round yet)
    unsigned long long* st = ensure_cull(c).stats;
    HIPCHK(hipMemcpyAsync(out, st, kCullStats * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    if (reset) HIPCHK(hipMemsetAsync(st, 0, kCullStats * sizeof(unsigned long long), c->stream));
    sync(c);
  });
}

dlg_status dlg_knn_stats(dlg_ctx* c, dlg_knn_record* out) {
  if (!c || !out) return DLG_ERR_INVALID;
  *out = c->knn_rec;  // (host bookkeeping of normals_core's level loop: nothing to read back)
  return DLG_OK;
}

dlg_status dlg_set_profiling(dlg_ctx* c, int enable) {
  if (!c) return DLG_ERR_INVALID;
  if (enable < 0 || enable > 2) return DLG_ERR_INVALID;
  c->profiling = enable != 0;
  c->walk_events = enable == 1;
  return DLG_OK;
}

dlg_status dlg_synchronize(dlg_ctx* c) {
  if (!c) return DLG_ERR_INVALID;
  return guarded(c, [&] { HIPCHK(hipDeviceSynchronize()); });
}

dlg_status dlg_allreduce_max_f64(dlg_ctx* c, double* v) {
  if (!c || !v) return DLG_ERR_INVALID;
  if (c->comm->world() == 1) return DLG_OK;
  return guarded_group(c, [&] {
    c->scratch_f64.ensure(1);
    HIPCHK(hipMemcpyAsync(c->scratch_f64.p, v, 8, hipMemcpyHostToDevice, c->stream));
    c->comm->allreduce_max_f64(c->scratch_f64.p, 1, c->stream);
    HIPCHK(hipMemcpyAsync(v, c->scratch_f64.p, 8, hipMemcpyDeviceToHost, c->stream));
    sync(c);
  });
}

dlg_status dlg_shard_range(int64_t n_global, int rank, int world, int64_t* lo, int64_t* hi,
                           int* replicated) {
  if (n_global < 0 || world < 1 || rank < 0 || rank >= world || !lo || !hi) return DLG_ERR_INVALID;
  const bool repl = world > 1 && n_global / world < kPruneMinPoints;
  if (replicated) *replicated = repl ? 1 : 0;
  if (repl) {
    *lo = 0;
    *hi = n_global;
  } else {
    *lo = n_global * rank / world;
    *hi = n_global * (rank + 1) / world;
  }
  return DLG_OK;
}

dlg_status dlg_barrier(dlg_ctx* c) {
  double v = 0.0;
  return dlg_allreduce_max_f64(c, &v);
}

}  // extern "C"
