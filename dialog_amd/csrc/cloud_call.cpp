// cloud_call.cpp -- the device-side front end of the calls that take a cloud and an index list
// (cloud_call.hpp).
#include "cloud_call.hpp"

#include <chrono>
#include <cmath>
#include <memory>

namespace dlg {

const int32_t* stage_list(dlg_ctx* c, const int32_t* indices, int m) {
  if (!indices || m <= 0) return nullptr;
  DevBuf<int32_t>& lst = c->nw.lst;
  lst.ensure(m);
  HIPCHK(hipMemcpyAsync(lst.p, indices, 4 * (size_t)m, hipMemcpyHostToDevice, c->stream));
  return lst.p;
}

int count_flagged(dlg_ctx* c, const uint8_t* flags, int n, int32_t* out) {
  NormalsWork& w = c->nw;
  w.sort_tmp.ensure(select_tmp_bytes(n));
  w.counters.ensure(8);
  w.h_cnt.ensure(8);
  HIPCHK(select_flagged(w.sort_tmp.p, w.sort_tmp.cap, flags, n, out, w.counters.p, c->stream));
  HIPCHK(hipMemcpyAsync(w.h_cnt.p, w.counters.p, 4, hipMemcpyDeviceToHost, c->stream));
  sync(c);
  return (int)w.h_cnt.p[0];
}

const float* upload_raw(dlg_ctx* c, const dlg_points* pts) {
  DevBuf<uint8_t>& raw = c->nw.raw;
  const size_t bytes = (size_t)pts->n * (size_t)pts->stride_bytes;
  raw.ensure(bytes);
  if (bytes) HIPCHK(hipMemcpyAsync(raw.p, pts->xyz, bytes, hipMemcpyHostToDevice, c->stream));
  return reinterpret_cast<const float*>(raw.p);
}

int flag_points(dlg_ctx* c, const dlg_points* pts, const RowFlagger& flag) {
  NormalsWork& w = c->nw;
  const int n = (int)pts->n;
  w.ax.ensure(n); w.ay.ensure(n); w.az.ensure(n);
  w.flags.ensure(n); w.fin_pos.ensure(n);
  launch_deinterleave(reinterpret_cast<const float*>(w.raw.p), n, pts->stride_bytes / 4, w.ax.p,
                      w.ay.p, w.az.p, c->stream);
  flag(w.ax.p, w.ay.p, w.az.p, n, w.flags.p);
  return count_flagged(c, w.flags.p, n, w.fin_pos.p);
}

BBox keep_flagged(dlg_ctx* c, int nf) {
  NormalsWork& w = c->nw;
  w.x.ensure(nf); w.y.ensure(nf); w.z.ensure(nf);
  launch_gather3(w.fin_pos.p, nf, w.ax.p, w.ay.p, w.az.p, w.x.p, w.y.p, w.z.p, c->stream);
  return bbox_of(c, w.x.p, w.y.p, w.z.p, nf);
}

Target build_target(dlg_ctx* c, const dlg_points* tgt, const RowFlagger& flag, int need,
                    const char* too_few) {
  Target T;
  T.nt = (int)tgt->n;
  if (T.nt < need) throw DlgError(DLG_ERR_INVALID, too_few);
  const auto t0 = std::chrono::steady_clock::now();
  upload_raw(c, tgt);
  T.nf = flag_points(c, tgt, flag);
  if (T.nf < need) throw DlgError(DLG_ERR_INVALID, too_few);
  const BBox b = keep_flagged(c, T.nf);
  for (int k = 0; k < 3; ++k)
    T.tmax = std::fmax(T.tmax, std::fmax(std::fabs(b.lo[k]), std::fabs(b.hi[k])));
  T.L = build_hierarchy(c, T.nf, b, 1);
  HIPCHK(hipGetLastError());
  if (c->profiling) {
    sync(c);
    T.build_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0)
                     .count();
  }
  return T;
}

SoA& cloud_rows(dlg_cloud& cl, int64_t k) {
  cl.n_total = cl.n_points = cl.n_active = k;
  cl.gid_ident = true;
  cl.pristine.ensure((size_t)std::max<int64_t>(k, 1));
  return cl.pristine;
}

dlg_status make_cloud(dlg_ctx* c, int32_t id_base, dlg_cloud** out,
                      const std::function<int64_t(dlg_cloud&)>& fill,
                      const std::function<void(dlg_cloud&)>& then) {
  *out = nullptr;
  auto cl = std::make_unique<dlg_cloud>();
  const dlg_status s = guarded(c, [&] {
    cl->ctx = c;
    cl->id_base = id_base;
    const int64_t k = fill(*cl);
    finish_upload(c, cl.get(), k);  // (synchronises)
    if (then) then(*cl);
  });
  if (s != DLG_OK) {
    (void)hipSetDevice(c->device);  // (the cloud's buffers are freed as cl goes)
    return s;
  }
  *out = cl.release();
  return DLG_OK;
}

}  // namespace dlg
