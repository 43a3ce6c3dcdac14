// cloud_call.hpp -- the device-side front end shared by the calls that take a cloud and an index
// list (cloud_call.cpp): staging the list, counting flagged rows, the finite-point pipeline, the
// registration target and the tail of the calls that hand out a cloud.  The staging buffers are the
// context's NormalsWork (driver.hpp): one set, whoever ran last owns its contents.
#pragma once

#include <functional>

#include "driver.hpp"
#include "grid_host.hpp"

namespace dlg {

// (profiling) records the context's timing event i behind what is queued
inline void mark(dlg_ctx* c, int i) {
  if (c->profiling) HIPCHK(hipEventRecord(c->ev[i], c->stream));
}

// the records as they are -> nw.raw (enqueued)
const float* upload_raw(dlg_ctx* c, const dlg_points* pts);

// the m entries of a checked list -> nw.lst (enqueued); null when there is no list or it is empty
const int32_t* stage_list(dlg_ctx* c, const int32_t* indices, int m);

// out = the ascending positions of the non-zero flags[0..n); returns their number (one
// synchronisation; nw.sort_tmp is grown to select_tmp_bytes(n) when smaller)
int count_flagged(dlg_ctx* c, const uint8_t* flags, int n, int32_t* out);

// The finite-point pipeline, in two steps around the caller's own "too few" verdict.
// flag_points: de-interleaves the records that upload_raw left in nw.raw into nw.ax/ay/az (original
// order), has `flag` mark the rows to keep in nw.flags, compacts their positions into nw.fin_pos
// and returns their number (one synchronisation).  keep_flagged: those nf points -> nw.x/y/z, and
// their bounding box (one more).
using RowFlagger = std::function<void(const float* X, const float* Y, const float* Z, int n,
                                      uint8_t* flags)>;
int flag_points(dlg_ctx* c, const dlg_points* pts, const RowFlagger& flag);
BBox keep_flagged(dlg_ctx* c, int nf);

// The target of a registration: its rows flagged by `flag`, the kept points in nw.x/y/z and every
// level of their hierarchy built.  Fewer than `need` rows, or kept rows: DLG_ERR_INVALID, too_few.
struct Target {
  int nt = 0, nf = 0;    // rows; kept rows
  float tmax = 0.0f;     // the kept points' largest |coordinate|
  KnnLevels L{};
  double build_ms = 0.0;  // (profiling) host time of all this, synchronised
};
Target build_target(dlg_ctx* c, const dlg_points* tgt, const RowFlagger& flag, int need,
                    const char* too_few);

// The tail of every call that hands out a cloud.  A new cloud on c (ids from id_base) goes through
// fill(cl), which sizes its pristine list with cloud_rows once it knows the k rows, queues what
// writes them and returns k; then finish_upload, then `then(cl)` for what has to follow the
// upload's synchronisation.  All of it runs under guarded(): on failure the status comes back,
// *out stays null and the cloud is let go with c's device current.
SoA& cloud_rows(dlg_cloud& cl, int64_t k);
dlg_status make_cloud(dlg_ctx* c, int32_t id_base, dlg_cloud** out,
                      const std::function<int64_t(dlg_cloud&)>& fill,
                      const std::function<void(dlg_cloud&)>& then = nullptr);

}  // namespace dlg
