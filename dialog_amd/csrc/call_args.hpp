// call_args.hpp -- the argument checks shared by the calls that take a cloud and an index list
// (voxel grid, outlier removal, moving least squares, FPFH, registration, SAC-IA, the upload and
// the normals path).  Pure host code over include/dialog_ransac.h: no HIP, so it compiles with
// plain g++ (tests/cpp/call_args_san.cpp).  Every check throws DlgError(DLG_ERR_INVALID, text).
#pragma once

#include <cmath>
#include <cstdint>
#include <stdexcept>
#include <string>

#include "../../include/dialog_ransac.h"

namespace dlg {

struct DlgError : std::runtime_error {
  DlgError(dlg_status c, const std::string& m) : std::runtime_error(m), code(c) {}
  dlg_status code;
};

constexpr int64_t kMaxPoints = INT32_MAX;             // these calls index points with an int
constexpr int64_t kMaxGridPoints = INT32_MAX / 2;     // the normals path (2^30 grid keys)

// a dlg_points record ("points", "source", "target"): present, sized, strided, at most max_n
// points.  xyz is not read.
inline void check_points(const dlg_points* p, const char* what = "points",
                         int64_t max_n = kMaxPoints) {
  if (!p || p->n < 0 || (p->n > 0 && !p->xyz))
    throw DlgError(DLG_ERR_INVALID, std::string(what) + ": null or negative size");
  if (p->stride_bytes < 12 || p->stride_bytes % 4)
    throw DlgError(DLG_ERR_INVALID, "stride_bytes must be >= 12 and a multiple of 4");
  if (p->n > max_n)
    throw DlgError(DLG_ERR_INVALID,
                   std::string(what) + ": more than " + std::to_string(max_n) + " points");
}

// an index list over n points (null: all of them, n_indices ignored) -> the entries m of the call
inline int check_list(const int32_t* indices, int64_t n_indices, int64_t n) {
  if (!indices) return (int)n;
  if (n_indices < 0) throw DlgError(DLG_ERR_INVALID, "negative n_indices");
  if (n_indices > kMaxPoints) throw DlgError(DLG_ERR_INVALID, "more than 2^31-1 indices");
  for (int64_t i = 0; i < n_indices; ++i)
    if (indices[i] < 0 || indices[i] >= n) throw DlgError(DLG_ERR_INVALID, "index out of range");
  return (int)n_indices;
}

inline void check_out_stride(int64_t out_stride_bytes) {
  if (out_stride_bytes != 12 && out_stride_bytes != 16)
    throw DlgError(DLG_ERR_INVALID, "out_stride_bytes must be 12 or 16");
}

// a row-major 4x4 guess (null: the identity) -> xf, which must be finite
inline void check_guess(const float* guess, float xf[16]) {
  for (int k = 0; k < 16; ++k) xf[k] = guess ? guess[k] : ((k % 5 == 0) ? 1.0f : 0.0f);
  for (int k = 0; k < 16; ++k)
    if (!std::isfinite(xf[k])) throw DlgError(DLG_ERR_INVALID, "the guess is not finite");
}

// the calls whose neighbourhoods cross a shard's cut refuse one rank's part of a cloud
inline void check_whole_cloud(int world, const char* call) {
  if (world > 1)
    throw DlgError(DLG_ERR_INVALID, std::string(call) + ": the points are one rank's shard "
                                    "(world > 1); the neighbours across its cut need the whole "
                                    "cloud");
}

}  // namespace dlg
