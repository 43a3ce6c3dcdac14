// icp.hpp -- device passes of the rigid registration (icp.hip), driven by icp_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "icp_model.hpp"
#include "normals.hpp"

namespace dlg {

struct IcpXf {
  float m[16];  // row-major 4x4
};

// The device state of one correspondence pass (zero between passes: k_icp_publish clears it).
struct IcpState {
  unsigned long long dig[kIcpDigits];  // the exact moments' digits (icp_model.hpp), two's complement
  uint32_t wmax;                       // bits of W's largest finite |coordinate|
  uint32_t d2max;                      // bits of the largest kept d2
  uint32_t qn[kMaxLevels + 1];         // queries deferred to each level
};

// Every launcher below takes max_blocks (DLG_OPT_ICP_MAX_BLOCKS): n >= 1 runs min(the default, n)
// workgroups, 0 the default shape; the kernels stride over their entries either way.

// W[i] = the source record idx[i] (idx null: i) of the strided upload, through xf when apply != 0
void launch_icp_gather(const float* raw, int64_t stride_f, const int32_t* idx, int m, const IcpXf& xf,
                       int apply, float* wx, float* wy, float* wz, int max_blocks, hipStream_t s);
// W <- xf W
void launch_icp_apply(const IcpXf& xf, float* wx, float* wy, float* wz, int m, int max_blocks,
                      hipStream_t s);

// One level of the correspondence search over the hierarchy L of the finite target points, one
// thread per query.  Level 0 visits every W entry (reversed != 0: from the last to the first), first
// moving it through xf when apply != 0 (written back), and records W's |coordinate| maximum; level
// l > 0 visits the st->qn[l] entries of qin.  A query whose nearest neighbour lies inside the
// level's guaranteed radius (the top level: always) is settled: nn[i] = fin_pos[neighbour] and
// d2[i], or nn[i] = -1, d2[i] = 0 when (double)d2 > md2, and also when nothing lies inside a
// guaranteed radius already beyond md2; a non-finite entry gets -1.  Any other query is appended to
// qout (count st->qn[l + 1]).  The launch is sized for every entry and leaves early on the count.
void launch_icp_level(const KnnLevels& L, int level, const IcpXf& xf, int apply, int reversed,
                      float* wx, float* wy, float* wz, int m, const int32_t* qin, int32_t* qout,
                      IcpState* st, const int32_t* fin_pos, double md2, int32_t* nn, float* d2,
                      int num_cus, int max_blocks, hipStream_t s);

// the exact moments of the settled pass: every entry with nn >= 0 adds q(W), q(target[nn]) and
// trunc(d2 2^(48 - e2)) to st->dig, e from max(tmax, st->wmax), e2 from st->d2max
void launch_icp_finish(const float* wx, const float* wy, const float* wz, int m, const int32_t* nn,
                       const float* d2, const float* tx, const float* ty, const float* tz, float tmax,
                       IcpState* st, int num_cus, int max_blocks, hipStream_t s);
// *pub (coherent pinned) = *st, then *st = 0
void launch_icp_publish(IcpState* st, IcpState* pub, hipStream_t s);

// out records of stride_f floats (3, or 4 with pad 1.0f) from W
void launch_icp_pack(const float* wx, const float* wy, const float* wz, int m, float* out,
                     int stride_f, int max_blocks, hipStream_t s);

}  // namespace dlg
