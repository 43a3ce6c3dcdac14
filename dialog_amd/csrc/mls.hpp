// mls.hpp -- device passes of the moving-least-squares filter (mls.hip), driven by mls_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "mls_model.hpp"
#include "normals.hpp"

namespace dlg {

// neighbours k_mls stages on the chip per query (12 KB of LDS per wave: three workgroups of four
// waves per CU, as many as the kernel's registers allow -- DESIGN.md 5g); a query with more reads
// them again from the grid
constexpr int kMlsCap = 1024;

// acc[] of a call (zeroed by the caller)
enum {
  kMlsFinite = 0,     // finite points of the cloud
  kMlsNTooFew = 1,    // list entries: finite, fewer than 3 neighbours
  kMlsNPlane = 2,     // rows without a fit
  kMlsNNonfinite = 3, // rows whose fit gave a non-finite c[0]
  kMlsMaxNb = 4,      // largest neighbour count of a finite entry
  kMlsNOverflow = 5,  // finite entries with more than kMlsCap neighbours
  kMlsAccWords = 8
};

// need[idx[e]] = 1 for every list entry (need preset to 0)
void launch_mls_need(const int32_t* idx, int n_list, uint8_t* need, hipStream_t s);

// The filter proper, one wave per query over the grid (G, B) of all n points, queries in sorted-cell
// order, skipped where need (nullable, by point) is 0 or the point is not finite.  Per query point
// i: cnt[i] = its neighbours; with 3 or more, res_p[i] = (x, y, z, branch code bits) and res_n[i] =
// (nx, ny, nz, curvature) (zeros when compute_normals is 0).
void launch_mls(const GridDesc& G, const GridBufs& B, int n, const uint8_t* need, float r2,
                int order, int polynomial_fit, int compute_normals, double sqr_gauss, float4* res_p,
                float4* res_n, int32_t* cnt, int num_cus, hipStream_t s);

// per list entry e = point p (idx null: e): nb[e] = cnt[p], or -1 where p is not finite;
// valid[e] = 1 where a row comes out; the branch counts into acc[]
void launch_mls_entries(const int32_t* idx, int n_list, const float* X, const float* Y,
                        const float* Z, const int32_t* cnt, const float4* res_p, int32_t* nb,
                        uint8_t* valid, unsigned long long* acc, hipStream_t s);
// row j < *count = list position sel[j]: xyz (records of stride_f floats, pad 1.0f), the normal
// row, the index value
void launch_mls_emit(const int32_t* sel, const uint32_t* count, int n_list, const int32_t* idx,
                     const float4* res_p, const float4* res_n, float* out_xyz, int64_t stride_f,
                     float4* out_nrm, int32_t* out_src, hipStream_t s);
// the same rows into a cloud's pristine list: x, y, z, gid = id_base + row
void launch_mls_emit_cloud(const int32_t* sel, const uint32_t* count, int n_list,
                           const int32_t* idx, const float4* res_p, const float4* res_n, float* X,
                           float* Y, float* Z, int32_t* gid, int32_t id_base, float4* out_nrm,
                           int32_t* out_src, hipStream_t s);

}  // namespace dlg
