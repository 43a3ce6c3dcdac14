// fpfh.hpp -- device passes of the FPFH descriptors (fpfh.hip), driven by fpfh_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "fpfh_model.hpp"
#include "normals.hpp"

namespace dlg {

// (d2, index) keys k_fpfh_weight stages and sorts on the chip per entry (8 KB of LDS per wave); an
// entry with more neighbours takes them in several sorted windows, each a scan of the grid
constexpr int kFpfhCap = 1024;

// acc[] of a call (zeroed by the caller)
enum {
  kFpfhFinite = 0,       // finite points of the cloud
  kFpfhNanRows = 1,      // list entries with a non-finite coordinate
  kFpfhZeroRows = 2,     // finite entries with no neighbour but themselves
  kFpfhMaxNb = 3,        // largest neighbour count of a finite entry
  kFpfhNOverflow = 4,    // finite entries with more than kFpfhCap neighbours
  kFpfhPairs = 5,        // pairs that added to the finite entries' own SPFHs
  kFpfhPairsFailed = 6,  // the other neighbours of those entries (themselves excluded)
  kFpfhLiteral = 7,      // entries whose double sums took the literal loop
  kFpfhAccWords = 8
};

// snrm[t] = nrm[idx_out[t]]: the normals in the grid's sorted order
void launch_fpfh_sort_normals(const GridBufs& B, int n, const float4* nrm, float4* snrm,
                              hipStream_t s);

// SPFH pass, one wave per finite point over the grid (G, B) of all n points.  Per point i:
// cnt[i] = its neighbours (itself included), spfh[33 i + b] = the bin values, pairs[i] = the pairs
// that added to them, counts[33 i + b] (nullable) = the integer bin counts.  Rows of non-finite
// points are left as they are.
void launch_fpfh_spfh(const GridDesc& G, const GridBufs& B, int n, float r2, const float4* snrm,
                      float* spfh, int32_t* counts, int32_t* cnt, int32_t* pairs, int num_cus,
                      hipStream_t s);

// Weighting pass, one wave per list entry e = point idx[e] (idx null: e): hist[33 e + b], nb[e] =
// the neighbour count (-1: non-finite entry), the call's counts into acc[].
void launch_fpfh_weight(const GridDesc& G, const GridBufs& B, int n, float r2, const int32_t* idx,
                        int n_list, const float* X, const float* Y, const float* Z,
                        const float* spfh, const int32_t* pairs, float* hist, int32_t* nb,
                        unsigned long long* acc, int num_cus, hipStream_t s);

}  // namespace dlg
