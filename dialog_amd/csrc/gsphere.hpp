// gsphere.hpp -- launch wrappers of the Gaussian-sphere plane seeds' kernels (gsphere.hip): the
// vote and its search of all cells, the filter's neighbour lists and ordered sums, the point
// labels, the labelled connected components, and the planes' order and compaction.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_model.hpp"
#include "normals.hpp"  // GridBufs

namespace dlg {

// the parameter space on the device (gsphere_model.hpp's Space)
struct GsSpaceDev {
  const int32_t* table;  // size^3
  const int32_t* coord;  // per PS cell: i << 20 | j << 10 | k
  const float* px;
  const float* py;
  const float* pz;
  int32_t cells;
  int size;
  float num_res;
};

// counters of one call (unsigned long long each)
enum { kGsQueued = 0, kGsKept = 1, kGsOccupied = 2, kGsPairs = 3, kGsCounters = 4 };

// voteForPS: cell_of_point[i] and votes[cell] (zeroed by the caller) from the normals' rows;
// points whose box bound fails are queued (queue: n entries; cnt[kGsQueued], zeroed) and
// launch_gs_vote_all searches all cells for them
void launch_gs_vote(const GsSpaceDev& S, const float4* nrm, int n, int32_t* cell_of_point,
                    int32_t* votes, int32_t* queue, unsigned long long* cnt, hipStream_t s);
void launch_gs_vote_all(const GsSpaceDev& S, const float4* nrm, const int32_t* queue,
                        const unsigned long long* cnt, int32_t* cell_of_point, int32_t* votes,
                        int num_cus, hipStream_t s);

// filtPS.  Pass 1 (keys == nullptr): every occupied cell adds 1 to reach[c] of each PS cell c
// within the radius (reach zeroed by the caller; cnt[kGsOccupied] counts the occupied cells,
// cnt[kGsPairs] the entries of all lists);
// pass 2: the same walk writes the key (d2, occupied cell) at keys[off[c] + cur[c]++] (cur zeroed).
// steps: gs::reach_steps(radius).
void launch_gs_reach(const GsSpaceDev& S, const int32_t* votes, int steps, float r2,
                     uint32_t* reach, const uint32_t* off, uint32_t* cur, uint64_t* keys,
                     unsigned long long* cnt, hipStream_t s);
size_t gs_scan_tmp_bytes(int32_t cells);
hipError_t launch_gs_scan(const uint32_t* reach, uint32_t* off, int32_t cells, void* tmp,
                          size_t tmp_bytes, hipStream_t s);
// one wave per PS cell: its keys sorted, the terms summed in that order; out[c] = the new vote
// (terms: one float per key, scratch)
void launch_gs_filter(const GsSpaceDev& S, const int32_t* votes, const uint32_t* reach,
                      const uint32_t* off, uint64_t* keys, float* terms, float std_dev,
                      int32_t* out, hipStream_t s);

// segmentPlanes.  label[i] = sink[cell_of_point[i]] for a point with finite coordinates, else -1;
// total[sink] (zeroed, one per PS cell) counts the labelled points
void launch_gs_label(const float* X, const float* Y, const float* Z, int n,
                     const int32_t* cell_of_point, const int32_t* sink, int32_t* label,
                     uint32_t* total, hipStream_t s);
// connected components of radius r over the grid's sorted positions, joining equal labels >= 0
// only; size[root] = the component's points (parent, size: n entries)
void launch_gs_cc(const GridDesc& G, const GridBufs& B, int n, float r2, const int32_t* label,
                  int32_t* lab_s, int32_t* parent, uint32_t* size, hipStream_t s);
// per point (original index): root_of[p]; key1[p] = sink rank << 32 | cell for a point of a kept
// component (its sink's total >= t_single and 2 size - 1 >= t_single), rank n_sinks otherwise;
// ids[p] = p; cnt[kGsKept] counts the kept points
void launch_gs_keys(const GridBufs& B, int n, const int32_t* lab_s, const int32_t* parent,
                    const uint32_t* size, const uint32_t* total, const int32_t* cell_of_point,
                    const int32_t* sink_rank, int32_t n_sinks, int64_t t_single, int32_t* root_of,
                    uint64_t* key1, int32_t* ids, unsigned long long* cnt, hipStream_t s);
size_t gs_sort_tmp_bytes(int n);
hipError_t launch_gs_sort_list(const uint64_t* key_in, uint64_t* key_out, const int32_t* ids_in,
                               int32_t* ids_out, int n, int end_bit, void* tmp, size_t tmp_bytes,
                               hipStream_t s);
// the kept points in list order (ids[0..nk)): first[root] (n entries, set to INT32_MAX here) = the
// component's first position; key2[pos] = first[root of ids[pos]]; then the stable sort by key2,
// the heads of the planes flagged and their positions compacted into offs (*n_planes of them)
hipError_t launch_gs_order(const int32_t* ids, int nk, int n, const int32_t* root_of,
                           int32_t* first, uint32_t* key2, uint32_t* key2_out, int32_t* ids_out,
                           uint8_t* heads, int32_t* offs, int32_t* n_planes, void* tmp,
                           size_t tmp_bytes, hipStream_t s);

}  // namespace dlg
