// voxel.hpp -- device passes of the voxel-grid filter (voxel.hip), driven by voxel_host.cpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "voxel_model.hpp"

namespace dlg {

// list entry i = record idx[i] (idx null: i) of the raw strided records -> X, Y, Z in list order,
// the same as (x, y, z, 0) records (the sorted gather's source) and flags[i] = 1 when x, y and z
// are all finite
void launch_voxel_gather(const float* raw, int64_t stride_f, const int32_t* idx, int n, float* X,
                         float* Y, float* Z, float4* rec, uint8_t* flags, hipStream_t s);
// (sx, sy, sz)[t] = the coordinates of list entry spos[t]
void launch_voxel_sorted(const int32_t* spos, int nf, const float4* rec, float* sx, float* sy,
                         float* sz, hipStream_t s);
// finite entry t (list position pos[t]) -> keys[t] = voxel_key, vals[t] = pos[t]
void launch_voxel_keys(const VoxelDesc& g, const int32_t* pos, int nf, const float* X,
                       const float* Y, const float* Z, uint32_t* keys, int32_t* vals,
                       hipStream_t s);

// device-side counts of a call (cnt[]): occupied voxels, voxels kept, voxels of the wave kernel
enum { kVoxN = 0, kVoxKept = 1, kVoxLong = 2, kVoxCounts = 4 };

// the sorted run structure.  Scratch (nf entries each unless noted): head, vid (inclusive scan of
// head: entry t lies in voxel vid[t] - 1), vstart (nf + 1: first sorted position of each voxel,
// then nf), keep / row (per voxel: kept by min_points, its output row), lflag / long_list (the
// kept voxels of >= long_run points).
struct VoxelRuns {
  int32_t* head;
  int32_t* vid;
  int32_t* vstart;
  int32_t* keep;
  int32_t* row;
  uint8_t* lflag;
  int32_t* long_list;
  uint32_t* cnt;  // kVoxCounts words
  void* tmp;      // hipcub temporaries
  size_t tmp_bytes;
};
size_t voxel_tmp_bytes(int n);
// stable radix sort of the (key, position) pairs over key bits [0, end_bit)
hipError_t voxel_sort(void* tmp, size_t tmp_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int nf, int end_bit,
                      hipStream_t s);
// sorted keys -> runs, the min_points filter, output rows, the long-voxel list and cnt[]
hipError_t voxel_runs(const uint32_t* skeys, int nf, int min_points, int long_run,
                      const VoxelRuns& R, hipStream_t s);
// voxel_of_entry[spos[t]] = output row of sorted entry t's voxel, -1 when it was dropped
void launch_voxel_scatter(const VoxelRuns& R, const int32_t* spos, int nf, int32_t* voxel_of_entry,
                          hipStream_t s);

// centroids of the kept voxels: three sequential float chains per voxel over its members in sorted
// order (sx, sy, sz), divided by float(count).  Row r of (ox, oy, oz); ocnt[r] = count and
// ogid[r] = id_base + r where non-null.  Voxels below long_run points: one thread each; the
// n_long others (R.long_list): one wave each.
struct VoxelOut {
  float* ox;
  float* oy;
  float* oz;
  int32_t* ocnt;
  int32_t* ogid;
  int32_t id_base;
};
void launch_voxel_centroids(const VoxelRuns& R, int n_voxels, int n_long, int long_run,
                            const float* sx, const float* sy, const float* sz, const VoxelOut& O,
                            hipStream_t s);
// SoA rows -> records of stride_f floats (3: xyz, 4: xyz and the pad 1.0f)
void launch_voxel_pack(const float* ox, const float* oy, const float* oz, int n, float* out,
                       int64_t stride_f, hipStream_t s);

}  // namespace dlg
