// voxel.hip -- pcl::VoxelGrid<PointXYZ> on the device (PCLViewer.cpp:245-253, 283-300, 313-332;
// the arithmetic: voxel_model.hpp): keys, a stable radix sort by key, the voxel runs of the sorted
// list, and the centroid of every kept voxel as three sequential float chains over its members in
// list order -- the order PCL's sums would take with a stable sort (its std::sort leaves the order
// inside a voxel unspecified: DESIGN.md §2).  No chain is reassociated: a voxel below the long-run
// cut-off is summed by one thread, a larger one by one wave that loads 64 members at a time and
// steps the chains through them from broadcast values.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <algorithm>
#include <cstdint>

#include "voxel.hpp"

namespace dlg {

namespace {

constexpr int kBS = 256;

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__global__ __launch_bounds__(kBS) void k_voxel_gather(const float* __restrict__ raw,
                                                      int64_t stride_f,
                                                      const int32_t* __restrict__ idx, int n,
                                                      float* __restrict__ X, float* __restrict__ Y,
                                                      float* __restrict__ Z,
                                                      float4* __restrict__ rec,
                                                      uint8_t* __restrict__ flags) {
  const int i = blockIdx.x * kBS + threadIdx.x;
  if (i >= n) return;
  const int64_t k = idx ? (int64_t)idx[i] : (int64_t)i;
  const float* p = raw + k * stride_f;
  const float x = p[0], y = p[1], z = p[2];
  X[i] = x;
  Y[i] = y;
  Z[i] = z;
  rec[i] = make_float4(x, y, z, 0.0f);  // (k_voxel_sorted's gather source: one 16-byte read)
  flags[i] = isfinite(x) && isfinite(y) && isfinite(z) ? 1 : 0;
}

__global__ __launch_bounds__(kBS) void k_voxel_keys(VoxelDesc g, const int32_t* __restrict__ pos,
                                                    int nf, const float* __restrict__ X,
                                                    const float* __restrict__ Y,
                                                    const float* __restrict__ Z,
                                                    uint32_t* __restrict__ keys,
                                                    int32_t* __restrict__ vals) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t >= nf) return;
  const int i = pos[t];
  keys[t] = voxel_key(g, X[i], Y[i], Z[i]);
  vals[t] = i;
}

// the coordinates in sorted order, contiguous, so that the sums read coalesced
__global__ __launch_bounds__(kBS) void k_voxel_sorted(const int32_t* __restrict__ spos, int nf,
                                                      const float4* __restrict__ rec,
                                                      float* __restrict__ sx, float* __restrict__ sy,
                                                      float* __restrict__ sz) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t >= nf) return;
  const float4 r = rec[spos[t]];
  sx[t] = r.x;
  sy[t] = r.y;
  sz[t] = r.z;
}

__global__ __launch_bounds__(kBS) void k_voxel_heads(const uint32_t* __restrict__ skeys, int nf,
                                                     int32_t* __restrict__ head) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t >= nf) return;
  head[t] = t == 0 || skeys[t] != skeys[t - 1] ? 1 : 0;
}

// vstart[v] = first sorted position of voxel v, vstart[n_voxels] = nf; cnt[kVoxN] = n_voxels
__global__ __launch_bounds__(kBS) void k_voxel_starts(const int32_t* __restrict__ head,
                                                      const int32_t* __restrict__ vid, int nf,
                                                      int32_t* __restrict__ vstart,
                                                      uint32_t* __restrict__ cnt) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t >= nf) return;
  const int32_t v = vid[t];  // 1-based
  if (head[t]) vstart[v - 1] = t;
  if (t == nf - 1) {
    vstart[v] = nf;
    cnt[kVoxN] = (uint32_t)v;
  }
}

// per voxel slot v < nf (slots past n_voxels are empty): kept by min_points, taken by the wave kernel
__global__ __launch_bounds__(kBS) void k_voxel_keep(const int32_t* __restrict__ vstart,
                                                    const uint32_t* __restrict__ cnt, int nf,
                                                    int min_points, int long_run,
                                                    int32_t* __restrict__ keep,
                                                    uint8_t* __restrict__ lflag) {
  const int v = blockIdx.x * kBS + threadIdx.x;
  if (v >= nf) return;
  int k = 0, l = 0;
  if ((uint32_t)v < cnt[kVoxN]) {
    const int c = vstart[v + 1] - vstart[v];
    k = c >= min_points ? 1 : 0;
    l = k && c >= long_run ? 1 : 0;
  }
  keep[v] = k;
  lflag[v] = (uint8_t)l;
}

__global__ void k_voxel_kept(const int32_t* __restrict__ keep, const int32_t* __restrict__ row,
                             int nf, uint32_t* __restrict__ cnt) {
  if (threadIdx.x == 0 && blockIdx.x == 0) cnt[kVoxKept] = (uint32_t)(row[nf - 1] + keep[nf - 1]);
}

__global__ __launch_bounds__(kBS) void k_voxel_scatter(const int32_t* __restrict__ vid,
                                                       const int32_t* __restrict__ keep,
                                                       const int32_t* __restrict__ row,
                                                       const int32_t* __restrict__ spos, int nf,
                                                       int32_t* __restrict__ voe) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t >= nf) return;
  const int v = vid[t] - 1;
  voe[spos[t]] = keep[v] ? row[v] : -1;
}

__device__ __forceinline__ void voxel_emit(const VoxelOut& O, int r, int c, float ax, float ay,
                                           float az) {
  const float d = (float)c;
  O.ox[r] = ax / d;
  O.oy[r] = ay / d;
  O.oz[r] = az / d;
  if (O.ocnt) O.ocnt[r] = c;
  if (O.ogid) O.ogid[r] = O.id_base + r;
}

// short runs: one thread per voxel, its members read in order
__global__ __launch_bounds__(kBS) void k_voxel_centroid_thread(
    const int32_t* __restrict__ vstart, const int32_t* __restrict__ keep,
    const int32_t* __restrict__ row, int n_voxels, int long_run, const float* __restrict__ sx,
    const float* __restrict__ sy, const float* __restrict__ sz, VoxelOut O) {
  const int v = blockIdx.x * kBS + threadIdx.x;
  if (v >= n_voxels || !keep[v]) return;
  const int b = vstart[v], e = vstart[v + 1];
  if (e - b >= long_run) return;  // the wave kernel's
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  for (int t = b; t < e; ++t) {
    ax += sx[t];
    ay += sy[t];
    az += sz[t];
  }
  voxel_emit(O, row[v], e - b, ax, ay, az);
}

__device__ __forceinline__ float lane_value(float v, int lane) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, v), lane));
}

struct Chunk {
  float x, y, z;
};

// lane l's member t0 + l of the run ending at e (clamped to the run's last member: the load is
// always in bounds and unconditional; a clamped lane's value is never stepped)
__device__ __forceinline__ Chunk chunk_load(const float* __restrict__ sx,
                                            const float* __restrict__ sy,
                                            const float* __restrict__ sz, int64_t t0, int lane,
                                            int64_t e) {
  const int64_t i = t0 + lane < e ? t0 + lane : e - 1;
  return Chunk{sx[i], sy[i], sz[i]};
}

// the three chains stepped through the chunk's first m members, in order
__device__ __forceinline__ void chunk_step(const Chunk& c, int64_t m, float& ax, float& ay,
                                           float& az) {
  if (m >= 64) {
#pragma unroll
    for (int j = 0; j < 64; ++j) {
      const float vx = lane_value(c.x, j), vy = lane_value(c.y, j), vz = lane_value(c.z, j);
      ax += vx;
      ay += vy;
      az += vz;
    }
  } else {  // (only the members: -0.0f + 0.0f would change a sign)
    for (int j = 0; j < (int)m; ++j) {
      const float vx = lane_value(c.x, j), vy = lane_value(c.y, j), vz = lane_value(c.z, j);
      ax += vx;
      ay += vy;
      az += vz;
    }
  }
}

// long runs: one wave per voxel.  The 64 lanes hold 64 consecutive members; every lane steps the
// same three chains through them from the broadcast values (lane j's value at step j), while the
// next 64 members are already being loaded into the other register set.  Time is proportional to
// the voxel's size on one wave.
__global__ __launch_bounds__(kBS) void k_voxel_centroid_wave(
    const int32_t* __restrict__ long_list, int n_long, const int32_t* __restrict__ vstart,
    const int32_t* __restrict__ row, const float* __restrict__ sx, const float* __restrict__ sy,
    const float* __restrict__ sz, VoxelOut O) {
  const int lane = threadIdx.x & 63;
  const int w = blockIdx.x * (kBS / 64) + (threadIdx.x >> 6);
  if (w >= n_long) return;  // (the whole wave)
  const int v = __builtin_amdgcn_readfirstlane(long_list[w]);
  const int64_t b = __builtin_amdgcn_readfirstlane(vstart[v]);
  const int64_t e = __builtin_amdgcn_readfirstlane(vstart[v + 1]);
  float ax = 0.0f, ay = 0.0f, az = 0.0f;
  Chunk A = chunk_load(sx, sy, sz, b, lane, e);
  for (int64_t t = b; t < e; t += 128) {
    const Chunk B = chunk_load(sx, sy, sz, t + 64, lane, e);
    chunk_step(A, e - t, ax, ay, az);
    if (t + 64 >= e) break;
    A = chunk_load(sx, sy, sz, t + 128, lane, e);
    chunk_step(B, e - t - 64, ax, ay, az);
  }
  if (lane == 0) voxel_emit(O, row[v], (int)(e - b), ax, ay, az);
}

__global__ __launch_bounds__(kBS) void k_voxel_pack(const float* __restrict__ ox,
                                                    const float* __restrict__ oy,
                                                    const float* __restrict__ oz, int n,
                                                    float* __restrict__ out, int64_t stride_f) {
  const int i = blockIdx.x * kBS + threadIdx.x;
  if (i >= n) return;
  float* p = out + (int64_t)i * stride_f;
  p[0] = ox[i];
  p[1] = oy[i];
  p[2] = oz[i];
  if (stride_f >= 4) p[3] = 1.0f;  // pcl::PointXYZ's data[3]
}

}  // namespace

void launch_voxel_gather(const float* raw, int64_t stride_f, const int32_t* idx, int n, float* X,
                         float* Y, float* Z, float4* rec, uint8_t* flags, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_voxel_gather, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, raw, stride_f, idx, n, X,
                     Y, Z, rec, flags);
}

void launch_voxel_sorted(const int32_t* spos, int nf, const float4* rec, float* sx, float* sy,
                         float* sz, hipStream_t s) {
  if (nf <= 0) return;
  hipLaunchKernelGGL(k_voxel_sorted, dim3(cdiv(nf, kBS)), dim3(kBS), 0, s, spos, nf, rec, sx, sy,
                     sz);
}

void launch_voxel_keys(const VoxelDesc& g, const int32_t* pos, int nf, const float* X,
                       const float* Y, const float* Z, uint32_t* keys, int32_t* vals,
                       hipStream_t s) {
  if (nf <= 0) return;
  hipLaunchKernelGGL(k_voxel_keys, dim3(cdiv(nf, kBS)), dim3(kBS), 0, s, g, pos, nf, X, Y, Z, keys,
                     vals);
}

size_t voxel_tmp_bytes(int n) {
  size_t a = 0, b = 0, c = 0, d = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                           (const int32_t*)nullptr, (int32_t*)nullptr, n, 0, 32);
  (void)hipcub::DeviceScan::InclusiveSum(nullptr, b, (const int32_t*)nullptr, (int32_t*)nullptr, n);
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, c, (const int32_t*)nullptr, (int32_t*)nullptr, n);
  (void)hipcub::DeviceSelect::Flagged(nullptr, d, hipcub::CountingInputIterator<int32_t>(0),
                                      (const uint8_t*)nullptr, (int32_t*)nullptr,
                                      (uint32_t*)nullptr, (int64_t)n);
  return std::max(std::max(a, b), std::max(c, d));
}

hipError_t voxel_sort(void* tmp, size_t tmp_bytes, const uint32_t* keys_in, uint32_t* keys_out,
                      const int32_t* vals_in, int32_t* vals_out, int nf, int end_bit,
                      hipStream_t s) {
  size_t t = tmp_bytes;
  return hipcub::DeviceRadixSort::SortPairs(tmp, t, keys_in, keys_out, vals_in, vals_out, nf, 0,
                                            end_bit, s);
}

hipError_t voxel_runs(const uint32_t* skeys, int nf, int min_points, int long_run,
                      const VoxelRuns& R, hipStream_t s) {
  if (nf <= 0) return hipErrorInvalidValue;
  const dim3 g(cdiv(nf, kBS)), b(kBS);
  hipLaunchKernelGGL(k_voxel_heads, g, b, 0, s, skeys, nf, R.head);
  size_t t = R.tmp_bytes;
  hipError_t e = hipcub::DeviceScan::InclusiveSum(R.tmp, t, (const int32_t*)R.head, R.vid, nf, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_voxel_starts, g, b, 0, s, (const int32_t*)R.head, (const int32_t*)R.vid, nf,
                     R.vstart, R.cnt);
  hipLaunchKernelGGL(k_voxel_keep, g, b, 0, s, (const int32_t*)R.vstart, (const uint32_t*)R.cnt,
                     nf, min_points, long_run, R.keep, R.lflag);
  t = R.tmp_bytes;
  e = hipcub::DeviceScan::ExclusiveSum(R.tmp, t, (const int32_t*)R.keep, R.row, nf, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_voxel_kept, dim3(1), dim3(64), 0, s, (const int32_t*)R.keep,
                     (const int32_t*)R.row, nf, R.cnt);
  t = R.tmp_bytes;
  e = hipcub::DeviceSelect::Flagged(R.tmp, t, hipcub::CountingInputIterator<int32_t>(0),
                                    (const uint8_t*)R.lflag, R.long_list, R.cnt + kVoxLong,
                                    (int64_t)nf, s);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

void launch_voxel_scatter(const VoxelRuns& R, const int32_t* spos, int nf, int32_t* voxel_of_entry,
                          hipStream_t s) {
  if (nf <= 0) return;
  hipLaunchKernelGGL(k_voxel_scatter, dim3(cdiv(nf, kBS)), dim3(kBS), 0, s, (const int32_t*)R.vid,
                     (const int32_t*)R.keep, (const int32_t*)R.row, spos, nf, voxel_of_entry);
}

void launch_voxel_centroids(const VoxelRuns& R, int n_voxels, int n_long, int long_run,
                            const float* sx, const float* sy, const float* sz, const VoxelOut& O,
                            hipStream_t s) {
  if (n_voxels > n_long)  // (with every kept voxel a long one the thread kernel would find nothing)
    hipLaunchKernelGGL(k_voxel_centroid_thread, dim3(cdiv(n_voxels, kBS)), dim3(kBS), 0, s,
                       (const int32_t*)R.vstart, (const int32_t*)R.keep, (const int32_t*)R.row,
                       n_voxels, long_run, sx, sy, sz, O);
  if (n_long > 0)
    hipLaunchKernelGGL(k_voxel_centroid_wave, dim3(cdiv(n_long, kBS / 64)), dim3(kBS), 0, s,
                       (const int32_t*)R.long_list, n_long, (const int32_t*)R.vstart,
                       (const int32_t*)R.row, sx, sy, sz, O);
}

void launch_voxel_pack(const float* ox, const float* oy, const float* oz, int n, float* out,
                       int64_t stride_f, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_voxel_pack, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, ox, oy, oz, n, out,
                     stride_f);
}

}  // namespace dlg
