// sor.hip -- pcl::StatisticalOutlierRemoval<PointXYZ> on the device (PCLViewer.cpp:334-358; the
// arithmetic: sor_model.hpp).  k_sor_knn is the search: one wave per query over the grid hierarchy
// of the normals path, the K = mean_k + 1 smallest squared distances kept as bit patterns in
// R = ceil(K / 64) registers per lane (position r * 64 + lane holds the (r * 64 + lane)-th
// smallest).  Only the multiset of the distances enters the result, so no index is carried.
#include <hip/hip_runtime.h>

#include <cstdint>

#include "grid_dev.hpp"
#include "sor.hpp"

namespace dlg {

namespace {

using namespace grid;

constexpr int kBS = 256;
constexpr int kSorB = 4;  // k_sor_knn: candidate batches of 64 in flight

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__device__ __forceinline__ uint32_t umin(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax(uint32_t a, uint32_t b) { return a < b ? b : a; }
__device__ __forceinline__ uint32_t rlane(uint32_t v, int j) {
  return (uint32_t)__builtin_amdgcn_readlane((int)v, j);
}

// a bitonic sequence over the wave's lanes -> ascending
__device__ __forceinline__ uint32_t wave_merge64(uint32_t v, int lane) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint32_t p = (uint32_t)__shfl_xor((int)v, s, 64);
    v = (lane & s) ? umax(v, p) : umin(v, p);
  }
  return v;
}

// any 64 keys -> ascending by lane
__device__ __forceinline__ uint32_t wave_sort64(uint32_t v, int lane) {
#pragma unroll
  for (int k = 2; k <= 64; k <<= 1) {
#pragma unroll
    for (int s = k >> 1; s >= 1; s >>= 1) {
      const uint32_t p = (uint32_t)__shfl_xor((int)v, s, 64);
      const bool up = (lane & k) == 0;         // (k = 64: every lane)
      const bool low = ((lane & s) == 0) == up;  // this lane keeps the smaller of the pair
      v = low ? umin(v, p) : umax(v, p);
    }
  }
  return v;
}

// One batch of 64 candidate keys (~0: none) into the wave's ascending best keys under the bound
// kth (the K-th best so far; keys equal to it change nothing).  The admitted keys are sorted, then
// merged register by register: min / max against the reversed batch splits the 128 keys into the
// 64 smallest and the 64 largest, both bitonic; the smallest stay in the register, the largest
// carry on to the next one, which holds nothing smaller than the register before it.
template <int R>
__device__ __forceinline__ void sor_admit(uint32_t key, int K, int lane, uint32_t (&best)[R],
                                          uint32_t& kth) {
  const bool adm = key < kth;
  if (!__ballot(adm)) return;
  uint32_t b = wave_sort64(adm ? key : 0xffffffffu, lane);
#pragma unroll
  for (int r = 0; r < R; ++r) {
    if (rlane(b, 0) >= rlane(best[r], 63)) continue;  // (uniform: nothing of b enters register r)
    const uint32_t brev = (uint32_t)__shfl((int)b, 63 - lane, 64);
    const uint32_t lo = umin(best[r], brev), hi = umax(best[r], brev);
    best[r] = wave_merge64(lo, lane);
    b = wave_merge64(hi, lane);
  }
  const int kr = (K - 1) >> 6, kl = (K - 1) & 63;
#pragma unroll
  for (int r = 0; r < R; ++r)
    if (r == kr) kth = rlane(best[r], kl);
}

template <typename T>
__device__ __forceinline__ T wave_sum(T v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
  return v;
}

template <int R>
__global__ __launch_bounds__(kBS) void k_sor_knn(KnnLevels L, int l, const int32_t* __restrict__ qpos,
                                                 int nq, const uint8_t* __restrict__ need, int K,
                                                 int force_literal, float* __restrict__ dist_pt,
                                                 uint8_t* __restrict__ dflags, int64_t dstride,
                                                 int tnext,
                                                 unsigned long long* __restrict__ n_literal) {
  const int lane = threadIdx.x & 63;
  const int wq = __builtin_amdgcn_readfirstlane((int)((blockIdx.x * kBS + threadIdx.x) >> 6));
  if (wq >= nq) return;
  const int uq = qpos ? qpos[wq] : wq;
  const int qi = L.idx[l][uq];
  if (need && !need[qi]) return;
  const float qx = L.sx[l][uq], qy = L.sy[l][uq], qz = L.sz[l][uq];
  const GridDesc& G = L.G[l];
  const bool top = l == L.levels - 1;
  const float lim = top ? INFINITY : G.cell * G.cell;
  const float* __restrict__ sx = L.sx[l];
  const float* __restrict__ sy = L.sy[l];
  const float* __restrict__ sz = L.sz[l];
  uint32_t best[R];
#pragma unroll
  for (int r = 0; r < R; ++r) best[r] = 0xffffffffu;
  uint32_t kth = 0xffffffffu;  // (uniform) the K-th smallest so far: the admission bound
  int cnt = 0;                 // (uniform) candidates inside the level's guaranteed radius
  // the 27 cells in k_normals_knn's order with its bounds (normals.hip)
  const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
  const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
  const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
  const float w = knn_width(G.inv_cell);
  const float fx = knn_frac(qx, G.lo[0], G.inv_cell, cx);
  const float fy = knn_frac(qy, G.lo[1], G.inv_cell, cy);
  const float fz = knn_frac(qz, G.lo[2], G.inv_cell, cz);
  auto side = [&](float f, int d) { return knn_side(f, d, w, G.slack); };
  const float bx0 = side(fx, -1), bx1 = side(fx, 1), by0 = side(fy, -1), by1 = side(fy, 1);
  const float bz0 = side(fz, -1), bz1 = side(fz, 1);
  constexpr uint64_t kOrd[3] = {0x904416665151515ull, 0x1a9864a9261058ull, 0x2a2a20a8220ull};
#pragma unroll 1
  for (int c3 = 0; c3 < 27; ++c3) {
    const uint32_t code = (uint32_t)(kOrd[c3 / 10] >> (6 * (c3 % 10))) & 63u;
    const int dx = (int)(code & 3u) - 1, dy = (int)((code >> 2) & 3u) - 1,
              dz = (int)((code >> 4) & 3u) - 1;
    const int x = cx + dx, y = cy + dy, z = cz + dz;
    if (x < 0 || x >= G.g[0] || y < 0 || y >= G.g[1] || z < 0 || z >= G.g[2]) continue;
    const float ex = dx < 0 ? bx0 : dx > 0 ? bx1 : 0.0f;
    const float ey = dy < 0 ? by0 : dy > 0 ? by1 : 0.0f;
    const float ez = dz < 0 ? bz0 : dz > 0 ? bz1 : 0.0f;
    const float md = knn_bound(ex, ey, ez);
    if (md >= lim || (kth != 0xffffffffu && md > __uint_as_float(kth))) continue;
    const int2 rg = cell_range(L.tkeys[l], L.trange[l], L.tmask[l], cell_key(G, x, y, z));
    const int a = __builtin_amdgcn_readfirstlane(rg.x), b = __builtin_amdgcn_readfirstlane(rg.y);
#pragma unroll 1
    for (int u0 = a; u0 < b; u0 += 64 * kSorB) {
      float px[kSorB], py[kSorB], pz[kSorB];
#pragma unroll
      for (int j = 0; j < kSorB; ++j) {
        const int u = u0 + 64 * j + lane;
        const bool valid = u < b;
        px[j] = valid ? sx[u] : 0.0f;
        py[j] = valid ? sy[u] : 0.0f;
        pz[j] = valid ? sz[u] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < kSorB; ++j) {
        if (u0 + 64 * j >= b) break;  // (uniform)
        const float d2 = flann_d2(qx, qy, qz, px[j], py[j], pz[j]);
        // (the top level takes every point, a distance that overflowed to +inf too)
        const bool in = u0 + 64 * j + lane < b && (top || d2 < lim);
        cnt += (int)__popcll(__ballot(in));
        sor_admit<R>(in ? __float_as_uint(d2) : 0xffffffffu, K, lane, best, kth);
      }
    }
  }
  if (cnt < K && !top) {
    if (lane == 0) dflags[(int64_t)tnext * dstride + qi] = 1;
    return;
  }
  // the mean_k terms: positions 1..K-1 (position 0 is the query itself or a duplicate)
  float t[R];
  bool fin = true;
  int q = kSorNoExp;
#pragma unroll
  for (int r = 0; r < R; ++r) {
    const int pos = r * 64 + lane;
    const bool on = pos >= 1 && pos < K;
    // the IEEE float square root: (float)sqrt((double)x) rounds to the same value
    t[r] = on ? (float)sqrt((double)__uint_as_float(best[r])) : 0.0f;
    fin = fin && sor_finite(t[r]);
    const int e = fin ? sor_low_exp(t[r]) : kSorNoExp;
    q = e < q ? e : q;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int o = __shfl_xor(q, s, 64);
    q = o < q ? o : q;
  }
  bool ok = !force_literal && __ballot(!fin) == 0;
  if (ok) {
    unsigned long long units = 0;
    bool fits = true;
#pragma unroll
    for (int r = 0; r < R; ++r) {
      uint64_t u = 0;
      fits = sor_units(t[r], q, &u) && fits;
      units += u;
    }
    ok = __ballot(!fits) == 0;
    if (ok) ok = (wave_sum(units) >> 53) == 0;  // (<= 256 terms below 2^53: no overflow)
  }
  double sum = 0.0;
  if (ok) {
    // certified: no partial sum rounds, in any order
#pragma unroll
    for (int r = 0; r < R; ++r) sum += (double)t[r];
    sum = wave_sum(sum);
  } else {
    // the literal chain, uniform in every lane
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int jn = K - r * 64 < 64 ? K - r * 64 : 64;
#pragma unroll 1
      for (int j = r == 0 ? 1 : 0; j < jn; ++j)
        sum = sor_chain(sum, __uint_as_float(rlane(__float_as_uint(t[r]), j)));
    }
  }
  if (lane == 0) {
    dist_pt[qi] = sor_distance(sum, K - 1);
    if (!ok) atomicAdd(n_literal, 1ull);
  }
}

__global__ __launch_bounds__(kBS) void k_sor_rank(const int32_t* __restrict__ fin_pos, int nf,
                                                  int32_t* __restrict__ rank) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t < nf) rank[fin_pos[t]] = t;
}

__global__ __launch_bounds__(kBS) void k_sor_need(const int32_t* __restrict__ idx, int n_list,
                                                  const int32_t* __restrict__ rank,
                                                  uint8_t* __restrict__ need) {
  const int e = blockIdx.x * kBS + threadIdx.x;
  if (e >= n_list) return;
  const int r = rank[idx[e]];
  if (r >= 0) need[r] = 1;
}

__global__ __launch_bounds__(kBS) void k_sor_entries(const int32_t* __restrict__ idx, int n_list,
                                                     const int32_t* __restrict__ rank,
                                                     const float* __restrict__ dist_pt,
                                                     float* __restrict__ dist) {
  const int e = blockIdx.x * kBS + threadIdx.x;
  if (e >= n_list) return;
  const int r = rank[idx ? idx[e] : e];
  dist[e] = r >= 0 ? dist_pt[r] : 0.0f;
}

// pass 1: the valid entries, the two units, the non-finite terms
__global__ __launch_bounds__(kBS) void k_sor_stats_units(const int32_t* __restrict__ idx, int n_list,
                                                         const int32_t* __restrict__ rank,
                                                         const float* __restrict__ dist,
                                                         unsigned long long* __restrict__ acc) {
  unsigned long long valid = 0;
  int qd = kSorNoExp, qs = kSorNoExp;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * kBS + threadIdx.x; e < n_list;
       e += (int64_t)gridDim.x * kBS) {
    valid += rank[idx ? idx[e] : e] >= 0 ? 1u : 0u;
    const float d = dist[e], sq = sor_square(d);
    if (!sor_finite(d) || !sor_finite(sq)) { bad = true; continue; }
    const int ed = sor_low_exp(d), es = sor_low_exp(sq);
    qd = ed < qd ? ed : qd;
    qs = es < qs ? es : qs;
  }
  valid = wave_sum(valid);
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const int od = __shfl_xor(qd, s, 64), os = __shfl_xor(qs, s, 64);
    qd = od < qd ? od : qd;
    qs = os < qs ? os : qs;
  }
  const bool any_bad = __ballot(bad) != 0;
  if ((threadIdx.x & 63) == 0) {
    if (valid) atomicAdd(acc + kSorValid, valid);
    atomicMin(acc + kSorQd, (unsigned long long)(qd + kSorQBias));
    atomicMin(acc + kSorQs, (unsigned long long)(qs + kSorQBias));
    if (any_bad) atomicOr(acc + kSorFail, 1ull);
  }
}

// pass 2: the exact integer sums in those units, as hi / lo halves (2^31 terms below 2^53 overflow
// neither)
__global__ __launch_bounds__(kBS) void k_sor_stats_sums(int n_list, const float* __restrict__ dist,
                                                        unsigned long long* __restrict__ acc) {
  if (acc[kSorFail]) return;
  const int qd = (int)acc[kSorQd] - kSorQBias, qs = (int)acc[kSorQs] - kSorQBias;
  unsigned long long dlo = 0, dhi = 0, slo = 0, shi = 0;
  bool bad = false;
  for (int64_t e = (int64_t)blockIdx.x * kBS + threadIdx.x; e < n_list;
       e += (int64_t)gridDim.x * kBS) {
    const float d = dist[e];
    uint64_t ud = 0, us = 0;
    if (!sor_units(d, qd, &ud) || !sor_units(sor_square(d), qs, &us)) { bad = true; continue; }
    dlo += ud & 0xffffffffu;
    dhi += ud >> 32;
    slo += us & 0xffffffffu;
    shi += us >> 32;
  }
  dlo = wave_sum(dlo);
  dhi = wave_sum(dhi);
  slo = wave_sum(slo);
  shi = wave_sum(shi);
  const bool any_bad = __ballot(bad) != 0;
  if ((threadIdx.x & 63) == 0) {
    atomicAdd(acc + kSorDLo, dlo);
    atomicAdd(acc + kSorDHi, dhi);
    atomicAdd(acc + kSorSLo, slo);
    atomicAdd(acc + kSorSHi, shi);
    if (any_bad) atomicOr(acc + kSorFail, 2ull);
  }
}

__global__ __launch_bounds__(kBS) void k_sor_acc_init(unsigned long long* __restrict__ acc) {
  const int i = threadIdx.x;
  if (i < kSorAccWords && i != kSorLiteral)
    acc[i] = (i == kSorQd || i == kSorQs) ? (unsigned long long)(kSorNoExp + kSorQBias) : 0ull;
}

__global__ __launch_bounds__(kBS) void k_sor_classify(const float* __restrict__ dist, int n_list,
                                                      double threshold, int negative,
                                                      uint8_t* __restrict__ keep,
                                                      uint8_t* __restrict__ rem) {
  const int e = blockIdx.x * kBS + threadIdx.x;
  if (e >= n_list) return;
  const bool r = sor_removed(dist[e], threshold, negative != 0);
  keep[e] = r ? 0 : 1;
  rem[e] = r ? 1 : 0;
}

__global__ __launch_bounds__(kBS) void k_sor_emit(const int32_t* __restrict__ sel,
                                                  const uint32_t* __restrict__ count, int n_list,
                                                  const int32_t* __restrict__ idx,
                                                  int32_t* __restrict__ out) {
  const int j = blockIdx.x * kBS + threadIdx.x;
  if (j >= n_list || (uint32_t)j >= *count) return;
  const int e = sel[j];
  out[j] = idx ? idx[e] : e;
}

__global__ __launch_bounds__(kBS) void k_sor_ids(int32_t* __restrict__ gid, int n,
                                                 int32_t id_base) {
  const int j = blockIdx.x * kBS + threadIdx.x;
  if (j < n) gid[j] = id_base + j;
}

int stats_blocks(int n) {
  const unsigned b = cdiv(n, kBS * 8);
  return (int)(b < 1u ? 1u : b > 2048u ? 2048u : b);
}

}  // namespace

void launch_sor_rank(const int32_t* fin_pos, int nf, int32_t* rank, hipStream_t s) {
  if (nf <= 0) return;
  hipLaunchKernelGGL(k_sor_rank, dim3(cdiv(nf, kBS)), dim3(kBS), 0, s, fin_pos, nf, rank);
}

void launch_sor_need(const int32_t* idx, int n_list, const int32_t* rank, uint8_t* need,
                     hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_sor_need, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, idx, n_list, rank, need);
}

void launch_sor_knn(const KnnLevels& L, int level, const int32_t* qpos, int nq, const uint8_t* need,
                    int mean_k, int force_literal, float* dist_pt, uint8_t* defer,
                    int64_t defer_stride, int tnext, unsigned long long* n_literal, hipStream_t s) {
  if (nq <= 0) return;
  const int K = mean_k + 1;
  const dim3 grid(cdiv((int64_t)nq * 64, kBS)), block(kBS);
  auto go = [&](auto kern) {
    hipLaunchKernelGGL(kern, grid, block, 0, s, L, level, qpos, nq, need, K, force_literal, dist_pt,
                       defer, defer_stride, tnext, n_literal);
  };
  if (K <= 64) go(k_sor_knn<1>);
  else if (K <= 128) go(k_sor_knn<2>);
  else if (K <= 192) go(k_sor_knn<3>);
  else go(k_sor_knn<4>);
}

void launch_sor_entries(const int32_t* idx, int n_list, const int32_t* rank, const float* dist_pt,
                        float* dist, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_sor_entries, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, idx, n_list, rank,
                     dist_pt, dist);
}

void launch_sor_stats(const int32_t* idx, int n_list, const int32_t* rank, const float* dist,
                      unsigned long long* acc, hipStream_t s) {
  hipLaunchKernelGGL(k_sor_acc_init, dim3(1), dim3(kBS), 0, s, acc);
  if (n_list <= 0) return;
  const int nb = stats_blocks(n_list);
  hipLaunchKernelGGL(k_sor_stats_units, dim3(nb), dim3(kBS), 0, s, idx, n_list, rank, dist, acc);
  hipLaunchKernelGGL(k_sor_stats_sums, dim3(nb), dim3(kBS), 0, s, n_list, dist, acc);
}

void launch_sor_classify(const float* dist, int n_list, double threshold, int negative,
                         uint8_t* keep, uint8_t* rem, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_sor_classify, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, dist, n_list,
                     threshold, negative, keep, rem);
}

void launch_sor_emit(const int32_t* sel, const uint32_t* count, int n_list, const int32_t* idx,
                     int32_t* out, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_sor_emit, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, sel, count, n_list, idx,
                     out);
}

void launch_sor_ids(int32_t* gid, int n, int32_t id_base, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sor_ids, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, gid, n, id_base);
}

}  // namespace dlg
