// sacia.hip -- device passes of the SAC-IA initial alignment (dlg_sac_ia_align, dlg_sac_ia_score,
// dlg_fpfh_knn; sacia_host.cpp drives them, sacia_model.hpp holds the arithmetic).
//
// Descriptor search: lanes as queries.  A wave holds 64 queries' 33 values in registers and scans a
// slab of the table; every row is a wave-uniform load, its distance 99 separately rounded VALU
// operations per lane (an FMA chain, and so the f32 MFMA, gives other bits).  Each lane keeps its
// sorted nearest rows in registers; the last one is the cheap reject, an insert is a statically
// unrolled compare-exchange chain.  k_sacia_knn_merge joins the slabs' lists in (d, index) order.
//
// Scorer: k_sacia_score0 and k_sacia_score_level (sacia.hpp).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>

#include "dev_common.hpp"
#include "grid_dev.hpp"
#include "sacia.hpp"

namespace dlg {
namespace {

using namespace grid;

constexpr int kBS = 256;
inline int cdiv_i(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ bool fin3(float x, float y, float z) {
  return sacia_finite(x) && sacia_finite(y) && sacia_finite(z);
}

__global__ __launch_bounds__(kBS) void k_sacia_row_flags(
    const float* __restrict__ rows, int64_t stride, const float* __restrict__ px,
    const float* __restrict__ py, const float* __restrict__ pz, int n, uint8_t* __restrict__ flags,
    uint32_t* __restrict__ n_valid) {
  uint32_t mine = 0;
  for (int r = blockIdx.x * kBS + threadIdx.x; r < n; r += gridDim.x * kBS) {
    bool ok = true;
    if (px) ok = fin3(px[r], py[r], pz[r]);
    if (rows && ok) ok = sacia_row_finite(rows + (int64_t)r * stride);
    flags[r] = ok ? 1 : 0;
    mine += ok ? 1u : 0u;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) mine += __shfl_xor(mine, o, 64);
  if (n_valid != nullptr && (threadIdx.x & 63) == 0 && mine != 0u) atomicAdd(n_valid, mine);
}

// (d, i) before (e, j) in the search's order
__device__ __forceinline__ bool before(float d, int i, float e, int j) {
  return d < e || (d == e && i < j);
}

template <int KC>
__global__ __launch_bounds__(64) void k_sacia_knn(
    const float* __restrict__ queries, int nq, const float* __restrict__ rows, int64_t stride,
    int n_rows, const uint8_t* __restrict__ flags, int k, float* __restrict__ part_d,
    int32_t* __restrict__ part_i) {
  const int qi = blockIdx.x * 64 + (int)threadIdx.x;
  const int slab = blockIdx.y, n_slabs = gridDim.y;
  const bool active = qi < nq;
  float a[kSaciaDim];
  bool qok = active;
  {
    const float* q = queries + (int64_t)(active ? qi : nq - 1) * kSaciaDim;
#pragma unroll
    for (int j = 0; j < kSaciaDim; ++j) {
      a[j] = q[j];
      qok = qok && sacia_finite(a[j]);
    }
  }
  float ld[KC];
  int li[KC];
#pragma unroll
  for (int s = 0; s < KC; ++s) {
    ld[s] = INFINITY;
    li[s] = INT_MAX;
  }
  const int r0 = slab * kSaciaSlab, r1 = min(n_rows, r0 + kSaciaSlab);
  for (int r = r0; r < r1; ++r) {
    if (!flags[r]) continue;  // (wave-uniform)
    const float* __restrict__ row = rows + (int64_t)r * stride;
    float d = 0.0f;
#pragma unroll
    for (int j = 0; j < kSaciaDim; ++j) {
      const float e = a[j] - row[j];
      d += e * e;
    }
    if (qok && before(d, r, ld[KC - 1], li[KC - 1])) {
      float cd = d;
      int ci = r;
#pragma unroll
      for (int s = 0; s < KC; ++s) {
        const bool sw = before(cd, ci, ld[s], li[s]);
        const float td = sw ? ld[s] : cd;
        const int ti = sw ? li[s] : ci;
        ld[s] = sw ? cd : ld[s];
        li[s] = sw ? ci : li[s];
        cd = td;
        ci = ti;
      }
    }
  }
  if (!active) return;
  const int64_t o = ((int64_t)qi * n_slabs + slab) * k;
#pragma unroll
  for (int s = 0; s < KC; ++s)
    if (s < k) {
      part_d[o + s] = ld[s];
      part_i[o + s] = li[s];
    }
}

// one thread per query: k times the smallest (d, index) after the last one written, over the
// slabs' lists (rows are distinct, so the pairs are)
__global__ __launch_bounds__(64) void k_sacia_knn_merge(const float* __restrict__ part_d,
                                                        const int32_t* __restrict__ part_i, int nq,
                                                        int n_slabs, int k, float* __restrict__ d_out,
                                                        int32_t* __restrict__ i_out) {
  const int qi = blockIdx.x * 64 + (int)threadIdx.x;
  if (qi >= nq) return;
  const int64_t o = (int64_t)qi * n_slabs * k;
  const int cnt = n_slabs * k;
  float last_d = -1.0f;
  int last_i = -1;
  for (int t = 0; t < k; ++t) {
    float bd = INFINITY;
    int bi = INT_MAX;
    for (int u = 0; u < cnt; ++u) {
      const float d = part_d[o + u];
      const int i = part_i[o + u];
      if (i == INT_MAX) continue;
      if (before(last_d, last_i, d, i) && before(d, i, bd, bi)) {
        bd = d;
        bi = i;
      }
    }
    const bool got = bi != INT_MAX;
    d_out[(int64_t)qi * k + t] = got ? bd : 0.0f;
    i_out[(int64_t)qi * k + t] = got ? bi : -1;
    last_d = got ? bd : INFINITY;
    last_i = got ? bi : INT_MAX;
  }
}

// the nearest target point's squared distance at level l inside lim (false: nothing inside)
__device__ __forceinline__ bool nearest_at(const KnnLevels& L, int l, float lim, float qx, float qy,
                                           float qz, float& best) {
  const GridDesc& G = L.G[l];
  const float* __restrict__ sx = L.sx[l];
  const float* __restrict__ sy = L.sy[l];
  const float* __restrict__ sz = L.sz[l];
  const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
  const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
  const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
  float bd = INFINITY;
  bool found = false;
  for (int z = max(cz - 1, 0); z <= min(cz + 1, G.g[2] - 1); ++z)
    for (int y = max(cy - 1, 0); y <= min(cy + 1, G.g[1] - 1); ++y)
      for (int x = max(cx - 1, 0); x <= min(cx + 1, G.g[0] - 1); ++x) {
        const int2 rg = cell_range(L.tkeys[l], L.trange[l], L.tmask[l], cell_key(G, x, y, z));
        for (int u = rg.x; u < rg.y; ++u) {
          const float d2 = icp_d2(qx, qy, qz, sx[u], sy[u], sz[u]);
          if (!(d2 < lim) || d2 > bd) continue;
          bd = d2;
          found = true;
        }
      }
  best = bd;
  return found;
}

// the wave's deferred pairs appended to qout (count *qn)
__device__ __forceinline__ void append_deferred(bool defer, unsigned long long entry,
                                                unsigned long long* __restrict__ qout,
                                                uint32_t* qn) {
  const uint64_t mask = __ballot(defer);
  if (mask == 0) return;
  const int lane = threadIdx.x & 63;
  const int leader = __ffsll((unsigned long long)mask) - 1;
  uint32_t at = 0;
  if (lane == leader) at = atomicAdd(qn, (uint32_t)__popcll(mask));
  at = __shfl(at, leader, 64);
  const int below =
      __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
  if (defer) qout[at + below] = entry;
}

// The wave's settled terms into acc.  When every settled lane scores the same hypothesis (always at
// level 0; at the coarser levels wherever a wave's stretch of the queue came from one hypothesis)
// the quantised terms and the counts are reduced over the wave and added with one atomic per word;
// a wave of mixed hypotheses adds lane by lane.  Either way the sums are the same integers.
__device__ __forceinline__ void add_terms(bool settled, int h, float term,
                                          SaciaAcc* __restrict__ acc) {
  const uint64_t mask = __ballot(settled);
  if (mask == 0) return;
  const int h0 = __shfl(h, __ffsll((unsigned long long)mask) - 1, 64);
  unsigned long long q = settled ? (unsigned long long)sacia_quantise(term) : 0ull;
  unsigned long long cn = settled ? ((1ull << 32) | (term == 1.0f ? 1ull : 0ull)) : 0ull;
  if (__ballot(settled && h != h0) == 0) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      q += __shfl_xor(q, o, 64);
      cn += __shfl_xor(cn, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
      if (q != 0ull) {
        atomicAdd(&acc[h0].lo, q & 0xFFFFFFull);
        atomicAdd(&acc[h0].hi, q >> 24);
      }
      atomicAdd(&acc[h0].cnt, cn);
    }
  } else if (settled) {
    if (q != 0ull) {
      atomicAdd(&acc[h].lo, q & 0xFFFFFFull);
      atomicAdd(&acc[h].hi, q >> 24);
    }
    atomicAdd(&acc[h].cnt, cn);
  }
}

__global__ __launch_bounds__(kBS) void k_sacia_score0(
    KnnLevels L, const float* __restrict__ sx, const float* __restrict__ sy,
    const float* __restrict__ sz, int n, const IcpXf* __restrict__ xfs, int nb, int per_y, float thr,
    float tmax, unsigned long long* __restrict__ qout, SaciaState* __restrict__ st,
    SaciaAcc* __restrict__ acc) {
  const bool top = L.levels == 1;
  const float cell = L.G[0].cell;
  const float lim = top ? INFINITY : cell * cell;
  const bool beyond = !top && lim > thr;
  const bool no_search = thr == INFINITY;
  const int h0 = blockIdx.y * per_y, h1 = min(nb, h0 + per_y);
  // (whole workgroups step together: the reduction and the append are wave operations)
  for (int base = blockIdx.x * kBS; base < n; base += gridDim.x * kBS) {
    const int i = base + (int)threadIdx.x;
    const bool active = i < n;
    float px = 0.0f, py = 0.0f, pz = 0.0f;
    if (active) {
      px = sx[i]; py = sy[i]; pz = sz[i];
    }
    const bool pok = active && fin3(px, py, pz);
    for (int h = h0; h < h1; ++h) {
      float qx, qy, qz;
      icp_xf(xfs[h].m, px, py, pz, qx, qy, qz);
      const bool ok = pok && fin3(qx, qy, qz);
      bool settled = false, defer = false;
      float term = 0.0f;
      if (ok) {
        // thr = +inf: e / thr is 0 unless e overflows; it cannot when every difference is < 2^63
        if (no_search && fmaxf(fabsf(qx), fmaxf(fabsf(qy), fabsf(qz))) + tmax < 0x1p62f) {
          settled = true;
        } else {
          float bd;
          const bool found = nearest_at(L, 0, lim, qx, qy, qz, bd);
          if (found) {
            term = sacia_term(bd, thr);
            settled = true;
          } else if (top || beyond) {
            term = 1.0f;
            settled = true;
          } else {
            defer = true;
          }
        }
      }
      add_terms(settled, h, term, acc);
      append_deferred(defer, ((unsigned long long)(uint32_t)h << 32) | (uint32_t)i, qout,
                      &st->qn[1]);
    }
  }
}

__global__ __launch_bounds__(kBS) void k_sacia_score_level(
    KnnLevels L, int l, const float* __restrict__ sx, const float* __restrict__ sy,
    const float* __restrict__ sz, const IcpXf* __restrict__ xfs, float thr,
    const unsigned long long* __restrict__ qin, unsigned long long* __restrict__ qout, uint32_t cap,
    SaciaState* __restrict__ st, SaciaAcc* __restrict__ acc) {
  const uint32_t cnt = min(st->qn[l], cap);
  const bool top = l == L.levels - 1;
  const float cell = L.G[l].cell;
  const float lim = top ? INFINITY : cell * cell;
  const bool beyond = !top && lim > thr;
  if (cnt != 0u && blockIdx.x == 0 && threadIdx.x == 0) atomicMax(&st->levels, (uint32_t)l + 1u);
  for (uint32_t base = blockIdx.x * kBS; base < cnt; base += gridDim.x * kBS) {
    const uint32_t t = base + threadIdx.x;
    const bool active = t < cnt;
    const unsigned long long entry = active ? qin[t] : 0ull;
    const int h = (int)(entry >> 32), i = (int)(uint32_t)entry;
    bool settled = false, defer = false;
    float term = 0.0f;
    if (active) {
      float qx, qy, qz, bd;
      icp_xf(xfs[h].m, sx[i], sy[i], sz[i], qx, qy, qz);
      const bool found = nearest_at(L, l, lim, qx, qy, qz, bd);
      if (found) {
        term = sacia_term(bd, thr);
        settled = true;
      } else if (top || beyond) {
        term = 1.0f;
        settled = true;
      } else {
        defer = true;
      }
    }
    add_terms(settled, h, term, acc);
    append_deferred(defer, entry, qout, &st->qn[l + 1]);
  }
}

inline int capped(int grid, int max_blocks) {
  return max_blocks >= 1 ? std::min(grid, max_blocks) : grid;
}

}  // namespace

void launch_sacia_row_flags(const float* rows, int64_t row_stride_f, const float* px,
                            const float* py, const float* pz, int n, uint8_t* flags,
                            uint32_t* n_valid, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_sacia_row_flags, dim3(std::min(cdiv_i(n, kBS), 4096)), dim3(kBS), 0, s, rows,
                     row_stride_f, px, py, pz, n, flags, n_valid);
}

void launch_sacia_knn(const float* queries, int nq, const float* rows, int64_t row_stride_f,
                      int n_rows, const uint8_t* flags, int k, float* part_d, int32_t* part_i,
                      float* d_out, int32_t* i_out, hipStream_t s) {
  if (nq <= 0 || n_rows <= 0) return;
  const int n_slabs = sacia_slabs(n_rows);
  const dim3 grid(cdiv_i(nq, 64), n_slabs);
  if (k <= 4)
    hipLaunchKernelGGL(k_sacia_knn<4>, grid, dim3(64), 0, s, queries, nq, rows, row_stride_f, n_rows,
                       flags, k, part_d, part_i);
  else if (k <= 16)
    hipLaunchKernelGGL(k_sacia_knn<16>, grid, dim3(64), 0, s, queries, nq, rows, row_stride_f, n_rows,
                       flags, k, part_d, part_i);
  else
    hipLaunchKernelGGL(k_sacia_knn<kSaciaMaxK>, grid, dim3(64), 0, s, queries, nq, rows, row_stride_f,
                       n_rows, flags, k, part_d, part_i);
  hipLaunchKernelGGL(k_sacia_knn_merge, dim3(cdiv_i(nq, 64)), dim3(64), 0, s, part_d, part_i, nq,
                     n_slabs, k, d_out, i_out);
}

void launch_sacia_score0(const KnnLevels& L, const float* sx, const float* sy, const float* sz, int n,
                         const IcpXf* xfs, int nb, float thr, float tmax, unsigned long long* qout,
                         SaciaState* st, SaciaAcc* acc, int num_cus, int max_blocks, hipStream_t s) {
  if (n <= 0 || nb <= 0) return;
  const int want = std::max(num_cus, 1) * 8;
  const int gx = capped(std::max(1, std::min(cdiv_i(n, kBS), want)), max_blocks);
  // few source tiles: the batch's hypotheses are spread over blockIdx.y instead
  const int gy = max_blocks >= 1 ? 1 : std::max(1, std::min(nb, want / gx));
  const int per_y = cdiv_i(nb, gy);
  hipLaunchKernelGGL(k_sacia_score0, dim3(gx, cdiv_i(nb, per_y)), dim3(kBS), 0, s, L, sx, sy, sz, n,
                     xfs, nb, per_y, thr, tmax, qout, st, acc);
}

void launch_sacia_score_level(const KnnLevels& L, int l, const float* sx, const float* sy,
                              const float* sz, const IcpXf* xfs, float thr,
                              const unsigned long long* qin, unsigned long long* qout, uint32_t cap,
                              SaciaState* st, SaciaAcc* acc, int num_cus, int max_blocks,
                              hipStream_t s) {
  if (cap == 0u) return;
  const int grid =
      capped(std::max(1, std::min(cdiv_i(cap, kBS), std::max(num_cus, 1) * 8)), max_blocks);
  hipLaunchKernelGGL(k_sacia_score_level, dim3(grid), dim3(kBS), 0, s, L, l, sx, sy, sz, xfs, thr, qin,
                     qout, cap, st, acc);
}

}  // namespace dlg
