// icp.hip -- device passes of the rigid registration (dlg_icp_align, dlg_icp_correspondences;
// icp_host.cpp drives them, icp_model.hpp holds the arithmetic).
//
// One correspondence pass = k_icp_level at level 0 over every W entry (the pending transformation
// applied as the entry is loaded), k_icp_level at each coarser level over the queries the level
// below deferred (device-side counts: no read-back in between), k_icp_finish (the exact moments of
// the settled pairs, once W's and the kept d2's maxima are known) and k_icp_publish.
#include <hip/hip_runtime.h>

#include <climits>

#include "dev_common.hpp"
#include "grid_dev.hpp"
#include "icp.hpp"

namespace dlg {
namespace {

using namespace grid;

constexpr int kBS = 256;
inline int cdiv_i(int64_t a, int64_t b) { return (int)((a + b - 1) / b); }

__device__ __forceinline__ bool icp_finite3(float x, float y, float z) {
  return icp_finite(x) && icp_finite(y) && icp_finite(z);
}

// max of non-negative floats over the wave, then into *dst (their bits order as unsigned)
__device__ __forceinline__ void wave_max_bits(float v, uint32_t* dst) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o, 64));
  if ((threadIdx.x & 63) == 0 && v > 0.0f) atomicMax(dst, __float_as_uint(v));
}

__global__ __launch_bounds__(kBS) void k_icp_gather(const float* __restrict__ raw, int64_t stride,
                                                    const int32_t* __restrict__ idx, int m, IcpXf xf,
                                                    int apply, float* __restrict__ wx,
                                                    float* __restrict__ wy, float* __restrict__ wz) {
  for (int i = blockIdx.x * kBS + threadIdx.x; i < m; i += gridDim.x * kBS) {
    const float* p = raw + (int64_t)(idx ? idx[i] : i) * stride;
    float x = p[0], y = p[1], z = p[2];
    if (apply) icp_xf(xf.m, x, y, z, x, y, z);
    wx[i] = x;
    wy[i] = y;
    wz[i] = z;
  }
}

__global__ __launch_bounds__(kBS) void k_icp_apply(IcpXf xf, float* __restrict__ wx,
                                                   float* __restrict__ wy, float* __restrict__ wz,
                                                   int m) {
  for (int i = blockIdx.x * kBS + threadIdx.x; i < m; i += gridDim.x * kBS) {
    float x, y, z;
    icp_xf(xf.m, wx[i], wy[i], wz[i], x, y, z);
    wx[i] = x;
    wy[i] = y;
    wz[i] = z;
  }
}

template <bool FIRST>
__global__ __launch_bounds__(kBS) void k_icp_level(
    KnnLevels L, int l, IcpXf xf, int apply, int reversed, float* __restrict__ wx,
    float* __restrict__ wy, float* __restrict__ wz, int m, const int32_t* __restrict__ qin,
    int32_t* __restrict__ qout, IcpState* __restrict__ st, const int32_t* __restrict__ fin_pos,
    double md2, int32_t* __restrict__ nn, float* __restrict__ d2o) {
  const int cnt = FIRST ? m : (int)min(st->qn[l], (uint32_t)m);
  const GridDesc& G = L.G[l];
  const bool top = l == L.levels - 1;
  const float lim = top ? INFINITY : G.cell * G.cell;
  const bool beyond = !top && (double)lim > md2;  // nothing inside lim: every pair is dropped
  const float* __restrict__ sx = L.sx[l];
  const float* __restrict__ sy = L.sy[l];
  const float* __restrict__ sz = L.sz[l];
  const int32_t* __restrict__ sidx = L.idx[l];
  float wmax = 0.0f, dmax = 0.0f;
  // (whole workgroups step together: the append below is a wave operation)
  for (int base = blockIdx.x * kBS; base < cnt; base += gridDim.x * kBS) {
    const int t = base + (int)threadIdx.x;
    const bool active = t < cnt;
    const int i = active ? (FIRST ? (reversed ? m - 1 - t : t) : qin[t]) : 0;
    float qx = 0.0f, qy = 0.0f, qz = 0.0f;
    if (active) {
      qx = wx[i]; qy = wy[i]; qz = wz[i];
      if (FIRST && apply) {
        icp_xf(xf.m, qx, qy, qz, qx, qy, qz);
        wx[i] = qx; wy[i] = qy; wz[i] = qz;
      }
    }
    const bool ok = active && icp_finite3(qx, qy, qz);
    if (FIRST && ok) wmax = fmaxf(wmax, fmaxf(fabsf(qx), fmaxf(fabsf(qy), fabsf(qz))));
    float bd = INFINITY;
    int bi = INT_MAX;
    if (ok) {
      const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
      const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
      const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
      for (int z = max(cz - 1, 0); z <= min(cz + 1, G.g[2] - 1); ++z)
        for (int y = max(cy - 1, 0); y <= min(cy + 1, G.g[1] - 1); ++y)
          for (int x = max(cx - 1, 0); x <= min(cx + 1, G.g[0] - 1); ++x) {
            const int2 rg = cell_range(L.tkeys[l], L.trange[l], L.tmask[l], cell_key(G, x, y, z));
            for (int u = rg.x; u < rg.y; ++u) {
              const float d2 = icp_d2(qx, qy, qz, sx[u], sy[u], sz[u]);
              if (!(d2 < lim) || d2 > bd) continue;
              const int iu = sidx[u];
              if (d2 < bd || iu < bi) { bd = d2; bi = iu; }
            }
          }
    }
    const bool found = bi != INT_MAX;
    const bool defer = ok && !found && !top && !beyond;
    if (active && !defer) {
      const bool keep = found && !((double)bd > md2);
      nn[i] = keep ? fin_pos[bi] : -1;
      d2o[i] = keep ? bd : 0.0f;
      if (keep) dmax = fmaxf(dmax, bd);
    }
    // deferred queries, appended wave by wave
    const uint64_t mask = __ballot(defer);
    if (mask != 0) {
      const int lane = threadIdx.x & 63;
      const int leader = __ffsll((unsigned long long)mask) - 1;
      uint32_t at = 0;
      if (lane == leader) at = atomicAdd(&st->qn[l + 1], (uint32_t)__popcll(mask));
      at = __shfl(at, leader, 64);
      const int below = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32),
                                                  __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
      if (defer) qout[at + below] = i;
    }
  }
  if (blockIdx.x * kBS >= cnt) return;  // (uniform per workgroup: it visited nothing)
  if (FIRST) wave_max_bits(wmax, &st->wmax);
  wave_max_bits(dmax, &st->d2max);
}

__global__ __launch_bounds__(kBS) void k_icp_finish(
    const float* __restrict__ wx, const float* __restrict__ wy, const float* __restrict__ wz, int m,
    const int32_t* __restrict__ nn, const float* __restrict__ d2, const float* __restrict__ tx,
    const float* __restrict__ ty, const float* __restrict__ tz, float tmax,
    IcpState* __restrict__ st) {
  __shared__ unsigned long long sdig[kIcpDigits];
  for (int k = threadIdx.x; k < kIcpDigits; k += kBS) sdig[k] = 0ull;
  __syncthreads();
  const float wmax = __uint_as_float(st->wmax);
  const int e = icp_qexp(fmaxf(tmax, wmax));
  const int e2 = icp_qexp(__uint_as_float(st->d2max));
  const double sc = pow2d(kFastBits - e), sc2 = pow2d(kFastBits - e2);
  IcpAcc acc;
  icp_acc_zero(acc);
  int64_t inc[kIcpDigits];
#pragma unroll
  for (int k = 0; k < kIcpDigits; ++k) inc[k] = 0;
  // (the launch gives a thread kIcpFlush entries at most unless the cloud is huge: the flush
  // inside the loop is rarely taken)
  for (int i = blockIdx.x * kBS + threadIdx.x; i < m; i += gridDim.x * kBS) {
    const int j = nn[i];
    if (j < 0) continue;
    const double qw[3] = {icp_q(wx[i], sc), icp_q(wy[i], sc), icp_q(wz[i], sc)};
    const double qt[3] = {icp_q(tx[j], sc), icp_q(ty[j], sc), icp_q(tz[j], sc)};
    icp_acc_point(acc, qw, qt, icp_q(d2[i], sc2));
    if (acc.n == (double)kIcpFlush) icp_acc_flush(inc, acc);
  }
  icp_acc_flush(inc, acc);
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int k = 0; k < kIcpDigits; ++k) {
    unsigned long long v = (unsigned long long)inc[k];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    if (lane == 0 && v != 0ull) atomicAdd(&sdig[k], v);
  }
  __syncthreads();
  for (int k = threadIdx.x; k < kIcpDigits; k += kBS)
    if (sdig[k] != 0ull) atomicAdd(&st->dig[k], sdig[k]);
}

__global__ void k_icp_publish(IcpState* __restrict__ st, IcpState* __restrict__ pub) {
  constexpr int kWords = (int)(sizeof(IcpState) / 4);
  uint32_t* s = reinterpret_cast<uint32_t*>(st);
  uint32_t* p = reinterpret_cast<uint32_t*>(pub);
  for (int k = threadIdx.x; k < kWords; k += blockDim.x) {
    p[k] = s[k];
    s[k] = 0u;
  }
  __threadfence_system();
}

__global__ __launch_bounds__(kBS) void k_icp_pack(const float* __restrict__ wx,
                                                  const float* __restrict__ wy,
                                                  const float* __restrict__ wz, int m,
                                                  float* __restrict__ out, int stride) {
  for (int i = blockIdx.x * kBS + threadIdx.x; i < m; i += gridDim.x * kBS) {
    float* o = out + (int64_t)i * stride;
    o[0] = wx[i];
    o[1] = wy[i];
    o[2] = wz[i];
    if (stride > 3) o[3] = 1.0f;
  }
}

// DLG_OPT_ICP_MAX_BLOCKS: at most max_blocks workgroups when it is >= 1 (0: the default shape)
inline int capped(int grid, int max_blocks) {
  return max_blocks >= 1 ? std::min(grid, max_blocks) : grid;
}
inline int stream_grid(int m, int max_blocks) {
  return capped(std::max(1, std::min(cdiv_i(m, kBS), 2048)), max_blocks);
}

}  // namespace

void launch_icp_gather(const float* raw, int64_t stride_f, const int32_t* idx, int m, const IcpXf& xf,
                       int apply, float* wx, float* wy, float* wz, int max_blocks, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_icp_gather, dim3(stream_grid(m, max_blocks)), dim3(kBS), 0, s, raw, stride_f,
                     idx, m, xf, apply, wx, wy, wz);
}

void launch_icp_apply(const IcpXf& xf, float* wx, float* wy, float* wz, int m, int max_blocks,
                      hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_icp_apply, dim3(stream_grid(m, max_blocks)), dim3(kBS), 0, s, xf, wx, wy, wz,
                     m);
}

void launch_icp_level(const KnnLevels& L, int level, const IcpXf& xf, int apply, int reversed,
                      float* wx, float* wy, float* wz, int m, const int32_t* qin, int32_t* qout,
                      IcpState* st, const int32_t* fin_pos, double md2, int32_t* nn, float* d2,
                      int num_cus, int max_blocks, hipStream_t s) {
  if (m <= 0) return;
  const int grid =
      capped(std::max(1, std::min(cdiv_i(m, kBS), std::max(num_cus, 1) * 8)), max_blocks);
  if (level == 0)
    hipLaunchKernelGGL(k_icp_level<true>, dim3(grid), dim3(kBS), 0, s, L, level, xf, apply, reversed,
                       wx, wy, wz, m, qin, qout, st, fin_pos, md2, nn, d2);
  else
    hipLaunchKernelGGL(k_icp_level<false>, dim3(grid), dim3(kBS), 0, s, L, level, xf, apply,
                       reversed, wx, wy, wz, m, qin, qout, st, fin_pos, md2, nn, d2);
}

void launch_icp_finish(const float* wx, const float* wy, const float* wz, int m, const int32_t* nn,
                       const float* d2, const float* tx, const float* ty, const float* tz, float tmax,
                       IcpState* st, int num_cus, int max_blocks, hipStream_t s) {
  if (m <= 0) return;
  // kIcpFlush entries a thread, at least enough workgroups to fill the device, 65536 at most
  const int need = std::min(cdiv_i(m, (int64_t)kBS * kIcpFlush), 65536);
  const int grid = capped(
      std::max(1, std::min(cdiv_i(m, kBS), std::max(std::max(num_cus, 1) * 4, need))), max_blocks);
  hipLaunchKernelGGL(k_icp_finish, dim3(grid), dim3(kBS), 0, s, wx, wy, wz, m, nn, d2, tx, ty, tz,
                     tmax, st);
}

void launch_icp_publish(IcpState* st, IcpState* pub, hipStream_t s) {
  hipLaunchKernelGGL(k_icp_publish, dim3(1), dim3(64), 0, s, st, pub);
}

void launch_icp_pack(const float* wx, const float* wy, const float* wz, int m, float* out,
                     int stride_f, int max_blocks, hipStream_t s) {
  if (m <= 0) return;
  hipLaunchKernelGGL(k_icp_pack, dim3(stream_grid(m, max_blocks)), dim3(kBS), 0, s, wx, wy, wz, m, out,
                     stride_f);
}

}  // namespace dlg
