// mls.hip -- pcl::MovingLeastSquares<PointXYZ, PointNormal> on the device (PCLViewer.cpp:387-423;
// the arithmetic: mls_model.hpp).  k_mls runs one wave per query over the uniform grid of the
// normals path: the 27 cells around the query are scanned as k_nbr_fused scans them (9 candidate
// rows, 64 candidates per step, four steps' loads in flight, FLANN's d2 and test), the neighbours
// are staged in the wave's LDS buffer as (x, y, z) floats -- unsorted: the order of the sums is not
// part of the contract -- and three sweeps over them, one neighbour per lane, give the centroid,
// the covariance and, after the lane-uniform eigen33 and frame, the weighted normal equations.
// The sums are reduced over the wave by a transposing butterfly (below) that leaves entry e of the
// equations in lane e; lane a then takes row a of the lower triangle and b[a], so the Cholesky
// factorisation and the two solves run with compile-time register indices and readlane
// broadcasts, the same operations in the same order as mls_llt_solve.  A query with more than
// kMlsCap neighbours sweeps the grid's candidates again instead of the buffer.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>
#include <utility>

#include "grid_dev.hpp"
#include "mls.hpp"

namespace dlg {

namespace {

using namespace grid;

constexpr int kBS = 256;
constexpr int kMlsRun = 16;  // consecutive sorted positions per wave: they share their cells
constexpr int kMlsB = 4;     // candidate steps whose loads are in flight together

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__device__ __forceinline__ bool finite3(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z);
}

__device__ __forceinline__ double rl64(double v, int l) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

template <int CTRL>
__device__ __forceinline__ double dpp64(double v) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)b, CTRL, 0xF, 0xF, false);
  const uint32_t hi =
      (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)(b >> 32), CTRL, 0xF, 0xF, false);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

// ---- the normal equations' reduction --------------------------------------------------------
// The N(N+1)/2 + N entries of (A's lower triangle, b) are numbered e = r(r+1)/2 + k for A[r][k]
// and T + r for b[r].  Each lane has one neighbour's term of every entry; a transposing butterfly
// (step s: the lanes whose bit s is clear keep the even-numbered values and pass the odd ones to
// their partner lane ^ 2^s, the others the reverse, both add what they receive) halves the number
// of values per step instead of repeating a full reduction per entry: 16 entries cost 15 + 2
// exchanges where 16 wave sums cost 96.  After the six steps lane e holds the wave's sum of entry
// e (entry 64 + e in the second word), which it accumulates over the query's chunks.
template <int S>
__device__ __forceinline__ double xchg(double v) {
  if constexpr (S == 0) return dpp64<0xB1>(v);       // quad_perm [1,0,3,2]: lane ^ 1
  else if constexpr (S == 1) return dpp64<0x4E>(v);  // quad_perm [2,3,0,1]: lane ^ 2
  else return __shfl_xor(v, 1 << S, 64);
}

template <int S, int NIN>
__device__ __forceinline__ void fold(const double (&in)[NIN], double (&out)[(NIN + 1) / 2],
                                     int lane) {
  const bool hi = (lane >> S) & 1;
#pragma unroll
  for (int j = 0; j < (NIN + 1) / 2; ++j) {
    const double a = in[2 * j];
    const double b = 2 * j + 1 < NIN ? in[2 * j + 1] : 0.0;
    out[j] = (hi ? b : a) + xchg<S>(hi ? a : b);
  }
}

// the wave's sums of M <= 64 values by the same butterfly, each made uniform (lane k ends up
// holding the sum of value k)
template <int S, int NIN>
__device__ __forceinline__ double fold_all(const double (&in)[NIN], int lane) {
  double out[(NIN + 1) / 2];
  fold<S, NIN>(in, out, lane);
  if constexpr (S == 5) {
    static_assert(NIN <= 2, "64 values at most");
    return out[0];
  } else {
    return fold_all<S + 1, (NIN + 1) / 2>(out, lane);
  }
}
template <int M>
__device__ __forceinline__ void wave_sums(double (&v)[M], int lane) {
  const double r = fold_all<0, M>(v, lane);
#pragma unroll
  for (int k = 0; k < M; ++k) v[k] = rl64(r, k);
}

template <int N>
struct MlsEntries {
  static constexpr int T = N * (N + 1) / 2;
  static constexpr int kCount = T + N;
  static constexpr int kGroups = (kCount + 15) / 16;
  static constexpr int kWords = (kGroups + 3) / 4;  // accumulators per lane
  static constexpr int row(int e) {
    int r = 0;
    while ((r + 1) * (r + 2) / 2 <= e) ++r;
    return r;
  }
};

template <int N, int E>
__device__ __forceinline__ double entry_term(const double (&t)[N], double w, double f) {
  using En = MlsEntries<N>;
  if constexpr (E < En::T) {
    constexpr int r = En::row(E), k = E - r * (r + 1) / 2;
    return (t[r] * w) * t[k];
  } else if constexpr (E < En::kCount) {
    return (t[E - En::T] * w) * f;
  } else {
    return 0.0;
  }
}

template <int N, int G, int... J>
__device__ __forceinline__ double group_sum(const double (&t)[N], double w, double f, bool in,
                                            int lane, std::integer_sequence<int, J...>) {
  double v16[16] = {(in ? entry_term<N, 16 * G + J>(t, w, f) : 0.0)...};
  double v8[8], v4[4], v2[2], v1[1];
  fold<0, 16>(v16, v8, lane);
  fold<1, 8>(v8, v4, lane);
  fold<2, 4>(v4, v2, lane);
  fold<3, 2>(v2, v1, lane);
  return v1[0];  // lane l: entry 16 G + (l & 15) summed over the lane's row of 16
}

template <int N, int... G>
__device__ __forceinline__ void equations_add(const double (&t)[N], double w, double f, bool in,
                                              int lane, double (&acc)[MlsEntries<N>::kWords],
                                              std::integer_sequence<int, G...>) {
  constexpr int NG = MlsEntries<N>::kGroups;
  double g[NG];
  // (one group at a time: 16 terms live, not all of them)
  ((g[G] = group_sum<N, G>(t, w, f, in, lane, std::make_integer_sequence<int, 16>()),
    __builtin_amdgcn_sched_barrier(0)), ...);
  double h[(NG + 1) / 2], o[MlsEntries<N>::kWords];
  fold<4, NG>(g, h, lane);
  fold<5, (NG + 1) / 2>(h, o, lane);
  static_assert(((NG + 1) / 2 + 1) / 2 == MlsEntries<N>::kWords, "two folds leave kWords values");
#pragma unroll
  for (int k = 0; k < MlsEntries<N>::kWords; ++k) acc[k] = acc[k] + o[k];
}

// mls_llt_solve over the wave: lane a holds row[c] = A[a][c] (c <= a) and bb = b[a]; c[] uniform
template <int N>
__device__ __forceinline__ void wave_llt_solve(double (&row)[N], double bb, int lane,
                                               double (&c)[N]) {
  bool alive = true;
#pragma unroll
  for (int k = 0; k < N; ++k) {
    if (alive) {  // (uniform)
      double dot = 0.0;
#pragma unroll
      for (int j = 0; j < k; ++j) dot = dot + row[j] * rl64(row[j], k);
      const double s = row[k] - dot;
      const double x = rl64(s, k);
      if (x <= 0.0) {
        alive = false;
      } else {
        const double sx = sqrt(x);
        row[k] = lane == k ? sx : s / sx;  // (lanes above k: column k of L)
      }
    }
  }
  double y[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double dot = 0.0;
#pragma unroll
    for (int j = 0; j < i; ++j) dot = dot + row[j] * y[j];
    y[i] = rl64((bb - dot) / row[i], i);
  }
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double dot = 0.0;
#pragma unroll
    for (int j = i + 1; j < N; ++j) dot = dot + rl64(row[i], j) * c[j];
    c[i] = (y[i] - dot) / rl64(row[i], i);
  }
}

struct MlsArgs {
  const float* sx;
  const float* sy;
  const float* sz;
  const int32_t* sidx;
  int n;
  GridDesc G;
  const uint32_t* tkeys;
  const int2* trange;
  uint32_t tmask;
  float r2;
  const uint8_t* need;
  int polynomial_fit, compute_normals;
  double sqr_gauss;
  float4* res_p;
  float4* res_n;
  int32_t* cnt;
};

// the packed candidate list of a query's 27 cells (k_nbr_fused's): position v lies in row q, the
// last row whose start r_start[q] <= v, at sorted position v + r_off[q]
struct Cand {
  int r_start[9], r_off[9], tot;
  float qx, qy, qz, r2;
  const float* __restrict__ sx;
  const float* __restrict__ sy;
  const float* __restrict__ sz;
  // f(in, px, py, pz) per step of 64 candidates, in = a neighbour in this lane
  template <typename F>
  __device__ __forceinline__ void each(int lane, F&& f) const {
    for (int k0 = 0; k0 < tot; k0 += 64 * kMlsB) {
      float px[kMlsB], py[kMlsB], pz[kMlsB];
      bool ok[kMlsB];
#pragma unroll
      for (int j = 0; j < kMlsB; ++j) {
        const int v = k0 + 64 * j + lane;
        int u = v + r_off[0];
#pragma unroll
        for (int q = 1; q < 9; ++q) u = v >= r_start[q] ? v + r_off[q] : u;
        ok[j] = v < tot;
        px[j] = ok[j] ? sx[u] : 0.0f;
        py[j] = ok[j] ? sy[u] : 0.0f;
        pz[j] = ok[j] ? sz[u] : 0.0f;
      }
#pragma unroll
      for (int j = 0; j < kMlsB; ++j) {
        if (k0 + 64 * j >= tot) break;  // (uniform)
        const bool in = ok[j] && flann_d2(qx, qy, qz, px[j], py[j], pz[j]) < r2;
        f(in, px[j], py[j], pz[j]);
      }
    }
  }
};

// the neighbours of the current query: the staged ones, or the grid's candidates again
template <typename F>
__device__ __forceinline__ void sweep(const Cand& cd, const uint32_t* buf, int cnt, int lane,
                                      F&& f) {
  if (cnt <= kMlsCap) {
    for (int e0 = 0; e0 < cnt; e0 += 64) {
      const int e = e0 + lane;
      const bool in = e < cnt;
      const float px = in ? __uint_as_float(buf[3 * e]) : 0.0f;
      const float py = in ? __uint_as_float(buf[3 * e + 1]) : 0.0f;
      const float pz = in ? __uint_as_float(buf[3 * e + 2]) : 0.0f;
      f(in, px, py, pz);
    }
  } else {
    cd.each(lane, f);
  }
}

template <int ORDER>
__global__ __launch_bounds__(kBS) __attribute__((amdgpu_waves_per_eu(ORDER >= 2 ? 2 : 3))) void k_mls(MlsArgs a) {
  constexpr int N = mls_nr_coeff(ORDER);
  constexpr int kW = kBS / 64;
  __shared__ uint32_t s_buf[kW][3 * kMlsCap];
  __shared__ int32_t s_rows[kW][20];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint32_t* buf = s_buf[wv];
  int32_t* rows = s_rows[wv];
  const GridDesc& G = a.G;
  Cand cd;
  cd.sx = a.sx; cd.sy = a.sy; cd.sz = a.sz; cd.r2 = a.r2;
  const int nruns = (a.n + kMlsRun - 1) / kMlsRun;
  const int gw = (int)((blockIdx.x * kBS + threadIdx.x) >> 6), nw = (int)((gridDim.x * kBS) >> 6);
  for (int run = gw; run < nruns; run += nw) {
    int pcx = -1, pcy = -1, pcz = -1;
    const int i_end = min(a.n, (run + 1) * kMlsRun);
    for (int t = run * kMlsRun; t < i_end; ++t) {
      const int pt = a.sidx[t];
      if (a.need && !a.need[pt]) continue;
      const float qx = a.sx[t], qy = a.sy[t], qz = a.sz[t];
      if (!finite3(qx, qy, qz)) continue;
      const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
      const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
      const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
      if (cx != pcx || cy != pcy || cz != pcz) {
        pcx = cx; pcy = cy; pcz = cz;
        // lanes 0..26 look up one cell each; a row's range is its cells' union (contiguous)
        int2 c = make_int2(INT_MAX, INT_MIN);
        if (lane < 27) {
          const int x = cx + lane % 3 - 1, y = cy + (lane / 3) % 3 - 1, z = cz + lane / 9 - 1;
          if (x >= 0 && y >= 0 && z >= 0 && x < G.g[0] && y < G.g[1] && z < G.g[2]) {
            const int2 r = cell_range(a.tkeys, a.trange, a.tmask, cell_key(G, x, y, z));
            if (r.y > r.x) c = r;
          }
        }
        int lo = c.x, hi = c.y;
#pragma unroll
        for (int o = 1; o <= 2; o <<= 1) {  // (min / max over each aligned triple of lanes)
          const int l2 = __shfl(lo, (lane / 3) * 3 + ((lane % 3 + o) % 3), 64);
          const int h2 = __shfl(hi, (lane / 3) * 3 + ((lane % 3 + o) % 3), 64);
          lo = min(lo, l2);
          hi = max(hi, h2);
        }
        const int rl = __shfl(lo, 3 * (lane < 9 ? lane : 0), 64);
        const int rh = __shfl(hi, 3 * (lane < 9 ? lane : 0), 64);
        const int2 rg = lane < 9 && rl < rh ? make_int2(rl, rh) : make_int2(0, 0);
        const int rlen = rg.y - rg.x;
        int incl = rlen;  // (lanes 0..8: inclusive prefix of the row lengths)
#pragma unroll
        for (int o = 1; o < 16; o <<= 1) {
          const int w = __shfl_up(incl, o, 64);
          if (lane >= o) incl += w;
        }
        const int excl = incl - rlen;
        __builtin_amdgcn_wave_barrier();
        if (lane < 9) {
          rows[lane] = excl;
          rows[9 + lane] = rg.x - excl;
        }
        if (lane == 8) rows[18] = incl;
        __builtin_amdgcn_wave_barrier();
      }
#pragma unroll
      for (int q = 0; q < 9; ++q) {
        cd.r_start[q] = __builtin_amdgcn_readfirstlane(rows[q]);
        cd.r_off[q] = __builtin_amdgcn_readfirstlane(rows[9 + q]);
      }
      cd.tot = __builtin_amdgcn_readfirstlane(rows[18]);
      cd.qx = qx; cd.qy = qy; cd.qz = qz;
      // the search: count, and stage what fits
      int cnt = 0;
      cd.each(lane, [&](bool in, float px, float py, float pz) {
        const uint64_t m = __ballot(in);
        const int p = cnt + __builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                                      __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
        if (in && p < kMlsCap) {
          buf[3 * p] = __float_as_uint(px);
          buf[3 * p + 1] = __float_as_uint(py);
          buf[3 * p + 2] = __float_as_uint(pz);
        }
        cnt += (int)__popcll(m);
      });
      if (lane == 0) a.cnt[pt] = cnt;
      if (cnt < 3) continue;
      __builtin_amdgcn_wave_barrier();
      // pass 1: centroid, then covariance
      double sp[3] = {0.0, 0.0, 0.0};
      sweep(cd, buf, cnt, lane, [&](bool in, float px, float py, float pz) {
        sp[0] = sp[0] + (in ? (double)px : 0.0);
        sp[1] = sp[1] + (in ? (double)py : 0.0);
        sp[2] = sp[2] + (in ? (double)pz : 0.0);
      });
      wave_sums<3>(sp, lane);
      const double m = (double)cnt;
      const double cen[3] = {sp[0] / m, sp[1] / m, sp[2] / m};
      double cv[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
      sweep(cd, buf, cnt, lane, [&](bool in, float px, float py, float pz) {
        const double dx = in ? (double)px - cen[0] : 0.0, dy = in ? (double)py - cen[1] : 0.0,
                     dz = in ? (double)pz - cen[2] : 0.0;
        cv[0] = cv[0] + dx * dx; cv[1] = cv[1] + dx * dy; cv[2] = cv[2] + dx * dz;
        cv[3] = cv[3] + dy * dy; cv[4] = cv[4] + dy * dz; cv[5] = cv[5] + dz * dz;
      });
      wave_sums<6>(cv, lane);
      MlsFrame F;
      const float q[3] = {qx, qy, qz};
      mls_frame(cv, cen, q, &F);
      // pass 2: the weighted normal equations, the factorisation and the solves
      const bool fit = a.polynomial_fit && cnt >= N;
      double c0 = 0.0, cu = 0.0, cvv = 0.0;
      if (fit) {
        using En = MlsEntries<N>;
        double acc[En::kWords];
#pragma unroll
        for (int k = 0; k < En::kWords; ++k) acc[k] = 0.0;
        sweep(cd, buf, cnt, lane, [&](bool in, float px, float py, float pz) {
          double t[N], w, f;
          mls_terms<ORDER>(px, py, pz, F, a.sqr_gauss, t, &w, &f);
          equations_add<N>(t, w, f, in, lane, acc, std::make_integer_sequence<int, En::kGroups>());
        });
        // entry e sits in lane e & 63 of word e >> 6: to lane r its row of A and b[r]
        double row[N], bb = 0.0;
#pragma unroll
        for (int k = 0; k < N; ++k) row[k] = 0.0;
#pragma unroll
        for (int r = 0; r < N; ++r) {
#pragma unroll
          for (int k = 0; k < N; ++k) {
            if (k > r) continue;
            const int e = r * (r + 1) / 2 + k;
            const double sv = rl64(acc[e >> 6], e & 63);
            row[k] = lane == r ? sv : row[k];
          }
          const int eb = En::T + r;
          const double sb = rl64(acc[eb >> 6], eb & 63);
          bb = lane == r ? sb : bb;
        }
        double c[N];
        wave_llt_solve<N>(row, bb, lane, c);
        c0 = c[0]; cu = c[ORDER + 1]; cvv = c[1];
      }
      MlsRow out;
      mls_finish(F, fit, c0, cu, cvv, a.compute_normals != 0, &out);
      if (lane == 0) {
        a.res_p[pt] = make_float4(out.xyz[0], out.xyz[1], out.xyz[2], __int_as_float(out.code));
        a.res_n[pt] = make_float4(out.nrm[0], out.nrm[1], out.nrm[2], out.nrm[3]);
      }
      __builtin_amdgcn_wave_barrier();  // (the next query's neighbours overwrite the buffer)
    }
  }
}

__global__ __launch_bounds__(kBS) void k_mls_count_finite(const float* __restrict__ X,
                                                          const float* __restrict__ Y,
                                                          const float* __restrict__ Z, int n,
                                                          unsigned long long* __restrict__ dst) {
  unsigned c = 0;
  for (int64_t i = (int64_t)blockIdx.x * kBS + threadIdx.x; i < n; i += (int64_t)gridDim.x * kBS)
    c += finite3(X[i], Y[i], Z[i]) ? 1u : 0u;
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) c += __shfl_xor(c, s, 64);
  if ((threadIdx.x & 63) == 0 && c) atomicAdd(dst, (unsigned long long)c);
}

__global__ __launch_bounds__(kBS) void k_mls_need(const int32_t* __restrict__ idx, int n_list,
                                                  uint8_t* __restrict__ need) {
  const int e = blockIdx.x * kBS + threadIdx.x;
  if (e < n_list) need[idx[e]] = 1;
}

__global__ __launch_bounds__(kBS) void k_mls_entries(
    const int32_t* __restrict__ idx, int n_list, const float* __restrict__ X,
    const float* __restrict__ Y, const float* __restrict__ Z, const int32_t* __restrict__ cnt,
    const float4* __restrict__ res_p, int32_t* __restrict__ nb, uint8_t* __restrict__ valid,
    unsigned long long* __restrict__ acc) {
  const int e = blockIdx.x * kBS + threadIdx.x;
  bool few = false, plane = false, nonfin = false, ovf = false;
  int mx = 0;
  if (e < n_list) {
    const int p = idx ? idx[e] : e;
    const bool fin = finite3(X[p], Y[p], Z[p]);
    const int k = fin ? cnt[p] : -1;
    nb[e] = k;
    const bool row = k >= 3;
    valid[e] = row ? 1 : 0;
    few = fin && !row;
    if (row) {
      const int code = __float_as_int(res_p[p].w);
      plane = code == kMlsPlaneOnly;
      nonfin = code == kMlsFitNonfinite;
    }
    ovf = k > kMlsCap;
    mx = k > 0 ? k : 0;
  }
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) mx = max(mx, __shfl_xor(mx, s, 64));
  const uint64_t bf = __ballot(few), bp = __ballot(plane), bn = __ballot(nonfin), bo = __ballot(ovf);
  if ((threadIdx.x & 63) == 0) {
    if (bf) atomicAdd(acc + kMlsNTooFew, (unsigned long long)__popcll(bf));
    if (bp) atomicAdd(acc + kMlsNPlane, (unsigned long long)__popcll(bp));
    if (bn) atomicAdd(acc + kMlsNNonfinite, (unsigned long long)__popcll(bn));
    if (bo) atomicAdd(acc + kMlsNOverflow, (unsigned long long)__popcll(bo));
    if (mx) atomicMax(acc + kMlsMaxNb, (unsigned long long)mx);
  }
}

__global__ __launch_bounds__(kBS) void k_mls_emit(
    const int32_t* __restrict__ sel, const uint32_t* __restrict__ count, int n_list,
    const int32_t* __restrict__ idx, const float4* __restrict__ res_p,
    const float4* __restrict__ res_n, float* __restrict__ out_xyz, int64_t stride_f,
    float* __restrict__ X, float* __restrict__ Y, float* __restrict__ Z, int32_t* __restrict__ gid,
    int32_t id_base, float4* __restrict__ out_nrm, int32_t* __restrict__ out_src) {
  const int j = blockIdx.x * kBS + threadIdx.x;
  if (j >= n_list || (uint32_t)j >= *count) return;
  const int e = sel[j];
  const int p = idx ? idx[e] : e;
  const float4 r = res_p[p];
  if (out_xyz) {
    float* o = out_xyz + (int64_t)j * stride_f;
    o[0] = r.x; o[1] = r.y; o[2] = r.z;
    if (stride_f >= 4) o[3] = 1.0f;  // pcl::PointXYZ's data[3]
  } else {
    X[j] = r.x; Y[j] = r.y; Z[j] = r.z;
    gid[j] = id_base + j;
  }
  out_nrm[j] = res_n[p];
  out_src[j] = p;
}

}  // namespace

void launch_count_finite(const float* X, const float* Y, const float* Z, int n,
                         unsigned long long* dst, hipStream_t s) {
  if (n <= 0) return;
  const unsigned b = std::min(cdiv(n, kBS * 8), 2048u);
  hipLaunchKernelGGL(k_mls_count_finite, dim3(b), dim3(kBS), 0, s, X, Y, Z, n, dst);
}

void launch_mls_need(const int32_t* idx, int n_list, uint8_t* need, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_mls_need, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, idx, n_list, need);
}

void launch_mls(const GridDesc& G, const GridBufs& B, int n, const uint8_t* need, float r2,
                int order, int polynomial_fit, int compute_normals, double sqr_gauss, float4* res_p,
                float4* res_n, int32_t* cnt, int num_cus, hipStream_t s) {
  if (n <= 0) return;
  MlsArgs a;
  a.sx = B.sx; a.sy = B.sy; a.sz = B.sz; a.sidx = B.idx_out; a.n = n; a.G = G;
  a.tkeys = B.tkeys; a.trange = B.trange; a.tmask = B.tmask; a.r2 = r2; a.need = need;
  a.polynomial_fit = polynomial_fit; a.compute_normals = compute_normals;
  a.sqr_gauss = sqr_gauss; a.res_p = res_p; a.res_n = res_n; a.cnt = cnt;
  const int64_t waves = cdiv(n, kMlsRun);
  const unsigned g = (unsigned)std::max<int64_t>(
      1, std::min<int64_t>(cdiv(waves, kBS / 64), (int64_t)num_cus * 64));
  if (order == 1) hipLaunchKernelGGL(k_mls<1>, dim3(g), dim3(kBS), 0, s, a);
  else if (order == 2) hipLaunchKernelGGL(k_mls<2>, dim3(g), dim3(kBS), 0, s, a);
  else hipLaunchKernelGGL(k_mls<3>, dim3(g), dim3(kBS), 0, s, a);
}

void launch_mls_entries(const int32_t* idx, int n_list, const float* X, const float* Y,
                        const float* Z, const int32_t* cnt, const float4* res_p, int32_t* nb,
                        uint8_t* valid, unsigned long long* acc, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_mls_entries, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, idx, n_list, X, Y, Z,
                     cnt, res_p, nb, valid, acc);
}

void launch_mls_emit(const int32_t* sel, const uint32_t* count, int n_list, const int32_t* idx,
                     const float4* res_p, const float4* res_n, float* out_xyz, int64_t stride_f,
                     float4* out_nrm, int32_t* out_src, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_mls_emit, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, sel, count, n_list, idx,
                     res_p, res_n, out_xyz, stride_f, (float*)nullptr, (float*)nullptr,
                     (float*)nullptr, (int32_t*)nullptr, 0, out_nrm, out_src);
}

void launch_mls_emit_cloud(const int32_t* sel, const uint32_t* count, int n_list,
                           const int32_t* idx, const float4* res_p, const float4* res_n, float* X,
                           float* Y, float* Z, int32_t* gid, int32_t id_base, float4* out_nrm,
                           int32_t* out_src, hipStream_t s) {
  if (n_list <= 0) return;
  hipLaunchKernelGGL(k_mls_emit, dim3(cdiv(n_list, kBS)), dim3(kBS), 0, s, sel, count, n_list, idx,
                     res_p, res_n, (float*)nullptr, (int64_t)0, X, Y, Z, gid, id_base, out_nrm,
                     out_src);
}

}  // namespace dlg
