// fpfh.hip -- pcl::FPFHEstimation<PointXYZ, Normal, FPFHSignature33> on the device
// (PCLViewer.cpp:524-543; the arithmetic: fpfh_model.hpp).  Both passes run one wave per point over
// the uniform grid of the normals path and scan the 27 cells around the point as k_mls scans them
// (9 candidate rows, 64 candidates per step, FLANN's d2 and test).
//
// k_fpfh_spfh: each lane takes one neighbour's pair feature and adds 1 to its three bins in the
// wave's LDS histogram (integer adds: the counts do not depend on the order); a lane per bin then
// turns the count into the sequential float sum of incr.
//
// k_fpfh_weight: the neighbours' (d2 bits << 32 | index) keys are compacted into the wave's LDS
// buffer and sorted there (FLANN's (d2, index) order), and a lane per bin walks them: hist[b] +=
// spfh[nbr][b] * w in float, in that order.  An entry with more than kFpfhCap neighbours takes them
// in windows: a scan keeps the smallest keys above the last one walked (when the buffer fills it is
// sorted and cut to its lower half, whose last key bounds what the rest of the scan admits), so the
// windows come in ascending order.  The three double sums: each lane also sums its bin's values in
// double, and where fpfh_cert_holds() proves that no partial sum of the entry's values can round,
// the histogram's sum is the 11 lanes' partial sums added up; otherwise the windows are walked again
// with lane g adding histogram g's values in the literal order (neighbour-major, bin-minor).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cstdint>

#include "fpfh.hpp"
#include "grid_dev.hpp"
#include "wave_sort_dev.hpp"

namespace dlg {

namespace {

using namespace grid;

constexpr int kBS = 256;
constexpr int kW = kBS / 64;
constexpr int kRun = 16;  // consecutive queries per wave: in sorted order they share their cells
constexpr int kWalk = 16;  // k_fpfh_weight: SPFH rows whose loads are in flight together

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

__device__ __forceinline__ double rl64(double v, int l) {
  const uint64_t b = (uint64_t)__double_as_longlong(v);
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)b, l);
  const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(b >> 32), l);
  return __longlong_as_double((long long)(((uint64_t)hi << 32) | lo));
}

__device__ __forceinline__ int lanes_below(uint64_t m) {
  return (int)__builtin_amdgcn_mbcnt_hi((uint32_t)(m >> 32),
                                        __builtin_amdgcn_mbcnt_lo((uint32_t)m, 0u));
}

struct GridArgs {
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
};

// the 27 cells around cell (cx, cy, cz) as 9 rows of contiguous sorted positions (k_mls's table):
// rows[r] = row r's start in the packed candidate list, rows[9 + r] = its offset to sorted
// positions, rows[18] = the list's length.  The whole wave calls it.
__device__ __forceinline__ void cell_rows(const GridArgs& a, int cx, int cy, int cz, int lane,
                                          int32_t* rows) {
  const GridDesc& G = a.G;
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

// a query's packed candidate list (k_mls's): position v lies in row q, the last row whose start
// r_start[q] <= v, at sorted position v + r_off[q].  Wave-uniform, read from cell_rows' table.
struct Cand {
  int r_start[9], r_off[9], tot;
  float qx, qy, qz;
};
#define DLG_FPFH_CAND_LOAD(cd, rows, x, y, z)                                             \
  Cand cd;                                                                                \
  _Pragma("unroll") for (int q_ = 0; q_ < 9; ++q_) {                                      \
    cd.r_start[q_] = __builtin_amdgcn_readfirstlane((rows)[q_]);                          \
    cd.r_off[q_] = __builtin_amdgcn_readfirstlane((rows)[9 + q_]);                        \
  }                                                                                       \
  cd.tot = __builtin_amdgcn_readfirstlane((rows)[18]);                                    \
  cd.qx = (x); cd.qy = (y); cd.qz = (z)
__device__ __forceinline__ int cand_pos(const Cand& cd, int v) {
  // (the offsets' steps added up, not one offset selected: every table entry is read on every
  // path, which keeps the table in registers; the starts ascend, so the steps of the rows that
  // start at or below v telescope to the last such row's offset)
  int u = v + cd.r_off[0];
#pragma unroll
  for (int q = 1; q < 9; ++q) u += v >= cd.r_start[q] ? cd.r_off[q] - cd.r_off[q - 1] : 0;
  return u;
}

// one step of a query's scan: candidate k0 + lane of the packed list
#define DLG_FPFH_CAND(cd, a, k0, lane)                                                   \
  const int v_ = (k0) + (lane);                                                           \
  const bool ok_ = v_ < (cd).tot;                                                         \
  const int u_ = cand_pos(cd, v_);                                                            \
  const int u = ok_ ? u_ : 0;                                                             \
  const float px = ok_ ? (a).sx[u] : 0.0f, py = ok_ ? (a).sy[u] : 0.0f,                   \
              pz = ok_ ? (a).sz[u] : 0.0f;                                                \
  const float d2 = flann_d2((cd).qx, (cd).qy, (cd).qz, px, py, pz);                       \
  const bool nbr = ok_ && d2 < (a).r2

__global__ __launch_bounds__(kBS) void k_fpfh_sort_normals(const int32_t* __restrict__ sidx, int n,
                                                           const float4* __restrict__ nrm,
                                                           float4* __restrict__ snrm) {
  const int t = blockIdx.x * kBS + threadIdx.x;
  if (t < n) snrm[t] = nrm[sidx[t]];
}

__global__ __launch_bounds__(kBS) void k_fpfh_spfh(GridArgs a, const float4* __restrict__ snrm,
                                                   float* __restrict__ spfh,
                                                   int32_t* __restrict__ counts,
                                                   int32_t* __restrict__ cnt,
                                                   int32_t* __restrict__ pairs) {
  __shared__ int32_t s_hist[kW][kFpfhDim + 3];
  __shared__ int32_t s_rows[kW][20];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int32_t* hist = s_hist[wv];
  int32_t* rows = s_rows[wv];
  if (lane < kFpfhDim) hist[lane] = 0;
  __builtin_amdgcn_wave_barrier();
  const GridDesc& G = a.G;
  const int nruns = (a.n + kRun - 1) / kRun;
  const int gw = (int)((blockIdx.x * kBS + threadIdx.x) >> 6), nw = (int)((gridDim.x * kBS) >> 6);
  for (int run = gw; run < nruns; run += nw) {
    int pcx = -1, pcy = -1, pcz = -1;
    const int i_end = min(a.n, (run + 1) * kRun);
    for (int t = run * kRun; t < i_end; ++t) {
      const float qx = a.sx[t], qy = a.sy[t], qz = a.sz[t];
      if (!fpfh_finite3(qx, qy, qz)) continue;
      const int pt = a.sidx[t];
      const float4 n4 = snrm[t];
      const float p[3] = {qx, qy, qz}, np[3] = {n4.x, n4.y, n4.z};
      const bool np_ok = fpfh_finite3(n4.x, n4.y, n4.z);
      const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
      const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
      const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
      if (cx != pcx || cy != pcy || cz != pcz) {
        pcx = cx; pcy = cy; pcz = cz;
        cell_rows(a, cx, cy, cz, lane, rows);
      }
      DLG_FPFH_CAND_LOAD(cd, rows, qx, qy, qz);
      int m = 0;
      for (int k0 = 0; k0 < cd.tot; k0 += 64) {
        DLG_FPFH_CAND(cd, a, k0, lane);
        m += (int)__popcll(__ballot(nbr));
        if (!(nbr && np_ok && u != t)) continue;
        const float4 q4 = snrm[u];
        if (!fpfh_finite3(q4.x, q4.y, q4.z)) continue;
        const float q[3] = {px, py, pz}, nq[3] = {q4.x, q4.y, q4.z};
        float f[3];
        if (!fpfh_pair(p, np, q, nq, f)) continue;
        int b[3];
        fpfh_bins(f, b);
        atomicAdd(&hist[b[0]], 1);
        atomicAdd(&hist[kFpfhBins + b[1]], 1);
        atomicAdd(&hist[2 * kFpfhBins + b[2]], 1);
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < kFpfhDim) {
        const int c = hist[lane];
        const int64_t o = (int64_t)pt * kFpfhDim + lane;
        spfh[o] = fpfh_bin_value(m, c);
        if (counts) counts[o] = c;
      }
      if (lane == 0) {
        int ok = 0;
#pragma unroll
        for (int k = 0; k < kFpfhBins; ++k) ok += hist[k];
        cnt[pt] = m;
        pairs[pt] = ok;
      }
      __builtin_amdgcn_wave_barrier();
      if (lane < kFpfhDim) hist[lane] = 0;
      __builtin_amdgcn_wave_barrier();
    }
  }
}

// the wave's cnt (<= 64 E) keys in buf, ascending
template <int E>
__device__ __forceinline__ void sort_keys(uint64_t* buf, int cnt, int lane) {
  uint64_t v[E];
#pragma unroll
  for (int j = 0; j < E; ++j) {
    const int e = lane + 64 * j;
    v[j] = e < cnt ? buf[e] : ~0ull;
  }
  wave_bitonic<E>(v);
  __builtin_amdgcn_wave_barrier();
#pragma unroll
  for (int j = 0; j < E; ++j) buf[lane + 64 * j] = v[j];
}
__device__ __forceinline__ void sort_window(uint64_t* buf, int cnt, int lane) {
  __builtin_amdgcn_wave_barrier();
  if (cnt <= 64) sort_keys<1>(buf, cnt, lane);
  else if (cnt <= 128) sort_keys<2>(buf, cnt, lane);
  else if (cnt <= 256) sort_keys<4>(buf, cnt, lane);
  else if (cnt <= 512) sort_keys<8>(buf, cnt, lane);
  else sort_keys<16>(buf, cnt, lane);
  static_assert(kFpfhCap == 64 * 16, "sort_keys<16> holds a full buffer");
  __builtin_amdgcn_wave_barrier();
}

struct WeightArgs {
  GridArgs g;
  const int32_t* idx;
  int n_list;
  const float* X;
  const float* Y;
  const float* Z;
  const float* spfh;
  const int32_t* pairs;
  float* hist;
  int32_t* nb;
  unsigned long long* acc;
};

// One entry's neighbours in (d2, index) order, window by window.  LIT = false: lane b < 33 adds bin
// b's values to h (float) and ds (double) and keeps the certificate's bounds; LIT = true: lane g < 3
// adds histogram g's values to ds in the literal order.  Returns the neighbour count.
template <bool LIT>
__device__ __forceinline__ int walk_entry(const GridArgs& a, const Cand& cd, uint64_t* keys,
                                          const float* __restrict__ spfh, int lane, float& h,
                                          double& ds, FpfhCert& cert) {
  uint64_t lo_key = 0;
  bool have_lo = false;
  int m = 0, done = 0;
  do {
    int cnt = 0, seen = 0;
    uint64_t hi_key = ~0ull;
    for (int k0 = 0; k0 < cd.tot; k0 += 64) {
      DLG_FPFH_CAND(cd, a, k0, lane);
      seen += (int)__popcll(__ballot(nbr));
      const uint64_t key =
          ((uint64_t)__float_as_uint(d2) << 32) | (uint32_t)(nbr ? a.sidx[u] : 0);
      bool in = nbr && (!have_lo || key > lo_key) && key < hi_key;
      uint64_t bm = __ballot(in);
      if (cnt + (int)__popcll(bm) > kFpfhCap) {  // (uniform) full: keep the lower half
        sort_window(keys, cnt, lane);
        cnt = kFpfhCap / 2;
        hi_key = keys[cnt - 1];
        in = in && key < hi_key;
        bm = __ballot(in);
      }
      if (in) keys[cnt + lanes_below(bm)] = key;
      cnt += (int)__popcll(bm);
    }
    sort_window(keys, cnt, lane);
    m = seen;
    if (cnt == 0) break;  // (m == 0 cannot happen: the query is its own neighbour)
    // the window's last key bounds the next window; then each key's d2 gives way to the weight
    // w = 1.0f / d2, once per neighbour (0: a neighbour the walk skips, d2 == 0 -- no d2 below the
    // squared radius has a reciprocal of 0)
    lo_key = keys[cnt - 1];
    have_lo = true;
    __builtin_amdgcn_wave_barrier();
    for (int e = lane; e < cnt; e += 64) {
      const uint64_t key = keys[e];
      const float d2 = __uint_as_float((uint32_t)(key >> 32));
      const float w = d2 == 0.0f ? 0.0f : 1.0f / d2;
      keys[e] = ((uint64_t)__float_as_uint(w) << 32) | (uint32_t)key;
    }
    __builtin_amdgcn_wave_barrier();
    if (!LIT) {
      if (lane < kFpfhDim) {
        // kWalk rows' loads in flight, then their terms in order (a key past the window reads as
        // w == 0, point 0: loaded, skipped)
        for (int e0 = 0; e0 < cnt; e0 += kWalk) {
          float wv[kWalk], row[kWalk];
#pragma unroll
          for (int j = 0; j < kWalk; ++j) {
            const uint64_t key = e0 + j < cnt ? keys[e0 + j] : 0ull;
            wv[j] = __uint_as_float((uint32_t)(key >> 32));
            row[j] = spfh[(int64_t)(uint32_t)key * kFpfhDim + lane];
          }
#pragma unroll
          for (int j = 0; j < kWalk; ++j) {
            if (wv[j] == 0.0f) continue;  // (uniform)
            const float val = row[j] * wv[j];
            h = h + val;
            ds = ds + (double)val;
            fpfh_cert_add(cert, val);
          }
        }
      }
    } else if (lane < 3) {
      for (int e = 0; e < cnt; ++e) {
        const uint64_t key = keys[e];
        const float w = __uint_as_float((uint32_t)(key >> 32));
        if (w == 0.0f) continue;
        const float* row = spfh + (int64_t)(uint32_t)key * kFpfhDim + kFpfhBins * lane;
#pragma unroll
        for (int k = 0; k < kFpfhBins; ++k) ds = ds + (double)(row[k] * w);
      }
    }
    done += cnt;
    __builtin_amdgcn_wave_barrier();  // (the next window overwrites the keys)
  } while (done < m);
  return m;
}

__global__ __launch_bounds__(kBS) void k_fpfh_weight(WeightArgs w) {
  __shared__ uint64_t s_keys[kW][kFpfhCap];
  __shared__ int32_t s_rows[kW][20];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  uint64_t* keys = s_keys[wv];
  int32_t* rows = s_rows[wv];
  const GridArgs& a = w.g;
  const GridDesc& G = a.G;
  // (uniform) the wave's share of the call's counts
  unsigned long long n_nan = 0, n_zero = 0, n_ovf = 0, n_pairs = 0, n_failed = 0, n_lit = 0;
  int max_nb = 0;
  const int nruns = (w.n_list + kRun - 1) / kRun;
  const int gw = (int)((blockIdx.x * kBS + threadIdx.x) >> 6), nw = (int)((gridDim.x * kBS) >> 6);
  for (int run = gw; run < nruns; run += nw) {
    int pcx = -1, pcy = -1, pcz = -1;
    const int i_end = min(w.n_list, (run + 1) * kRun);
    for (int i = run * kRun; i < i_end; ++i) {
      // no list: the entries in the grid's sorted order (entry = the point's index)
      const int pt = w.idx ? w.idx[i] : a.sidx[i];
      const int e = w.idx ? i : pt;
      const float qx = w.X[pt], qy = w.Y[pt], qz = w.Z[pt];
      const int64_t o = (int64_t)e * kFpfhDim + lane;
      if (!fpfh_finite3(qx, qy, qz)) {
        if (lane < kFpfhDim) w.hist[o] = __uint_as_float(0x7fc00000u);
        if (lane == 0) w.nb[e] = -1;
        ++n_nan;
        continue;
      }
      const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
      const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
      const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
      if (cx != pcx || cy != pcy || cz != pcz) {
        pcx = cx; pcy = cy; pcz = cz;
        cell_rows(a, cx, cy, cz, lane, rows);
      }
      DLG_FPFH_CAND_LOAD(cd, rows, qx, qy, qz);
      float h = 0.0f;
      double ds = 0.0;
      FpfhCert cert;
      const int m = walk_entry<false>(a, cd, keys, w.spfh, lane, h, ds, cert);
      // the 11 lanes' partial sums per histogram, and the certificate over the 33 lanes
      int clo = cert.lo;
      FpfhCert all;
      all.bad = __ballot(cert.bad) != 0;
#pragma unroll
      for (int s = 32; s >= 1; s >>= 1) clo = min(clo, __shfl_xor(clo, s, 64));
      all.lo = clo;
      double sum[3];
#pragma unroll
      for (int g = 0; g < 3; ++g) {
        sum[g] = 0.0;
#pragma unroll
        for (int k = 0; k < kFpfhBins; ++k) sum[g] = sum[g] + rl64(ds, kFpfhBins * g + k);
      }
      if (!fpfh_cert_holds(all, fmax(fmax(sum[0], sum[1]), sum[2]))) {
        float h2 = 0.0f;
        double dl = 0.0;
        FpfhCert c2;
        (void)walk_entry<true>(a, cd, keys, w.spfh, lane, h2, dl, c2);
#pragma unroll
        for (int g = 0; g < 3; ++g) sum[g] = rl64(dl, g);
        ++n_lit;
      }
      if (lane < kFpfhDim) {
        const double sg = lane < kFpfhBins ? sum[0] : lane < 2 * kFpfhBins ? sum[1] : sum[2];
        if (sg != 0.0) h = h * fpfh_scale(sg);
        w.hist[o] = h;
      }
      if (lane == 0) w.nb[e] = m;
      const int ok = w.pairs[pt];
      n_zero += m == 1 ? 1u : 0u;
      n_ovf += m > kFpfhCap ? 1u : 0u;
      n_pairs += (unsigned)ok;
      n_failed += (unsigned)(m - 1 - ok);
      max_nb = max(max_nb, m);
    }
  }
  if (lane == 0) {
    if (n_nan) atomicAdd(w.acc + kFpfhNanRows, n_nan);
    if (n_zero) atomicAdd(w.acc + kFpfhZeroRows, n_zero);
    if (n_ovf) atomicAdd(w.acc + kFpfhNOverflow, n_ovf);
    if (n_pairs) atomicAdd(w.acc + kFpfhPairs, n_pairs);
    if (n_failed) atomicAdd(w.acc + kFpfhPairsFailed, n_failed);
    if (n_lit) atomicAdd(w.acc + kFpfhLiteral, n_lit);
    if (max_nb) atomicMax(w.acc + kFpfhMaxNb, (unsigned long long)max_nb);
  }
}

GridArgs grid_args(const GridDesc& G, const GridBufs& B, int n, float r2) {
  GridArgs a;
  a.sx = B.sx; a.sy = B.sy; a.sz = B.sz; a.sidx = B.idx_out; a.n = n; a.G = G;
  a.tkeys = B.tkeys; a.trange = B.trange; a.tmask = B.tmask; a.r2 = r2;
  return a;
}

unsigned wave_grid(int64_t queries, int num_cus) {
  const int64_t waves = cdiv(queries, kRun);
  return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(waves, kW), (int64_t)num_cus * 64));
}

}  // namespace

void launch_fpfh_sort_normals(const GridBufs& B, int n, const float4* nrm, float4* snrm,
                              hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_fpfh_sort_normals, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, B.idx_out, n, nrm,
                     snrm);
}

void launch_fpfh_spfh(const GridDesc& G, const GridBufs& B, int n, float r2, const float4* snrm,
                      float* spfh, int32_t* counts, int32_t* cnt, int32_t* pairs, int num_cus,
                      hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_fpfh_spfh, dim3(wave_grid(n, num_cus)), dim3(kBS), 0, s,
                     grid_args(G, B, n, r2), snrm, spfh, counts, cnt, pairs);
}

void launch_fpfh_weight(const GridDesc& G, const GridBufs& B, int n, float r2, const int32_t* idx,
                        int n_list, const float* X, const float* Y, const float* Z,
                        const float* spfh, const int32_t* pairs, float* hist, int32_t* nb,
                        unsigned long long* acc, int num_cus, hipStream_t s) {
  if (n_list <= 0) return;
  WeightArgs w;
  w.g = grid_args(G, B, n, r2);
  w.idx = idx; w.n_list = n_list; w.X = X; w.Y = Y; w.Z = Z; w.spfh = spfh; w.pairs = pairs;
  w.hist = hist; w.nb = nb; w.acc = acc;
  hipLaunchKernelGGL(k_fpfh_weight, dim3(wave_grid(n_list, num_cus)), dim3(kBS), 0, s, w);
}

}  // namespace dlg
