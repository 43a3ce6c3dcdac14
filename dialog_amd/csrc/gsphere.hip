// gsphere.hip -- the data-parallel phases of the Gaussian-sphere plane seeds on gfx950
// (Dialog/PlaneDetect.h:761-803 voteForPS and filtPS, :933-1005 segmentPlanes).  The arithmetic
// is gsphere_model.hpp's; the sequential phases between them run on the host (gsphere_host.cpp).
//
// Vote: one thread per point looks at the 5^3 lattice box around its query through the dense
// lattice -> PS table; the box bound (gsphere_model.hpp) proves the result the nearest of all
// cells, or the point is queued and one wave searches every cell for it.  Votes are integer
// atomics, one per distinct cell of a wave.
//
// Filter: the occupied cells are few, so the neighbour lists are built from their side: one wave
// per occupied cell walks the lattice box of the radius and enters itself in the list of every PS
// cell within reach (a count pass, a scan, a fill pass).  Then one wave per PS cell with a
// non-empty list sorts its (d2, index) keys -- in registers up to 256 keys (wave_sort_dev.hpp), by
// rank counting above -- and adds the terms in that order, every lane carrying the same sum.
//
// Seeds: the points carry their cell's sink as a label; one union-find pass over the radius grid
// joins equal labels (the reference's BFS per sink finds the same components, sinks partition the
// points); a component of m points is kept iff 2 m - 1 >= T_num_of_single_plane (the reference
// pushes every point but the seed twice before it tests the size).  Two stable radix sorts order
// the kept points: by (sink rank, cell) -- the reference's `planes` lists, one after the other --
// then by their component's first position in that list.
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <climits>
#include <cstdint>

#include "grid_dev.hpp"
#include "gsphere.hpp"
#include "gsphere_model.hpp"
#include "union_find_dev.hpp"
#include "wave_sort_dev.hpp"

namespace dlg {

namespace {

using namespace grid;

constexpr int kBS = 256;
constexpr int kSortRegs = 4;  // register sort: up to 64 * kSortRegs keys

inline unsigned cdiv(int64_t a, int64_t b) { return (unsigned)((a + b - 1) / b); }

// arr[key] += 1 for every lane with todo, one atomic per distinct key of the wave
template <typename T>
__device__ __forceinline__ void wave_count(bool todo, int key, T* arr) {
  const int lane = threadIdx.x & 63;
  uint64_t act = __ballot(todo);
  while (act) {
    const int leader = __ffsll((unsigned long long)act) - 1;
    const int kl = __shfl(key, leader, 64);
    const uint64_t same = __ballot(todo && key == kl);
    if (lane == leader) atomicAdd(&arr[kl], (T)__popcll(same));
    if (key == kl) todo = false;
    act = __ballot(todo);
  }
}

__device__ __forceinline__ uint64_t wave_min64(uint64_t v) {
#pragma unroll
  for (int s = 32; s >= 1; s >>= 1) {
    const uint64_t o = __shfl_xor((unsigned long long)v, s, 64);
    v = o < v ? o : v;
  }
  return v;
}

__global__ __launch_bounds__(kBS) void k_gs_vote(GsSpaceDev S, const float4* __restrict__ nrm,
                                                 int n, int32_t* __restrict__ cell_of_point,
                                                 int32_t* votes, int32_t* __restrict__ queue,
                                                 unsigned long long* cnt) {
  const int i = blockIdx.x * kBS + threadIdx.x;
  int cell = -1;
  bool defer = false;
  if (i < n) {
    const float4 v = nrm[i];
    if (gs::finite3(v.x, v.y, v.z)) {
      const float r = S.num_res;
      const float qx = gs::query(v.x, r), qy = gs::query(v.y, r), qz = gs::query(v.z, r);
      const int cx = gs::near_coord(qx, r, S.size), cy = gs::near_coord(qy, r, S.size),
                cz = gs::near_coord(qz, r, S.size);
      uint64_t best = gs::kNoKey;
      for (int a = max(cx - gs::kBoxHalf, 0); a <= min(cx + gs::kBoxHalf, S.size - 1); ++a)
        for (int b = max(cy - gs::kBoxHalf, 0); b <= min(cy + gs::kBoxHalf, S.size - 1); ++b)
          for (int c = max(cz - gs::kBoxHalf, 0); c <= min(cz + gs::kBoxHalf, S.size - 1); ++c) {
            const int32_t o = S.table[(a * S.size + b) * S.size + c];
            if (o < 0) continue;
            const uint64_t k = gs::make_key(
                gs::d2(qx, qy, qz, gs::cell_min(a, r), gs::cell_min(b, r), gs::cell_min(c, r)), o);
            best = k < best ? k : best;
          }
      const float reach = fminf(gs::axis_reach(qx, cx, r),
                                fminf(gs::axis_reach(qy, cy, r), gs::axis_reach(qz, cz, r)));
      if (best != gs::kNoKey && gs::box_proves(gs::key_d2(best), reach))
        cell = gs::key_index(best);
      else
        defer = true;
    }
    if (!defer) cell_of_point[i] = cell;
  }
  wave_count(cell >= 0, cell, votes);
  if (defer) queue[atomicAdd(&cnt[kGsQueued], 1ull)] = i;
}

// one wave per queued point: the smallest (d2, index) over all PS cells
__global__ __launch_bounds__(kBS) void k_gs_vote_all(GsSpaceDev S, const float4* __restrict__ nrm,
                                                     const int32_t* __restrict__ queue,
                                                     const unsigned long long* cnt,
                                                     int32_t* __restrict__ cell_of_point,
                                                     int32_t* votes) {
  const int lane = threadIdx.x & 63;
  const long long nq = (long long)cnt[kGsQueued];
  const long long waves = (long long)gridDim.x * (kBS / 64);
  for (long long w = (long long)blockIdx.x * (kBS / 64) + (threadIdx.x >> 6); w < nq; w += waves) {
    const int i = queue[w];
    const float4 v = nrm[i];
    const float r = S.num_res;
    const float qx = gs::query(v.x, r), qy = gs::query(v.y, r), qz = gs::query(v.z, r);
    uint64_t best = gs::kNoKey;
    for (int32_t o = lane; o < S.cells; o += 64) {
      const uint64_t k = gs::make_key(gs::d2(qx, qy, qz, S.px[o], S.py[o], S.pz[o]), o);
      best = k < best ? k : best;
    }
    best = wave_min64(best);
    if (lane == 0) {
      const int32_t cell = best == gs::kNoKey ? -1 : gs::key_index(best);
      cell_of_point[i] = cell;
      if (cell >= 0) atomicAdd(&votes[cell], 1);
    }
  }
}

// one wave per occupied cell o: every PS cell c with d2(c, o) < r2 gets o in its list
template <bool FILL>
__global__ __launch_bounds__(kBS) void k_gs_reach(GsSpaceDev S, const int32_t* __restrict__ votes,
                                                  int steps, float r2, uint32_t* reach,
                                                  const uint32_t* __restrict__ off, uint32_t* cur,
                                                  uint64_t* __restrict__ keys,
                                                  unsigned long long* cnt) {
  const int lane = threadIdx.x & 63;
  const int32_t o = blockIdx.x * (kBS / 64) + (threadIdx.x >> 6);
  if (o >= S.cells || votes[o] == 0) return;
  if (!FILL && lane == 0) atomicAdd(&cnt[kGsOccupied], 1ull);
  const int32_t co = S.coord[o];
  const int oi = co >> 20, oj = (co >> 10) & 1023, ok = co & 1023;
  const float ox = S.px[o], oy = S.py[o], oz = S.pz[o];
  const int i0 = max(oi - steps, 0), j0 = max(oj - steps, 0), k0 = max(ok - steps, 0);
  const int ni = min(oi + steps, S.size - 1) - i0 + 1, nj = min(oj + steps, S.size - 1) - j0 + 1,
            nk = min(ok + steps, S.size - 1) - k0 + 1;
  const int total = ni * nj * nk;  // <= 512^3
  unsigned long long mine = 0;
  for (int t = lane; t < total; t += 64) {
    const int k = k0 + t % nk, j = j0 + (t / nk) % nj, i = i0 + t / (nk * nj);
    const int32_t c = S.table[(i * S.size + j) * S.size + k];
    if (c < 0) continue;
    // the search runs from c: d = query - point = c - o
    const float dd = gs::d2(S.px[c], S.py[c], S.pz[c], ox, oy, oz);
    if (!(dd < r2)) continue;
    if (FILL)
      keys[(size_t)off[c] + atomicAdd(&cur[c], 1u)] = gs::make_key(dd, o);
    else
      atomicAdd(&reach[c], 1u);
    ++mine;
  }
  if (!FILL) {
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) mine += __shfl_xor(mine, sft, 64);
    if (lane == 0 && mine) atomicAdd(&cnt[kGsPairs], mine);
  }
}

// one wave per PS cell
__global__ __launch_bounds__(64) void k_gs_filter(GsSpaceDev S, const int32_t* __restrict__ votes,
                                                  const uint32_t* __restrict__ reach,
                                                  const uint32_t* __restrict__ off,
                                                  const uint64_t* __restrict__ keys,
                                                  float* terms, float std_dev,
                                                  int32_t* __restrict__ out) {
  const int lane = threadIdx.x;
  const int32_t c = blockIdx.x;
  const int m = (int)reach[c];
  if (m == 0) {
    if (lane == 0) out[c] = 0;
    return;
  }
  const uint64_t* K = keys + off[c];
  float* T = terms + off[c];
  if (m <= 64 * kSortRegs) {
    uint64_t v[kSortRegs];
#pragma unroll
    for (int j = 0; j < kSortRegs; ++j) {
      const int e = lane + 64 * j;
      v[j] = e < m ? K[e] : gs::kNoKey;
    }
    wave_bitonic<kSortRegs>(v);
#pragma unroll
    for (int j = 0; j < kSortRegs; ++j) {
      const int e = lane + 64 * j;
      if (e < m) T[e] = gs::filter_term(gs::key_d2(v[j]), votes[gs::key_index(v[j])], std_dev);
    }
  } else {
    // the keys are distinct (the index is part of them): a key's rank is its sorted position
    for (int e = lane; e < m; e += 64) {
      const uint64_t k = K[e];
      int rank = 0;
      for (int t = 0; t < m; ++t) rank += K[t] < k ? 1 : 0;
      T[rank] = gs::filter_term(gs::key_d2(k), votes[gs::key_index(k)], std_dev);
    }
  }
  __threadfence_block();
  __syncthreads();
  float G = 0.0f;
  for (int e0 = 0; e0 < m; e0 += 64) {
    const float t = e0 + lane < m ? T[e0 + lane] : 0.0f;
    const int here = min(64, m - e0);
    for (int k = 0; k < here; ++k) G = G + __shfl(t, k, 64);
  }
  if (lane == 0) out[c] = gs::filtered_vote(G);
}

__global__ __launch_bounds__(kBS) void k_gs_label(const float* __restrict__ X,
                                                  const float* __restrict__ Y,
                                                  const float* __restrict__ Z, int n,
                                                  const int32_t* __restrict__ cell_of_point,
                                                  const int32_t* __restrict__ sink,
                                                  int32_t* __restrict__ label, uint32_t* total) {
  const int i = blockIdx.x * kBS + threadIdx.x;
  int lab = -1;
  if (i < n) {
    const int32_t c = cell_of_point[i];
    if (c >= 0 && gs::finite3(X[i], Y[i], Z[i])) lab = sink[c];
    label[i] = lab;
  }
  wave_count(lab >= 0, lab, total);
}

__global__ __launch_bounds__(kBS) void k_gs_cc_init(const int32_t* __restrict__ sidx,
                                                    const int32_t* __restrict__ label, int n,
                                                    int32_t* __restrict__ lab_s,
                                                    int32_t* __restrict__ parent,
                                                    uint32_t* __restrict__ size) {
  const int u = blockIdx.x * kBS + threadIdx.x;
  if (u >= n) return;
  lab_s[u] = label[sidx[u]];
  parent[u] = u;
  size[u] = 0;
}

// k_cc_hook (postprocess.hip) between equal labels
__global__ __launch_bounds__(kBS) void k_gs_cc_hook(const float* __restrict__ sx,
                                                    const float* __restrict__ sy,
                                                    const float* __restrict__ sz, int n, GridDesc G,
                                                    const uint32_t* __restrict__ tkeys,
                                                    const int2* __restrict__ trange, uint32_t tmask,
                                                    float r2, const int32_t* __restrict__ lab_s,
                                                    int32_t* parent) {
  const int u = blockIdx.x * kBS + threadIdx.x;
  if (u >= n) return;
  const int32_t lab = lab_s[u];
  if (lab < 0) return;
  const float qx = sx[u], qy = sy[u], qz = sz[u];
  const int cx = cell_of(qx, G.lo[0], G.inv_cell, G.g[0]);
  const int cy = cell_of(qy, G.lo[1], G.inv_cell, G.g[1]);
  const int cz = cell_of(qz, G.lo[2], G.inv_cell, G.g[2]);
  for (int z = max(cz - 1, 0); z <= min(cz + 1, G.g[2] - 1); ++z)
    for (int y = max(cy - 1, 0); y <= min(cy + 1, G.g[1] - 1); ++y)
      for (int x = max(cx - 1, 0); x <= min(cx + 1, G.g[0] - 1); ++x) {
        const int2 rg = cell_range(tkeys, trange, tmask, cell_key(G, x, y, z));
        const int end = min(rg.y, u);  // each undirected edge once: v < u
        for (int v = rg.x; v < end; ++v) {
          if (lab_s[v] != lab) continue;
          if (!(flann_d2(qx, qy, qz, sx[v], sy[v], sz[v]) < r2)) continue;
          uf_unite(parent, u, v);
        }
      }
}

__global__ __launch_bounds__(kBS) void k_gs_cc_count(int32_t* parent, int n,
                                                     const int32_t* __restrict__ lab_s,
                                                     uint32_t* size) {
  const int u = blockIdx.x * kBS + threadIdx.x;
  const bool on = u < n && lab_s[u] >= 0;
  const int r = on ? uf_find(parent, u) : -1;
  wave_count(on, r, size);
}

__global__ __launch_bounds__(kBS) void k_gs_keys(
    const int32_t* __restrict__ sidx, int n, const int32_t* __restrict__ lab_s,
    const int32_t* __restrict__ parent, const uint32_t* __restrict__ size,
    const uint32_t* __restrict__ total, const int32_t* __restrict__ cell_of_point,
    const int32_t* __restrict__ sink_rank, int32_t n_sinks, long long t_single,
    int32_t* __restrict__ root_of, uint64_t* __restrict__ key1, int32_t* __restrict__ ids,
    unsigned long long* cnt) {
  const int u = blockIdx.x * kBS + threadIdx.x;
  bool kept = false;
  if (u < n) {
    const int32_t p = sidx[u];
    int r = u;  // read-only walk: every chain ends at its final root once the hooks are done
    while (parent[r] != r) r = parent[r];
    const int32_t lab = lab_s[u];
    kept = lab >= 0 && (long long)total[lab] >= t_single &&
           2ll * (long long)size[r] - 1ll >= t_single;
    root_of[p] = r;
    ids[p] = p;
    key1[p] = kept ? ((uint64_t)(uint32_t)sink_rank[lab] << 32) | (uint32_t)cell_of_point[p]
                   : (uint64_t)(uint32_t)n_sinks << 32;
  }
  const uint64_t m = __ballot(kept);
  if ((threadIdx.x & 63) == 0 && m) atomicAdd(&cnt[kGsKept], (unsigned long long)__popcll(m));
}

__global__ __launch_bounds__(kBS) void k_gs_fill_i32(int32_t* __restrict__ a, int n, int32_t v) {
  const int i = blockIdx.x * kBS + threadIdx.x;
  if (i < n) a[i] = v;
}

__global__ __launch_bounds__(kBS) void k_gs_first(const int32_t* __restrict__ ids, int nk,
                                                  const int32_t* __restrict__ root_of,
                                                  int32_t* first) {
  const int pos = blockIdx.x * kBS + threadIdx.x;
  if (pos < nk) atomicMin(&first[root_of[ids[pos]]], pos);
}

__global__ __launch_bounds__(kBS) void k_gs_key2(const int32_t* __restrict__ ids, int nk,
                                                 const int32_t* __restrict__ root_of,
                                                 const int32_t* __restrict__ first,
                                                 uint32_t* __restrict__ key2) {
  const int pos = blockIdx.x * kBS + threadIdx.x;
  if (pos < nk) key2[pos] = (uint32_t)first[root_of[ids[pos]]];
}

__global__ __launch_bounds__(kBS) void k_gs_heads(const uint32_t* __restrict__ key2, int nk,
                                                  uint8_t* __restrict__ heads) {
  const int j = blockIdx.x * kBS + threadIdx.x;
  if (j < nk) heads[j] = j == 0 || key2[j] != key2[j - 1] ? 1 : 0;
}

}  // namespace

void launch_gs_vote(const GsSpaceDev& S, const float4* nrm, int n, int32_t* cell_of_point,
                    int32_t* votes, int32_t* queue, unsigned long long* cnt, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gs_vote, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, S, nrm, n, cell_of_point,
                     votes, queue, cnt);
}

void launch_gs_vote_all(const GsSpaceDev& S, const float4* nrm, const int32_t* queue,
                        const unsigned long long* cnt, int32_t* cell_of_point, int32_t* votes,
                        int num_cus, hipStream_t s) {
  hipLaunchKernelGGL(k_gs_vote_all, dim3(num_cus * 8), dim3(kBS), 0, s, S, nrm, queue, cnt,
                     cell_of_point, votes);
}

void launch_gs_reach(const GsSpaceDev& S, const int32_t* votes, int steps, float r2,
                     uint32_t* reach, const uint32_t* off, uint32_t* cur, uint64_t* keys,
                     unsigned long long* cnt, hipStream_t s) {
  if (S.cells <= 0) return;
  const dim3 g(cdiv(S.cells, kBS / 64));
  if (keys)
    hipLaunchKernelGGL(k_gs_reach<true>, g, dim3(kBS), 0, s, S, votes, steps, r2, reach, off, cur,
                       keys, cnt);
  else
    hipLaunchKernelGGL(k_gs_reach<false>, g, dim3(kBS), 0, s, S, votes, steps, r2, reach, off, cur,
                       keys, cnt);
}

size_t gs_scan_tmp_bytes(int32_t cells) {
  size_t t = 0;
  (void)hipcub::DeviceScan::ExclusiveSum(nullptr, t, (const uint32_t*)nullptr, (uint32_t*)nullptr,
                                         cells);
  return t;
}

hipError_t launch_gs_scan(const uint32_t* reach, uint32_t* off, int32_t cells, void* tmp,
                          size_t tmp_bytes, hipStream_t s) {
  size_t t = tmp_bytes;
  return hipcub::DeviceScan::ExclusiveSum(tmp, t, reach, off, cells, s);
}

void launch_gs_filter(const GsSpaceDev& S, const int32_t* votes, const uint32_t* reach,
                      const uint32_t* off, uint64_t* keys, float* terms, float std_dev,
                      int32_t* out, hipStream_t s) {
  if (S.cells <= 0) return;
  hipLaunchKernelGGL(k_gs_filter, dim3(S.cells), dim3(64), 0, s, S, votes, reach, off, keys, terms,
                     std_dev, out);
}

void launch_gs_label(const float* X, const float* Y, const float* Z, int n,
                     const int32_t* cell_of_point, const int32_t* sink, int32_t* label,
                     uint32_t* total, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gs_label, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, X, Y, Z, n, cell_of_point,
                     sink, label, total);
}

void launch_gs_cc(const GridDesc& G, const GridBufs& B, int n, float r2, const int32_t* label,
                  int32_t* lab_s, int32_t* parent, uint32_t* size, hipStream_t s) {
  if (n <= 0) return;
  const dim3 g(cdiv(n, kBS)), b(kBS);
  hipLaunchKernelGGL(k_gs_cc_init, g, b, 0, s, B.idx_out, label, n, lab_s, parent, size);
  hipLaunchKernelGGL(k_gs_cc_hook, g, b, 0, s, B.sx, B.sy, B.sz, n, G, B.tkeys, B.trange, B.tmask,
                     r2, lab_s, parent);
  hipLaunchKernelGGL(k_gs_cc_count, g, b, 0, s, parent, n, lab_s, size);
}

void launch_gs_keys(const GridBufs& B, int n, const int32_t* lab_s, const int32_t* parent,
                    const uint32_t* size, const uint32_t* total, const int32_t* cell_of_point,
                    const int32_t* sink_rank, int32_t n_sinks, int64_t t_single, int32_t* root_of,
                    uint64_t* key1, int32_t* ids, unsigned long long* cnt, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(k_gs_keys, dim3(cdiv(n, kBS)), dim3(kBS), 0, s, B.idx_out, n, lab_s, parent,
                     size, total, cell_of_point, sink_rank, n_sinks, (long long)t_single, root_of,
                     key1, ids, cnt);
}

size_t gs_sort_tmp_bytes(int n) {
  size_t a = 0, b = 0, c = 0;
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, a, (const uint64_t*)nullptr,
                                           (uint64_t*)nullptr, (const int32_t*)nullptr,
                                           (int32_t*)nullptr, n);
  (void)hipcub::DeviceRadixSort::SortPairs(nullptr, b, (const uint32_t*)nullptr,
                                           (uint32_t*)nullptr, (const int32_t*)nullptr,
                                           (int32_t*)nullptr, n);
  (void)hipcub::DeviceSelect::Flagged(nullptr, c, hipcub::CountingInputIterator<int32_t>(0),
                                      (const uint8_t*)nullptr, (int32_t*)nullptr,
                                      (int32_t*)nullptr, n);
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

hipError_t launch_gs_sort_list(const uint64_t* key_in, uint64_t* key_out, const int32_t* ids_in,
                               int32_t* ids_out, int n, int end_bit, void* tmp, size_t tmp_bytes,
                               hipStream_t s) {
  size_t t = tmp_bytes;
  return hipcub::DeviceRadixSort::SortPairs(tmp, t, key_in, key_out, ids_in, ids_out, n, 0, end_bit,
                                            s);
}

hipError_t launch_gs_order(const int32_t* ids, int nk, int n, const int32_t* root_of,
                           int32_t* first, uint32_t* key2, uint32_t* key2_out, int32_t* ids_out,
                           uint8_t* heads, int32_t* offs, int32_t* n_planes, void* tmp,
                           size_t tmp_bytes, hipStream_t s) {
  if (nk <= 0) return hipSuccess;
  const dim3 g(cdiv(nk, kBS)), b(kBS);
  hipLaunchKernelGGL(k_gs_fill_i32, dim3(cdiv(n, kBS)), b, 0, s, first, n, INT32_MAX);
  hipLaunchKernelGGL(k_gs_first, g, b, 0, s, ids, nk, root_of, first);
  hipLaunchKernelGGL(k_gs_key2, g, b, 0, s, ids, nk, root_of, first, key2);
  int bits = 1;
  while (bits < 32 && (1ll << bits) < (long long)nk) ++bits;
  size_t t = tmp_bytes;
  hipError_t e = hipcub::DeviceRadixSort::SortPairs(tmp, t, key2, key2_out, ids, ids_out, nk, 0,
                                                    bits, s);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(k_gs_heads, g, b, 0, s, key2_out, nk, heads);
  t = tmp_bytes;
  e = hipcub::DeviceSelect::Flagged(tmp, t, hipcub::CountingInputIterator<int32_t>(0), heads, offs,
                                    n_planes, nk, s);
  if (e != hipSuccess) return e;
  return hipGetLastError();
}

}  // namespace dlg
