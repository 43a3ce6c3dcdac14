// gsphere_model.hpp -- the arithmetic of the Gaussian-sphere (normal-space Hough) plane seeds, the
// reference's createPS -> voteForPS -> filtPS -> createGradientField -> rectifySinkFields
// (Dialog/PlaneDetect.h:667-931), for the kernels (gsphere.hip), the host driver (gsphere_host.cpp)
// and the host-only harness (tests/cpp/gsphere_model_san.cpp) alike.  Plain C++ without HIP too;
// build with -ffp-contract=off.
//
// The parameter space (PS) is the set of lattice cubes of edge num_res in [-1, 1)^3 whose eight
// corner norms straddle 1, numbered in enumeration order (x outer, z inner).  A PS cell's point is
// its min corner.  Every search over PS cells is KdTreeFLANN's: the float distance
// ((0 + dx dx) + dy dy) + dz dz, a radius hit when d2 < (float)((double)r * (double)r), hits in
// (d2, index) order, the nearest cell the smallest (d2, index).
//
// First half: what the device shares (cell test, query, distance, kernel weight, the vote's box
// bound).  Second half, host only: the PS with its dense lattice table, the lattice radius search,
// and the two sequential phases (gradient field, sink rectification).
#pragma once

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

#include "host_math.hpp"  // DLG_HD

namespace dlg {
namespace gs {

constexpr float kPi = 3.141592653f;  // the reference's PI and e, as floats
constexpr float kE = 2.7182818f;
constexpr int kMaxSize = 512;   // lattice cells per axis (the dense table has size^3 entries)
constexpr int kBoxHalf = 2;     // the vote searches the (2 kBoxHalf + 1)^3 lattice box first
constexpr uint64_t kNoKey = ~0ull;

DLG_HD inline int lattice_size(float num_res) { return (int)floorf(2.0f / num_res + 0.5f); }
DLG_HD inline float cell_min(int i, float num_res) { return (float)i * num_res - 1.0f; }
DLG_HD inline float norm3(float x, float y, float z) { return sqrtf((x * x + y * y) + z * z); }

// isCubeIntersectWithUnitSphere: the corners are min + length in float
DLG_HD inline bool cube_on_sphere(float x, float y, float z, float len) {
  const float cx[2] = {x, x + len}, cy[2] = {y, y + len}, cz[2] = {z, z + len};
  float mn = FLT_MAX, mx = FLT_MIN;
  for (int a = 0; a < 2; ++a)
    for (int b = 0; b < 2; ++b)
      for (int c = 0; c < 2; ++c) {
        const float nr = norm3(cx[a], cy[b], cz[c]);
        if (nr < mn) mn = nr;
        if (nr > mx) mx = nr;
      }
  return mx >= 1.0f && mn <= 1.0f;
}

DLG_HD inline bool finite3(float x, float y, float z) {
  const float s = (x - x) + (y - y) + (z - z);  // 0 unless a component is NaN or inf
  return s == 0.0f;
}

// voteForPS's query of one normal component
DLG_HD inline float query(float v, float num_res) { return floorf(v / num_res) * num_res; }

// FLANN's L2_Simple from the query q to the point p
DLG_HD inline float d2(float qx, float qy, float qz, float px, float py, float pz) {
  const float ex = qx - px, ey = qy - py, ez = qz - pz;
  return ((0.0f + ex * ex) + ey * ey) + ez * ez;
}

// (d2, index) as one ascending key (d2 >= 0 or +inf, never NaN: its bits order as the floats)
DLG_HD inline uint64_t make_key(float dd, int32_t index) {
  uint32_t b;
#if defined(__HIP_DEVICE_COMPILE__)
  b = __float_as_uint(dd);
#else
  std::memcpy(&b, &dd, 4);
#endif
  return ((uint64_t)b << 32) | (uint32_t)index;
}
DLG_HD inline float key_d2(uint64_t k) {
  const uint32_t b = (uint32_t)(k >> 32);
  float f;
#if defined(__HIP_DEVICE_COMPILE__)
  f = __uint_as_float(b);
#else
  std::memcpy(&f, &b, 4);
#endif
  return f;
}
DLG_HD inline int32_t key_index(uint64_t k) { return (int32_t)(uint32_t)k; }

// gaussianKernal(x, std_dev), returned as the float the reference's `float` return makes of it
DLG_HD inline float weight(float x, float std_dev) {
  const double sigma = (double)std_dev * (double)std_dev;
  const double A = 2.0 * (double)kPi * sigma;
  const double B = (double)x * (double)x / (-2.0 * sigma);
  const double C = pow((double)kE, B);
  return (float)(C / A);
}
// one neighbour's term of filtPS: d = pow(d2, 0.5f) taken as sqrtf
DLG_HD inline float filter_term(float dd, int32_t vote, float std_dev) {
  return weight(sqrtf(dd), std_dev) * (float)vote;
}
DLG_HD inline int32_t filtered_vote(float G) { return (int32_t)floorf(G + 0.5f); }

// ---- the vote's box bound.  The vote goes to the smallest (d2, index) over ALL PS cells.  The
// kernel looks at the lattice box of half width kBoxHalf around c = near_coord(q) per axis.  A cell
// outside the box differs from c by >= kBoxHalf + 1 lattice steps on some axis a, so its distance
// to the query is at least (kBoxHalf + 1) num_res - |q_a - cell_min(c_a)| on that axis.
// axis_reach is that figure; box_proves takes the smallest of the three, takes 4e-6 off for the
// roundings of cell_min (two roundings of values below 2 per position, 3.6e-7 for a pair), of the
// product and of the difference (each relative 2^-24 of values below 3), and (1 - 1e-5) off the
// square for FLANN's own three roundings: a box result strictly below that bound is strictly
// nearer than every cell outside, ties included.  Anything else -- no PS cell in the box, a query
// far outside the lattice (a non-unit normal), an infinite d2 -- goes to the search of all cells.
DLG_HD inline int near_coord(float q, float num_res, int size) {
  const float t = floorf((q + 1.0f) / num_res + 0.5f);
  return !(t > 0.0f) ? 0 : (t >= (float)(size - 1) ? size - 1 : (int)t);
}
DLG_HD inline float axis_reach(float q, int c, float num_res) {
  return (float)(kBoxHalf + 1) * num_res - fabsf(q - cell_min(c, num_res));
}
DLG_HD inline bool box_proves(float best_d2, float reach) {
  const float L = reach - 4e-6f;
  return L > 0.0f && best_d2 < (L * L) * (1.0f - 1e-5f);
}

// ---------------------------------------------------------------------------------------------
// host only

struct Space {
  float num_res = 0.0f;
  int size = 0;
  std::vector<int32_t> table;  // size^3: lattice (i, j, k) -> PS index, -1 when not a PS cell
  std::vector<int32_t> coord;  // per PS cell: i << 20 | j << 10 | k
  std::vector<float> px, py, pz;  // per PS cell: its min corner
  int32_t cells() const { return (int32_t)coord.size(); }
  size_t slot(int i, int j, int k) const { return ((size_t)i * size + j) * size + k; }
};

inline bool valid_res(float num_res) {
  if (!std::isfinite(num_res) || !(num_res > 0.0f)) return false;
  const float s = floorf(2.0f / num_res + 0.5f);
  return s >= 1.0f && s <= (float)kMaxSize;
}

// createPS (table = false: the cells only)
inline Space build_space(float num_res, bool table = true) {
  Space S;
  S.num_res = num_res;
  S.size = lattice_size(num_res);
  const int n = S.size;
  if (table) S.table.assign((size_t)n * n * n, -1);
  for (int i = 0; i < n; ++i)
    for (int j = 0; j < n; ++j)
      for (int k = 0; k < n; ++k) {
        const float x = cell_min(i, num_res), y = cell_min(j, num_res), z = cell_min(k, num_res);
        if (!cube_on_sphere(x, y, z, num_res)) continue;
        if (table) S.table[S.slot(i, j, k)] = S.cells();
        S.coord.push_back(i << 20 | j << 10 | k);
        S.px.push_back(x);
        S.py.push_back(y);
        S.pz.push_back(z);
      }
  return S;
}

inline float radius2(float radius) { return (float)((double)radius * (double)radius); }
// lattice steps that cover `radius` around a cell: a cell more than this many steps away on an
// axis is farther than radius + num_res - 4e-7
inline int reach_steps(float radius, float num_res, int size) {
  const float t = floorf(radius / num_res) + 1.0f;
  return !(t > 0.0f) ? 0 : (t >= (float)size ? size : (int)t);
}

// KdTreeFLANN::radiusSearch from PS cell c over the PS cells: keys (d2, index) ascending
inline void radius_search(const Space& S, int32_t c, float radius, std::vector<uint64_t>& out) {
  out.clear();
  const float r2 = radius2(radius);
  const int K = reach_steps(radius, S.num_res, S.size);
  const int ci = S.coord[c] >> 20, cj = (S.coord[c] >> 10) & 1023, ck = S.coord[c] & 1023;
  const float qx = S.px[c], qy = S.py[c], qz = S.pz[c];
  for (int i = std::max(ci - K, 0); i <= std::min(ci + K, S.size - 1); ++i)
    for (int j = std::max(cj - K, 0); j <= std::min(cj + K, S.size - 1); ++j)
      for (int k = std::max(ck - K, 0); k <= std::min(ck + K, S.size - 1); ++k) {
        const int32_t o = S.table[S.slot(i, j, k)];
        if (o < 0) continue;
        const float dd = d2(qx, qy, qz, S.px[o], S.py[o], S.pz[o]);
        if (dd < r2) out.push_back(make_key(dd, o));
      }
  std::sort(out.begin(), out.end());
}

// the nearest PS cell of a query by looking at every cell (the vote's definition)
inline int32_t nearest_all(const Space& S, float qx, float qy, float qz) {
  uint64_t best = kNoKey;
  for (int32_t o = 0; o < S.cells(); ++o)
    best = std::min(best, make_key(d2(qx, qy, qz, S.px[o], S.py[o], S.pz[o]), o));
  return best == kNoKey ? -1 : key_index(best);
}

// the vote of one normal as the kernel takes it: the box, then nearest_all when the bound fails
// (*fallback says which); -1 for a non-finite normal
inline int32_t vote_cell(const Space& S, float nx, float ny, float nz, bool* fallback = nullptr) {
  if (fallback) *fallback = false;
  if (!finite3(nx, ny, nz)) return -1;
  const float r = S.num_res;
  const float qx = query(nx, r), qy = query(ny, r), qz = query(nz, r);
  const int cx = near_coord(qx, r, S.size), cy = near_coord(qy, r, S.size),
            cz = near_coord(qz, r, S.size);
  uint64_t best = kNoKey;
  for (int i = std::max(cx - kBoxHalf, 0); i <= std::min(cx + kBoxHalf, S.size - 1); ++i)
    for (int j = std::max(cy - kBoxHalf, 0); j <= std::min(cy + kBoxHalf, S.size - 1); ++j)
      for (int k = std::max(cz - kBoxHalf, 0); k <= std::min(cz + kBoxHalf, S.size - 1); ++k) {
        const int32_t o = S.table[S.slot(i, j, k)];
        if (o < 0) continue;
        best = std::min(best, make_key(d2(qx, qy, qz, cell_min(i, r), cell_min(j, r),
                                          cell_min(k, r)), o));
      }
  const float reach = std::min(axis_reach(qx, cx, r), std::min(axis_reach(qy, cy, r),
                                                               axis_reach(qz, cz, r)));
  if (best != kNoKey && box_proves(key_d2(best), reach)) return key_index(best);
  if (fallback) *fallback = true;
  return nearest_all(S, qx, qy, qz);
}

// filtPS of one cell on the host (the kernel's arithmetic; zero-vote neighbours add nothing)
inline int32_t filter_cell(const Space& S, const int32_t* vote, int32_t c, float std_dev,
                           std::vector<uint64_t>& scratch) {
  radius_search(S, c, (float)(3.0 * std_dev), scratch);
  float G = 0.0f;
  for (uint64_t k : scratch) {
    const int32_t v = vote[key_index(k)];
    if (v != 0) G += filter_term(key_d2(k), v, std_dev);
  }
  return filtered_vote(G);
}

struct Sink {
  int32_t index;
  int64_t vote_num;
};

// createGradientField.  vote: the filtered votes; raw: the points of each cell.  findMaxVoteInPS
// (the unassigned cell of the largest non-zero vote, the first of equals) is a walk down the cells
// sorted by (vote descending, index ascending): votes do not change here and a cell is assigned
// once.  Returns the kept sinks in order; sink_init per cell.
inline std::vector<Sink> gradient_field(const Space& S, const int32_t* vote, const int32_t* raw,
                                        float radius, int32_t t_vote_num,
                                        std::vector<int32_t>& sink_init) {
  const int32_t n = S.cells();
  sink_init.assign((size_t)n, -1);
  std::vector<int32_t> order;
  for (int32_t c = 0; c < n; ++c)
    if (vote[c] != 0 && vote[c] > -1) order.push_back(c);
  std::stable_sort(order.begin(), order.end(),
                   [&](int32_t a, int32_t b) { return vote[a] > vote[b]; });
  std::vector<Sink> sinks;
  std::vector<int32_t> Q;
  std::vector<uint64_t> hits;
  for (int32_t s : order) {
    if (sink_init[s] != -1) continue;
    sink_init[s] = s;
    Sink sp{s, (int64_t)raw[s]};
    Q.clear();
    Q.push_back(s);
    for (size_t head = 0; head < Q.size(); ++head) {
      const int32_t cur = Q[head];
      radius_search(S, cur, radius, hits);
      for (size_t i = 1; i < hits.size(); ++i) {  // (the first hit is skipped, as the reference)
        const int32_t o = key_index(hits[i]);
        if (vote[o] == 0) continue;
        if (vote[o] > vote[cur]) continue;
        if (sink_init[o] == -1) {
          sink_init[o] = s;
          sp.vote_num += raw[o];
          Q.push_back(o);
        }
      }
    }
    if (sp.vote_num > (int64_t)t_vote_num) sinks.push_back(sp);
  }
  return sinks;
}

// rectifySinkFields' largest radius: 2 sin(dev_threshold_rad / 2) in float; the sine is the double
// one rounded to float
inline float rectify_radius_max(float dev_threshold) {
  const float rad = dev_threshold * kPi / 180.0f;
  return (float)std::sin((double)(rad * 0.5f)) * 2.0f;
}

// rectifySinkFields: sink per cell.  delta_radius must be > 0 (the reference's loop does not end
// otherwise).
inline void rectify_sinks(const Space& S, const std::vector<Sink>& sinks,
                          const std::vector<int32_t>& sink_init, float radius_base,
                          float delta_radius, float s_threshold, float dev_threshold,
                          std::vector<int32_t>& sink) {
  sink.assign((size_t)S.cells(), -1);
  const float rmax = rectify_radius_max(dev_threshold);
  std::vector<uint64_t> hits;
  for (const Sink& sp : sinks) {
    float radius = radius_base;
    while (true) {
      if (radius > rmax) break;
      float s_total = 0.0f, s_sink = 0.0f;
      radius_search(S, sp.index, radius, hits);
      for (uint64_t k : hits) {
        ++s_total;
        if (sink_init[key_index(k)] == sp.index) ++s_sink;
      }
      if (s_sink / s_total < s_threshold) break;
      for (uint64_t k : hits) {
        const int32_t o = key_index(k);
        if (sink_init[o] == sp.index && sink[o] == -1) sink[o] = sp.index;
      }
      radius += delta_radius;
    }
  }
}
}  // namespace gs
}  // namespace dlg
