// grid_model.hpp -- the arithmetic of the uniform neighbour-search grid, for the host and the
// device alike: the grid of a bounding box (make_grid), the float map from a coordinate to its
// cell (cell_of) and the k-NN kernels' lower bound of the distance to a neighbouring cell
// (knn_side, knn_bound).  The kernels (normals.hip, sor.hip, icp.hip, mls.hip, postprocess.hip)
// and the host drivers call these; tests/cpp/grid_model_host.cpp drives them without a device.
// Plain C++ without HIP too; build with -ffp-contract=off.
//
// The invariant every search relies on.  cell_of() is t = fl(fl(v - lo) * inv_cell), c = floor(t).
// Each of the two roundings is relative (2^-24), and t < g cells, so |t - t_exact| <= g * 2^-23
// cells for every point of the box: two points' map values are off against each other by at most
//     E(g) = g * 2^-22 cells          (g = the widest axis; 2.4e-4 at 1,024 cells)
// whatever their distance.  (The error does not shrink for close pairs: fl(v - lo) is rounded at
// the magnitude of v - lo, which exceeds that of v itself when the box straddles zero.)
//   * adjacency: two points closer than `cell` have |t_q - t_p| < cell * inv_cell + E.  make_grid
//     sets inv_cell = (1 - shrink) / cell with shrink >= E + 1e-5 (1e-3 up to 3,900 cells), so the
//     difference stays below 1 and the cell indices differ by at most 1 on every axis;
//   * the k-NN bound: a query at fraction f of its cell is at least (f - E) cells from every point
//     of the cell below (and (1 - f - E) from the one above): GridDesc::slack >= E is taken off
//     before the bound is squared (1e-4 up to 390 cells).
// E reaches 1/4 at 2^20 cells, where the shrink costs a third of the cell: make_grid grows the cell
// until no axis has more than kMaxAxisCells = 2^20 cells, as it does for the 2^30 key space.
#pragma once

#include <cmath>
#include <cstdint>

#include "host_math.hpp"  // DLG_HD

namespace dlg {

struct BBox {
  float lo[3], hi[3];
  bool any;
};

// Uniform grid over the cloud's bounding box; cell edge >= the search radius so a radius query
// touches at most the 27 cells around its own.  Cell key = (cz * gy + cy) * gx + cx < ncells
// <= 2^30; key ncells marks a non-finite point (sorted last, never inserted).
struct GridDesc {
  float lo[3];
  float cell;
  float inv_cell;
  int g[3];
  uint32_t ncells;
  int key_bits;
  float slack;  // the map's rounding allowance of the k-NN bound, in cells (>= E(g), above)
};

namespace grid {

constexpr int kMaxAxisCells = 1 << 20;
constexpr double kMaxCells = (double)(1u << 30);

// the map's worst pairwise error E(g) in cells, with 1/16 to spare (the roundings of 1 / inv_cell,
// of 1 - f and of the cast to float are 2^-24 each)
inline double map_error(int gmax) { return ((double)gmax + 1.0) * 0x1p-22 * 1.0625; }

DLG_HD inline float cell_coord(float v, float lo, float inv_cell) { return (v - lo) * inv_cell; }

DLG_HD inline int cell_of(float v, float lo, float inv_cell, int g) {
  int c = (int)floorf(cell_coord(v, lo, inv_cell));
  return c < 0 ? 0 : (c >= g ? g - 1 : c);
}

// ---- the k-NN kernels' bound: per axis the query's distance to the face it shares with the
// neighbour on side d (-1, 0, +1), in units of the map's cell width w = 1 / inv_cell, less the
// map's allowance; the squared sum is scaled by (1 - 1e-5) (FLANN's d2 rounding): never above the
// d2 of a point of that cell.
DLG_HD inline float knn_width(float inv_cell) { return 1.0f / inv_cell; }
// the query's fraction of its own cell c = cell_of(v, ...)
DLG_HD inline float knn_frac(float v, float lo, float inv_cell, int c) {
  return cell_coord(v, lo, inv_cell) - (float)c;
}
DLG_HD inline float knn_side(float f, int d, float w, float slack) {
  const float v = d < 0 ? f : d > 0 ? 1.0f - f : 0.0f;
  return v > slack ? (v - slack) * w : 0.0f;
}
DLG_HD inline float knn_bound(float ex, float ey, float ez) {
  return (ex * ex + ey * ey + ez * ez) * (1.0f - 1e-5f);
}

}  // namespace grid

// grid with cell edge >= `cell`: grown until the key space fits 2^30 cells and no axis has more
// than grid::kMaxAxisCells
inline GridDesc make_grid(const BBox& b, double cell) {
  GridDesc G;
  int gmax = 1;
  for (;;) {
    double tot = 1.0, widest = 1.0;
    for (int k = 0; k < 3; ++k) {
      const double ext = b.any ? (double)b.hi[k] - (double)b.lo[k] : 0.0;
      const double gk = std::floor(ext / cell) + 1.0;
      G.g[k] = (int)(gk < 1e9 ? gk : 1e9);
      tot *= gk;
      widest = gk > widest ? gk : widest;
    }
    if (tot <= grid::kMaxCells && widest <= (double)grid::kMaxAxisCells) {
      gmax = (int)widest;
      break;
    }
    cell *= 1.25;
  }
  for (int k = 0; k < 3; ++k) G.lo[k] = b.any ? b.lo[k] : 0.0f;
  // the allowances of the header comment: 1e-4 and 1e-3 wherever they cover E(g) (up to 390 and
  // 3,900 cells on the widest axis), E(g) itself above
  const double err = grid::map_error(gmax);
  const double slack = err > 1e-4 ? err : 1e-4;
  const double shrink = err + 1e-5 > 1e-3 ? err + 1e-5 : 1e-3;
  G.slack = (float)slack;
  G.inv_cell = (float)((1.0 / cell) * (1.0 - shrink));
  G.cell = (float)(cell * (1.0 - 1e-6));  // guaranteed coverage radius of the 27 cells
  G.ncells = (uint32_t)((uint64_t)G.g[0] * G.g[1] * G.g[2]);
  int bits = 1;
  while (bits < 32 && ((uint64_t)1 << bits) <= (uint64_t)G.ncells) ++bits;
  G.key_bits = bits;
  return G;
}

}  // namespace dlg
