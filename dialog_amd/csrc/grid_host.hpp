// grid_host.hpp -- host helpers of the neighbour-search grids (normals_host.cpp), shared by the
// normals, preProcess and postProcessPlanes drivers.
#pragma once

#include "driver.hpp"
#include "grid_model.hpp"
#include "normals.hpp"

namespace dlg {

// bounding box of the finite points of (X, Y, Z)[0..n)
BBox bbox_of(dlg_ctx* c, const float* X, const float* Y, const float* Z, int n);
// points -> device SoA (nw.x/y/z) + bounding box of the finite points
BBox upload_points(dlg_ctx* c, const dlg_points* pts);
// (BBox and make_grid: grid_model.hpp)
// builds grid level `lv` over (X, Y, Z) (default nw.x/y/z); returns the number of occupied
// cells (and the point-weighted mean occupancy sum(occ^2) / n in *pw_occ)
uint32_t build_grid(dlg_ctx* c, int n, const GridDesc& G, int lv, GridBufs* B,
                    const float* X = nullptr, const float* Y = nullptr, const float* Z = nullptr,
                    double* pw_occ = nullptr);
// k-nearest-neighbour grid hierarchy over nw.x/y/z
KnnLevels build_hierarchy(dlg_ctx* c, int n, const BBox& b, int k_nn);
// the hierarchy's plan: level 0 built (cell tuned on the occupancy), the coarser cells recorded;
// build_level() builds a planned level on demand.  build_hierarchy_plan builds `eager_levels`
// levels (all: -1); L.levels is the planned count either way.
struct KnnPlan {
  BBox b;
  int n = 0;
  double cell[kMaxLevels] = {};
  int planned = 0;
};
void build_level(dlg_ctx* c, const KnnPlan& P, KnnLevels& L, int l, const GridBufs* B0);
KnnLevels build_hierarchy_plan(dlg_ctx* c, int n, const BBox& b, int k_nn, KnnPlan* plan,
                               int eager_levels);

}  // namespace dlg
