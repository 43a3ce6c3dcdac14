// shim_gauss_sphere.cpp -- dialog::segmentPlanesGaussSphere used where the reference calls
// createPS() ... segmentPlanes() (PCLViewer.cpp:1133-1151), with the reference's struct Plane
// (Dialog/HeaderFile.h:81-88) and its globals.  A box corner of three faces with exact outward
// normals: three seed planes, each one face's points in cloud order, points_set alone filled.
// Compiled, linked and run by tests/test_gauss_sphere_gpu.py.
#include <cstdio>
#include <memory>
#include <random>
#include <vector>

#include <dialog/sac_segmentation.hpp>

typedef pcl::PointXYZ PointT;
typedef pcl::PointCloud<PointT> PointCloudT;

struct Triangle_HeadFile {  // HeaderFile.h:74-79
  pcl::PointXYZ p_a, p_b, p_c;
};
struct Plane {  // HeaderFile.h:81-88
  PointCloudT::Ptr border;
  PointCloudT::Ptr points_set;
  pcl::ModelCoefficients coeff;
  std::vector<Triangle_HeadFile> triangles_headfile;
};

PointCloudT::Ptr source_cloud(new PointCloudT);
pcl::PointCloud<pcl::Normal>::Ptr source_normal(new pcl::PointCloud<pcl::Normal>);
std::vector<Plane> plane_clouds;

int main() {
  const int per_face = 1500;
  std::mt19937 g(11);
  std::uniform_real_distribution<float> u(0.f, 1.f);
  for (int f = 0; f < 3; ++f)
    for (int i = 0; i < per_face; ++i) {
      float p[3] = {u(g), u(g), u(g)};
      p[f] = 0.f;
      source_cloud->push_back(PointT(p[0], p[1], p[2]));
      pcl::Normal nr;
      nr.normal_x = f == 0 ? -1.f : 0.f;
      nr.normal_y = f == 1 ? -1.f : 0.f;
      nr.normal_z = f == 2 ? -1.f : 0.f;
      source_normal->push_back(nr);
    }
  dlg_gs_params prm;
  dlg_gs_params_default(&prm);
  prm.num_res = 0.05f;  // config.txt's lattice scaled by 5, the radii with it
  prm.search_radius_create_gradient = 0.15f;
  prm.radius_base = 0.15f;
  prm.delta_radius = 0.05f;
  prm.t_vote_num = 100;
  prm.t_num_of_single_plane = 100;
  try {
    dlg_gs_stats st;
    const size_t added =
        dialog::segmentPlanesGaussSphere(*source_cloud, *source_normal, prm, plane_clouds, nullptr, &st);
    int bad = added == 3 && plane_clouds.size() == 3 && st.n_sinks == 3 ? 0 : 1;
    std::vector<int> seen(3, 0);
    for (const Plane& pl : plane_clouds) {
      if (!pl.points_set || pl.border || !pl.coeff.values.empty()) { ++bad; continue; }
      if ((int)pl.points_set->points.size() != per_face) ++bad;
      int f = -1;
      for (int a = 0; a < 3; ++a) {
        bool flat = true;
        for (const auto& p : pl.points_set->points) flat = flat && (&p.x)[a] == 0.f;
        if (flat) f = a;
      }
      if (f < 0) { ++bad; continue; }
      ++seen[(size_t)f];
      // the face's points in cloud order
      for (size_t i = 0; i < pl.points_set->points.size() && i < (size_t)per_face; ++i) {
        const PointT& a = pl.points_set->points[i];
        const PointT& b = source_cloud->points[(size_t)f * per_face + i];
        if (a.x != b.x || a.y != b.y || a.z != b.z) { ++bad; break; }
      }
    }
    for (int v : seen) bad += v != 1;
    std::printf("planes %zu sinks %lld bad %d%s\n", plane_clouds.size(), (long long)st.n_sinks, bad,
                bad ? "" : " ok");
    return bad ? 1 : 0;
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "dialog error %d: %s\n", (int)e.status, e.what());
    return 1;
  }
}
