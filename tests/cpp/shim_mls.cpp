// shim_mls.cpp -- dialog::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> used the way the
// reference uses pcl::MovingLeastSquares (PCLViewer.cpp:387-423, on_rebuildPlaneAction_triggered:
// setComputeNormals(true), setInputCloud, setPolynomialFit(true), setSearchMethod, setSearchRadius,
// process into a PointNormal cloud whose x, y, z then replace source_cloud).  Compiled and linked
// by the CPU tests; the GPU tests run it on a file of raw float32 xyz triples:
//   shim_mls <file> <radius>
// prints the sizes and bit checksums of the smoothed positions, the normals and the indices.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "dialog/sac_segmentation.hpp"

#ifndef DIALOG_HAVE_PCL
namespace pcl {
namespace search {
template <typename PointT>
struct KdTree {
  typedef std::shared_ptr<KdTree<PointT>> Ptr;
};
}  // namespace search
}  // namespace pcl
#endif

static unsigned long long bits_sum(const float* v, size_t n, size_t row) {
  unsigned long long s = 0;
  for (size_t i = 0; i < n; ++i) {
    uint32_t u;
    std::memcpy(&u, v + i, 4);
    s += (unsigned long long)(row * 7 + i + 1) * u;
  }
  return s;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  typedef pcl::PointCloud<pcl::PointXYZ> PointCloudT;
  PointCloudT::Ptr source_cloud(new PointCloudT);
  if (FILE* f = std::fopen(argv[1], "rb")) {
    float p[3];
    while (std::fread(p, 4, 3, f) == 3) source_cloud->push_back(pcl::PointXYZ(p[0], p[1], p[2]));
    std::fclose(f);
  } else {
    return 2;
  }
  const size_t n_in = source_cloud->size();
  try {
    pcl::search::KdTree<pcl::PointXYZ>::Ptr treerebuild(new pcl::search::KdTree<pcl::PointXYZ>);
    PointCloudT::Ptr mls_cloud(new PointCloudT);
    pcl::PointCloud<pcl::PointNormal> mls_points;
    dialog::MovingLeastSquares<pcl::PointXYZ, pcl::PointNormal> mls;
    mls.setComputeNormals(true);
    mls.setInputCloud(source_cloud);
    mls.setPolynomialFit(true);
    mls.setSearchMethod(treerebuild);
    const float felta = (float)std::atof(argv[2]);
    mls.setSearchRadius(felta);
    mls.process(mls_points);
    mls_cloud->points.resize(mls_points.size());
    mls_cloud->width = (uint32_t)mls_points.size();
    unsigned long long sp = 0, sn = 0, si = 0;
    const std::vector<int>& src = mls.getCorrespondingIndices()->indices;
    if (src.size() != mls_points.size() || mls_points.height != 1) return 1;
    for (size_t i = 0; i < mls_points.points.size(); ++i) {
      mls_cloud->points[i].x = mls_points.points[i].x;
      mls_cloud->points[i].y = mls_points.points[i].y;
      mls_cloud->points[i].z = mls_points.points[i].z;
      sp += bits_sum(&mls_points.points[i].x, 3, i);
      sn += bits_sum(&mls_points.points[i].normal_x, 3, i) +
            bits_sum(&mls_points.points[i].curvature, 1, i);
      si += (unsigned long long)(i + 1) * (unsigned)src[i];
    }
    std::printf("rows %zu %zu %llu %llu %llu\n", n_in, mls_cloud->size(), sp, sn, si);
    const dlg_mls_stats& st = mls.lastStats();
    std::printf("stats %lld %lld %lld %lld %lld\n", (long long)st.n_finite, (long long)st.n_too_few,
                (long long)st.n_plane_only, (long long)st.n_fit_nonfinite,
                (long long)st.max_neighbours);
    source_cloud = mls_cloud;
    // positions only into a PointXYZ cloud, without the polynomial
    dialog::MovingLeastSquares<pcl::PointXYZ, pcl::PointXYZ> plane;
    plane.setInputCloud(source_cloud);
    plane.setSearchRadius(felta);
    PointCloudT flat;
    plane.process(flat);
    std::printf("plane %zu %lld\n", flat.size(), (long long)plane.lastStats().n_plane_only);
    if ((long long)flat.size() != plane.lastStats().n_plane_only) return 1;
    // an empty index list: nothing out
    plane.setIndices(std::vector<int>());
    plane.process(flat);
    if (flat.size() != 0) return 1;
    std::printf("empty 0\n");
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "dialog error %d: %s\n", (int)e.status, e.what());
    return e.status == DLG_ERR_NO_DEVICE ? 0 : 1;
  }
  return 0;
}
