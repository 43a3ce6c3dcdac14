// shim_fpfh.cpp -- dialog::FPFHEstimation<pcl::PointXYZ, pcl::Normal, dialog::FPFHSignature33> used
// the way the reference uses pcl::FPFHEstimation (PCLViewer.cpp:495-543, on "registration": radius
// normals of the cloud, then setInputCloud, setInputNormals, setSearchMethod, setRadiusSearch,
// compute).  Compiled and linked by the CPU tests; the GPU tests run it on a file of raw float32 xyz
// triples:
//   shim_fpfh <file> <normals radius> <fpfh radius>
// prints the sizes, a bit checksum of the descriptors and the call's counts.
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

typedef dialog::FPFHSignature33 FPFH;

static unsigned long long bits_sum(const pcl::PointCloud<FPFH>& f) {
  unsigned long long s = 0;
  for (size_t i = 0; i < f.points.size(); ++i)
    for (size_t b = 0; b < 33; ++b) {
      uint32_t u;
      std::memcpy(&u, &f.points[i].histogram[b], 4);
      s += (unsigned long long)(i * 33 + b + 1) * u;
    }
  return s;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  typedef pcl::PointCloud<pcl::PointXYZ> PointCloudT;
  PointCloudT::Ptr cloud(new PointCloudT);
  if (FILE* f = std::fopen(argv[1], "rb")) {
    float p[3];
    while (std::fread(p, 4, 3, f) == 3) cloud->push_back(pcl::PointXYZ(p[0], p[1], p[2]));
    std::fclose(f);
  } else {
    return 2;
  }
  try {
    pcl::PointCloud<pcl::Normal>::Ptr normals(new pcl::PointCloud<pcl::Normal>);
    dialog::NormalEstimation<pcl::PointXYZ, pcl::Normal> ne;
    ne.setInputCloud(cloud);
    ne.setRadiusSearch(std::atof(argv[2]));
    ne.compute(*normals);
    pcl::search::KdTree<pcl::PointXYZ>::Ptr tree(new pcl::search::KdTree<pcl::PointXYZ>);
    pcl::PointCloud<FPFH>::Ptr fpfhs(new pcl::PointCloud<FPFH>);
    dialog::FPFHEstimation<pcl::PointXYZ, pcl::Normal, FPFH> fpfh;
    fpfh.setInputCloud(cloud);
    fpfh.setInputNormals(normals);
    fpfh.setSearchMethod(tree);
    fpfh.setRadiusSearch(std::atof(argv[3]));
    fpfh.compute(*fpfhs);
    if (fpfhs->size() != cloud->size() || fpfhs->height != 1) return 1;
    const dlg_fpfh_stats& st = fpfh.lastStats();
    std::printf("rows %zu %zu %llu\n", cloud->size(), fpfhs->size(), bits_sum(*fpfhs));
    std::printf("stats %lld %lld %lld %lld %lld %lld\n", (long long)st.n_finite,
                (long long)st.n_nan_rows, (long long)st.n_zero_rows, (long long)st.max_neighbours,
                (long long)st.n_pairs, (long long)st.n_pairs_failed);
    // every third point through setIndices: the same descriptors at those points
    std::vector<int> idx;
    for (size_t i = 0; i < cloud->size(); i += 3) idx.push_back((int)i);
    pcl::PointCloud<FPFH> some;
    fpfh.setIndices(idx);
    fpfh.compute(some);
    if (some.size() != idx.size()) return 1;
    for (size_t k = 0; k < idx.size(); ++k)
      if (std::memcmp(some.points[k].histogram, fpfhs->points[(size_t)idx[k]].histogram, 132))
        return 1;
    std::printf("indices %zu\n", some.size());
    // an empty index list: nothing out
    fpfh.setIndices(std::vector<int>());
    fpfh.compute(some);
    if (some.size() != 0) return 1;
    std::printf("empty 0\n");
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "dialog error %d: %s\n", (int)e.status, e.what());
    return e.status == DLG_ERR_NO_DEVICE ? 0 : 1;
  }
  return 0;
}
