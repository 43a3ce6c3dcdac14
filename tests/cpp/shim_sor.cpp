// shim_sor.cpp -- dialog::StatisticalOutlierRemoval<pcl::PointXYZ> used the way the reference uses
// pcl::StatisticalOutlierRemoval (PCLViewer.cpp:334-358: setInputCloud, setMeanK,
// setStddevMulThresh, filter into a new cloud that then replaces source_cloud).  Compiled and
// linked by the CPU tests; the GPU tests run it on a file of raw float32 xyz triples:
//   shim_sor <file> <mean_k> <stddev_mul>
// prints the sizes, the threshold and checksums of the kept and removed index lists.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "dialog/sac_segmentation.hpp"

static unsigned long long list_sum(const std::vector<int>& v) {
  unsigned long long s = 0;
  for (size_t i = 0; i < v.size(); ++i) s += (unsigned long long)(i + 1) * (unsigned)v[i];
  return s;
}

int main(int argc, char** argv) {
  if (argc < 4) return 2;
  pcl::PointCloud<pcl::PointXYZ>::Ptr source_cloud(new pcl::PointCloud<pcl::PointXYZ>);
  if (FILE* f = std::fopen(argv[1], "rb")) {
    float p[3];
    while (std::fread(p, 4, 3, f) == 3) source_cloud->push_back(pcl::PointXYZ(p[0], p[1], p[2]));
    std::fclose(f);
  } else {
    return 2;
  }
  const size_t n_in = source_cloud->size();
  try {
    dialog::StatisticalOutlierRemoval<pcl::PointXYZ> sor;
    sor.setInputCloud(source_cloud);
    sor.setMeanK(std::atoi(argv[2]));
    sor.setStddevMulThresh(std::atof(argv[3]));
    std::vector<int> kept;
    sor.filter(kept);
    const std::vector<int> removed = sor.getRemovedIndices();
    std::printf("lists %zu %zu %zu %llu %llu\n", n_in, kept.size(), removed.size(), list_sum(kept),
                list_sum(removed));
    std::printf("threshold %a\n", sor.lastStats().threshold);
    // into the cloud it reads, as the reference's assignment to source_cloud amounts to
    sor.filter(*source_cloud);
    if (source_cloud->size() != kept.size() || source_cloud->height != 1) return 1;
    std::printf("cloud %zu %d\n", source_cloud->size(), (int)source_cloud->is_dense);
    // the complement
    dialog::StatisticalOutlierRemoval<pcl::PointXYZ> neg;
    neg.setInputCloud(source_cloud);
    neg.setMeanK(std::atoi(argv[2]));
    neg.setStddevMulThresh(std::atof(argv[3]));
    neg.setNegative(true);
    std::vector<int> a;
    neg.filter(a);
    if (a.size() + neg.getRemovedIndices().size() != source_cloud->size()) return 1;
    std::printf("negative %zu %zu\n", a.size(), neg.getRemovedIndices().size());
    // an empty index list: nothing kept, nothing removed
    neg.setIndices(std::vector<int>());
    neg.filter(a);
    if (!a.empty() || !neg.getRemovedIndices().empty()) return 1;
    std::printf("empty 0\n");
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "dialog error %d: %s\n", (int)e.status, e.what());
    return e.status == DLG_ERR_NO_DEVICE ? 0 : 1;
  }
  return 0;
}
