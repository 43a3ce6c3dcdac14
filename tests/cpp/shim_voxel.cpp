// shim_voxel.cpp -- dialog::VoxelGrid<pcl::PointXYZ> used the way the reference uses
// pcl::VoxelGrid (PCLViewer.cpp:313-332: filter the cloud into itself; :245-253 the same on the
// registration clouds).  Compiled and linked by the CPU tests; the GPU tests run it: it prints
// each filter's sizes and a checksum of the output bits, and checks the map back to the input.
#include <cstdio>
#include <cstring>
#include <memory>

#include "dialog/sac_segmentation.hpp"

// xor of the output's coordinate bit patterns and pads (the test recomputes it from voxel_ref)
static unsigned bits_xor(const pcl::PointCloud<pcl::PointXYZ>& c) {
  unsigned x = 0;
  for (const pcl::PointXYZ& p : c.points) {
    unsigned b[4];
    std::memcpy(b, &p.x, 16);
    x ^= b[0] ^ (b[1] * 3u) ^ (b[2] * 5u) ^ (b[3] * 7u);
  }
  return x;
}

int main() {
  pcl::PointCloud<pcl::PointXYZ>::Ptr source_cloud(new pcl::PointCloud<pcl::PointXYZ>);
  for (int i = 0; i < 4000; ++i)
    source_cloud->push_back(pcl::PointXYZ(0.001f * (float)(i % 100), 0.002f * (float)(i / 100),
                                          0.0005f * (float)(i % 7)));
  const size_t n_in = source_cloud->size();
  try {
    dialog::VoxelGrid<pcl::PointXYZ> sor;
    sor.setInputCloud(source_cloud);
    sor.setLeafSize(0.01f, 0.01f, 0.01f);
    sor.setMinimumPointsNumberPerVoxel(0);
    sor.filter(*source_cloud);  // output aliases the input, as at PCLViewer.cpp:253
    const std::vector<int>& of = sor.getVoxelOfPoint();
    if (of.size() != n_in || source_cloud->height != 1 || !source_cloud->is_dense) return 1;
    for (int v : of)
      if (v < 0 || (size_t)v >= source_cloud->size()) return 1;
    std::printf("first %zu %zu %lld %08x\n", n_in, source_cloud->size(),
                (long long)sor.lastStats().n_voxels, bits_xor(*source_cloud));

    // setIndices + a minimum occupancy
    std::vector<int> idx;
    for (int i = 0; i < (int)source_cloud->size(); i += 2) idx.push_back(i);
    dialog::VoxelGrid<pcl::PointXYZ> sub;
    pcl::PointCloud<pcl::PointXYZ> out;
    sub.setInputCloud(source_cloud);
    sub.setIndices(idx);
    sub.setLeafSize(0.05f, 0.05f, 0.05f);
    sub.setMinimumPointsNumberPerVoxel(2);
    sub.filter(out);
    std::printf("second %zu %zu %u %08x\n", idx.size(), out.size(),
                sub.getMinimumPointsNumberPerVoxel(), bits_xor(out));

    // an empty index list: an empty cloud, as PCL gives
    dialog::VoxelGrid<pcl::PointXYZ> none;
    none.setInputCloud(source_cloud);
    none.setIndices(std::vector<int>());
    none.setLeafSize(0.05f, 0.05f, 0.05f);
    none.filter(out);
    if (out.size() != 0 || !none.getVoxelOfPoint().empty()) return 1;
    std::printf("empty %zu\n", out.size());

    // PCL's "Leaf size is too small": a warning, output = input
    dialog::VoxelGrid<pcl::PointXYZ> tiny;
    tiny.setInputCloud(source_cloud);
    tiny.setLeafSize(1e-7f, 1e-7f, 1e-7f);
    tiny.filter(out);
    if (out.size() != source_cloud->size() || bits_xor(out) != bits_xor(*source_cloud)) return 1;
    std::printf("tiny %zu\n", out.size());
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "dialog error %d: %s\n", (int)e.status, e.what());
    return e.status == DLG_ERR_NO_DEVICE ? 0 : 1;
  }
  return 0;
}
