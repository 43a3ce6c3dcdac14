// shim_icp.cpp -- dialog::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> used the way the
// reference uses pcl::IterativeClosestPoint (PCLViewer.cpp:581-636,
// on_registrationICPAction_triggered: setInputSource, setInputTarget, align into a cloud,
// hasConverged, getFitnessScore, getFinalTransformation).  Compiled and linked by the CPU tests; the
// GPU tests run it on files of raw float32 values:
//   shim_icp <source xyz> <target xyz> <source xyz of the guess run> <guess: 16 floats>
// prints hasConverged, the bits of the final transformation and of the fitness score, a bit
// checksum of the aligned cloud, and the final transformation of align(output, guess).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "dialog/sac_segmentation.hpp"

typedef pcl::PointCloud<pcl::PointXYZ> PointCloudT;

static PointCloudT::Ptr read_cloud(const char* path) {
  PointCloudT::Ptr cloud(new PointCloudT);
  if (FILE* f = std::fopen(path, "rb")) {
    float p[3];
    while (std::fread(p, 4, 3, f) == 3) cloud->push_back(pcl::PointXYZ(p[0], p[1], p[2]));
    std::fclose(f);
  }
  return cloud;
}

static void print_matrix(const char* name, const dialog::Matrix4f& m) {
  std::printf("%s", name);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const float v = m(r, c);
      uint32_t u;
      std::memcpy(&u, &v, 4);
      std::printf(" %u", u);
    }
  std::printf("\n");
}

int main(int argc, char** argv) {
  if (argc < 5) return 2;
  PointCloudT::Ptr cloud_icp = read_cloud(argv[1]);
  PointCloudT::Ptr target_cloud_registration = read_cloud(argv[2]);
  try {
    dialog::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp;
    icp.setInputSource(cloud_icp);
    icp.setInputTarget(target_cloud_registration);
    PointCloudT Final;
    icp.align(Final);
    std::printf("converged %d\n", icp.hasConverged() ? 1 : 0);
    print_matrix("final", icp.getFinalTransformation());
    const double score = icp.getFitnessScore();
    uint64_t sb;
    std::memcpy(&sb, &score, 8);
    std::printf("fitness %llu\n", (unsigned long long)sb);
    unsigned long long chk = 0;
    for (size_t i = 0; i < Final.size(); ++i) {
      const float v[3] = {Final.points[i].x, Final.points[i].y, Final.points[i].z};
      for (int j = 0; j < 3; ++j) {
        uint32_t u;
        std::memcpy(&u, &v[j], 4);
        chk += (unsigned long long)(i * 3 + j + 1) * u;
      }
    }
    std::printf("aligned %zu %llu\n", Final.size(), chk);
    // align(output, guess)
    PointCloudT::Ptr plain = read_cloud(argv[3]);
    dialog::Matrix4f guess;
    if (FILE* f = std::fopen(argv[4], "rb")) {
      if (std::fread(guess.v, 4, 16, f) != 16) return 2;
      std::fclose(f);
    } else {
      return 2;
    }
    dialog::IterativeClosestPoint<pcl::PointXYZ, pcl::PointXYZ> icp2;
    icp2.setInputSource(plain);
    icp2.setInputTarget(target_cloud_registration);
    icp2.setMaximumIterations(10);
    icp2.setMaxCorrespondenceDistance(icp.getMaxCorrespondenceDistance());
    icp2.setTransformationEpsilon(0.0);
    icp2.setEuclideanFitnessEpsilon(icp.getEuclideanFitnessEpsilon());
    PointCloudT out2;
    icp2.align(out2, guess);
    print_matrix("guess", icp2.getFinalTransformation());
  } catch (const std::exception& e) {
    std::fprintf(stderr, "shim_icp: %s\n", e.what());
    return 1;
  }
  return 0;
}
