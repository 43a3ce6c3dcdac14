// shim_sac_ia.cpp -- dialog::SampleConsensusInitialAlignment<pcl::PointXYZ, pcl::PointXYZ,
// dialog::FPFHSignature33> used the way the reference uses pcl::SampleConsensusInitialAlignment
// (PCLViewer.cpp:546-558: setInputSource, setInputTarget, setSourceFeatures, setTargetFeatures,
// align into the source cloud itself, hasConverged, getFitnessScore, getFinalTransformation).
// Compiled and linked by the CPU tests; the GPU tests run it on files of raw float32 values:
//   shim_sac_ia <source xyz> <source rows> <target xyz> <target rows> <iterations> <max distance>
// (rows: 33 floats a point; max distance <= 0: PCL's default).  Prints hasConverged, the bits of the
// final transformation and of the fitness score, and a bit checksum of the aligned cloud.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "dialog/sac_segmentation.hpp"

typedef pcl::PointCloud<pcl::PointXYZ> PointCloudT;
typedef dialog::FPFHSignature33 FPFH;

static PointCloudT::Ptr read_cloud(const char* path) {
  PointCloudT::Ptr cloud(new PointCloudT);
  if (FILE* f = std::fopen(path, "rb")) {
    float p[3];
    while (std::fread(p, 4, 3, f) == 3) cloud->push_back(pcl::PointXYZ(p[0], p[1], p[2]));
    std::fclose(f);
  }
  return cloud;
}

static pcl::PointCloud<FPFH>::Ptr read_rows(const char* path) {
  pcl::PointCloud<FPFH>::Ptr rows(new pcl::PointCloud<FPFH>);
  if (FILE* f = std::fopen(path, "rb")) {
    FPFH r;
    while (std::fread(r.histogram, 4, 33, f) == 33) rows->push_back(r);
    std::fclose(f);
  }
  return rows;
}

int main(int argc, char** argv) {
  if (argc < 7) return 2;
  PointCloudT::Ptr cloud_sac = read_cloud(argv[1]);
  pcl::PointCloud<FPFH>::Ptr fpfhs_src = read_rows(argv[2]);
  PointCloudT::Ptr target_cloud_registration = read_cloud(argv[3]);
  pcl::PointCloud<FPFH>::Ptr fpfhs_tgt = read_rows(argv[4]);
  try {
    dialog::SampleConsensusInitialAlignment<pcl::PointXYZ, pcl::PointXYZ, FPFH> scia;
    scia.setInputSource(cloud_sac);
    scia.setInputTarget(target_cloud_registration);
    scia.setSourceFeatures(fpfhs_src);
    scia.setTargetFeatures(fpfhs_tgt);
    scia.setMaximumIterations(std::atoi(argv[5]));
    if (std::atof(argv[6]) > 0.0) scia.setMaxCorrespondenceDistance(std::atof(argv[6]));
    scia.align(*cloud_sac);
    std::printf("converged %d\n", scia.hasConverged() ? 1 : 0);
    const dialog::Matrix4f sac_trans = scia.getFinalTransformation();
    std::printf("final");
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) {
        const float v = sac_trans(r, c);
        uint32_t u;
        std::memcpy(&u, &v, 4);
        std::printf(" %u", u);
      }
    const double score = scia.getFitnessScore();
    uint64_t sb;
    std::memcpy(&sb, &score, 8);
    std::printf("\nfitness %llu\n", (unsigned long long)sb);
    unsigned long long chk = 0;
    for (size_t i = 0; i < cloud_sac->size(); ++i) {
      const float v[3] = {cloud_sac->points[i].x, cloud_sac->points[i].y, cloud_sac->points[i].z};
      for (int j = 0; j < 3; ++j) {
        uint32_t u;
        std::memcpy(&u, &v[j], 4);
        chk += (unsigned long long)(3 * i + j + 1) * u;
      }
    }
    const dlg_sac_ia_stats& st = scia.lastStats();
    std::printf("aligned %zu %llu\nstats %d %d %d\n", cloud_sac->size(), chk, st.iterations,
                st.best_iteration, st.n_valid);
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "dialog error %d: %s\n", (int)e.status, e.what());
    return e.status == DLG_ERR_NO_DEVICE ? 0 : 1;
  }
  return 0;
}
