// The axis-constrained models through the C++ host shim (include/dialog/sac_segmentation.hpp),
// written the way PCL is called: setModelType(pcl::SACMODEL_PARALLEL_PLANE), setAxis,
// setEpsAngle, segment.  usage: shim_axis <points.bin> <n>  (n x 3 float32).  Prints
//   coeff <4 hex words>          the shim's refined coefficients
//   inliers <count>
//   same <0|1>                   the C ABI (dlg_ctx_set_axis + dlg_sac_segment_host) gives the
//                                same coefficient bits and inlier list
//   perpendicular_eps0_same_as_plane <0|1>
//   vertical_planes <count>      extractPlanes with ExtractParams::model / axis / eps_angle
// Without a GPU it fails loudly (exit 3 = no device).
#include <dialog/sac_segmentation.hpp>

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static bool same_bits(const std::vector<float>& a, const float* b) {
  return a.size() == 4 && std::memcmp(a.data(), b, 16) == 0;
}

int main(int argc, char** argv) {
  if (argc < 3) return 2;
  const long n = std::atol(argv[2]);
  std::vector<float> xyz(3 * (size_t)n);
  FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(xyz.data(), 12, (size_t)n, f) != (size_t)n) return 2;
  std::fclose(f);
  pcl::PointCloud<pcl::PointXYZ>::Ptr cloud(new pcl::PointCloud<pcl::PointXYZ>);
  for (long i = 0; i < n; ++i) cloud->push_back(pcl::PointXYZ(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]));
  const float axis[3] = {0.0f, 0.0f, 1.0f};
  const double eps = 5.0 * 3.14159265358979323846 / 180.0;
  try {
    dialog::SACSegmentation<pcl::PointXYZ> seg;
    seg.setOptimizeCoefficients(true);
    seg.setModelType(pcl::SACMODEL_PARALLEL_PLANE);
    seg.setMethodType(pcl::SAC_RANSAC);
    seg.setDistanceThreshold(0.02);
    seg.setAxis(axis);
    seg.setEpsAngle(eps);
    seg.setInputCloud(cloud);
    pcl::PointIndices inliers;
    pcl::ModelCoefficients coeff;
    seg.segment(inliers, coeff);
    if (coeff.values.size() != 4) return 4;
    if (seg.getAxis()[2] != 1.0f || seg.getEpsAngle() != eps) return 5;
    uint32_t w[4];
    std::memcpy(w, coeff.values.data(), 16);
    std::printf("coeff %x %x %x %x\n", w[0], w[1], w[2], w[3]);
    std::printf("inliers %zu\n", inliers.indices.size());
    // the C ABI on the same points
    dialog::Context ctx(0);
    dlg_sac_params prm;
    dlg_sac_params_default(&prm);
    prm.threshold = 0.02;
    prm.model = DLG_SACMODEL_PARALLEL_PLANE;
    dialog::check(dlg_ctx_set_axis(ctx.get(), axis, eps), ctx.get());
    dlg_points pts{&cloud->points[0].x, (int64_t)n, 16};
    std::vector<int32_t> ids((size_t)n);
    float c[4];
    int64_t nin = 0;
    dialog::check(dlg_sac_segment_host(ctx.get(), &pts, nullptr, 0, &prm, c, ids.data(), n, &nin, nullptr),
                  ctx.get());
    bool same = same_bits(coeff.values, c) && (size_t)nin == inliers.indices.size();
    for (int64_t i = 0; same && i < nin; ++i) same = ids[(size_t)i] == inliers.indices[(size_t)i];
    std::printf("same %d\n", same ? 1 : 0);
    // eps 0: the perpendicular model is SACMODEL_PLANE
    pcl::PointIndices in0, in9;
    pcl::ModelCoefficients c0, c9;
    seg.setModelType(pcl::SACMODEL_PLANE);
    seg.segment(in0, c0);
    seg.setModelType(pcl::SACMODEL_PERPENDICULAR_PLANE);
    seg.setEpsAngle(0.0);
    seg.segment(in9, c9);
    std::printf("perpendicular_eps0_same_as_plane %d\n",
                c0.values.size() == 4 && same_bits(c9.values, c0.values.data()) &&
                        in0.indices == in9.indices ? 1 : 0);
    // "the vertical planes only"
    std::vector<dialog::PlaneResult> planes;
    dialog::ExtractParams ep;
    ep.threshold = 0.02;
    ep.min_inliers = 200;
    ep.max_planes = 4;
    ep.max_iterations = 200;
    ep.model = pcl::SACMODEL_PARALLEL_PLANE;
    ep.axis[2] = 1.0f;
    ep.eps_angle = eps;
    dialog::extractPlanes(*cloud, ep, planes);
    size_t vertical = 0;
    for (const dialog::PlaneResult& p : planes) vertical += std::fabs(p.coeff[2]) < 0.1f ? 1 : 0;
    std::printf("vertical_planes %zu of %zu\n", vertical, planes.size());
  } catch (const dialog::Error& e) {
    std::fprintf(stderr, "%s\n", e.what());
    return e.status == DLG_ERR_NO_DEVICE ? 3 : 1;
  }
  return 0;
}
