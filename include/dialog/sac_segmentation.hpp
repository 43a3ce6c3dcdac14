// dialog/sac_segmentation.hpp -- header-only C++ host shim over the C ABI (dialog_ransac.h).
//
// Keeps the interface the reference's code is written against:
//   * pcl::SACSegmentation<PointT> (setModelType / setMethodType / setDistanceThreshold /
//     setMaxIterations / setProbability / setOptimizeCoefficients / setInputCloud / setIndices /
//     segment(PointIndices&, ModelCoefficients&)), as called at
//     Dialog/SimplifyVerticesSize.cpp:62-67, :86-87 -> dialog::SACSegmentation<PointT>;
//   * the plane-stage slot of Dialog/PlaneDetect.h:667-1355 that fills
//     `plane_clouds` (PlaneDetect.h:100, struct Plane HeaderFile.h:81-88) ->
//     dialog::extractPlanes(cloud, params, planes) (sequential extract-and-remove RANSAC);
//     with SACMODEL_PLANE, or with setAxis / setEpsAngle and SACMODEL_PERPENDICULAR_PLANE /
//     SACMODEL_PARALLEL_PLANE;
//   * pcl::SACSegmentationFromNormals (SACMODEL_NORMAL_PLANE) -> dialog::SACSegmentationFromNormals;
//   * estimateNormal() (PlaneDetect.h:515-545, pcl::NormalEstimationOMP with a radius; k = 20 at
//     PCLViewer.cpp:507-522) -> dialog::NormalEstimation<PointT, pcl::Normal>;
//   * regulateNormal() (PlaneDetect.h:547-665) -> dialog::regulateNormals (first round) and
//     dialog::orientNormalsToBackup (later rounds);
//   * preProcess() (PlaneDetect.h:448-512) -> dialog::preProcess;
//   * pcl::VoxelGrid<PointT> (PCLViewer.cpp:245-253, 283-300, 313-332) -> dialog::VoxelGrid<PointT>;
//   * pcl::StatisticalOutlierRemoval<PointT> (PCLViewer.cpp:334-358) ->
//     dialog::StatisticalOutlierRemoval<PointT>;
//   * pcl::MovingLeastSquares<PointInT, PointOutT> (PCLViewer.cpp:387-423, "rebuild plane") ->
//     dialog::MovingLeastSquares<PointInT, PointOutT>;
//   * pcl::FPFHEstimation<PointInT, PointNT, pcl::FPFHSignature33> (PCLViewer.cpp:524-543, the
//     descriptors of "registration") -> dialog::FPFHEstimation<PointInT, PointNT, PointOutT>.
// With real PCL available define DIALOG_HAVE_PCL before including; otherwise minimal
// layout-identical stand-ins for pcl::PointXYZ (16 B), pcl::Normal (32 B), pcl::PointNormal (48 B),
// pcl::PointCloud, pcl::ModelCoefficients and pcl::PointIndices are declared here.
// PCL failure behaviour is kept: segment() never throws for "no model" -- it prints an error in
// PCL_ERROR style and leaves inliers/coefficients empty.  Device/runtime errors throw
// dialog::Error (there is no CPU fallback).
#pragma once

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../dialog_ransac.h"

#ifdef DIALOG_HAVE_PCL
#include <pcl/ModelCoefficients.h>
#include <pcl/PointIndices.h>
#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/sample_consensus/method_types.h>
#include <pcl/sample_consensus/model_types.h>
#else
namespace pcl {
struct alignas(16) PointXYZ {
  float x, y, z, data_pad;
  PointXYZ() : x(0.f), y(0.f), z(0.f), data_pad(1.f) {}
  PointXYZ(float a, float b, float c) : x(a), y(b), z(c), data_pad(1.f) {}
};
struct alignas(16) Normal {
  float normal_x, normal_y, normal_z, data_pad;
  float curvature, pad_[3];
};
struct alignas(16) PointNormal {
  float x, y, z, data_pad;
  float normal_x, normal_y, normal_z, normal_pad;
  float curvature, pad_[3];
  PointNormal()
      : x(0.f), y(0.f), z(0.f), data_pad(1.f), normal_x(0.f), normal_y(0.f), normal_z(0.f),
        normal_pad(0.f), curvature(0.f), pad_{0.f, 0.f, 0.f} {}
};
template <typename T>
struct PointCloud {
  typedef std::shared_ptr<PointCloud<T>> Ptr;
  typedef std::shared_ptr<const PointCloud<T>> ConstPtr;
  std::vector<T> points;
  uint32_t width = 0, height = 1;
  bool is_dense = true;
  size_t size() const { return points.size(); }
  void push_back(const T& p) { points.push_back(p); width = (uint32_t)points.size(); }
};
struct ModelCoefficients {
  typedef std::shared_ptr<ModelCoefficients> Ptr;
  std::vector<float> values;
};
struct PointIndices {
  typedef std::shared_ptr<PointIndices> Ptr;
  std::vector<int> indices;
};
enum SacModel {
  SACMODEL_PLANE = 0,
  SACMODEL_PERPENDICULAR_PLANE = 9,
  SACMODEL_NORMAL_PLANE = 11,
  SACMODEL_PARALLEL_PLANE = 15
};
static const int SAC_RANSAC = 0;
}  // namespace pcl
#endif

static_assert(sizeof(pcl::PointXYZ) == 16, "pcl::PointXYZ must be 16 bytes (x, y, z, pad)");
static_assert(sizeof(pcl::PointNormal) == 48, "pcl::PointNormal must be 48 bytes");
static_assert((int)pcl::SACMODEL_PERPENDICULAR_PLANE == DLG_SACMODEL_PERPENDICULAR_PLANE &&
                  (int)pcl::SACMODEL_PARALLEL_PLANE == DLG_SACMODEL_PARALLEL_PLANE,
              "pcl::SacModel values are passed to the C ABI as they are");

namespace dialog {

struct Error : std::runtime_error {
  Error(dlg_status s, const std::string& m) : std::runtime_error(m), status(s) {}
  dlg_status status;
};

inline void check(dlg_status s, const dlg_ctx* c) {
  if (s != DLG_OK)
    throw Error(s, std::string(dlg_status_string(s)) + ": " + dlg_last_error(c));
}

// one device context per host thread (RAII)
class Context {
 public:
  explicit Context(int device = 0) { check(dlg_ctx_create(&c_, device), nullptr); }
  ~Context() { dlg_ctx_destroy(c_); }
  Context(const Context&) = delete;
  Context& operator=(const Context&) = delete;
  dlg_ctx* get() const { return c_; }
  static Context& thread_default() {
    thread_local Context ctx(0);
    return ctx;
  }

 private:
  dlg_ctx* c_ = nullptr;
};

template <typename PointT>
class SACSegmentation {
 public:
  typedef typename pcl::PointCloud<PointT>::ConstPtr PointCloudConstPtr;

  explicit SACSegmentation(Context* ctx = nullptr) : ctx_(ctx) { dlg_sac_params_default(&prm_); }

  void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  void setIndices(const pcl::PointIndices::Ptr& idx) { indices_ = idx ? idx->indices : std::vector<int>(); has_idx_ = (bool)idx; }
  void setIndices(const std::vector<int>& idx) { indices_ = idx; has_idx_ = true; }
  void setModelType(int m) { model_ = m; }
  void setMethodType(int m) { method_ = m; }
  void setDistanceThreshold(double t) { prm_.threshold = t; }
  void setMaxIterations(int n) { prm_.max_iterations = n; }
  void setProbability(double p) { prm_.probability = p; }
  void setOptimizeCoefficients(bool b) { prm_.optimize = b ? 1 : 0; }
  // SACMODEL_PERPENDICULAR_PLANE / SACMODEL_PARALLEL_PLANE: the axis (any type with ax[0..2]:
  // float[3], Eigen::Vector3f; not normalised) and the angle in radians (dlg_ctx_set_axis)
  template <typename Vec3>
  void setAxis(const Vec3& ax) { axis_ = {(float)ax[0], (float)ax[1], (float)ax[2]}; }
  std::array<float, 3> getAxis() const { return axis_; }
  void setEpsAngle(double ea) { eps_angle_ = ea; }
  double getEpsAngle() const { return eps_angle_; }
  // extension: DLG_REFIT_PCL (bit-exact with PCL, default) or DLG_REFIT_FAST
  void setRefitMode(int m) { prm_.refit_mode = m; }
  const dlg_sac_stats& lastStats() const { return stats_; }

  void segment(pcl::PointIndices& inliers, pcl::ModelCoefficients& coefficients) {
    inliers.indices.clear();
    coefficients.values.clear();
    if (!input_) {
      std::fprintf(stderr, "[dialog::SACSegmentation::segment] No input dataset given!\n");
      return;
    }
    const bool constrained =
        model_ == pcl::SACMODEL_PERPENDICULAR_PLANE || model_ == pcl::SACMODEL_PARALLEL_PLANE;
    if ((model_ != pcl::SACMODEL_PLANE && !constrained) || method_ != pcl::SAC_RANSAC) {
      std::fprintf(stderr, "[dialog::SACSegmentation::segment] Error initializing the SAC model!\n");
      return;
    }
    prm_.model = model_;  // (pcl::SacModel's values are the C ABI's)
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    if (constrained) check(dlg_ctx_set_axis(c, axis_.data(), eps_angle_), c);
    dlg_points pts{input_->points.empty() ? nullptr : &input_->points[0].x,
                   (int64_t)input_->points.size(), (int64_t)sizeof(PointT)};
    const int64_t n = has_idx_ ? (int64_t)indices_.size() : pts.n;
    std::vector<int32_t> out((size_t)(n > 0 ? n : 1));
    std::vector<int32_t> idx32(indices_.begin(), indices_.end());
    float coeff[4];
    int64_t nin = 0;
    check(dlg_sac_segment_host(c, &pts, has_idx_ ? idx32.data() : nullptr, n, &prm_, coeff,
                               out.data(), (int64_t)out.size(), &nin, &stats_),
          c);
    if (!stats_.has_model) {
      std::fprintf(stderr, "[dialog::SACSegmentation::segment] Error segmenting the model! No solution found.\n");
      return;
    }
    inliers.indices.assign(out.begin(), out.begin() + nin);
    coefficients.values.assign(coeff, coeff + 4);
  }

 protected:
  Context* ctx_;
  dlg_sac_params prm_;
  dlg_sac_stats stats_{};
  PointCloudConstPtr input_;
  std::vector<int> indices_;
  bool has_idx_ = false;
  int model_ = -1, method_ = -1;
  std::array<float, 3> axis_{{0.f, 0.f, 0.f}};
  double eps_angle_ = 0.0;
};

// pcl::SACSegmentationFromNormals<PointT, pcl::Normal>: SACMODEL_NORMAL_PLANE (or PLANE) with the
// input normals (one pcl::Normal per input point; setIndices selects from both)
template <typename PointT, typename PointNT = pcl::Normal>
class SACSegmentationFromNormals : public SACSegmentation<PointT> {
 public:
  typedef typename pcl::PointCloud<PointNT>::ConstPtr NormalsConstPtr;
  explicit SACSegmentationFromNormals(Context* ctx = nullptr) : SACSegmentation<PointT>(ctx) {}
  void setInputNormals(const NormalsConstPtr& normals) { normals_ = normals; }
  void setNormalDistanceWeight(double w) { weight_ = w; }

  void segment(pcl::PointIndices& inliers, pcl::ModelCoefficients& coefficients) {
    if (this->model_ != pcl::SACMODEL_NORMAL_PLANE) {
      SACSegmentation<PointT>::segment(inliers, coefficients);
      return;
    }
    inliers.indices.clear();
    coefficients.values.clear();
    if (!this->input_ || !normals_ || normals_->points.size() != this->input_->points.size()) {
      std::fprintf(stderr, "[dialog::SACSegmentationFromNormals::segment] No input dataset containing normals was given!\n");
      return;
    }
    if (this->method_ != pcl::SAC_RANSAC) {
      std::fprintf(stderr, "[dialog::SACSegmentationFromNormals::segment] Error initializing the SAC model!\n");
      return;
    }
    dlg_ctx* c = (this->ctx_ ? this->ctx_ : &Context::thread_default())->get();
    dlg_points pts{this->input_->points.empty() ? nullptr : &this->input_->points[0].x,
                   (int64_t)this->input_->points.size(), (int64_t)sizeof(PointT)};
    std::vector<int32_t> idx32(this->indices_.begin(), this->indices_.end());
    const int64_t n = this->has_idx_ ? (int64_t)idx32.size() : pts.n;
    dlg_cloud* cl = nullptr;
    check(dlg_cloud_upload(c, &pts, this->has_idx_ ? idx32.data() : nullptr, n, 0, &cl), c);
    std::unique_ptr<dlg_cloud, dlg_status (*)(dlg_cloud*)> guard(cl, dlg_cloud_destroy);
    check(dlg_cloud_set_normals(c, cl, normals_->points.empty() ? nullptr : &normals_->points[0].normal_x,
                                (int64_t)normals_->points.size(), (int64_t)sizeof(PointNT)),
          c);
    dlg_sac_params prm = this->prm_;
    prm.model = DLG_SACMODEL_NORMAL_PLANE;
    prm.normal_distance_weight = weight_;
    std::vector<int32_t> out((size_t)(n > 0 ? n : 1));
    float coeff[4];
    int64_t nin = 0;
    check(dlg_sac_segment(c, cl, &prm, coeff, out.data(), (int64_t)out.size(), &nin, &this->stats_), c);
    if (!this->stats_.has_model) {
      std::fprintf(stderr, "[dialog::SACSegmentationFromNormals::segment] Error segmenting the model! No solution found.\n");
      return;
    }
    inliers.indices.assign(out.begin(), out.begin() + nin);
    coefficients.values.assign(coeff, coeff + 4);
  }

 private:
  NormalsConstPtr normals_;
  double weight_ = 0.1;  // PCL default distance_weight_
};

// pcl::NormalEstimation(OMP)<PointT, pcl::Normal> (estimateNormal(), PlaneDetect.h:515-545)
template <typename PointT, typename PointNT = pcl::Normal>
class NormalEstimation {
 public:
  typedef typename pcl::PointCloud<PointT>::ConstPtr PointCloudConstPtr;
  explicit NormalEstimation(Context* ctx = nullptr) : ctx_(ctx) {}
  void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  void setRadiusSearch(double r) { radius_ = r; k_ = 0; }
  void setKSearch(int k) { k_ = k; radius_ = 0.0; }
  void setViewPoint(float vx, float vy, float vz) { vp_[0] = vx; vp_[1] = vy; vp_[2] = vz; }
  // output: one PointNT per input point (NaN normal/curvature where < 3 neighbours)
  void compute(pcl::PointCloud<PointNT>& output) {
    output.points.clear();
    if (!input_) {
      std::fprintf(stderr, "[dialog::NormalEstimation::compute] No input dataset given!\n");
      return;
    }
    output.points.resize(input_->points.size());
    output.width = (uint32_t)output.points.size();
    output.height = 1;
    if (output.points.empty()) return;
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points pts{&input_->points[0].x, (int64_t)input_->points.size(), (int64_t)sizeof(PointT)};
    check(dlg_estimate_normals(c, &pts, (float)radius_, k_, vp_, &output.points[0].normal_x,
                               (int64_t)sizeof(PointNT)),
          c);
  }

 private:
  Context* ctx_;
  PointCloudConstPtr input_;
  double radius_ = 0.0;
  int k_ = 0;
  float vp_[3] = {0.f, 0.f, 0.f};
};

// regulateNormal() first round (PlaneDetect.h:586-646): returns the number of points reached;
// processed (optional) receives isProcessed[]
template <typename PointT, typename PointNT>
inline int64_t regulateNormals(const pcl::PointCloud<PointT>& cloud, pcl::PointCloud<PointNT>& normals,
                               int64_t selected_point_index, bool is_norm_direction_valid,
                               float r_for_regulate_normal, std::vector<uint8_t>* processed = nullptr,
                               Context* ctx = nullptr) {
  if (normals.points.size() != cloud.points.size()) throw Error(DLG_ERR_INVALID, "normals/cloud size mismatch");
  if (cloud.points.empty()) return 0;
  dlg_ctx* c = (ctx ? ctx : &Context::thread_default())->get();
  dlg_points pts{&cloud.points[0].x, (int64_t)cloud.points.size(), (int64_t)sizeof(PointT)};
  if (processed) processed->assign(cloud.points.size(), 0);
  int64_t count = 0;
  check(dlg_regulate_normals(c, &pts, &normals.points[0].normal_x, (int64_t)sizeof(PointNT),
                             selected_point_index, is_norm_direction_valid ? 1 : 0,
                             r_for_regulate_normal, processed ? processed->data() : nullptr, &count),
        c);
  return count;
}

// regulateNormal() later rounds (PlaneDetect.h:553-584): orientation from the nearest point of
// the backup cloud
template <typename PointT, typename PointNT>
inline void orientNormalsToBackup(const pcl::PointCloud<PointT>& cloud, pcl::PointCloud<PointNT>& normals,
                                  const pcl::PointCloud<PointT>& backup,
                                  const pcl::PointCloud<PointNT>& backup_normals, Context* ctx = nullptr) {
  if (normals.points.size() != cloud.points.size() || backup_normals.points.size() != backup.points.size())
    throw Error(DLG_ERR_INVALID, "normals/cloud size mismatch");
  if (cloud.points.empty()) return;
  dlg_ctx* c = (ctx ? ctx : &Context::thread_default())->get();
  dlg_points pts{&cloud.points[0].x, (int64_t)cloud.points.size(), (int64_t)sizeof(PointT)};
  dlg_points ref{backup.points.empty() ? nullptr : &backup.points[0].x, (int64_t)backup.points.size(),
                 (int64_t)sizeof(PointT)};
  check(dlg_orient_normals_nn(c, &pts, &normals.points[0].normal_x, (int64_t)sizeof(PointNT), &ref,
                              backup_normals.points.empty() ? nullptr : &backup_normals.points[0].normal_x,
                              (int64_t)sizeof(PointNT)),
        c);
}

// preProcess() (PlaneDetect.h:448-512) / removeRedundantPoints (PCLViewer.cpp:781-805): NaN
// removal, optional translation to the centroid (returned in *translation), redundancy removal
// with min_dist_between_points.  out: the kept points (translated); kept_index: their input index.
template <typename PointT>
inline void preProcess(const pcl::PointCloud<PointT>& cloud, bool translate, float min_dist,
                       pcl::PointCloud<PointT>& out, std::vector<int>* kept_index = nullptr,
                       float translation[3] = nullptr, Context* ctx = nullptr) {
  static_assert(sizeof(PointT) == 16, "preProcess writes pcl::PointXYZ records");
  out.points.clear();
  if (kept_index) kept_index->clear();
  if (cloud.points.empty()) return;
  dlg_ctx* c = (ctx ? ctx : &Context::thread_default())->get();
  dlg_points pts{&cloud.points[0].x, (int64_t)cloud.points.size(), (int64_t)sizeof(PointT)};
  out.points.resize(cloud.points.size());
  std::vector<int32_t> idx(cloud.points.size());
  int64_t n = 0;
  float tr[3];
  check(dlg_preprocess(c, &pts, translate ? 1 : 0, min_dist, &out.points[0].x, (int64_t)sizeof(PointT),
                       idx.data(), (int64_t)idx.size(), &n, tr),
        c);
  out.points.resize((size_t)n);
  out.width = (uint32_t)n;
  out.height = 1;
  if (kept_index) kept_index->assign(idx.begin(), idx.begin() + n);
  if (translation) { translation[0] = tr[0]; translation[1] = tr[1]; translation[2] = tr[2]; }
}

// pcl::VoxelGrid<PointT> as the reference calls it (PCLViewer.cpp:245-253, 283-300, 313-332):
// setInputCloud / setIndices / setLeafSize / setMinimumPointsNumberPerVoxel / filter(output), on
// dlg_voxel_grid.  filter() may write the cloud it reads (the reference passes *source_cloud for
// both, :253).  A leaf too small for 32-bit voxel indices: PCL's warning on stderr and output =
// input.  The order of a voxel's points in its sum is list order (PCL's std::sort leaves it
// unspecified).  getVoxelOfPoint(): for every list entry of the last filter(), the
// output point it went into (-1: non-finite, or its voxel had fewer than the minimum points) --
// what maps a plane found on the filtered cloud back to the original points.
template <typename PointT>
class VoxelGrid {
 public:
  typedef typename pcl::PointCloud<PointT>::ConstPtr PointCloudConstPtr;
  explicit VoxelGrid(Context* ctx = nullptr) : ctx_(ctx) {}
  void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  void setIndices(const pcl::PointIndices::Ptr& idx) { indices_ = idx ? idx->indices : std::vector<int>(); has_idx_ = (bool)idx; }
  void setIndices(const std::vector<int>& idx) { indices_ = idx; has_idx_ = true; }
  void setLeafSize(float lx, float ly, float lz) { prm_.leaf[0] = lx; prm_.leaf[1] = ly; prm_.leaf[2] = lz; }
  void setMinimumPointsNumberPerVoxel(unsigned int n) { prm_.min_points_per_voxel = (int32_t)n; }
  unsigned int getMinimumPointsNumberPerVoxel() const { return (unsigned int)prm_.min_points_per_voxel; }
  const std::vector<int>& getVoxelOfPoint() const { return voxel_of_; }
  const dlg_voxel_stats& lastStats() const { return stats_; }

  void filter(pcl::PointCloud<PointT>& output) {
    static_assert(sizeof(PointT) == 16, "VoxelGrid writes pcl::PointXYZ records");
    voxel_of_.clear();
    if (!input_) {
      std::fprintf(stderr, "[dialog::VoxelGrid::filter] No input dataset given!\n");
      output.points.clear();
      output.width = 0;
      output.height = 1;
      return;
    }
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points pts{input_->points.empty() ? nullptr : &input_->points[0].x,
                   (int64_t)input_->points.size(), (int64_t)sizeof(PointT)};
    std::vector<int32_t> idx32(indices_.begin(), indices_.end());
    const int64_t n = has_idx_ ? (int64_t)idx32.size() : pts.n;
    if (n == 0) {  // (an empty index list has a null data(): the C ABI would read "no indices")
      output.points.clear();
      output.width = 0;
      output.height = 1;
      output.is_dense = true;
      return;
    }
    std::vector<PointT> res((size_t)n);  // (a buffer of its own: output may be the input)
    std::vector<int32_t> voe((size_t)(n > 0 ? n : 1));
    int64_t k = 0;
    const dlg_status s = dlg_voxel_grid(c, &pts, has_idx_ ? idx32.data() : nullptr, n, &prm_, &res[0].x,
                                        (int64_t)sizeof(PointT), n, &k, nullptr, voe.data(), &stats_);
    if (s == DLG_ERR_INVALID && std::string(dlg_last_error(c)).find("leaf size too small: voxel indices") == 0) {
      std::fprintf(stderr, "[dialog::VoxelGrid::applyFilter] Leaf size is too small for the input dataset. "
                           "Integer indices would overflow.\n");
      if (&output != input_.get()) output = *input_;
      return;
    }
    check(s, c);
    res.resize((size_t)k);
    output.points.swap(res);
    output.width = (uint32_t)k;
    output.height = 1;
    output.is_dense = true;
    voxel_of_.assign(voe.begin(), voe.begin() + n);
  }

 private:
  Context* ctx_;
  PointCloudConstPtr input_;
  std::vector<int> indices_;
  bool has_idx_ = false;
  dlg_voxel_params prm_{{0.f, 0.f, 0.f}, 0};
  dlg_voxel_stats stats_{};
  std::vector<int> voxel_of_;
};

// pcl::StatisticalOutlierRemoval<PointT> as the reference calls it (PCLViewer.cpp:334-358):
// setInputCloud / setMeanK / setStddevMulThresh / filter(output), plus setIndices, setNegative,
// filter(indices) and getRemovedIndices(), on dlg_statistical_outlier_removal.  filter(output) may
// write the cloud it reads (the reference assigns the result to source_cloud).  The neighbours
// come from the whole input cloud whatever the index list; a cloud with fewer than mean_k + 1
// finite points throws dialog::Error (PCL reads past FLANN's result there).
template <typename PointT>
class StatisticalOutlierRemoval {
 public:
  typedef typename pcl::PointCloud<PointT>::ConstPtr PointCloudConstPtr;
  explicit StatisticalOutlierRemoval(Context* ctx = nullptr) : ctx_(ctx) {}
  void setInputCloud(const PointCloudConstPtr& cloud) { input_ = cloud; }
  void setIndices(const pcl::PointIndices::Ptr& idx) { indices_ = idx ? idx->indices : std::vector<int>(); has_idx_ = (bool)idx; }
  void setIndices(const std::vector<int>& idx) { indices_ = idx; has_idx_ = true; }
  void setMeanK(int k) { prm_.mean_k = k; }
  int getMeanK() const { return prm_.mean_k; }
  void setStddevMulThresh(double m) { prm_.stddev_mul = m; }
  double getStddevMulThresh() const { return prm_.stddev_mul; }
  void setNegative(bool negative) { prm_.negative = negative ? 1 : 0; }
  bool getNegative() const { return prm_.negative != 0; }
  const std::vector<int>& getRemovedIndices() const { return removed_; }
  const dlg_sor_stats& lastStats() const { return stats_; }

  // the kept entries' index values, in list order
  void filter(std::vector<int>& kept) {
    kept.clear();
    removed_.clear();
    stats_ = dlg_sor_stats{};
    if (!input_) {
      std::fprintf(stderr, "[dialog::StatisticalOutlierRemoval::filter] No input dataset given!\n");
      return;
    }
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points pts{input_->points.empty() ? nullptr : &input_->points[0].x,
                   (int64_t)input_->points.size(), (int64_t)sizeof(PointT)};
    std::vector<int32_t> idx32(indices_.begin(), indices_.end());
    const int64_t n = has_idx_ ? (int64_t)idx32.size() : pts.n;
    if (n == 0) return;  // (an empty index list has a null data(): the C ABI would read "no indices")
    std::vector<int32_t> k32((size_t)n), r32((size_t)n);
    int64_t nk = 0, nr = 0;
    check(dlg_statistical_outlier_removal(c, &pts, has_idx_ ? idx32.data() : nullptr, n, &prm_,
                                          k32.data(), n, &nk, r32.data(), n, &nr, nullptr, &stats_),
          c);
    kept.assign(k32.begin(), k32.begin() + nk);
    removed_.assign(r32.begin(), r32.begin() + nr);
  }

  void filter(pcl::PointCloud<PointT>& output) {
    std::vector<int> kept;
    filter(kept);
    std::vector<PointT> res;  // (a buffer of its own: output may be the input)
    res.reserve(kept.size());
    bool dense = true;
    for (int i : kept) {
      const PointT& p = input_->points[(size_t)i];
      dense = dense && std::isfinite(p.x) && std::isfinite(p.y) && std::isfinite(p.z);
      res.push_back(p);
    }
    output.points.swap(res);
    output.width = (uint32_t)output.points.size();
    output.height = 1;
    output.is_dense = dense;
  }

 private:
  Context* ctx_;
  PointCloudConstPtr input_;
  std::vector<int> indices_;
  bool has_idx_ = false;
  dlg_sor_params prm_{1, 0, 0.0};
  dlg_sor_stats stats_{};
  std::vector<int> removed_;
};

// pcl::MovingLeastSquares<PointInT, PointOutT> as the reference calls it (PCLViewer.cpp:387-423):
// setComputeNormals / setInputCloud / setPolynomialFit / setSearchMethod (accepted and ignored: the
// search is the library's grid) / setSearchRadius / process(output), plus setIndices,
// setPolynomialOrder, setSqrGaussParam and getCorrespondingIndices(), on dlg_moving_least_squares
// (upsampling NONE).  PointOutT needs x, y, z; normal_x / normal_y / normal_z / curvature are
// written when it has them (pcl::PointNormal) and setComputeNormals(true).  The normals are not
// normalised (PCL 1.8).  A non-finite entry and one with fewer than 3 neighbours give no point.
template <typename PointInT, typename PointOutT>
class MovingLeastSquares {
 public:
  typedef typename pcl::PointCloud<PointInT>::ConstPtr PointCloudInConstPtr;
  explicit MovingLeastSquares(Context* ctx = nullptr) : ctx_(ctx) {}
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setIndices(const pcl::PointIndices::Ptr& idx) { indices_ = idx ? idx->indices : std::vector<int>(); has_idx_ = (bool)idx; }
  void setIndices(const std::vector<int>& idx) { indices_ = idx; has_idx_ = true; }
  template <typename TreePtr>
  void setSearchMethod(const TreePtr&) {}
  void setSearchRadius(double r) { prm_.search_radius = (float)r; sqr_gauss_set_ = false; }
  double getSearchRadius() const { return prm_.search_radius; }
  void setPolynomialFit(bool fit) { prm_.polynomial_fit = fit ? 1 : 0; }
  bool getPolynomialFit() const { return prm_.polynomial_fit != 0; }
  void setPolynomialOrder(int order) { prm_.polynomial_order = order; }
  int getPolynomialOrder() const { return prm_.polynomial_order; }
  // (PCL: setSearchRadius resets the parameter to radius^2; set it after the radius)
  void setSqrGaussParam(double g) { prm_.sqr_gauss_param = g; sqr_gauss_set_ = true; }
  double getSqrGaussParam() const {
    return sqr_gauss_set_ ? prm_.sqr_gauss_param
                          : (double)prm_.search_radius * (double)prm_.search_radius;
  }
  void setComputeNormals(bool on) { prm_.compute_normals = on ? 1 : 0; }
  // the input index of every output point (PCL: a PointIndices::Ptr)
  pcl::PointIndices::Ptr getCorrespondingIndices() const { return corresponding_; }
  const dlg_mls_stats& lastStats() const { return stats_; }

  void process(pcl::PointCloud<PointOutT>& output) {
    corresponding_.reset(new pcl::PointIndices);
    stats_ = dlg_mls_stats{};
    output.points.clear();
    output.width = 0;
    output.height = 1;
    output.is_dense = true;
    if (!input_) {
      std::fprintf(stderr, "[dialog::MovingLeastSquares::process] No input dataset given!\n");
      return;
    }
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points pts{input_->points.empty() ? nullptr : &input_->points[0].x,
                   (int64_t)input_->points.size(), (int64_t)sizeof(PointInT)};
    std::vector<int32_t> idx32(indices_.begin(), indices_.end());
    const int64_t n = has_idx_ ? (int64_t)idx32.size() : pts.n;
    if (n == 0) return;  // (an empty index list has a null data(): the C ABI would read "no indices")
    dlg_mls_params prm = prm_;
    if (!sqr_gauss_set_) prm.sqr_gauss_param = 0.0;
    std::vector<float> xyz((size_t)n * 3), nrm((size_t)n * 4);
    std::vector<int32_t> src((size_t)n);
    int64_t k = 0;
    check(dlg_moving_least_squares(c, &pts, has_idx_ ? idx32.data() : nullptr, n, &prm, xyz.data(),
                                   12, nrm.data(), n, &k, src.data(), nullptr, &stats_),
          c);
    output.points.resize((size_t)k);
    for (int64_t i = 0; i < k; ++i) {
      PointOutT& o = output.points[(size_t)i];
      o.x = xyz[3 * i]; o.y = xyz[3 * i + 1]; o.z = xyz[3 * i + 2];
      if (prm.compute_normals) set_normal(o, &nrm[4 * i], 0);
    }
    output.width = (uint32_t)k;
    corresponding_->indices.assign(src.begin(), src.begin() + k);
  }

 private:
  template <typename P>
  static auto set_normal(P& o, const float* r, int) -> decltype((void)o.normal_x, (void)o.curvature) {
    o.normal_x = r[0]; o.normal_y = r[1]; o.normal_z = r[2]; o.curvature = r[3];
  }
  template <typename P>
  static void set_normal(P&, const float*, long) {}

  Context* ctx_;
  PointCloudInConstPtr input_;
  std::vector<int> indices_;
  bool has_idx_ = false;
  bool sqr_gauss_set_ = false;
  dlg_mls_params prm_{0.0f, 0, 2, 0, 0.0};
  dlg_mls_stats stats_{};
  pcl::PointIndices::Ptr corresponding_;
};

// pcl::FPFHSignature33's layout (pcl::FPFHSignature33 itself works as PointOutT too)
struct FPFHSignature33 {
  float histogram[33];
};

// pcl::FPFHEstimation<PointInT, PointNT, PointOutT> with setRadiusSearch (PCLViewer.cpp:524-543):
// one descriptor per point of the input cloud, or per index; the search surface is the input
// cloud.  PointNT needs normal_x / normal_y / normal_z first in its record (pcl::Normal,
// pcl::PointNormal's are not: pass pcl::Normal), PointOutT a float histogram[33].  A non-finite
// entry gets 33 NaNs (and output.is_dense = false), one with no neighbour but itself 33 zeros.
template <typename PointInT, typename PointNT, typename PointOutT = FPFHSignature33>
class FPFHEstimation {
 public:
  typedef typename pcl::PointCloud<PointInT>::ConstPtr PointCloudInConstPtr;
  typedef typename pcl::PointCloud<PointNT>::ConstPtr PointCloudNConstPtr;
  explicit FPFHEstimation(Context* ctx = nullptr) : ctx_(ctx) {}
  void setInputCloud(const PointCloudInConstPtr& cloud) { input_ = cloud; }
  void setInputNormals(const PointCloudNConstPtr& normals) { normals_ = normals; }
  void setIndices(const pcl::PointIndices::Ptr& idx) { indices_ = idx ? idx->indices : std::vector<int>(); has_idx_ = (bool)idx; }
  void setIndices(const std::vector<int>& idx) { indices_ = idx; has_idx_ = true; }
  template <typename TreePtr>
  void setSearchMethod(const TreePtr&) {}
  void setRadiusSearch(double r) { prm_.search_radius = (float)r; }
  double getRadiusSearch() const { return prm_.search_radius; }
  const dlg_fpfh_stats& lastStats() const { return stats_; }

  void compute(pcl::PointCloud<PointOutT>& output) {
    static_assert(sizeof(((PointOutT*)nullptr)->histogram) == 33 * sizeof(float),
                  "PointOutT::histogram must be float[33]");
    stats_ = dlg_fpfh_stats{};
    output.points.clear();
    output.width = 0;
    output.height = 1;
    output.is_dense = true;
    if (!input_ || !normals_) {
      std::fprintf(stderr, "[dialog::FPFHEstimation::compute] No input dataset or normals given!\n");
      return;
    }
    if (normals_->points.size() != input_->points.size()) {
      std::fprintf(stderr, "[dialog::FPFHEstimation::compute] The number of points differs from "
                           "the number of normals!\n");
      return;
    }
    std::vector<int32_t> idx32(indices_.begin(), indices_.end());
    const int64_t n = has_idx_ ? (int64_t)idx32.size() : (int64_t)input_->points.size();
    // (an empty index list has a null data(): the C ABI would read "no indices")
    if (n == 0 || input_->points.empty()) return;
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points pts{&input_->points[0].x, (int64_t)input_->points.size(), (int64_t)sizeof(PointInT)};
    output.points.resize((size_t)n);
    check(dlg_fpfh_estimate(c, &pts, &normals_->points[0].normal_x, (int64_t)sizeof(PointNT),
                            has_idx_ ? idx32.data() : nullptr, n, &prm_,
                            &output.points[0].histogram[0], (int64_t)sizeof(PointOutT), nullptr,
                            nullptr, &stats_),
          c);
    output.width = (uint32_t)n;
    output.is_dense = stats_.n_nan_rows == 0;
  }

 private:
  Context* ctx_;
  PointCloudInConstPtr input_;
  PointCloudNConstPtr normals_;
  std::vector<int> indices_;
  bool has_idx_ = false;
  dlg_fpfh_params prm_{0.0f};
  dlg_fpfh_stats stats_{};
};

// A row-major 4x4 float matrix: what getFinalTransformation returns here (no Eigen): m(r, c).
struct Matrix4f {
  float v[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  float& operator()(int r, int c) { return v[4 * r + c]; }
  float operator()(int r, int c) const { return v[4 * r + c]; }
  const float* data() const { return v; }
  static Matrix4f Identity() { return Matrix4f(); }
};

// Registration::getFitnessScore(max_range): the mean squared distance of the aligned points to
// their nearest target points, over those with d2 <= max_range (DBL_MAX when there is none), summed
// as dlg_icp_align sums its mse.
inline double registration_fitness(dlg_ctx* c, const dlg_points& src, const dlg_points& tgt,
                                   double max_dist, double max_range) {
  const int64_t n = src.n;
  std::vector<int32_t> nn((size_t)n);
  std::vector<float> d2((size_t)n);
  int64_t k = 0;
  check(dlg_icp_correspondences(c, &src, nullptr, 0, &tgt, nullptr,
                                max_dist, nn.data(), d2.data(), &k),
        c);
  float dmax = 0.0f;
  int64_t kept = 0;
  for (int64_t i = 0; i < n; ++i)
    if (nn[(size_t)i] >= 0 && (double)d2[(size_t)i] <= max_range) {
      ++kept;
      if (d2[(size_t)i] > dmax) dmax = d2[(size_t)i];
    }
  if (kept == 0) return std::numeric_limits<double>::max();
  int e2 = 0;
  if (dmax > 0.0f) (void)std::frexp((double)dmax, &e2);
  unsigned __int128 sum = 0;
  for (int64_t i = 0; i < n; ++i)
    if (nn[(size_t)i] >= 0 && (double)d2[(size_t)i] <= max_range)
      sum += (unsigned __int128)(uint64_t)std::trunc(std::ldexp((double)d2[(size_t)i], 48 - e2));
  return std::ldexp((double)sum / (double)kept, e2 - 48);
}

// pcl::IterativeClosestPoint<PointSource, PointTarget> as the reference calls it
// (PCLViewer.cpp:581-636): setInputSource / setInputTarget / setMaximumIterations /
// setMaxCorrespondenceDistance / setTransformationEpsilon / setEuclideanFitnessEpsilon /
// align(output[, guess]) / hasConverged / getFinalTransformation / getFitnessScore, plus setIndices,
// on dlg_icp_align.  No reciprocal correspondences and no RANSAC rejector.  getFitnessScore runs
// the library's correspondence kernel on the aligned cloud and sums the kept squared distances
// exactly, as dlg_icp_stats.fitness is summed.
template <typename PointSource, typename PointTarget>
class IterativeClosestPoint {
 public:
  typedef typename pcl::PointCloud<PointSource>::ConstPtr PointCloudSourceConstPtr;
  typedef typename pcl::PointCloud<PointTarget>::ConstPtr PointCloudTargetConstPtr;
  explicit IterativeClosestPoint(Context* ctx = nullptr) : ctx_(ctx) {
    dlg_icp_params_default(&prm_);
  }
  void setInputSource(const PointCloudSourceConstPtr& cloud) { source_ = cloud; }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) { target_ = cloud; }
  void setIndices(const pcl::PointIndices::Ptr& idx) { indices_ = idx ? idx->indices : std::vector<int>(); has_idx_ = (bool)idx; }
  void setIndices(const std::vector<int>& idx) { indices_ = idx; has_idx_ = true; }
  void setMaximumIterations(int n) { prm_.max_iterations = n; }
  int getMaximumIterations() const { return prm_.max_iterations; }
  void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
  double getMaxCorrespondenceDistance() const { return prm_.max_correspondence_distance; }
  void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
  double getTransformationEpsilon() const { return prm_.transformation_epsilon; }
  void setEuclideanFitnessEpsilon(double e) { prm_.euclidean_fitness_epsilon = e; }
  double getEuclideanFitnessEpsilon() const { return prm_.euclidean_fitness_epsilon; }
  bool hasConverged() const { return stats_.converged != 0; }
  Matrix4f getFinalTransformation() const { return final_; }
  const dlg_icp_stats& lastStats() const { return stats_; }

  void align(pcl::PointCloud<PointSource>& output) { align_impl(output, nullptr); }
  void align(pcl::PointCloud<PointSource>& output, const Matrix4f& guess) {
    align_impl(output, guess.data());
  }

  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) {
    if (!target_ || aligned_.empty()) return std::numeric_limits<double>::max();
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    const int64_t n = (int64_t)aligned_.size() / 3;
    dlg_points src{aligned_.data(), n, 12};
    dlg_points tgt = target_points();
    return registration_fitness(c, src, tgt, prm_default_.max_correspondence_distance, max_range);
  }

 private:
  dlg_points target_points() const {
    return dlg_points{target_->points.empty() ? nullptr : &target_->points[0].x,
                      (int64_t)target_->points.size(), (int64_t)sizeof(PointTarget)};
  }
  void align_impl(pcl::PointCloud<PointSource>& output, const float* guess) {
    stats_ = dlg_icp_stats{};
    final_ = Matrix4f();
    aligned_.clear();
    output.points.clear();
    output.width = 0;
    output.height = 1;
    output.is_dense = true;
    if (!source_ || !target_) {
      std::fprintf(stderr, "[dialog::IterativeClosestPoint::align] No input source or target!\n");
      return;
    }
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points src{source_->points.empty() ? nullptr : &source_->points[0].x,
                   (int64_t)source_->points.size(), (int64_t)sizeof(PointSource)};
    dlg_points tgt = target_points();
    std::vector<int32_t> idx32(indices_.begin(), indices_.end());
    const int64_t n = has_idx_ ? (int64_t)idx32.size() : src.n;
    if (has_idx_ && n == 0) return;  // (an empty index list has a null data(): the C ABI would read "no indices")
    aligned_.resize((size_t)n * 3);
    check(dlg_icp_align(c, &src, has_idx_ ? idx32.data() : nullptr, n, &tgt, &prm_, guess, final_.v,
                        n > 0 ? aligned_.data() : nullptr, 12, nullptr, 0, &stats_),
          c);
    output.points.resize((size_t)n);
    bool dense = true;
    for (int64_t i = 0; i < n; ++i) {
      PointSource& o = output.points[(size_t)i];
      o = source_->points[(size_t)(has_idx_ ? idx32[(size_t)i] : i)];
      o.x = aligned_[3 * i]; o.y = aligned_[3 * i + 1]; o.z = aligned_[3 * i + 2];
      dense = dense && std::isfinite(o.x) && std::isfinite(o.y) && std::isfinite(o.z);
    }
    output.width = (uint32_t)n;
    output.is_dense = dense;
  }

  Context* ctx_;
  PointCloudSourceConstPtr source_;
  PointCloudTargetConstPtr target_;
  std::vector<int> indices_;
  bool has_idx_ = false;
  dlg_icp_params prm_{};
  dlg_icp_params prm_default_ = [] { dlg_icp_params p; dlg_icp_params_default(&p); return p; }();
  dlg_icp_stats stats_{};
  Matrix4f final_;
  std::vector<float> aligned_;
};

// pcl::SampleConsensusInitialAlignment<PointSource, PointTarget, FeatureT> as the reference calls it
// (PCLViewer.cpp:546-558): setInputSource / setSourceFeatures / setInputTarget / setTargetFeatures,
// align(output[, guess]), hasConverged, getFitnessScore, getFinalTransformation (dlg_sac_ia_align).
// FeatureT needs a float histogram[33] first in its record.  setRandGenerator / setRandSeed are
// not PCL's: rand() is glibc's (0) or the Visual C++ runtime's (1), seeded as srand would.
template <typename PointSource, typename PointTarget, typename FeatureT = FPFHSignature33>
class SampleConsensusInitialAlignment {
 public:
  typedef typename pcl::PointCloud<PointSource>::ConstPtr PointCloudSourceConstPtr;
  typedef typename pcl::PointCloud<PointTarget>::ConstPtr PointCloudTargetConstPtr;
  typedef typename pcl::PointCloud<FeatureT>::ConstPtr FeatureCloudConstPtr;
  explicit SampleConsensusInitialAlignment(Context* ctx = nullptr) : ctx_(ctx) {
    dlg_sac_ia_params_default(&prm_);
  }
  void setInputSource(const PointCloudSourceConstPtr& cloud) { source_ = cloud; }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) { target_ = cloud; }
  void setSourceFeatures(const FeatureCloudConstPtr& f) { source_features_ = f; }
  void setTargetFeatures(const FeatureCloudConstPtr& f) { target_features_ = f; }
  void setMinSampleDistance(float d) { prm_.min_sample_distance = d; }
  float getMinSampleDistance() const { return prm_.min_sample_distance; }
  void setNumberOfSamples(int n) { prm_.nr_samples = n; }
  int getNumberOfSamples() const { return prm_.nr_samples; }
  void setCorrespondenceRandomness(int k) { prm_.k_correspondences = k; }
  int getCorrespondenceRandomness() const { return prm_.k_correspondences; }
  void setMaximumIterations(int n) { prm_.max_iterations = n; }
  int getMaximumIterations() const { return prm_.max_iterations; }
  void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
  double getMaxCorrespondenceDistance() const { return prm_.max_correspondence_distance; }
  void setRandGenerator(int rng) { prm_.rng = rng; }
  void setRandSeed(uint32_t seed) { prm_.seed = seed; }
  bool hasConverged() const { return stats_.converged != 0; }
  Matrix4f getFinalTransformation() const { return final_; }
  const dlg_sac_ia_stats& lastStats() const { return stats_; }

  void align(pcl::PointCloud<PointSource>& output) { align_impl(output, nullptr); }
  void align(pcl::PointCloud<PointSource>& output, const Matrix4f& guess) {
    align_impl(output, guess.data());
  }

  double getFitnessScore(double max_range = std::numeric_limits<double>::max()) {
    if (!target_ || aligned_.empty()) return std::numeric_limits<double>::max();
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points src{aligned_.data(), (int64_t)aligned_.size() / 3, 12};
    dlg_icp_params icp;
    dlg_icp_params_default(&icp);
    return registration_fitness(c, src, target_points(), icp.max_correspondence_distance, max_range);
  }

 private:
  dlg_points target_points() const {
    return dlg_points{target_->points.empty() ? nullptr : &target_->points[0].x,
                      (int64_t)target_->points.size(), (int64_t)sizeof(PointTarget)};
  }
  void align_impl(pcl::PointCloud<PointSource>& output, const float* guess) {
    // (output may be the source cloud itself, as at PCLViewer.cpp:553: it is written last)
    stats_ = dlg_sac_ia_stats{};
    final_ = Matrix4f();
    aligned_.clear();
    if (!source_ || !target_ || !source_features_ || !target_features_) {
      std::fprintf(stderr, "[dialog::SampleConsensusInitialAlignment::align] No input source, "
                           "target or features!\n");
      output.points.clear();
      output.width = 0;
      output.height = 1;
      output.is_dense = true;
      return;
    }
    if (source_features_->points.size() != source_->points.size() ||
        target_features_->points.size() != target_->points.size())
      throw Error(DLG_ERR_INVALID, "SampleConsensusInitialAlignment: one feature per point");
    dlg_ctx* c = (ctx_ ? ctx_ : &Context::thread_default())->get();
    dlg_points src{source_->points.empty() ? nullptr : &source_->points[0].x,
                   (int64_t)source_->points.size(), (int64_t)sizeof(PointSource)};
    dlg_points tgt = target_points();
    const int64_t n = src.n;
    aligned_.resize((size_t)n * 3);
    check(dlg_sac_ia_align(
              c, &src, n > 0 ? &source_features_->points[0].histogram[0] : nullptr,
              (int64_t)sizeof(FeatureT), &tgt,
              tgt.n > 0 ? &target_features_->points[0].histogram[0] : nullptr,
              (int64_t)sizeof(FeatureT), &prm_, guess, final_.v, n > 0 ? aligned_.data() : nullptr,
              12, nullptr, 0, &stats_),
          c);
    std::vector<PointSource> moved(source_->points.begin(), source_->points.end());
    bool dense = true;
    for (int64_t i = 0; i < n; ++i) {
      PointSource& o = moved[(size_t)i];
      o.x = aligned_[3 * i]; o.y = aligned_[3 * i + 1]; o.z = aligned_[3 * i + 2];
      dense = dense && std::isfinite(o.x) && std::isfinite(o.y) && std::isfinite(o.z);
    }
    output.points.assign(moved.begin(), moved.end());
    output.width = (uint32_t)n;
    output.height = 1;
    output.is_dense = dense;
  }

  Context* ctx_;
  PointCloudSourceConstPtr source_;
  PointCloudTargetConstPtr target_;
  FeatureCloudConstPtr source_features_, target_features_;
  dlg_sac_ia_params prm_{};
  dlg_sac_ia_stats stats_{};
  Matrix4f final_;
  std::vector<float> aligned_;
};

// The fields of the reference's struct Plane (HeaderFile.h:81-88) that postProcessPlanes reads
// and writes: points_set, coeff.values (3 = outward normal before the first post-process, 4
// after) and border (the polyPlanes polygon, PlaneDetect.h:1358-1436).
template <typename PointT>
struct PlaneSet {
  pcl::PointCloud<PointT> points_set;
  std::vector<float> coeff;
  pcl::PointCloud<PointT> border;
};

struct PostProcessParams {
  float t_dist_point_plane = 0.1f;  // config.ini [PlaneDetect] T_dist_point_plane
  float radius_local = 0.1f;        // radius_local (clusterFilt)
  int t_cluster_num = 500;          // T_cluster_num
  uint32_t rand_seed = 0;           // the time(0) value isPointInPoly seeds rand() with
};

// postProcessPlanes() (PlaneDetect.h:1454-1579) on the GPU: every plane's coeff becomes the
// oriented computePointNormal refit (4 values); planes [plane_start_index, size) absorb the
// cloud points inside their border polygon (appended to points_set in cloud order);
// source_cloud is replaced by the points left after clusterFilt; plane_start_index advances to
// planes.size() as in the reference (:1557-1558).
template <typename PointT>
inline void postProcessPlanes(pcl::PointCloud<PointT>& source_cloud,
                              std::vector<PlaneSet<PointT>>& planes, int& plane_start_index,
                              const PostProcessParams& pp, Context* ctx = nullptr) {
  dlg_ctx* c = (ctx ? ctx : &Context::thread_default())->get();
  const size_t np = planes.size();
  std::vector<float> coeffs(4 * (np ? np : 1), 0.0f), out(4 * (np ? np : 1), 0.0f);
  std::vector<PointT> pts, bor;
  std::vector<int64_t> poff(np + 1, 0), boff(np + 1, 0);
  for (size_t k = 0; k < np; ++k) {
    for (size_t j = 0; j < planes[k].coeff.size() && j < 4; ++j) coeffs[4 * k + j] = planes[k].coeff[j];
    pts.insert(pts.end(), planes[k].points_set.points.begin(), planes[k].points_set.points.end());
    bor.insert(bor.end(), planes[k].border.points.begin(), planes[k].border.points.end());
    poff[k + 1] = (int64_t)pts.size();
    boff[k + 1] = (int64_t)bor.size();
  }
  dlg_planes P{(int32_t)np, coeffs.data(), pts.empty() ? nullptr : &pts[0].x, (int64_t)sizeof(PointT),
               poff.data(), bor.empty() ? nullptr : &bor[0].x, (int64_t)sizeof(PointT), boff.data()};
  dlg_postprocess_params prm{pp.t_dist_point_plane, pp.radius_local, (int32_t)pp.t_cluster_num,
                             (int32_t)plane_start_index, pp.rand_seed};
  dlg_points cl{source_cloud.points.empty() ? nullptr : &source_cloud.points[0].x,
                (int64_t)source_cloud.points.size(), (int64_t)sizeof(PointT)};
  std::vector<int64_t> aoff(np + 1, 0);
  std::vector<int32_t> ids(source_cloud.points.size() ? source_cloud.points.size() : 1);
  std::vector<int32_t> rem(source_cloud.points.size() ? source_cloud.points.size() : 1);
  int64_t nrem = 0;
  dlg_status st = dlg_post_process_planes(c, &cl, &P, &prm, out.data(), aoff.data(), ids.data(),
                                          (int64_t)ids.size(), rem.data(), (int64_t)rem.size(), &nrem);
  if (st == DLG_ERR_CAPACITY && aoff[np] > (int64_t)ids.size()) {  // a point joined several planes
    ids.resize((size_t)aoff[np]);
    st = dlg_post_process_planes(c, &cl, &P, &prm, out.data(), aoff.data(), ids.data(),
                                 (int64_t)ids.size(), rem.data(), (int64_t)rem.size(), &nrem);
  }
  check(st, c);
  for (size_t k = 0; k < np; ++k) {
    planes[k].coeff.assign(out.begin() + 4 * k, out.begin() + 4 * k + 4);
    for (int64_t t = aoff[k]; t < aoff[k + 1]; ++t) planes[k].points_set.push_back(source_cloud.points[ids[t]]);
  }
  pcl::PointCloud<PointT> kept;
  kept.points.reserve((size_t)nrem);
  for (int64_t t = 0; t < nrem; ++t) kept.points.push_back(source_cloud.points[rem[t]]);
  kept.width = (uint32_t)kept.points.size();
  source_cloud = std::move(kept);
  plane_start_index = (int)np;
}

// Result of the plane stage for one plane: coefficients (a, b, c, d) and inlier ids.  The
// reference's struct Plane (HeaderFile.h:81-88) is filled from it by copying the inlier points
// into points_set and coeff.values (see INTEGRATION.md for the PlaneDetect.h adapter).
struct PlaneResult {
  float coeff[4];
  std::vector<int> indices;
};

struct ExtractParams {
  double threshold = 0.1;          // config.txt T_dist_point_plane (Dialog/config.txt:29)
  int64_t min_inliers = 500;       // config.txt T_num_of_single_plane (Dialog/config.txt:20)
  int max_planes = 64;
  int max_iterations = 1000;
  double probability = 0.99;
  int refit_mode = DLG_REFIT_PCL;
  // SACMODEL_NORMAL_PLANE when set: one pcl::Normal per cloud point
  const pcl::PointCloud<pcl::Normal>* normals = nullptr;
  double normal_distance_weight = 0.1;
  // axis-constrained extraction (without normals): pcl::SACMODEL_PERPENDICULAR_PLANE ("the
  // horizontal planes": normal within eps_angle of axis) or pcl::SACMODEL_PARALLEL_PLANE ("the
  // vertical planes only"); pcl::SACMODEL_PLANE (default) ignores axis and eps_angle
  int model = pcl::SACMODEL_PLANE;
  float axis[3] = {0.f, 0.f, 0.f};
  double eps_angle = 0.0;  // radians
};

template <typename PointT>
inline dlg_extract_stats extractPlanes(const pcl::PointCloud<PointT>& cloud, const ExtractParams& ep,
                                       std::vector<PlaneResult>& planes, Context* ctx = nullptr) {
  planes.clear();
  dlg_ctx* c = (ctx ? ctx : &Context::thread_default())->get();
  dlg_points pts{cloud.points.empty() ? nullptr : &cloud.points[0].x, (int64_t)cloud.points.size(),
                 (int64_t)sizeof(PointT)};
  dlg_cloud* cl = nullptr;
  check(dlg_cloud_upload(c, &pts, nullptr, 0, 0, &cl), c);
  std::unique_ptr<dlg_cloud, dlg_status (*)(dlg_cloud*)> guard(cl, dlg_cloud_destroy);
  dlg_sac_params prm;
  dlg_sac_params_default(&prm);
  if (ep.normals) {
    check(dlg_cloud_set_normals(c, cl, ep.normals->points.empty() ? nullptr : &ep.normals->points[0].normal_x,
                                (int64_t)ep.normals->points.size(), (int64_t)sizeof(pcl::Normal)),
          c);
    prm.model = DLG_SACMODEL_NORMAL_PLANE;
    prm.normal_distance_weight = ep.normal_distance_weight;
  } else if (ep.model == pcl::SACMODEL_PERPENDICULAR_PLANE || ep.model == pcl::SACMODEL_PARALLEL_PLANE) {
    check(dlg_ctx_set_axis(c, ep.axis, ep.eps_angle), c);
    prm.model = ep.model;
  }
  prm.threshold = ep.threshold;
  prm.max_iterations = ep.max_iterations;
  prm.probability = ep.probability;
  prm.refit_mode = ep.refit_mode;
  std::vector<float> coeffs(4 * (size_t)(ep.max_planes > 0 ? ep.max_planes : 1));
  std::vector<int64_t> offs((size_t)ep.max_planes + 1);
  std::vector<int32_t> ids(cloud.points.size() ? cloud.points.size() : 1);
  int np = 0;
  dlg_extract_stats xs{};
  check(dlg_extract_planes(c, cl, &prm, ep.max_planes, ep.min_inliers, coeffs.data(), offs.data(),
                           ids.data(), (int64_t)ids.size(), &np, &xs),
        c);
  for (int p = 0; p < np; ++p) {
    PlaneResult r;
    for (int k = 0; k < 4; ++k) r.coeff[k] = coeffs[4 * p + k];
    r.indices.assign(ids.begin() + offs[p], ids.begin() + offs[p + 1]);
    planes.push_back(std::move(r));
  }
  return xs;
}

// The plane stage's output for the reference's polyPlanes (PlaneDetect.h:1358-1440): one entry
// of `plane_clouds` (PlaneDetect.h:100) per RANSAC plane, PlaneT being the reference's struct
// Plane (HeaderFile.h:81-88: border, points_set, coeff, triangles_headfile).  As the reference's
// segmentation leaves it (PlaneDetect.h:997-999, 1094-1096): points_set = copies of the inlier
// points, border = null (polyPlanes builds the ConcaveHull border for every plane whose border is
// still null and skips the others, :1364), coeff.values = the 3 components of the plane normal
// pointing out of the object.  Orientation as the reference's (:1048-1050, 1086-1093): the
// regulated normal of the source point nearest plane->points[0] -- the first inlier itself --
// flips the normal when p_n . n < 0 (float dot in Eigen's Vector3f order; a NaN normal never
// flips).  Returns the number of planes appended.
template <typename PlaneT, typename Alloc, typename PointT, typename PointNT>
inline size_t fillPlaneClouds(const pcl::PointCloud<PointT>& cloud,
                              const pcl::PointCloud<PointNT>& normals,
                              const std::vector<PlaneResult>& found,
                              std::vector<PlaneT, Alloc>& plane_clouds) {
  if (normals.points.size() != cloud.points.size())
    throw Error(DLG_ERR_INVALID, "fillPlaneClouds: one normal per cloud point");
  size_t added = 0;
  for (const PlaneResult& pr : found) {
    if (pr.indices.empty()) continue;
    PlaneT pl;
    pl.points_set.reset(new pcl::PointCloud<PointT>);
    pl.points_set->points.reserve(pr.indices.size());
    for (int i : pr.indices) pl.points_set->push_back(cloud.points[(size_t)i]);
    const PointNT& nr = normals.points[(size_t)pr.indices[0]];
    const float dot = (nr.normal_x * pr.coeff[0] + nr.normal_y * pr.coeff[1]) + nr.normal_z * pr.coeff[2];
    const float sg = dot < 0.0f ? -1.0f : 1.0f;
    pl.coeff.values.assign({sg * pr.coeff[0], sg * pr.coeff[1], sg * pr.coeff[2]});
    plane_clouds.push_back(std::move(pl));
    ++added;
  }
  return added;
}

// createPS() ... segmentPlanes() (PlaneDetect.h:667-1005) on dlg_gs_segment: the reference's own
// detector up to its seed planes.  Appends one PlaneT per seed plane to plane_clouds with
// points_set alone filled, as segmentPlanes leaves it (border null, coeff empty: growPlaneArea
// sets those), in the reference's plane order; each plane holds its distinct points.  PointNT needs
// normal_x / normal_y / normal_z first in its record (pcl::Normal).  prm: dlg_gs_params_default()
// gives the config.txt values.  Returns the number of planes added.
template <typename PointT, typename PointNT, typename PlaneT, typename Alloc>
inline size_t segmentPlanesGaussSphere(const pcl::PointCloud<PointT>& cloud,
                                       const pcl::PointCloud<PointNT>& normals,
                                       const dlg_gs_params& prm,
                                       std::vector<PlaneT, Alloc>& plane_clouds,
                                       Context* ctx = nullptr, dlg_gs_stats* stats = nullptr) {
  if (normals.points.size() != cloud.points.size())
    throw Error(DLG_ERR_INVALID, "segmentPlanesGaussSphere: one normal per cloud point");
  const int64_t n = (int64_t)cloud.points.size();
  if (n == 0) return 0;
  dlg_ctx* c = (ctx ? ctx : &Context::thread_default())->get();
  dlg_points pts{&cloud.points[0].x, n, (int64_t)sizeof(PointT)};
  std::vector<int64_t> off((size_t)n + 1), votes(64);
  std::vector<int32_t> ids((size_t)n), cells(64);
  dlg_gs_result r = dlg_gs_result();
  dlg_status st;
  for (;;) {
    r.plane_offsets = off.data(); r.planes_cap = n;
    r.plane_ids = ids.data(); r.ids_cap = n;
    r.sink_cells = cells.data(); r.sink_votes = votes.data(); r.sinks_cap = (int64_t)cells.size();
    st = dlg_gs_segment(c, &pts, &normals.points[0].normal_x, (int64_t)sizeof(PointNT), &prm, &r,
                        stats);
    if (st != DLG_ERR_CAPACITY || r.n_sinks <= (int64_t)cells.size()) break;
    cells.resize((size_t)r.n_sinks);
    votes.resize((size_t)r.n_sinks);
  }
  check(st, c);
  for (int64_t k = 0; k < r.n_planes; ++k) {
    PlaneT pl;
    pl.points_set.reset(new pcl::PointCloud<PointT>);
    pl.points_set->points.reserve((size_t)(off[(size_t)k + 1] - off[(size_t)k]));
    for (int64_t j = off[(size_t)k]; j < off[(size_t)k + 1]; ++j)
      pl.points_set->push_back(cloud.points[(size_t)ids[(size_t)j]]);
    plane_clouds.push_back(std::move(pl));
  }
  return (size_t)r.n_planes;
}

// polyPointCloud() (PlaneDetect.h:1376-1440) on dlg_plane_border: the plane's points projected
// onto their least-squares plane (pcl::computePointNormal + projPoint2Plane), the concave border
// of pcl::ConcaveHull (alpha shape of the projected points, alpha = alpha_poly, config.txt:28;
// the reference takes polygons[0], here the boundary polygon of largest area) appended to
// `border` in the reference's orientation (reversed when normalize(normalize(p1 - p0) x
// normalize(p2 - p1)) . pn < 0).  pn: any type with pn[0..2] (float[3], Eigen::Vector3f).  The
// input cloud is not modified (the reference projects a copy, :1367-1368).  A plane of fewer than
// 3 points gets no border.  Host arithmetic: replaces pcl::ConcaveHull (qhull) in polyPlanes.
template <typename PointT, typename Vec3>
inline void polyPointCloud(const pcl::PointCloud<PointT>& cloud, pcl::PointCloud<PointT>& border,
                           const Vec3& pn, float alpha_poly) {
  const int64_t n = (int64_t)cloud.points.size();
  static_assert(sizeof(PointT) >= 12, "PointT must start with float x, y, z");
  dlg_points pts{reinterpret_cast<const float*>(cloud.points.data()), n, (int64_t)sizeof(PointT)};
  const float v[3] = {(float)pn[0], (float)pn[1], (float)pn[2]};
  std::vector<PointT> out((size_t)std::max<int64_t>(n, 1));
  int64_t nb = 0;
  const dlg_status s = dlg_plane_border(&pts, v, alpha_poly, reinterpret_cast<float*>(out.data()),
                                        (int64_t)sizeof(PointT), n, &nb);
  if (s != DLG_OK) throw Error(s, std::string("dlg_plane_border: ") + dlg_status_string(s));
  for (int64_t i = 0; i < nb; ++i) {
    PointT q = PointT();
    q.x = out[(size_t)i].x; q.y = out[(size_t)i].y; q.z = out[(size_t)i].z;
    border.push_back(q);
  }
}

// polyPlanes() (PlaneDetect.h:1357-1374): every plane whose border is still null gets one from
// polyPointCloud over its points_set, oriented by its coeff.values[0..2] (the outward normal
// fillPlaneClouds stored); planes with a border are skipped, as in the reference.  PlaneT: the
// reference's struct Plane (HeaderFile.h:81-88).  Returns the number of borders built.
template <typename PlaneT, typename Alloc>
inline size_t polyPlanes(std::vector<PlaneT, Alloc>& plane_clouds, float alpha_poly) {
  size_t built = 0;
  for (PlaneT& pl : plane_clouds) {
    if (pl.border) continue;
    typedef typename std::remove_reference<decltype(*pl.points_set)>::type CloudT;
    pl.border.reset(new CloudT);
    if (!pl.points_set || pl.coeff.values.size() < 3) continue;
    const float pn[3] = {pl.coeff.values[0], pl.coeff.values[1], pl.coeff.values[2]};
    polyPointCloud(*pl.points_set, *pl.border, pn, alpha_poly);
    ++built;
  }
  return built;
}

}  // namespace dialog
