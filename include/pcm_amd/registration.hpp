// include/pcm_amd/registration.hpp -- header-only pcl::Registration adapter over the
// C ABI of include/pcm_amd.h.
//
// Drop-in for the reference's registration operators: same base class
// (pcl::Registration<PointSource, PointTarget, float>), same setters and call order
// as fast_gicp::LsqRegistration / FastGICP / FastVGICP
// (/root/reference/src/pointcloud_match/fast_gicp/include/fast_gicp/gicp/lsq_registration.hpp:15-85,
//  fast_gicp.hpp:19-100, fast_vgicp.hpp) so that call sites such as
// jueying_slam/src/localization.cpp:162-189,277,317-340 compile unchanged after
//     using Registration = pcm_amd::P2PlaneRegistration<pcl::PointXYZ, pcl::PointXYZ>;
// This header needs PCL + Eigen and therefore only compiles inside a ROS/PCL
// workspace (neither exists in the build container of this repository); it contains
// no algorithm, only the translation between PCL/Eigen types and plain pointers.
#pragma once

#if __has_include(<pcl/registration/registration.h>)

#include <pcl/point_cloud.h>
#include <pcl/point_types.h>
#include <pcl/registration/registration.h>

#include <Eigen/Core>
#include <Eigen/Eigenvalues>
#include <Eigen/Geometry>
#include <cfloat>
#include <cstdio>
#include <iostream>
#include <memory>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../pcm_amd.h"

namespace pcm_amd {

enum class LSQ_OPTIMIZER_TYPE { GaussNewton, LevenbergMarquardt };   // lsq_registration.hpp:13

template <typename PointSource, typename PointTarget>
class LsqRegistration : public pcl::Registration<PointSource, PointTarget, float> {
public:
  using Scalar = float;
  using Base = pcl::Registration<PointSource, PointTarget, Scalar>;
  using Matrix4 = typename Base::Matrix4;
  using PointCloudSource = typename Base::PointCloudSource;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTarget = typename Base::PointCloudTarget;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;

protected:
  using Base::converged_;
  using Base::final_transformation_;
  using Base::input_;
  using Base::max_iterations_;
  using Base::nr_iterations_;
  using Base::reg_name_;
  using Base::target_;
  using Base::transformation_epsilon_;

public:
  EIGEN_MAKE_ALIGNED_OPERATOR_NEW

  explicit LsqRegistration(int model, int device = 0) {
    reg_name_ = "pcm_amd::LsqRegistration";
    pcm_default_config(&cfg_);
    cfg_.model = model;
    max_iterations_ = cfg_.max_iterations;                 // 64    lsq_registration_impl.hpp:11
    transformation_epsilon_ = cfg_.translation_eps;        // 5e-4  :13
    ctx_ = pcm_create(device, &cfg_);
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    final_hessian_.setIdentity();                          // :21
  }
  ~LsqRegistration() override { pcm_destroy(ctx_); }
  LsqRegistration(const LsqRegistration&) = delete;
  LsqRegistration& operator=(const LsqRegistration&) = delete;

  // ---- LsqRegistration surface (lsq_registration_impl.hpp:26-49) ----
  void setRotationEpsilon(double eps) { cfg_.rotation_eps = eps; }
  void setInitialLambdaFactor(double f) { cfg_.lm_init_lambda_factor = f; }
  void setDebugPrint(bool) {}
  void setOptimizer(LSQ_OPTIMIZER_TYPE t) { cfg_.optimizer = t == LSQ_OPTIMIZER_TYPE::GaussNewton ? PCM_OPT_GAUSS_NEWTON : PCM_OPT_LEVENBERG_MARQUARDT; }
  const Eigen::Matrix<double, 6, 6>& getFinalHessian() const { return final_hessian_; }
  int getFinalNumIteration() const { return nr_iterations_; }                                    // ndt_omp.h:228-232

  // pcl::Registration::getFitnessScore(max_range) on the device (pcm_fitness_score): every reference call site asks for it right
  // after align() (localization.cpp:325-326, mapOptmization.cpp:693,719, align.cpp:63).  PCL's member is NOT virtual: a call through
  // a pcl::Registration base pointer still runs PCL's CPU kd-tree pass -- keep the adapter's type at the call site.
  double getFitnessScore(double max_range = DBL_MAX) {
    float T[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) T[i * 4 + j] = final_transformation_(i, j);
    double score = 0.0;
    check(pcm_fitness_score(ctx_, T, max_range, &score), "pcm_fitness_score");
    return score;
  }

  double evaluateCost(const Eigen::Matrix4f& relative_pose, Eigen::Matrix<double, 6, 6>* H = nullptr, Eigen::Matrix<double, 6, 1>* b = nullptr) {
    push_config();
    double T[16], Hr[36], br[6], cost = 0.0;
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) T[i * 4 + j] = static_cast<double>(relative_pose(i, j));   // Eigen is column-major: transpose into the row-major ABI
    check(pcm_linearize(ctx_, T, Hr, br, &cost, nullptr), "pcm_linearize");
    if (H) for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) (*H)(i, j) = Hr[i * 6 + j];
    if (b) for (int i = 0; i < 6; i++) (*b)(i) = br[i];
    return cost;
  }

  // ---- FastGICP surface (fast_gicp_impl.hpp:26-90) ----
  void setNumThreads(int) {}                                             // no meaning on the GPU
  // corr_dist_threshold_ of the GICP family (fast_gicp_impl.hpp:18,136).  The point-to-plane matcher does not read it: its
  // search radius is iVox's own max_range (ivox3d.h:132, 5.0 m), which stays what the configuration says.
  void setMaxCorrespondenceDistance(double d) { Base::setMaxCorrespondenceDistance(d); cfg_.max_corr_dist = static_cast<float>(d); }
  void setMaxRange(double r) { cfg_.max_range = static_cast<float>(r); }   // IVox::GetClosestPoint max_range
  void setResolution(double r) { cfg_.voxel_resolution = static_cast<float>(r); }      // fast_vgicp_impl.hpp:28-30
  void setNumNeighborCells(int n) { cfg_.num_neighbors = n; }            // ivox_nearby_type 0/6/18/26 -> 1/7/19/27
  // P2PLANE scan-to-submap mapping: the candidate lists follow a target that grows (PCM_FLAG_FOLLOWING_LISTS)
  void setFollowingLists(bool on) { cfg_.flags = on ? (cfg_.flags | PCM_FLAG_FOLLOWING_LISTS) : (cfg_.flags & ~PCM_FLAG_FOLLOWING_LISTS); }

  virtual void swapSourceAndTarget() {
    input_.swap(target_);
    check(pcm_swap_source_and_target(ctx_), "pcm_swap_source_and_target");
  }
  virtual void clearSource() { input_.reset(); check(pcm_clear_source(ctx_), "pcm_clear_source"); }
  virtual void clearTarget() { target_.reset(); check(pcm_clear_target(ctx_), "pcm_clear_target"); }

  void setInputSource(const PointCloudSourceConstPtr& cloud) override {
    if (input_ == cloud) return;                                         // fast_gicp_impl.hpp:72-74
    Base::setInputSource(cloud);
    check(pcm_set_source(ctx_, cloud->points.data(), cloud->size(), sizeof(PointSource), PCM_MEM_HOST, reinterpret_cast<uint64_t>(cloud.get())), "pcm_set_source");
  }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) override {
    if (target_ == cloud) return;                                        // :83-85
    Base::setInputTarget(cloud);
    check(pcm_set_target(ctx_, cloud->points.data(), cloud->size(), sizeof(PointTarget), PCM_MEM_HOST, reinterpret_cast<uint64_t>(cloud.get())), "pcm_set_target");
  }

  // One built target for several objects (pcm_share_target): this object registers against the target `other` holds from now on --
  // the cloud, its voxel map and what the model derives from them exist once on the device -- as the reference's objects do when they
  // are handed one PointCloud::ConstPtr.  Both are of one class with the settings that decide how a target is built equal (the
  // exception names the first that differs).  setInputTarget(cloud) keeps its meaning: with the shared cloud it is the reference's
  // no-op, with another it gives this object a target of its own again; the other holders are not touched either way.
  void shareTargetWith(LsqRegistration& other) {
    other.push_config();
    push_config();
    check(pcm_share_target(ctx_, other.ctx_), "pcm_share_target");
    target_ = other.target_;
  }
  int targetShareCount() const {
    const int n = pcm_target_share_count(ctx_);
    if (n < 0) check(n, "pcm_target_share_count");
    return n;
  }

protected:
  // pcl::Registration::align() calls this (lsq_registration_impl.hpp:52-79)
  void computeTransformation(PointCloudSource& output, const Matrix4& guess) override {
    push_config();
    float g[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) g[i * 4 + j] = guess(i, j);
    pcm_result r;
    const int rc = pcm_align(ctx_, g, &r);
    if (rc == PCM_ERR_NOT_CONVERGED) std::cerr << "lm not converged!!" << std::endl;      // :70
    else check(rc, "pcm_align");
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) final_transformation_(i, j) = r.T[i * 4 + j];
    for (int i = 0; i < 6; i++) for (int j = 0; j < 6; j++) final_hessian_(i, j) = r.H[i * 6 + j];
    nr_iterations_ = r.iterations;
    converged_ = r.converged != 0;
    last_cost_ = r.cost;
    pcl::transformPointCloud(*input_, output, final_transformation_);                    // :78
  }

  void push_config() {
    cfg_.max_iterations = max_iterations_;                   // setMaximumIterations
    cfg_.translation_eps = transformation_epsilon_;          // setTransformationEpsilon
    check(pcm_set_config(ctx_, &cfg_), "pcm_set_config");
  }
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }

  pcm_ctx* ctx_ = nullptr;
  pcm_config cfg_;
  Eigen::Matrix<double, 6, 6> final_hessian_;
  double last_cost_ = 0.0;   // cost (LSQ models) / score (pclomp NDT) of the last evaluation
};

// point-to-plane scan-to-submap ICP with jueying_lio's matcher semantics
template <typename PointSource, typename PointTarget>
class P2PlaneRegistration : public LsqRegistration<PointSource, PointTarget> {
public:
  explicit P2PlaneRegistration(int device = 0) : LsqRegistration<PointSource, PointTarget>(PCM_MODEL_P2PLANE, device) { this->reg_name_ = "pcm_amd::P2PlaneRegistration"; }
};

// fast_gicp::FastGICP (gicp/fast_gicp.hpp:24-95): setCorrespondenceRandomness, setRegularizationMethod, covariances
enum class RegularizationMethod { NONE, MIN_EIG, NORMALIZED_MIN_EIG, PLANE, FROBENIUS };   // gicp_settings.hpp
enum class NeighborSearchMethod { DIRECT27, DIRECT7, DIRECT1, /* VGICP_CUDA / NDTCuda only */ DIRECT_RADIUS };   // gicp_settings.hpp:8
enum class VoxelAccumulationMode { ADDITIVE, ADDITIVE_WEIGHTED, MULTIPLICATIVE };              // gicp_settings.hpp

template <typename PointSource, typename PointTarget>
class GicpRegistration : public LsqRegistration<PointSource, PointTarget> {
public:
  explicit GicpRegistration(int device = 0, int model = PCM_MODEL_GICP) : LsqRegistration<PointSource, PointTarget>(model, device) { this->reg_name_ = "pcm_amd::GicpRegistration"; }
  void setCorrespondenceRandomness(int k) { this->cfg_.k_correspondences = k; }                         // fast_gicp_impl.hpp:61-63
  void setRegularizationMethod(RegularizationMethod m) {                                                // :66-68
    static const int map[5] = {PCM_REG_NONE, PCM_REG_MIN_EIG, PCM_REG_NORMALIZED_MIN_EIG, PCM_REG_PLANE, PCM_REG_FROBENIUS};
    this->cfg_.regularization = map[static_cast<int>(m)];
  }
  // getSourceCovariances / getTargetCovariances  fast_gicp.hpp:64-70  (Matrix4d with the 3x3 block set)
  std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> getCovariances(bool target) {
    this->push_config();
    size_t n = 0;
    this->check(pcm_get_covariances(this->ctx_, target ? 1 : 0, nullptr, 0, &n), "pcm_get_covariances");
    std::vector<double> raw(n * 9);
    this->check(pcm_get_covariances(this->ctx_, target ? 1 : 0, raw.data(), n, &n), "pcm_get_covariances");
    std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> out(n, Eigen::Matrix4d::Zero());
    for (size_t i = 0; i < n; i++) for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) out[i](a, b) = raw[i * 9 + a * 3 + b];
    return out;
  }
  void setCovariances(bool target, const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>& covs) {
    this->push_config();
    std::vector<double> raw(covs.size() * 9);
    for (size_t i = 0; i < covs.size(); i++) for (int a = 0; a < 3; a++) for (int b = 0; b < 3; b++) raw[i * 9 + a * 3 + b] = covs[i](a, b);
    this->check(pcm_set_covariances(this->ctx_, target ? 1 : 0, raw.data(), covs.size(), 9), "pcm_set_covariances");
  }
  // setSourceCovariances / setTargetCovariances  fast_gicp.hpp:60-62 (Matrix4d, the 3x3 block is the covariance)
  void setSourceCovariances(const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>& covs) { setCovariances(false, covs); }
  void setTargetCovariances(const std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>>& covs) { setCovariances(true, covs); }
  std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> getSourceCovariances() { return getCovariances(false); }
  std::vector<Eigen::Matrix4d, Eigen::aligned_allocator<Eigen::Matrix4d>> getTargetCovariances() { return getCovariances(true); }
};

// fast_gicp::FastVGICP (gicp/fast_vgicp.hpp): resolution 1.0, DIRECT1, ADDITIVE  (impl/fast_vgicp_impl.hpp:22-25)
template <typename PointSource, typename PointTarget>
class VgicpRegistration : public GicpRegistration<PointSource, PointTarget> {
public:
  explicit VgicpRegistration(int device = 0) : GicpRegistration<PointSource, PointTarget>(device, PCM_MODEL_VGICP) {
    this->reg_name_ = "pcm_amd::VgicpRegistration";
    this->cfg_.voxel_resolution = 1.0f;
    this->cfg_.num_neighbors = 1;
  }
  void setNeighborSearchMethod(NeighborSearchMethod m) { this->cfg_.num_neighbors = m == NeighborSearchMethod::DIRECT27 ? 27 : (m == NeighborSearchMethod::DIRECT7 ? 7 : 1); }
  void setVoxelAccumulationMode(VoxelAccumulationMode m) { this->cfg_.voxel_mode = static_cast<int>(m); }   // fast_vgicp_impl.hpp:38-40
};

namespace detail {
// setNeighborSearchMethod(method, radius) of the CUDA-core classes (ndt_cuda_impl.hpp:30-32, fast_vgicp_cuda_impl.hpp:59-61):
// DIRECT_RADIUS takes the radius in voxels (ndt_cuda.cu:70-83); the other methods ignore it.  Against the reference: the radius
// is stored as a float and must lie in (0, 3] voxels (align() returns PCM_ERR_INVALID_ARGUMENT beyond; the reference accepts any double)
inline void set_search_method(pcm_config& cfg, NeighborSearchMethod m, double radius) {
  cfg.neighbor_search_radius = 0.f;
  if (m == NeighborSearchMethod::DIRECT_RADIUS) cfg.neighbor_search_radius = static_cast<float>(radius);
  else cfg.num_neighbors = m == NeighborSearchMethod::DIRECT27 ? 27 : (m == NeighborSearchMethod::DIRECT7 ? 7 : 1);
}
}  // namespace detail

// fast_gicp::FastVGICPCuda (gicp/fast_vgicp_cuda.hpp; impl/fast_vgicp_cuda_impl.hpp:21-31): the float CUDA core -- 20-NN covariances,
// PLANE, resolution 1.0, DIRECT1 (cuda/fast_vgicp_cuda.cu:26-34)
template <typename PointSource, typename PointTarget>
class VgicpCudaRegistration : public GicpRegistration<PointSource, PointTarget> {
public:
  explicit VgicpCudaRegistration(int device = 0) : GicpRegistration<PointSource, PointTarget>(device, PCM_MODEL_VGICP_CUDA) {
    this->reg_name_ = "pcm_amd::VgicpCudaRegistration";
    this->cfg_.voxel_resolution = 1.0f;
    this->cfg_.num_neighbors = 1;
  }
  void setCorrespondenceRandomness(int) {}                                                       // a no-op there too (fast_vgicp_cuda_impl.hpp:37-38)
  // setNearestNeighborSearchMethod (fast_vgicp_cuda_impl.hpp:64-66): CPU_PARALLEL_KDTREE and GPU_BRUTEFORCE both give the exact
  // k nearest neighbours the covariances are built from -- one device implementation serves both; GPU_RBF_KERNEL selects the
  // RBF-kernel covariance estimator (cuda/covariance_estimation_rbf.cu:59-151 -> pcm_config.covariance_method = PCM_COV_RBF_KERNEL)
  enum class NearestNeighborMethod { CPU_PARALLEL_KDTREE, GPU_BRUTEFORCE, GPU_RBF_KERNEL };      // fast_vgicp_cuda.hpp:21
  void setNearestNeighborSearchMethod(NearestNeighborMethod m) { this->cfg_.covariance_method = m == NearestNeighborMethod::GPU_RBF_KERNEL ? PCM_COV_RBF_KERNEL : PCM_COV_KNN; }
  void setKernelWidth(double kernel_width, double max_dist = -1.0) {                             // fast_vgicp_cuda_impl.hpp:46-52 (read in RBF mode only)
    this->cfg_.rbf_kernel_width = static_cast<float>(kernel_width);
    this->cfg_.rbf_max_dist = static_cast<float>(max_dist <= 0.0 ? kernel_width * 5.0 : max_dist);
  }

public:
  void setNeighborSearchMethod(NeighborSearchMethod m, double radius = -1.0) { detail::set_search_method(this->cfg_, m, radius); }
};

// fast_gicp::NDTCuda (ndt/ndt_cuda.hpp:21-71): D2D, DIRECT7, resolution 1.0  (cuda/ndt_cuda.cu:15-22)
enum class NDTDistanceMode { P2D, D2D };
template <typename PointSource, typename PointTarget>
class NdtRegistration : public LsqRegistration<PointSource, PointTarget> {
public:
  explicit NdtRegistration(int device = 0) : LsqRegistration<PointSource, PointTarget>(PCM_MODEL_NDT_D2D, device) {
    this->reg_name_ = "pcm_amd::NdtRegistration";
    this->cfg_.voxel_resolution = 1.0f;
    this->cfg_.num_neighbors = 7;
  }
  void setDistanceMode(NDTDistanceMode m) { this->cfg_.model = m == NDTDistanceMode::P2D ? PCM_MODEL_NDT_P2D : PCM_MODEL_NDT_D2D; }
  void setNeighborSearchMethod(NeighborSearchMethod m, double radius = -1.0) { detail::set_search_method(this->cfg_, m, radius); }
};

// pclomp::NormalDistributionsTransform (ndt_omp/include/pclomp/ndt_omp.h:77-310): the operator jueying_slam's
// localization constructs (jueying_slam/src/localization.cpp:162-189).  Defaults of that class (ndt_omp_impl.hpp:48,60-63).
enum NeighborSearchMethodOmp { KDTREE, DIRECT26, DIRECT7, DIRECT1 };   // ndt_omp.h:60
// pcl::IterativeClosestPoint (PCM_MODEL_ICP), as jueying_slam's performSCLoopClosure uses it (mapOptmization.cpp:768-779): point-to-point
// ICP with PCL's defaults and setter names; setMaximumIterations / setTransformationEpsilon are pcl::Registration's own.  The rules
// (PCL's, restated; one deliberate departure) are in include/pcm_amd.h and DESIGN.md section 37.  getFitnessScore is the base's.
template <typename PointSource, typename PointTarget>
class IterativeClosestPoint : public LsqRegistration<PointSource, PointTarget> {
  using Lsq = LsqRegistration<PointSource, PointTarget>;

public:
  explicit IterativeClosestPoint(int device = 0) : Lsq(PCM_MODEL_ICP, device) {
    this->reg_name_ = "pcm_amd::IterativeClosestPoint";
    pcm_icp_default_params(&icp_);
    this->max_iterations_ = icp_.max_iterations;                     // 10
    this->transformation_epsilon_ = icp_.transformation_epsilon;     // 0
  }
  void setMaxCorrespondenceDistance(double d) { Lsq::Base::setMaxCorrespondenceDistance(d); icp_.max_correspondence_distance = d; }
  void setEuclideanFitnessEpsilon(double e) { icp_.euclidean_fitness_epsilon = e; }
  void setTransformationRotationEpsilon(double e) { icp_.rotation_epsilon = e; }
  void setRANSACIterations(int) {}   // :773 sets 0: there is no RANSAC rejection here
  const pcm_icp_info& lastInfo() const { return info_; }   // stop reason (PCM_ICP_STOP_*), pair count and mse of the last align()

protected:
  void computeTransformation(typename Lsq::PointCloudSource& output, const typename Lsq::Matrix4& guess) override {
    icp_.max_iterations = this->max_iterations_;
    icp_.transformation_epsilon = this->transformation_epsilon_;
    this->check(pcm_set_config(this->ctx_, &this->cfg_), "pcm_set_config");   // setResolution: the cell of the search grid
    this->check(pcm_icp_set_params(this->ctx_, &icp_), "pcm_icp_set_params");
    float g[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) g[i * 4 + j] = guess(i, j);
    pcm_result r;
    this->check(pcm_align(this->ctx_, g, &r), "pcm_align");
    this->check(pcm_icp_last(this->ctx_, &info_), "pcm_icp_last");
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) this->final_transformation_(i, j) = r.T[i * 4 + j];
    this->nr_iterations_ = r.iterations;
    this->converged_ = r.converged != 0;
    this->last_cost_ = r.cost;
    pcl::transformPointCloud(*this->input_, output, this->final_transformation_);
  }
  pcm_icp_params icp_;
  pcm_icp_info info_{};
};

template <typename PointSource, typename PointTarget>
class PclNdtRegistration : public LsqRegistration<PointSource, PointTarget> {
public:
  explicit PclNdtRegistration(int device = 0) : LsqRegistration<PointSource, PointTarget>(PCM_MODEL_NDT_OMP, device) {
    this->reg_name_ = "pcm_amd::PclNdtRegistration";
    this->cfg_.voxel_resolution = 1.0f;
    this->cfg_.num_neighbors = 7;
    this->max_iterations_ = 35;
    this->transformation_epsilon_ = 0.1;
  }
  void setStepSize(double s) { this->cfg_.ndt_step_size = static_cast<float>(s); }               // ndt_omp.h:166
  double getStepSize() const { return this->cfg_.ndt_step_size; }                                 // ndt_omp.h:157
  void setOutlierRatio(double r) { this->cfg_.ndt_outlier_ratio = static_cast<float>(r); }       // ndt_omp.h:188
  double getOutlierRatio() const { return this->cfg_.ndt_outlier_ratio; }                         // ndt_omp.h:179
  float getResolution() const { return this->cfg_.voxel_resolution; }                             // ndt_omp.h:141
  void setNeighborhoodSearchMethod(NeighborSearchMethodOmp m) {                                  // ndt_omp.h:198
    this->cfg_.num_neighbors = m == KDTREE ? 0 : (m == DIRECT26 ? 27 : (m == DIRECT7 ? 7 : 1));
  }
  double getTransformationProbability() const { return trans_probability_; }                     // ndt_omp.h:207
  // getMaxEigen (ndt_omp.h:209-223): largest pseudo-eigenvalue of the final Hessian / 1e5 -- the degeneracy metric of the localisation node
  double getMaxEigen() const {
    Eigen::EigenSolver<Eigen::Matrix<double, 6, 6>> eigen_solver(this->final_hessian_);
    const Eigen::Matrix<double, 6, 6> mat_E = eigen_solver.pseudoEigenvalueMatrix();
    double max_eigen = mat_E(0, 0);
    for (int i = 0; i < 6; i++) if (mat_E(i, i) > max_eigen) max_eigen = mat_E(i, i);
    return max_eigen / 100000.0;
  }
  // calculateScore(cloud) (ndt_omp_impl.hpp:835-880): negative log likelihood of the ALREADY TRANSFORMED cloud the caller passes;
  // here the source cloud under the given pose (identity = the cloud as it is)
  double calculateScore(const Eigen::Matrix4f& pose = Eigen::Matrix4f::Identity()) {
    this->push_config();
    float T[16];
    for (int i = 0; i < 4; i++) for (int j = 0; j < 4; j++) T[i * 4 + j] = pose(i, j);
    double score = 0.0;
    this->check(pcm_ndt_score(this->ctx_, T, &score), "pcm_ndt_score");
    return score;
  }
protected:
  void computeTransformation(typename LsqRegistration<PointSource, PointTarget>::PointCloudSource& output,
                             const typename LsqRegistration<PointSource, PointTarget>::Matrix4& guess) override {
    LsqRegistration<PointSource, PointTarget>::computeTransformation(output, guess);
    trans_probability_ = this->last_cost_ / static_cast<double>(this->input_->points.size());   // ndt_omp_impl.hpp:145
  }
  double trans_probability_ = 0.0;
};

namespace detail {
// A PCL point is not a packed (x, y, z, intensity) record: pcl::PointXYZI keeps the padding of its xyz block as the fourth float
// and the intensity at byte 16.  The LOAM feature and key-frame calls read the fourth float of a record as its intensity, so the
// adapters repack member by member; a point type without an intensity member packs 0.
template <typename P> auto intensity_of(const P& p, int) -> decltype(static_cast<float>(p.intensity)) { return static_cast<float>(p.intensity); }
template <typename P> float intensity_of(const P&, long) { return 0.0f; }
template <typename CloudT>
void pack_xyzi(const CloudT& cloud, std::vector<float>& buf) {
  const size_t n = cloud.points.size();
  buf.resize(4 * n);
  for (size_t i = 0; i < n; i++) {
    const auto& q = cloud.points[i];
    buf[4 * i] = q.x; buf[4 * i + 1] = q.y; buf[4 * i + 2] = q.z; buf[4 * i + 3] = intensity_of(q, 0);
  }
}
}  // namespace detail

// jueying_slam's LOAM edge / plane scan-to-map optimisation with the call shape of mapOptmization.cpp:1560-1586:
//     loam.setInputMaps(laserCloudCornerFromMapDS, laserCloudSurfFromMapDS);   // replaces the two kdtree setInputCloud calls
//     loam.setInputFeatures(laserCloudCornerLastDS, laserCloudSurfLastDS);
//     if (loam.scan2MapOptimization(transformTobeMapped)) transformUpdate();  // false: "Not enough features!" (pose untouched)
// The mapping node refills its map clouds in place every frame, so the maps are uploaded at every call unless the caller passes a
// non-zero tag that changes with the content (a localisation node's fixed global map: any constant).  setLocalizationThresholds()
// selects the 0.05 deg rotation threshold of localization.cpp:985; the fitness scores are those of localization.cpp:1003-1022.
template <typename PointT>
class LoamScanToMap {
public:
  using Cloud = pcl::PointCloud<PointT>;
  using CloudConstPtr = typename Cloud::ConstPtr;

  explicit LoamScanToMap(int device = 0) {
    pcm_config cfg;
    pcm_default_config(&cfg);
    cfg.model = PCM_MODEL_LOAM;
    ctx_ = pcm_create(device, &cfg);
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    pcm_loam_default_params(&params_);
  }
  ~LoamScanToMap() { pcm_destroy(ctx_); }
  LoamScanToMap(const LoamScanToMap&) = delete;
  LoamScanToMap& operator=(const LoamScanToMap&) = delete;

  void setIterNum(int n) { params_.iter_num = n; }                                     // utility.h:253
  void setFeatureMinValidNum(int edge, int surf) { params_.edge_min_valid = edge; params_.surf_min_valid = surf; }   // utility.h:267-268
  void setLocalizationThresholds() { params_.rot_conv_deg = 0.05; }                    // localization.cpp:985
  pcm_loam_params& params() { return params_; }

  void setInputMaps(const CloudConstPtr& corner, const CloudConstPtr& surf, uint64_t tag = 0) {
    check(pcm_loam_set_target(ctx_, corner->points.data(), corner->size(), surf->points.data(), surf->size(), sizeof(PointT), PCM_MEM_HOST, tag),
          "pcm_loam_set_target");
  }
  // packed member by member (x, y, z, intensity): a key frame saved from this source keeps the points' intensity
  void setInputFeatures(const CloudConstPtr& corner, const CloudConstPtr& surf) {
    detail::pack_xyzi(*corner, corner_xyzi_);
    detail::pack_xyzi(*surf, surf_xyzi_);
    check(pcm_loam_set_source(ctx_, corner_xyzi_.data(), corner->size(), surf_xyzi_.data(), surf->size(), 4 * sizeof(float), PCM_MEM_HOST, 0),
          "pcm_loam_set_source");
  }
  // imageProjection + featureExtraction + downsampleCurrentScan of one ring-tagged scan (PointXYZIRT-like: x y z, intensity, ring
  // members) into the features on the device (pcm_loam_frame_begin).  The context keeps the nodes'
  // cross-frame state.  fp: the feature parameters (default: utility.h's), e.g. LoamFeatureExtraction::params().
  // deskew: LoamFeatureExtraction::deskewInfo's descriptor with its time field set (NULL: the points stay as they are).
  template <typename PointIn>
  void setInputScan(const std::shared_ptr<const pcl::PointCloud<PointIn>>& scan, const pcm_loam_feature_params* fp = nullptr, const pcm_loam_deskew* deskew = nullptr) {
    const PointIn probe{};
    const char* base = reinterpret_cast<const char*>(&probe);
    const size_t ioff = (size_t)(reinterpret_cast<const char*>(&probe.intensity) - base), roff = (size_t)(reinterpret_cast<const char*>(&probe.ring) - base);
    check(pcm_loam_frame_begin_deskew(ctx_, scan->points.data(), scan->size(), sizeof(PointIn), ioff, roff, PCM_MEM_HOST, fp, &features_, deskew),
          "pcm_loam_frame_begin");
  }
  // the same for ring-tagged records that already lie in device memory (ScanFusion::fuseToFrontEnd)
  void setInputScanDevice(const void* device_points, size_t n, size_t stride, size_t intensity_offset, size_t ring_offset, const pcm_loam_feature_params* fp = nullptr) {
    check(pcm_loam_frame_begin(ctx_, device_points, n, stride, intensity_offset, ring_offset, PCM_MEM_DEVICE, fp, &features_), "pcm_loam_frame_begin");
  }
  const pcm_loam_features_result& featuresResult() const { return features_; }

  // the loop of scan2MapOptimization; transformTobeMapped is updated in place.  false: too few features (left as it was).
  bool scan2MapOptimization(float transformTobeMapped[6]) {
    const int rc = pcm_loam_align(ctx_, &params_, transformTobeMapped, &last_);
    if (rc == PCM_ERR_TOO_FEW_FEATURES) return false;
    check(rc, "pcm_loam_align");
    for (int k = 0; k < 6; k++) transformTobeMapped[k] = last_.x[k];
    return true;
  }
  bool isDegenerate() const { return last_.degenerate != 0; }
  double cornerFitnessScore() const { return last_.corner_fitness; }   // Corner_fitness_score
  double surfFitnessScore() const { return last_.surf_fitness; }       // Surf_fitness_score
  int iterations() const { return last_.iterations; }
  const pcm_loam_result& result() const { return last_; }
  pcm_ctx* context() const { return ctx_; }   // for LoamKeyFrameMap, which works on the same context

private:
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  pcm_loam_params params_;
  pcm_loam_result last_{};
  pcm_loam_features_result features_{};
  std::vector<float> corner_xyzi_, surf_xyzi_;
};

// jueying_slam's key-frame clouds and surrounding-key-frame submap on the device, on the context of a LoamScanToMap, with the
// call shape of mapOptmization.cpp:
//     pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);                   // cornerCloudKeyFrames / surfCloudKeyFrames / cloudKeyPoses6D
//     keyframes.extractSurroundingKeyFrames(timeLaserInfoCur);               // :1224; the result is loam's maps (no setInputMaps)
//     if (loam.scan2MapOptimization(transformTobeMapped)) transformUpdate();
//     keyframes.saveKeyFrame(transformTobeMapped, timeLaserInfoCur);         // :1839-1840 after setInputScan: the features stay on the device
//     keyframes.correctPoses(poses, n);                                      // :1886-1917 after a loop closure
//     keyframes.loopFindNearKeyframes(cureKeyframeCloud, loopKeyCur, 0);     // :972
//     keyframes.loopFindNearKeyframesWithRespectTo(prevKeyframeCloud, loopKeyPre, historyKeyframeSearchNum, loopKeyCur);
//     if (keyframes.performLoopClosure(timeLaserInfoCur, &factor)) { ... }   // :619-733 on the device
//     keyframes.publishGlobalMap(globalMapKeyFramesDS);                      // :547-590
//     keyframes.exportMap(globalMapCloud);                                   // :524-542, what jueying.pcd holds
// Poses are transformTobeMapped vectors (roll, pitch, yaw, x, y, z).  The object does not own the context: it must not outlive `loam`.
template <typename PointT>
class LoamKeyFrameMap {
public:
  using Cloud = pcl::PointCloud<PointT>;
  using CloudConstPtr = typename Cloud::ConstPtr;

  explicit LoamKeyFrameMap(LoamScanToMap<PointT>& loam) : ctx_(loam.context()) { pcm_loam_default_submap_params(&params_); }

  void setSurroundingKeyframeSearchRadius(float v) { params_.search_radius = v; }   // surroundingKeyframeSearchRadius
  void setSurroundingKeyframeDensity(float v) { params_.keypose_density = v; }      // surroundingKeyframeDensity
  void setMappingCornerLeafSize(float v) { params_.corner_leaf = v; }               // mappingCornerLeafSize
  void setMappingSurfLeafSize(float v) { params_.surf_leaf = v; }                   // mappingSurfLeafSize
  void setLoopLeafSize(float v) { loop_leaf_ = v; }                                 // downSizeFilterICP (mappingSurfLeafSize); also performLoopClosure's leaf
  void setHistoryKeyframeSearchNum(int v) { loopParams().history_search_num = v; }  // historyKeyframeSearchNum
  void setHistoryKeyframeFitnessScore(float v) { loopParams().fitness_threshold = v; }   // historyKeyframeFitnessScore
  // the reference's values on first use; near_leaf is taken from setLoopLeafSize at every call
  pcm_loam_loop_params& loopParams() {
    if (!loop_params_set_) { pcm_loam_default_loop_params(&loop_params_); loop_params_set_ = true; }
    return loop_params_;
  }
  pcm_loam_submap_params& params() { return params_; }
  const pcm_loam_submap_result& result() const { return last_; }
  int size() const { return pcm_loam_keyframe_count(ctx_); }                        // cloudKeyPoses3D->size()

  // the scan the context holds (LoamScanToMap::setInputScan / setInputFeatures) becomes key frame size()
  void saveKeyFrame(const float pose[6], double time) {
    check(pcm_loam_keyframe_add(ctx_, pose, time, nullptr, 0, nullptr, 0, sizeof(PointT), PCM_MEM_HOST), "pcm_loam_keyframe_add");
  }
  void saveKeyFrame(const float pose[6], double time, const CloudConstPtr& corner, const CloudConstPtr& surf) {
    detail::pack_xyzi(*corner, buf_);
    detail::pack_xyzi(*surf, buf2_);
    check(pcm_loam_keyframe_add(ctx_, pose, time, buf_.data(), corner->size(), buf2_.data(), surf->size(), 4 * sizeof(float), PCM_MEM_HOST),
          "pcm_loam_keyframe_add");
  }
  // n x 6 floats for key frames 0 .. n - 1
  void correctPoses(const float* poses, int n) { check(pcm_loam_keyframe_set_poses(ctx_, 0, n, poses), "pcm_loam_keyframe_set_poses"); }
  void clear() { check(pcm_loam_keyframe_clear(ctx_), "pcm_loam_keyframe_clear"); }

  // true: the maps were rebuilt; false: nothing changed since the last call (or there is no key frame yet)
  bool extractSurroundingKeyFrames(double timeLaserInfoCur) {
    check(pcm_loam_submap_update(ctx_, &params_, timeLaserInfoCur, &last_), "pcm_loam_submap_update");
    return last_.rebuilt != 0;
  }
  int laserCloudCornerFromMapDSNum() const { return last_.num_corner_map; }
  int laserCloudSurfFromMapDSNum() const { return last_.num_surf_map; }

  void loopFindNearKeyframes(Cloud& nearKeyframes, int key, int searchNum) { near(nearKeyframes, key, searchNum, -1); }
  void loopFindNearKeyframesWithRespectTo(Cloud& nearKeyframes, int key, int searchNum, int wrtKey) { near(nearKeyframes, key, searchNum, wrtKey); }

  // What performLoopClosure pushes on its three queues (mapOptmization.cpp:724-726): loopIndexQueue's pair, loopPoseQueue's
  // poseFrom.between(poseTo) -- row-major 4 x 4 and (roll, pitch, yaw, x, y, z), for gtsam::Pose3(Rot3::RzRyRx(...), Point3(...)) --
  // and the variance that fills loopNoiseQueue's noiseModel::Diagonal::Variances.
  struct LoopFactor {
    std::pair<int, int> index{-1, -1};
    double between[16] = {};
    double between6[6] = {};
    float noise = 0.f;
  };
  const pcm_loam_loop_result& loopResult() const { return loop_last_; }
  // performLoopClosure :645-731 for a given pair, on the device (pcm_loam_loop_verify): true = the factor is in *out.  The
  // loopIndexContainer bookkeeping (:730) stays with the caller.
  bool performLoopClosure(int loopKeyCur, int loopKeyPre, LoopFactor* out) {
    loopParams().near_leaf = loop_leaf_;
    check(pcm_loam_loop_verify(ctx_, &loop_params_, loopKeyCur, loopKeyPre, &loop_last_), "pcm_loam_loop_verify");
    return take_factor(out);
  }
  // detectLoopClosureDistance (:638) and the verification in one call (pcm_loam_loop_closure); false also when there is no pair
  bool performLoopClosure(double timeLaserInfoCur, LoopFactor* out, float historyKeyframeSearchRadius = 10.0f, double historyKeyframeSearchTimeDiff = 30.0) {
    loopParams().near_leaf = loop_leaf_;
    check(pcm_loam_loop_closure(ctx_, &loop_params_, historyKeyframeSearchRadius, historyKeyframeSearchTimeDiff, timeLaserInfoCur, &loop_last_),
          "pcm_loam_loop_closure");
    return take_factor(out);
  }

  // performSCLoopClosure :750-834 for a pair Scan Context found, on the device (pcm_loam_sc_loop_verify): both near clouds under
  // key frame 0, point-to-point ICP (150 / 100 / 1e-6 / 1e-6), the fitness test; true = the factor is in *out (noise 0.5, to go under
  // mEstimator::Cauchy::Create(scLoopResult().cauchy_k)).  historyKeyframeSearchNum / FitnessScore / the leaf are the setters' above.
  pcm_loam_sc_loop_params& scLoopParams() {
    if (!sc_loop_params_set_) { pcm_loam_default_sc_loop_params(&sc_loop_params_); sc_loop_params_set_ = true; }
    return sc_loop_params_;
  }
  const pcm_loam_sc_loop_result& scLoopResult() const { return sc_loop_last_; }
  bool performSCLoopClosure(int loopKeyCur, int loopKeyPre, LoopFactor* out) {
    sync_sc_params();
    check(pcm_loam_sc_loop_verify(ctx_, &sc_loop_params_, loopKeyCur, loopKeyPre, &sc_loop_last_), "pcm_loam_sc_loop_verify");
    return take_sc_factor(out);
  }
  // detectLoopClosureID of the last descriptor (:741) and the verification in one call (pcm_loam_sc_loop_closure); false also
  // when there is no loop.  The loopIndexContainer insert (:840) stays with the caller.
  bool performSCLoopClosure(LoopFactor* out) {
    sync_sc_params();
    check(pcm_loam_sc_loop_closure(ctx_, &sc_loop_params_, &sc_loop_last_), "pcm_loam_sc_loop_closure");
    return take_sc_factor(out);
  }

  void setGlobalMapVisualizationSearchRadius(float v) { globalParams().search_radius = v; }   // globalMapVisualizationSearchRadius
  void setGlobalMapVisualizationPoseDensity(float v) { globalParams().keypose_density = v; }   // globalMapVisualizationPoseDensity
  void setGlobalMapVisualizationLeafSize(float v) { globalParams().leaf = v; }                 // globalMapVisualizationLeafSize
  // the reference's values on first use
  pcm_loam_global_params& globalParams() {
    if (!global_params_set_) { pcm_loam_default_global_params(&global_params_); global_params_set_ = true; }
    return global_params_;
  }
  const pcm_loam_global_result& globalResult() const { return global_last_; }
  // publishGlobalMap :555-588: globalMapKeyFramesDS (pcm_loam_global_map)
  void publishGlobalMap(Cloud& globalMapKeyFramesDS) {
    pcm_loam_global_params count = globalParams();
    count.leaf = 0.f;   // without a leaf and a buffer: the host-only query of points_in
    pcm_loam_global_result r{};
    const int rc = pcm_loam_global_map(ctx_, &count, nullptr, 0, PCM_MEM_HOST, &r);
    if (rc != PCM_OK && r.points_in == 0) check(rc, "pcm_loam_global_map");
    if (buf_.size() < 4 * r.points_in) buf_.resize(4 * r.points_in);
    check(pcm_loam_global_map(ctx_, &global_params_, buf_.data(), buf_.size() / 4, PCM_MEM_HOST, &global_last_), "pcm_loam_global_map");
    unpack(globalMapKeyFramesDS, global_last_.points_out);
  }
  // the same into a device buffer of `capacity` float4 (x, y, z, intensity) records, on the context's stream; returns the count
  size_t publishGlobalMap(void* device_out, size_t capacity) {
    check(pcm_loam_global_map(ctx_, &globalParams(), device_out, capacity, PCM_MEM_DEVICE, &global_last_), "pcm_loam_global_map");
    return global_last_.points_out;
  }
  // the saved map :530-541 of key frames [first, first + n) (n < 0: all from first): which 0 = globalCornerCloud, 1 =
  // globalSurfCloud, 2 = globalMapCloud (jueying.pcd when the range is the whole store)
  void exportMap(Cloud& out, int which = 2, int first = 0, int n = -1) {
    if (n < 0) n = size() - first;
    size_t total = 0;
    const int rc = pcm_loam_map_export(ctx_, which, first, n, nullptr, 0, PCM_MEM_HOST, &total);
    if (rc != PCM_OK && total == 0) check(rc, "pcm_loam_map_export");
    if (buf_.size() < 4 * total) buf_.resize(4 * total);
    check(pcm_loam_map_export(ctx_, which, first, n, buf_.data(), buf_.size() / 4, PCM_MEM_HOST, &total), "pcm_loam_map_export");
    unpack(out, total);
  }
  size_t exportMap(void* device_out, size_t capacity, int which, int first, int n) {
    size_t total = 0;
    check(pcm_loam_map_export(ctx_, which, first, n, device_out, capacity, PCM_MEM_DEVICE, &total), "pcm_loam_map_export");
    return total;
  }

private:
  // n (x, y, z, intensity) records of buf_ into a cloud, member by member
  void unpack(Cloud& out, size_t n) const {
    out.points.resize(n);
    for (size_t i = 0; i < n; i++) {
      PointT& q = out.points[i];
      q.x = buf_[4 * i]; q.y = buf_[4 * i + 1]; q.z = buf_[4 * i + 2]; q.intensity = buf_[4 * i + 3];
    }
  }
  void sync_sc_params() {
    scLoopParams().near_leaf = loop_leaf_;
    sc_loop_params_.history_search_num = loopParams().history_search_num;
    sc_loop_params_.fitness_threshold = loopParams().fitness_threshold;
  }
  bool take_sc_factor(LoopFactor* out) const {
    if (sc_loop_last_.status != PCM_LOAM_LOOP_ACCEPTED) return false;
    if (out) {
      out->index = std::make_pair((int)sc_loop_last_.key_cur, (int)sc_loop_last_.key_pre);
      for (int k = 0; k < 16; k++) out->between[k] = sc_loop_last_.between[k];
      for (int k = 0; k < 6; k++) out->between6[k] = sc_loop_last_.between6[k];
      out->noise = sc_loop_last_.noise_variance;
    }
    return true;
  }
  bool take_factor(LoopFactor* out) const {
    if (loop_last_.status != PCM_LOAM_LOOP_ACCEPTED) return false;
    if (out) {
      out->index = std::make_pair((int)loop_last_.key_cur, (int)loop_last_.key_pre);
      for (int k = 0; k < 16; k++) out->between[k] = loop_last_.between[k];
      for (int k = 0; k < 6; k++) out->between6[k] = loop_last_.between6[k];
      out->noise = loop_last_.noise_variance;
    }
    return true;
  }
  void near(Cloud& out, int key, int searchNum, int wrt) {
    // room for every point of the key frames in the window (the VoxelGrid can only shrink it), from the stored counts
    const int K = size();
    size_t total = 0;
    for (long long k = (long long)key - searchNum; k <= (long long)key + searchNum; ++k) {
      if (k < 0 || k >= K) continue;
      size_t nc = 0, ns = 0;
      check(pcm_loam_keyframe_get(ctx_, (int)k, nullptr, 0, nullptr, 0, &nc, &ns), "pcm_loam_keyframe_get");
      total += nc + ns;
    }
    if (buf_.size() < 4 * total) buf_.resize(4 * total);
    size_t n = 0;
    const int rc = pcm_loam_submap_near(ctx_, key, searchNum, wrt, loop_leaf_, buf_.data(), buf_.size() / 4, &n);
    check(rc, "pcm_loam_submap_near");
    unpack(out, n);
  }
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  pcm_loam_submap_params params_;
  pcm_loam_submap_result last_{};
  pcm_loam_loop_params loop_params_{};
  bool loop_params_set_ = false;
  pcm_loam_loop_result loop_last_{};
  pcm_loam_sc_loop_params sc_loop_params_{};
  bool sc_loop_params_set_ = false;
  pcm_loam_sc_loop_result sc_loop_last_{};
  float loop_leaf_ = 0.2f;
  pcm_loam_global_params global_params_{};
  bool global_params_set_ = false;
  pcm_loam_global_result global_last_{};
  std::vector<float> buf_, buf2_;
};

// jueying_slam's localisation map on the device, on the context of a LoamScanToMap, with the call shape of localization.cpp
// (DESIGN.md section 14):
//     pcm_amd::LoamDynamicMap<PointType> dynmap(loam);
//     for (const Area& a : all_Corner_areas) dynmap.addCornerArea(box_of(a), *cloud_of(a));     // once, instead of create_pcd per reload
//     for (const Area& a : all_Surf_areas) dynmap.addSurfArea(box_of(a), *cloud_of(a));
//     if (dynmap.needLoad(transformTobeMapped)) dynmap.load(transformTobeMapped);              // dynamic_load_map_run :295-311
//     dynmap.dynamic_load_map(transformTobeMapped);                                            // :256; the result is loam's maps
//     if (loam.scan2MapOptimization(transformTobeMapped)) transformUpdate();
//     dynmap.globalMap(ndt_target_device_buffer, capacity);                                    // :274-277, the "ndt" branch
// Tile clouds are repacked member by member (the PointXYZI rule of detail::pack_xyzi).  The object does not own the context.
template <typename PointT>
class LoamDynamicMap {
public:
  using Cloud = pcl::PointCloud<PointT>;

  explicit LoamDynamicMap(LoamScanToMap<PointT>& loam) : ctx_(loam.context()) { pcm_loam_default_dynmap_params(&params_); }

  void setMaxRange(float v) { params_.max_range = v; }     // max_range
  void setMargin(int v) { params_.margin = v; }            // globalmap_server/margin
  void setAreaSize(int v) { params_.area_size = v; }       // globalmap_server/area_size
  void setCropX(bool v) { params_.crop_x = v ? 1 : 0; }    // false: only the y window has an effect, as the reference behaves
  pcm_loam_dynmap_params& params() { return params_; }
  const pcm_loam_dynmap_load_result& loadResult() const { return load_; }
  const pcm_loam_dynmap_crop_result& result() const { return crop_; }

  // box: x_min, y_min, z_min, x_max, y_max, z_max of the area list; returns the tile's index in its list
  int addCornerArea(const double box[6], const Cloud& cloud) { return add(0, box, cloud); }
  int addSurfArea(const double box[6], const Cloud& cloud) { return add(1, box, cloud); }
  int cornerAreas() const { return pcm_loam_tile_count(ctx_, 0); }
  int surfAreas() const { return pcm_loam_tile_count(ctx_, 1); }
  void clear() { check(pcm_loam_tile_clear(ctx_), "pcm_loam_tile_clear"); }

  bool needLoad(const float transformTobeMapped[6]) {
    const int rc = pcm_loam_dynmap_need_load(ctx_, &params_, transformTobeMapped);
    if (rc < 0) check(rc, "pcm_loam_dynmap_need_load");
    return rc == 1;
  }
  // true: the selection changed
  bool load(const float transformTobeMapped[6]) {
    check(pcm_loam_dynmap_load(ctx_, &params_, transformTobeMapped, &load_), "pcm_loam_dynmap_load");
    return load_.changed != 0;
  }
  // true: the maps were rebuilt; false: same tiles through the same window as the last call
  bool dynamic_load_map(const float pose[6]) {
    check(pcm_loam_dynmap_crop(ctx_, &params_, pose, &crop_), "pcm_loam_dynmap_crop");
    return crop_.rebuilt != 0;
  }
  int laserCloudCornerFromMapDSNum() const { return crop_.num_corner; }
  int laserCloudSurfFromMapDSNum() const { return crop_.num_surf; }

  // A fleet on one site map: this map reads the areas `other` holds from now on (pcm_loam_tile_share); they exist once on the
  // device.  load() before the next dynamic_load_map.  While areas are shared, add*Area and buildFromKeyFrames throw on every
  // holder, and clear() detaches this map alone.
  void shareTilesWith(LoamDynamicMap& other) { check(pcm_loam_tile_share(ctx_, other.ctx_), "pcm_loam_tile_share"); }
  int tileShareCount() const {
    const int rc = pcm_loam_tile_share_count(ctx_);
    if (rc < 0) check(rc, "pcm_loam_tile_share_count");
    return rc;
  }
  // dynamic_load_map of several maps in one round of launches (pcm_loam_dynmap_crop_batch) with the parameters of maps[0]:
  // poses holds 6 floats per map; results (may be null) takes one record per map, and each map keeps its own as result().  A map
  // that could not be cropped carries its code in its record's status while the others complete; returns the first such code.
  static int cropBatch(const std::vector<LoamDynamicMap*>& maps, const float* poses, pcm_loam_dynmap_crop_result* results = nullptr) {
    if (maps.empty()) return PCM_ERR_INVALID_ARGUMENT;
    std::vector<pcm_ctx*> ctxs(maps.size());
    for (size_t i = 0; i < maps.size(); i++) ctxs[i] = maps[i]->ctx_;
    std::vector<pcm_loam_dynmap_crop_result> rec(maps.size());
    const int rc = pcm_loam_dynmap_crop_batch(ctxs.data(), (int)maps.size(), &maps[0]->params_, poses, rec.data());
    bool any = false;
    for (size_t i = 0; i < maps.size(); i++) {
      if (rec[i].status == PCM_OK) maps[i]->crop_ = rec[i]; else any = true;
      if (results) results[i] = rec[i];
    }
    if (rc != PCM_OK && !any) maps[0]->check(rc, "pcm_loam_dynmap_crop_batch");   // the call as a whole failed
    return rc;
  }

  // The hand-over from a mapping session on the same LoamScanToMap: the key frames of `keyframes` [first, first + n) (n < 0: all
  // from first), cut into area tiles on the device under their current poses (pcm_loam_tiles_build).  Replaces both area lists;
  // the map never visits the host.  params NULL: tile_size 50, leaves 0.2.
  const pcm_loam_tiles_result& buildFromKeyFrames(LoamKeyFrameMap<PointT>& keyframes, const pcm_loam_tiles_params* params = nullptr, int first = 0, int n = -1) {
    if (n < 0) n = keyframes.size() - first;
    check(pcm_loam_tiles_build(ctx_, params, first, n, &tiles_), "pcm_loam_tiles_build");
    return tiles_;
  }
  // area `index` of a list (0 corner, 1 surf): its box (the area list's columns), its index pair and its number of points
  size_t tileInfo(int which, int index, double box[6], int32_t ixy[2] = nullptr) const {
    size_t n = 0;
    check(pcm_loam_tile_info(ctx_, which, index, box, ixy, &n), "pcm_loam_tile_info");
    return n;
  }
  // the area's cloud on the host: what the caller writes to the PCD file the area list names
  void getTile(int which, int index, Cloud& out) {
    const size_t cap = tileInfo(which, index, nullptr);
    if (buf_.size() < 4 * cap) buf_.resize(4 * cap);
    size_t n = 0;
    check(pcm_loam_tile_get(ctx_, which, index, buf_.data(), buf_.size() / 4, PCM_MEM_HOST, &n), "pcm_loam_tile_get");
    out.points.resize(n);
    for (size_t i = 0; i < n; i++) {
      PointT& q = out.points[i];
      q.x = buf_[4 * i]; q.y = buf_[4 * i + 1]; q.z = buf_[4 * i + 2]; q.intensity = buf_[4 * i + 3];
    }
  }
  // ... or into a device buffer of `capacity` points; returns the number of points
  size_t getTile(int which, int index, void* device_out, size_t capacity) {
    size_t n = 0;
    check(pcm_loam_tile_get(ctx_, which, index, device_out, capacity, PCM_MEM_DEVICE, &n), "pcm_loam_tile_get");
    return n;
  }

  // globalMap as (x, y, z, intensity) records into a device buffer of `capacity` points (e.g. the target of an NDT context,
  // then pcm_set_target with PCM_MEM_DEVICE and a stride of 16); returns the number of points
  size_t globalMap(void* device_out, size_t capacity) {
    size_t n = 0;
    check(pcm_loam_dynmap_global(ctx_, device_out, capacity, &n, PCM_MEM_DEVICE), "pcm_loam_dynmap_global");
    return n;
  }
  // globalMap as a PCL cloud on the host (publishCloud)
  void globalMap(Cloud& out) {
    const size_t cap = (size_t)crop_.num_corner + (size_t)crop_.num_surf;
    if (buf_.size() < 4 * cap) buf_.resize(4 * cap);
    size_t n = 0;
    check(pcm_loam_dynmap_global(ctx_, buf_.data(), buf_.size() / 4, &n, PCM_MEM_HOST), "pcm_loam_dynmap_global");
    out.points.resize(n);
    for (size_t i = 0; i < n; i++) {
      PointT& q = out.points[i];
      q.x = buf_[4 * i]; q.y = buf_[4 * i + 1]; q.z = buf_[4 * i + 2]; q.intensity = buf_[4 * i + 3];
    }
  }

private:
  int add(int which, const double box[6], const Cloud& cloud) {
    detail::pack_xyzi(cloud, buf_);
    const int rc = pcm_loam_tile_add(ctx_, which, box, buf_.data(), cloud.points.size(), 4 * sizeof(float), PCM_MEM_HOST);
    if (rc < 0) check(rc, "pcm_loam_tile_add");
    return rc;
  }
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  pcm_loam_dynmap_params params_;
  pcm_loam_dynmap_load_result load_{};
  pcm_loam_dynmap_crop_result crop_{};
  pcm_loam_tiles_result tiles_{};
  std::vector<float> buf_;
};

// jueying_slam's SCManager (include/Scancontext.h) on the context of a LoamScanToMap, with SCManager's user-side names:
//     scManager.makeAndSaveScancontextAndKeys(*thisRawCloudKeyFrame);           // saveKeyFramesAndFactor, mapOptmization.cpp:1857
//     auto detectResult = scManager.detectLoopClosureID();                      // :741: (nearest node or -1, relative yaw)
// The descriptors live on the device (pcm_loam_sc_*).  Free of Eigen: getConstRefRecentSCD returns the last
// descriptor as column-major doubles (num_ring x num_sector, the memory of the reference's MatrixXd).
template <typename PointT>
class LoamScanContext {
public:
  using Cloud = pcl::PointCloud<PointT>;

  explicit LoamScanContext(LoamScanToMap<PointT>& loam) : ctx_(loam.context()) { pcm_loam_default_sc_params(&params_); }
  pcm_loam_sc_params& params() { return params_; }
  const pcm_loam_sc_result& result() const { return last_; }
  int size() const { return pcm_loam_sc_count(ctx_); }                              // polarcontexts_.size()
  void clear() { check(pcm_loam_sc_clear(ctx_), "pcm_loam_sc_clear"); }

  // SINGLE_SCAN_FULL: the cloud goes through the VoxelGrid of params().leaf on the device (downSizeFilterSC)
  void makeAndSaveScancontextAndKeys(const Cloud& scan) {
    detail::pack_xyzi(scan, buf_);
    check(pcm_loam_sc_add(ctx_, &params_, PCM_LOAM_SC_POINTS, -1, buf_.data(), scan.points.size(), 4 * sizeof(float), PCM_MEM_HOST, nullptr), "pcm_loam_sc_add");
  }
  // SINGLE_SCAN_FEAT: the stored surf cloud of a key frame of LoamKeyFrameMap, without leaving the device
  void makeAndSaveScancontextAndKeysOfKeyFrame(int key) {
    check(pcm_loam_sc_add(ctx_, &params_, PCM_LOAM_SC_KEYFRAME_SURF, key, nullptr, 0, 0, PCM_MEM_HOST, nullptr), "pcm_loam_sc_add");
  }
  // a descriptor of a saved map: column-major doubles
  void putScancontext(const std::vector<double>& desc) { check(pcm_loam_sc_put(ctx_, desc.data(), params_.num_ring, params_.num_sector), "pcm_loam_sc_put"); }

  std::pair<int, float> detectLoopClosureID() {
    check(pcm_loam_sc_detect(ctx_, &params_, &last_), "pcm_loam_sc_detect");
    return std::pair<int, float>(last_.loop_id, last_.yaw_diff_rad);
  }
  std::pair<double, int> distanceBtnScanContext(int i, int j) {
    double d = 0.0;
    int32_t s = 0;
    check(pcm_loam_sc_distance(ctx_, &params_, i, j, &d, &s), "pcm_loam_sc_distance");
    return std::pair<double, int>(d, (int)s);
  }
  const std::vector<double>& getConstRefRecentSCD() {
    int R = 0, S = 0;
    check(pcm_loam_sc_shape(ctx_, &R, &S), "pcm_loam_sc_shape");
    recent_.assign((size_t)R * (size_t)S, 0.0);
    if (size() > 0) check(pcm_loam_sc_get(ctx_, size() - 1, recent_.data(), nullptr, nullptr), "pcm_loam_sc_get");
    return recent_;
  }
  // detectLoopClosureDistance (mapOptmization.cpp:843-880) on LoamKeyFrameMap's key poses; the loopIndexContainer test stays with
  // the caller
  bool detectLoopClosureDistance(int* latestID, int* closestID, double timeLaserInfoCur, float historyKeyframeSearchRadius = 10.0f,
                                 double historyKeyframeSearchTimeDiff = 30.0) {
    int32_t cur = -1, pre = -1;
    const int rc = pcm_loam_loop_detect_distance(ctx_, historyKeyframeSearchRadius, historyKeyframeSearchTimeDiff, timeLaserInfoCur, &cur, &pre);
    if (rc < 0) check(rc, "pcm_loam_loop_detect_distance");
    if (rc != 1) return false;
    *latestID = cur; *closestID = pre;
    return true;
  }

private:
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  pcm_loam_sc_params params_;
  pcm_loam_sc_result last_{};
  std::vector<float> buf_;
  std::vector<double> recent_;
};

// pcl::VoxelGridLarge (jueying_slam/include/voxel_grid_large.h: the VoxelGrid that cuts a cloud whose leaf index overflows along its
// longest axis and filters the halves on their own) on the device, with the call surface its users have (setLeafSize,
// setInputCloud, filter; pcd2map's and the map server's VoxelGrid take the same three calls).  A point is handed over as the
// record of floats it is -- x y z first, every float of it averaged, padding included -- so PointT holds 3..16 floats and
// nothing else (PointXYZ, PointXYZI, PointXYZINormal).  One leaf size for the three axes, as every call site of the reference
// sets it; a leaf index that cannot be resolved (pcm_amd.h) throws.
template <typename PointT>
class VoxelGridLarge {
public:
  using Cloud = pcl::PointCloud<PointT>;
  static_assert(sizeof(PointT) % sizeof(float) == 0 && sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) <= 16 * sizeof(float), "a point of 3..16 floats");

  explicit VoxelGridLarge(int device = 0) : ctx_(pcm_create(device, nullptr)) {
    if (!ctx_) throw std::runtime_error("pcm_create failed");
  }
  ~VoxelGridLarge() { if (ctx_) pcm_destroy(ctx_); }
  VoxelGridLarge(const VoxelGridLarge&) = delete;
  VoxelGridLarge& operator=(const VoxelGridLarge&) = delete;

  void setLeafSize(float lx, float ly, float lz) {
    if (lx != ly || lx != lz) throw std::invalid_argument("pcm_amd::VoxelGridLarge: one leaf size for the three axes");
    leaf_ = lx;
  }
  void setInputCloud(const typename Cloud::ConstPtr& cloud) { input_ = cloud; }
  void filter(Cloud& output) {
    output.points.clear();
    if (!input_ || input_->points.empty()) return;     // "No input dataset given!": an empty output
    const size_t n = input_->points.size();
    std::vector<PointT> cells(n);
    const int rc = pcm_voxel_downsample_large(ctx_, input_->points.data(), n, sizeof(PointT), PCM_MEM_HOST, leaf_, cells.data(), n, &result_);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_voxel_downsample_large: ") + pcm_last_error(ctx_));
    cells.resize((size_t)result_.cells);
    output.points.assign(cells.begin(), cells.end());
  }
  const pcm_voxel_large_result& result() const { return result_; }   // pieces, depth, levels of the last filter()

private:
  pcm_ctx* ctx_ = nullptr;
  float leaf_ = 0.f;
  typename Cloud::ConstPtr input_;
  pcm_voxel_large_result result_{};
};

// pcl::ApproximateVoxelGrid on the device (pcm_approx_voxel_downsample; the rules are in pcm_amd.h), with the call surface
// fast_gicp/src/align.cpp:136-147 and kitti.cpp:81 use: setLeafSize, setInputCloud, filter.  A point is the record of floats it
// is, as for VoxelGridLarge; one leaf size for the three axes, as every call site sets it -- unequal leaves throw.
template <typename PointT>
class ApproximateVoxelGrid {
public:
  using Cloud = pcl::PointCloud<PointT>;
  static_assert(sizeof(PointT) % sizeof(float) == 0 && sizeof(PointT) >= 3 * sizeof(float) && sizeof(PointT) <= 16 * sizeof(float), "a point of 3..16 floats");

  explicit ApproximateVoxelGrid(int device = 0) : ctx_(pcm_create(device, nullptr)) {
    if (!ctx_) throw std::runtime_error("pcm_create failed");
  }
  ~ApproximateVoxelGrid() { if (ctx_) pcm_destroy(ctx_); }
  ApproximateVoxelGrid(const ApproximateVoxelGrid&) = delete;
  ApproximateVoxelGrid& operator=(const ApproximateVoxelGrid&) = delete;

  void setLeafSize(float lx, float ly, float lz) {
    if (lx != ly || lx != lz) throw std::invalid_argument("pcm_amd::ApproximateVoxelGrid: one leaf size for the three axes");
    leaf_ = lx;
  }
  // a cloud of any pointer type that reaches a const cloud (align.cpp hands a PointCloud::Ptr over)
  void setInputCloud(const typename Cloud::ConstPtr& cloud) { input_ = cloud; }
  void filter(Cloud& output) {
    output.points.clear();
    dropped_ = 0;
    if (!input_ || input_->points.empty()) return;     // "No input dataset given!": an empty output
    const size_t n = input_->points.size();
    std::vector<PointT> records(n);
    size_t m = 0;
    const int rc = pcm_approx_voxel_downsample(ctx_, input_->points.data(), n, sizeof(PointT), PCM_MEM_HOST, leaf_, records.data(), n, &m, &dropped_);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_approx_voxel_downsample: ") + pcm_last_error(ctx_));
    records.resize(m);
    output.points.assign(records.begin(), records.end());
  }
  size_t dropped() const { return dropped_; }   // points of the last filter() without a voxel (non-finite, or beyond the index range)

private:
  pcm_ctx* ctx_ = nullptr;
  float leaf_ = 0.f;
  typename Cloud::ConstPtr input_;
  size_t dropped_ = 0;
};

// jueying_slam's 2D occupancy mapping tool (src/tool/occupancy_mapping) on the device: OccupancyServer's getScan + processScan per
// cloud, getGridMap and saveMap's image.  Constructed alone it owns a context (the online node, OccupancyServerRealTime: tf lookups
// and the sensor-tilt pre-rotation stay with the caller); constructed over a LoamScanToMap it maps that context's key frames in
// place (the offline node with two files per frame, and the rebuild after a loop closure).  File writing stays with the caller.
template <typename PointT>
class OccupancyMap2D {
public:
  using Cloud = pcl::PointCloud<PointT>;

  explicit OccupancyMap2D(int device = 0) : ctx_(pcm_create(device, nullptr)), own_(true) {
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    pcm_occ_default_params(&params_);
  }
  explicit OccupancyMap2D(LoamScanToMap<PointT>& loam) : ctx_(loam.context()), own_(false) { pcm_occ_default_params(&params_); }
  ~OccupancyMap2D() { if (own_ && ctx_) pcm_destroy(ctx_); }
  OccupancyMap2D(const OccupancyMap2D&) = delete;
  OccupancyMap2D& operator=(const OccupancyMap2D&) = delete;

  pcm_occ_params& params() { return params_; }             // read by the next initializeMap()
  void initializeMap() { check(pcm_occ_reset(ctx_, &params_), "pcm_occ_reset"); }
  // getScan + processScan; robot_pose = roll, pitch, yaw, x, y, z
  void processCloud(const Cloud& cloud, const std::vector<double>& robot_pose) {
    detail::pack_xyzi(cloud, buf_);
    float pose[6];
    for (int k = 0; k < 6; k++) pose[k] = (float)robot_pose[(size_t)k];
    const size_t n = cloud.points.size();
    check(pcm_occ_insert_scans(ctx_, buf_.data(), &n, pose, 1, 4 * sizeof(float), PCM_MEM_HOST), "pcm_occ_insert_scans");
  }
  // key frames first .. first + n - 1 of LoamKeyFrameMap, corner and surf cloud as one scan, without leaving the device
  void processKeyFrames(int first, int n) { check(pcm_occ_insert_keyframes(ctx_, first, n), "pcm_occ_insert_keyframes"); }
  // nav_msgs/OccupancyGrid: info.width / height / resolution / origin.position and data
  void getGridMap(std::vector<int8_t>* data, int* width, int* height, double* origin_x, double* origin_y, double* resolution) {
    int32_t w = 0, h = 0;
    check(pcm_occ_info(ctx_, &w, &h, origin_x, origin_y, resolution, nullptr), "pcm_occ_info");
    data->assign((size_t)w * (size_t)h, (int8_t)-1);
    check(pcm_occ_get_map(ctx_, data->data(), data->size()), "pcm_occ_get_map");
    *width = w; *height = h;
  }
  // the body of saveMap's P5 image (after the "P5 ... 255" header), rows top-down
  void getPgm(std::vector<uint8_t>* bytes) {
    int32_t w = 0, h = 0;
    check(pcm_occ_info(ctx_, &w, &h, nullptr, nullptr, nullptr, nullptr), "pcm_occ_info");
    bytes->assign((size_t)w * (size_t)h, (uint8_t)205);
    check(pcm_occ_get_pgm(ctx_, bytes->data(), bytes->size()), "pcm_occ_get_pgm");
  }

private:
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  bool own_ = false;
  pcm_occ_params params_;
  std::vector<float> buf_;
};

// octomap_server's node (src/tool/octomap_server) on the device: insertCloudCallback + insertScan per cloud, the projected 2D map
// and map_saver's files.  The setters carry the node's parameter names; they are read by the next reset(),
// which the first insertCloud() runs when nothing did.  Constructed alone it owns a context; constructed over a LoamScanToMap it
// maps that context's key frames in place.  tf lookups and the ground segmentation (filter_ground) stay with the caller.
template <typename PointT>
class OccupancyMap3D {
public:
  using Cloud = pcl::PointCloud<PointT>;
  struct ProjectedMap {   // nav_msgs/OccupancyGrid
    std::vector<int8_t> data;
    int width = 0, height = 0;
    double resolution = 0, origin_x = 0, origin_y = 0;
  };

  explicit OccupancyMap3D(int device = 0) : ctx_(pcm_create(device, nullptr)), own_(true) {
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    pcm_octo_default_params(&params_);
  }
  explicit OccupancyMap3D(LoamScanToMap<PointT>& loam) : ctx_(loam.context()), own_(false) { pcm_octo_default_params(&params_); }
  ~OccupancyMap3D() { if (own_ && ctx_) pcm_destroy(ctx_); }
  OccupancyMap3D(const OccupancyMap3D&) = delete;
  OccupancyMap3D& operator=(const OccupancyMap3D&) = delete;

  pcm_octo_params& params() { return params_; }
  void setResolution(double res) { params_.resolution = res; }
  void setSensorModel(double hit, double miss, double min, double max) { params_.prob_hit = hit; params_.prob_miss = miss; params_.clamp_min = min; params_.clamp_max = max; }
  void setMaxRange(double max_range) { params_.max_range = max_range; }
  void setMinRange(double min_range) { params_.min_range = min_range; }
  void setPointcloudZ(double min_z, double max_z) { params_.pointcloud_min_z = min_z; params_.pointcloud_max_z = max_z; }
  void setOccupancyZ(double min_z, double max_z) { params_.occupancy_min_z = min_z; params_.occupancy_max_z = max_z; }
  void setFilterSpeckles(bool on) { params_.filter_speckles = on ? 1 : 0; }
  void setMinSize(double min_x_size, double min_y_size) { params_.min_x_size = min_x_size; params_.min_y_size = min_y_size; }
  void reset() { check(pcm_octo_reset(ctx_, &params_), "pcm_octo_reset"); ready_ = true; }

  // insertCloudCallback: the cloud in the sensor frame, sensor_to_world as the tf lookup gave it; every point non-ground
  pcm_octo_insert_result insertCloud(const Cloud& cloud, const Eigen::Matrix4f& sensor_to_world) { return insertCloud(Cloud(), cloud, sensor_to_world); }
  // the same with the caller's own ground / non-ground split
  pcm_octo_insert_result insertCloud(const Cloud& ground, const Cloud& nonground, const Eigen::Matrix4f& sensor_to_world) {
    if (!ready_) reset();
    detail::pack_xyzi(ground, gbuf_);
    detail::pack_xyzi(nonground, buf_);
    float T[16], origin[3];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) T[4 * r + c] = sensor_to_world(r, c);
    for (int r = 0; r < 3; r++) origin[r] = sensor_to_world(r, 3);
    pcm_octo_insert_result res;
    check(pcm_octo_insert_scan(ctx_, gbuf_.data(), ground.points.size(), buf_.data(), nonground.points.size(), 4 * sizeof(float), PCM_MEM_HOST, origin, T, &res),
          "pcm_octo_insert_scan");
    return res;
  }
  // key frames first .. first + n - 1 of LoamKeyFrameMap, one scan each, without leaving the device
  void insertKeyFrames(int first, int n) {
    if (!ready_) reset();
    check(pcm_octo_insert_keyframes(ctx_, first, n), "pcm_octo_insert_keyframes");
  }
  pcm_octo_map_info info() {
    pcm_octo_map_info i;
    check(pcm_octo_info(ctx_, &i), "pcm_octo_info");
    return i;
  }
  // projected_map
  ProjectedMap projectedMap() {
    ProjectedMap m;
    pcm_octo_grid_info g;
    check(pcm_octo_project(ctx_, &g, nullptr, 0, PCM_MEM_HOST), "pcm_octo_project");
    m.width = g.width; m.height = g.height; m.resolution = g.resolution; m.origin_x = g.origin_x; m.origin_y = g.origin_y;
    m.data.assign((size_t)g.width * (size_t)g.height, (int8_t)-1);
    if (!m.data.empty()) check(pcm_octo_project(ctx_, &g, m.data.data(), m.data.size(), PCM_MEM_HOST), "pcm_octo_project");
    return m;
  }
  // octomap_point_cloud_centers
  void occupiedCenters(Cloud* out) {
    size_t n = (size_t)info().occupied;   // an upper bound: the z window and the speckle filter only take away
    buf_.assign(4 * n, 0.f);
    if (n) check(pcm_octo_get_occupied(ctx_, buf_.data(), n, PCM_MEM_HOST, &n), "pcm_octo_get_occupied");
    out->points.resize(n);
    for (size_t i = 0; i < n; i++) { out->points[i].x = buf_[4 * i]; out->points[i].y = buf_[4 * i + 1]; out->points[i].z = buf_[4 * i + 2]; }
  }
  // map_saver: <mapname>.pgm and <mapname>.yaml; false when there is no map yet or a file cannot be written
  bool saveMap(const std::string& mapname) {
    const ProjectedMap m = projectedMap();
    if (m.data.empty()) return false;
    std::vector<uint8_t> bytes(m.data.size(), (uint8_t)205);
    check(pcm_octo_get_pgm(ctx_, bytes.data(), bytes.size(), PCM_MEM_HOST), "pcm_octo_get_pgm");
    const std::string pgm = mapname + ".pgm", yaml = mapname + ".yaml";
    FILE* out = fopen(pgm.c_str(), "w");
    if (!out) return false;
    fprintf(out, "P5\n# CREATOR: map_saver.cpp %.3f m/pix\n%d %d\n255\n", m.resolution, m.width, m.height);
    fwrite(bytes.data(), 1, bytes.size(), out);
    fclose(out);
    FILE* y = fopen(yaml.c_str(), "w");
    if (!y) return false;
    fprintf(y, "image: %s\nresolution: %f\norigin: [%f, %f, 0.00]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n\n", pgm.c_str(), m.resolution, m.origin_x,
            m.origin_y);
    fclose(y);
    return true;
  }

private:
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  bool own_ = false, ready_ = false;
  pcm_octo_params params_;
  std::vector<float> buf_, gbuf_;
};

// jueying_slam's LOAM front end (imageProjection.cpp:736-823, featureExtraction.cpp:84-247, mapOptmization.cpp:1232-1247) on the
// device, for callers that want the features on the host.  PointIn: the driver's ring-tagged point (members x y z, intensity as
// uint8, ring as uint16, e.g. imageProjection.cpp's PointXYZIRT); PointOut: PointType (x y z intensity).  One object per node: it
// holds the nodes' cross-frame arrays.  The setters are named after ParamServer's members (utility.h:223-272).
// With IMU / odometry queues the scan is motion-compensated first (an option of this library: the reference's deskewPoint is the
// identity as written).  cloudHandler's order (imageProjection.cpp:238-262):
//     // cachePointCloud: the queueing (cloudQueue, timeScanCur, timeScanNext) is the caller's; the per-point part -- the ring, the
//     // time and the NaN removal of the RoboSense types -- runs on the device from the message's bytes:
//     fe.setLidarType(PCM_LOAM_LIDAR_RSLIDAR_16); fe.setTimeField(timeField);          // utility.h:227-243, once
//     fe.cachePointCloud(currentCloudMsg);     // laserCloudIn on the device; or, with the tables set, fe.frameBegin(currentCloudMsg)
//     pcm_amd::LoamDeskewTables tables;
//     if (!fe.deskewInfo(timeScanCur, timeScanNext, imu.data(), imu.size(), odom.data(), odom.size(), &tables)) return;   // "Waiting for IMU data ..."
//     imu.erase(imu.begin(), imu.begin() + tables.info.imu_skipped);                  // the pops of imuDeskewInfo / odomDeskewInfo
//     odom.erase(odom.begin(), odom.begin() + tables.info.odom_skipped);
//     fe.setDeskew(tables, offsetof(PointXYZIRT, timestamp));
//     fe.extract(laserCloudIn, corner, surf);                                         // projectPointCloud with the live deskewPoint, ...
//     fe.clearDeskew();                                                               // resetParameters
// imuRollInit / initialGuess* need tf's getRPY and stay with the caller (tables.info.start_odom_index names startOdomMsg).
struct LoamDeskewTables {
  std::vector<double> imu, odom;     // four rows each: time, x, y, z
  pcm_loam_deskew desc{};            // points into imu / odom
  pcm_loam_deskew_result info{};
};

template <typename PointIn, typename PointOut = pcl::PointXYZI>
class LoamFeatureExtraction {
public:
  using CloudIn = pcl::PointCloud<PointIn>;
  using CloudOut = pcl::PointCloud<PointOut>;

  explicit LoamFeatureExtraction(int device = 0) {
    pcm_config cfg;
    pcm_default_config(&cfg);
    cfg.model = PCM_MODEL_LOAM;
    ctx_ = pcm_create(device, &cfg);
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    pcm_loam_default_feature_params(&params_);
  }
  ~LoamFeatureExtraction() { pcm_destroy(ctx_); }
  LoamFeatureExtraction(const LoamFeatureExtraction&) = delete;
  LoamFeatureExtraction& operator=(const LoamFeatureExtraction&) = delete;

  void setNScan(int v) { params_.n_scan = v; }                         // N_SCAN
  void setHorizonScan(int v) { params_.horizon_scan = v; }             // Horizon_SCAN
  void setDownsampleRate(int v) { params_.downsample_rate = v; }       // downsampleRate
  void setAreaNum(int v) { params_.area_num = v; }                     // area_num
  void setMinRange(float v) { params_.min_range = v; }                 // min_range
  void setMaxRange(float v) { params_.max_range = v; }                 // max_range
  void setEdgeThreshold(float v) { params_.edge_threshold = v; }       // edgeThreshold
  void setSurfThreshold(float v) { params_.surf_threshold = v; }       // surfThreshold
  void setOdometrySurfLeafSize(float v) { params_.odometry_surf_leaf = v; }     // odometrySurfLeafSize
  void setMappingCornerLeafSize(float v) { params_.mapping_corner_leaf = v; }   // mappingCornerLeafSize (0: no down-sampling)
  void setMappingSurfLeafSize(float v) { params_.mapping_surf_leaf = v; }       // mappingSurfLeafSize (localisation: x 1.5)
  const pcm_loam_feature_params& params() const { return params_; }
  const pcm_loam_features_result& result() const { return last_; }

  // deskewInfo (imageProjection.cpp:483-642; timeScanNext = +inf: new_localization.cpp:1733-1886): false while waiting for IMU data
  static bool deskewInfo(double timeScanCur, double timeScanNext, const pcm_loam_imu_sample* imu, size_t nImu, const pcm_loam_odom_sample* odom, size_t nOdom,
                         LoamDeskewTables* out) {
    pcm_loam_deskew_input in{};
    in.time_scan_cur = timeScanCur; in.time_scan_next = timeScanNext;
    in.imu = imu; in.odom = odom; in.n_imu = (int32_t)nImu; in.n_odom = (int32_t)nOdom;
    const size_t ci = nImu < 1 ? 1 : nImu > 1024 ? 1024 : nImu, co = nOdom < 1 ? 1 : nOdom > 1024 ? 1024 : nOdom;
    out->imu.assign(4 * ci, 0.0);
    out->odom.assign(4 * co, 0.0);
    const int rc = pcm_loam_deskew_tables(&in, out->imu.data(), ci, out->odom.data(), co, &out->desc, &out->info);
    if (rc != PCM_OK) throw std::runtime_error(rc == PCM_ERR_UNSUPPORTED ? "pcm_loam_deskew_tables: more than 1024 table entries" : "pcm_loam_deskew_tables: bad input");
    return out->info.status == PCM_LOAM_DESKEW_READY;
  }
  // the tables of the next extract() calls; timeOffset / timeKind: where a point's stamp lies (PCM_LOAM_TIME_*)
  void setDeskew(const LoamDeskewTables& t, size_t timeOffset, int timeKind = PCM_LOAM_TIME_DOUBLE) {
    deskew_ = t;
    const size_t ci = deskew_.imu.size() / 4, co = deskew_.odom.size() / 4;
    pcm_loam_deskew& d = deskew_.desc;
    if (d.n_imu) { d.imu_time = deskew_.imu.data(); d.imu_rot_x = d.imu_time + ci; d.imu_rot_y = d.imu_time + 2 * ci; d.imu_rot_z = d.imu_time + 3 * ci; }
    if (d.n_odom) { d.odom_time = deskew_.odom.data(); d.odom_incre_x = d.odom_time + co; d.odom_incre_y = d.odom_time + 2 * co; d.odom_incre_z = d.odom_time + 3 * co; }
    d.time_offset_bytes = timeOffset;
    d.time_kind = timeKind;
    have_deskew_ = true;
  }
  void clearDeskew() { have_deskew_ = false; }

  // cachePointCloud's per-point part on the device (imageProjection.cpp:258-479, new_localization.cpp:1560-1731; DESIGN.md section
  // 36).  Msg: sensor_msgs::PointCloud2 or anything with its members (fields[].name / .offset / .datatype, height, width, point_step,
  // is_dense, data); no ROS header enters here.
  void setLidarType(int v) { lidar_type_ = v; }                        // mlidar_type: PCM_LOAM_LIDAR_* (utility.h:116-121, default rslidar_ruby :227)
  void setRecordKind(int v) { record_kind_ = v; }                      // PCM_LOAM_CLOUD_MAPPING (imageProjection's struct) or _LOCALIZATION
  void setTimeField(const std::string& v) { time_field_ = v; }         // timeField (utility.h:243, default "time")
  // The descriptor of a message.  The ring of rslidar_16 / rslidar_ruby is synthesised on every frame (:328, :369); rslidar_32's
  // when the message lacks the ring or the time field (imageProjection.cpp:437) or always (new_localization.cpp:1692), by record
  // kind.  The time of a RoboSense message without a time field is synthesised ON EVERY FRAME: the reference does it on the first
  // frame only (deskewFlag turns 1) and leaves later frames with whatever fromROSMsg left in the re-used cloud; a caller that
  // wants that sets synth_time = 0 in the descriptor of later frames and calls pcm_loam_frame_begin_cloud itself.
  template <typename Msg>
  pcm_loam_cloud_desc cloudDesc(const Msg& msg) const {
    pcm_loam_cloud_desc d{};
    d.height = msg.height; d.width = msg.width; d.point_step = msg.point_step;
    d.ring_offset_bytes = PCM_LOAM_FIELD_ABSENT; d.time_offset_bytes = PCM_LOAM_FIELD_ABSENT;
    d.intensity_kind = record_kind_ == PCM_LOAM_CLOUD_MAPPING ? PCM_LOAM_INTENSITY_UINT8 : PCM_LOAM_INTENSITY_FLOAT;
    d.ring_kind = PCM_LOAM_RING_UINT16;
    d.time_kind = record_kind_ == PCM_LOAM_CLOUD_MAPPING ? PCM_LOAM_TIME_DOUBLE : PCM_LOAM_TIME_FLOAT;
    bool have_x = false, have_i = false;
    for (const auto& f : msg.fields) {
      if (f.name == "x") { d.xyz_offset_bytes = f.offset; have_x = true; }
      else if (f.name == "intensity") { d.intensity_offset_bytes = f.offset; d.intensity_kind = f.datatype == 7 ? PCM_LOAM_INTENSITY_FLOAT : f.datatype == 2 ? PCM_LOAM_INTENSITY_UINT8 : -1; have_i = true; }
      else if (f.name == "ring") { d.ring_offset_bytes = f.offset; d.ring_kind = f.datatype == 4 ? PCM_LOAM_RING_UINT16 : -1; }
      else if (f.name == time_field_) { d.time_offset_bytes = f.offset; d.time_kind = f.datatype == 8 ? PCM_LOAM_TIME_DOUBLE : f.datatype == 7 ? PCM_LOAM_TIME_FLOAT : -1; }
    }
    if (!have_x || !have_i) throw std::runtime_error("cachePointCloud: the message has no x or no intensity field");
    d.is_dense = msg.is_dense ? 1 : 0;
    d.lidar_type = lidar_type_; d.record_kind = record_kind_;
    const bool has_ring = d.ring_offset_bytes != PCM_LOAM_FIELD_ABSENT, has_time = d.time_offset_bytes != PCM_LOAM_FIELD_ABSENT;
    if (lidar_type_ == PCM_LOAM_LIDAR_RSLIDAR_16 || lidar_type_ == PCM_LOAM_LIDAR_RSLIDAR_RUBY) d.synth_ring = 1;
    if (lidar_type_ == PCM_LOAM_LIDAR_RSLIDAR_32) d.synth_ring = (record_kind_ == PCM_LOAM_CLOUD_LOCALIZATION || !has_ring || !has_time) ? 1 : 0;
    if (lidar_type_ != PCM_LOAM_LIDAR_VELODYNE) d.synth_time = has_time ? 0 : 1;
    return d;
  }
  // laserCloudIn of the message, prepared in this object's context (pcm_loam_cloud_cached).  Throws where the node shuts down
  // (Velodyne: not dense, no ring field) and for a field type that is not the record's.
  template <typename Msg>
  const pcm_loam_cloud_result& cachePointCloud(const Msg& msg) {
    const pcm_loam_cloud_desc d = cloudDesc(msg);
    const int rc = pcm_loam_cloud_prepare(ctx_, msg.data.data(), &d, PCM_MEM_HOST, nullptr, 0, PCM_MEM_DEVICE, &cloud_);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_loam_cloud_prepare: ") + pcm_last_error(ctx_));
    return cloud_;
  }
  // cachePointCloud + projectPointCloud ... downsampleCurrentScan of the message: the features become this context's LOAM source
  // (pcm_loam_frame_begin_cloud); the tables of setDeskew apply when the cloud has a time.  result() / cloudResult() hold the counts.
  template <typename Msg>
  const pcm_loam_features_result& frameBegin(const Msg& msg) {
    const pcm_loam_cloud_desc d = cloudDesc(msg);
    const int rc = pcm_loam_frame_begin_cloud(ctx_, msg.data.data(), &d, PCM_MEM_HOST, &params_, &last_, have_deskew_ ? &deskew_.desc : nullptr, &cloud_);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_loam_frame_begin_cloud: ") + pcm_last_error(ctx_));
    return last_;
  }
  const pcm_loam_cloud_result& cloudResult() const { return cloud_; }
  pcm_ctx* context() const { return ctx_; }

  // laserCloudCornerLastDS / laserCloudSurfLastDS of one scan (pcm_loam_extract_features[_deskew])
  void extract(const std::shared_ptr<const CloudIn>& scan, CloudOut& cornerOut, CloudOut& surfOut) {
    const PointIn probe{};
    const char* base = reinterpret_cast<const char*>(&probe);
    const size_t ioff = (size_t)(reinterpret_cast<const char*>(&probe.intensity) - base), roff = (size_t)(reinterpret_cast<const char*>(&probe.ring) - base);
    const size_t cap = scan->size() ? scan->size() : 1;   // both outputs hold at most one feature per input point
    corner_.resize(4 * cap);
    surf_.resize(4 * cap);
    const int rc = pcm_loam_extract_features_deskew(ctx_, scan->points.data(), scan->size(), sizeof(PointIn), ioff, roff, PCM_MEM_HOST, &params_,
                                                    corner_.data(), cap, surf_.data(), cap, &last_, have_deskew_ ? &deskew_.desc : nullptr);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_loam_extract_features: ") + pcm_last_error(ctx_));
    fill(corner_, (size_t)last_.num_corner, cornerOut);
    fill(surf_, (size_t)last_.num_surf, surfOut);
  }

private:
  static void fill(const std::vector<float>& v, size_t n, CloudOut& out) {
    out.points.resize(n);
    for (size_t i = 0; i < n; i++) {
      PointOut& q = out.points[i];
      q.x = v[4 * i]; q.y = v[4 * i + 1]; q.z = v[4 * i + 2]; q.intensity = v[4 * i + 3];
    }
  }
  pcm_ctx* ctx_ = nullptr;
  pcm_loam_feature_params params_;
  pcm_loam_features_result last_{};
  std::vector<float> corner_, surf_;
  LoamDeskewTables deskew_;
  bool have_deskew_ = false;
  int lidar_type_ = PCM_LOAM_LIDAR_RSLIDAR_RUBY, record_kind_ = PCM_LOAM_CLOUD_MAPPING;
  std::string time_field_ = "time";
  pcm_loam_cloud_result cloud_{};
};

// jueying_slam's fusion_lidar_camera node (src/tool/integrate_points/src/fusion_lidar_camera.cpp) on the device: the node's
// parameters (camera_T, depth_filter) and its own ring tables in, its callback's clouds in, the fused VelodynePointXYZIRT scan
// born in device memory and handed to the front end of a LoamScanToMap without a host copy.  Message
// synchronisation and fromROSMsg stay with the caller.  Over a LoamScanToMap it shares that context; alone it owns one.
//     pcm_amd::ScanFusion<PointType> fusion(loam);
//     fusion.setCameraT(camera_T); fusion.setDepthFilter(depth_filter); fusion.setPitchRingTable(RING_MAP_16, 52);
//     // callback(lidar_msg, depth_0_msg, ...):
//     fusion.begin();
//     fusion.addLidar(*pc_lidar);                                   // RsPointXYZIRT: members intensity, ring, timestamp
//     fusion.addDepth(*pc_depth_0, camera_fusion_index[0], time_0_sec, time_0_nsec);
//     fusion.fuseToFrontEnd(&feature_params);                       // replaces publish + imageProjection + featureExtraction
template <typename PointT>
class ScanFusion {
public:
  explicit ScanFusion(int device = 0) : ctx_(pcm_create(device, nullptr)), own_(true) {
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    pcm_scan_default_fuse_params(&params_);
  }
  explicit ScanFusion(LoamScanToMap<PointT>& loam) : ctx_(loam.context()), loam_(&loam), own_(false) { pcm_scan_default_fuse_params(&params_); }
  ~ScanFusion() { if (own_ && ctx_) pcm_destroy(ctx_); }
  ScanFusion(const ScanFusion&) = delete;
  ScanFusion& operator=(const ScanFusion&) = delete;

  pcm_scan_fuse_params& params() { return params_; }
  void setCameraT(const std::vector<std::vector<double>>& camera_T) { camera_T_ = camera_T; }          // camera_T0 .. camera_T2
  void setDepthFilter(double v) { params_.depth_filter = v; }                                           // depth_filter
  // the node's own arrays (they must outlive this object's calls)
  void setPitchRingTable(const int* table, int n) { params_.pitch_ring_table = table; params_.pitch_ring_table_len = n; }   // RING_MAP_16
  void setOutputType(int output_type) { params_.output_layout = output_type; }                          // the converters' output_type

  void begin() { n_segs_ = 0; }
  // handle_pc_msg: a vendor XYZIRT cloud (members intensity -- float or uint8_t --, ring, timestamp)
  template <typename PointIn>
  void addLidar(const pcl::PointCloud<PointIn>& cloud) {
    pcm_scan_segment& g = next(PCM_SCAN_LIDAR_XYZIRT, cloud.points.data(), cloud.points.size(), sizeof(PointIn));
    const PointIn probe{};
    const char* base = reinterpret_cast<const char*>(&probe);
    g.intensity_offset_bytes = (size_t)(reinterpret_cast<const char*>(&probe.intensity) - base);
    g.ring_offset_bytes = (size_t)(reinterpret_cast<const char*>(&probe.ring) - base);
    g.timestamp_offset_bytes = (size_t)(reinterpret_cast<const char*>(&probe.timestamp) - base);
    g.intensity_type = sizeof(probe.intensity) == 1 ? PCM_SCAN_INTENSITY_UINT8 : PCM_SCAN_INTENSITY_FLOAT;
  }
  // the XYZI branch: an organised cloud and the node's row -> ring table for its height (RING_MAP_16 / RING_ID_MAP_RUBY)
  template <typename PointIn>
  void addLidarOrganised(const pcl::PointCloud<PointIn>& cloud, int width, int height, const int* ring_table, int ring_table_len) {
    pcm_scan_segment& g = next(PCM_SCAN_LIDAR_XYZI, cloud.points.data(), cloud.points.size(), sizeof(PointIn));
    const PointIn probe{};
    g.intensity_offset_bytes = (size_t)(reinterpret_cast<const char*>(&probe.intensity) - reinterpret_cast<const char*>(&probe));
    g.intensity_type = PCM_SCAN_INTENSITY_FLOAT;
    g.ring_rule = PCM_SCAN_RING_BY_HEIGHT;
    g.width = width; g.height = height; g.ring_table = ring_table; g.ring_table_len = ring_table_len;
  }
  // convert_depth(pc_depth, ..., camera, time_depth_sec, time_depth_nsec)
  template <typename PointIn>
  void addDepth(const pcl::PointCloud<PointIn>& cloud, int camera, int time_depth_sec, int time_depth_nsec) {
    if (camera < 0 || (size_t)camera >= camera_T_.size() || camera_T_[(size_t)camera].size() < 16) throw std::runtime_error("ScanFusion: no camera_T for this camera");
    pcm_scan_segment& g = next(PCM_SCAN_DEPTH, cloud.points.data(), cloud.points.size(), sizeof(PointIn));
    for (int k = 0; k < 16; k++) g.T[k] = camera_T_[(size_t)camera][(size_t)k];
    g.dt_sec = time_depth_sec; g.dt_nsec = time_depth_nsec;
  }
  // the fused scan stays on the device (pcm_scan_fused)
  const pcm_scan_fuse_result& fuse() {
    check(pcm_scan_fuse(ctx_, segs_, n_segs_, &params_, nullptr, 0, PCM_MEM_DEVICE, &last_), "pcm_scan_fuse");
    return last_;
  }
  // ... and becomes the LOAM source of the LoamScanToMap this object was made over
  const pcm_scan_fuse_result& fuseToFrontEnd(const pcm_loam_feature_params* fp = nullptr) {
    if (!loam_) throw std::runtime_error("ScanFusion: not constructed over a LoamScanToMap");
    fuse();
    const void* d = nullptr;
    size_t n = 0;
    check(pcm_scan_fused(ctx_, &d, &n), "pcm_scan_fused");
    loam_->setInputScanDevice(d, n, 32, 16, 20, fp);
    return last_;
  }
  // the published cloud on the host, for a node that still publishes it: 32-byte VelodynePointXYZIRT records
  const pcm_scan_fuse_result& fuseToHost(std::vector<unsigned char>* records) {
    size_t total = 0;
    for (int s = 0; s < n_segs_; s++) total += segs_[s].n;
    records->resize(32 * (total ? total : 1));
    check(pcm_scan_fuse(ctx_, segs_, n_segs_, &params_, records->data(), total ? total : 1, PCM_MEM_HOST, &last_), "pcm_scan_fuse");
    records->resize(32 * (size_t)last_.n_out);
    return last_;
  }

private:
  pcm_scan_segment& next(int kind, const void* points, size_t n, size_t stride) {
    if (n_segs_ >= PCM_SCAN_MAX_SEGMENTS) throw std::runtime_error("ScanFusion: too many clouds");
    pcm_scan_segment& g = segs_[n_segs_++];
    g = pcm_scan_segment{};
    g.kind = kind; g.memory = PCM_MEM_HOST; g.points = points; g.n = n; g.stride_bytes = stride;
    return g;
  }
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  LoamScanToMap<PointT>* loam_ = nullptr;
  bool own_ = false;
  pcm_scan_fuse_params params_;
  pcm_scan_fuse_result last_{};
  pcm_scan_segment segs_[PCM_SCAN_MAX_SEGMENTS];
  int n_segs_ = 0;
  std::vector<std::vector<double>> camera_T_;
};

// jueying_lio's PointCloudPreprocess for sensor_msgs::PointCloud2 clouds (pointcloud_preprocess.cc: Velodyne, RoboSense, Ouster and
// Livox-PointCloud2 handlers) on the device.  No ROS type enters: the callback hands msg->data.data(), the point count and, when the
// driver's fields are not the reference's PCL struct, their offsets.
//     pcm_amd::LidarPreprocess pre(PCM_LIDAR_RSLIDAR);              // lidar_type of the config; layout and config defaults
//     pre.Blind() = blind; pre.NumScans() = scan_line; pre.PointFilterNum() = point_filter_num; pre.TimeScale() = time_scale;
//     pre.Process(msg->data.data(), msg->width * msg->height, &cloud_out);   // 12 floats per kept point (pcl::PointXYZINormal)
// or, over the pcm_ctx that registers the scan, the whole front end of a frame (pcm_lio_frame_begin_cloud):
//     pcm_amd::LidarPreprocess pre(PCM_LIDAR_RSLIDAR, ctx);
//     pre.FrameBegin(msg->data.data(), n, filter_size_surf, IMUpose.data(), IMUpose.size(), &end_state);
class LidarPreprocess {
public:
  explicit LidarPreprocess(int lidar_type, int device = 0) : ctx_(pcm_create(device, nullptr)), own_(true) {
    if (!ctx_) throw std::runtime_error("pcm_create failed");
    init(lidar_type);
  }
  LidarPreprocess(int lidar_type, pcm_ctx* ctx) : ctx_(ctx), own_(false) { init(lidar_type); }
  ~LidarPreprocess() { if (own_ && ctx_) pcm_destroy(ctx_); }
  LidarPreprocess(const LidarPreprocess&) = delete;
  LidarPreprocess& operator=(const LidarPreprocess&) = delete;

  // PointCloudPreprocess's accessors (pointcloud_preprocess.h)
  double& Blind() { return desc_.blind; }
  int32_t& NumScans() { return desc_.num_scans; }
  int32_t& PointFilterNum() { return desc_.point_filter_num; }
  float& TimeScale() { return desc_.time_scale; }
  pcm_lidar_desc& desc() { return desc_; }   // stride, offsets and kinds of a driver whose fields differ from the reference's struct
  bool GivenOffsetTime() const { return given_ != 0; }

  // the handler: `records` in host memory -> the kept points, 12 floats each, in input order; returns their number
  size_t Process(const void* records, size_t n, std::vector<float>* cloud_out) {
    cloud_out->resize(12 * (n ? n : 1));
    size_t m = 0;
    check(pcm_lidar_filter(ctx_, records, n, PCM_MEM_HOST, &desc_, cloud_out->data(), n ? n : 1, PCM_MEM_HOST, &m, &given_), "pcm_lidar_filter");
    cloud_out->resize(12 * m);
    return m;
  }
  // handler -> time sort -> motion compensation -> voxel grid -> source of the context; returns the scan's size
  size_t FrameBegin(const void* records, size_t n, float leaf_size, const pcm_imu_pose* poses, int num_poses, const pcm_lio_state* end_state, int memory = PCM_MEM_HOST) {
    size_t m = 0;
    check(pcm_lio_frame_begin_cloud(ctx_, records, n, memory, &desc_, leaf_size, poses, num_poses, end_state, &m), "pcm_lio_frame_begin_cloud");
    return m;
  }

private:
  void init(int lidar_type) {
    if (pcm_lidar_default_desc(lidar_type, &desc_) != PCM_OK) throw std::runtime_error("LidarPreprocess: unknown lidar type");
  }
  void check(int rc, const char* what) const {
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
  }
  pcm_ctx* ctx_ = nullptr;
  bool own_ = false;
  pcm_lidar_desc desc_;
  int given_ = 1;
};

// jueying_lio's iterated Kalman update over the pcm_ctx that holds the frame's scan and the map (pcm_lio_update): the replacement of
// kf_.update_iterated_dyn_share_modified(options::LASER_POINT_COV, solve_H_time)  (laser_mapping.cc:347).
//     pcm_amd::LioFilter kf(ctx);                       // R 0.001, max_iter 4, limit 0.001 (options.h:12, laser_mapping.cc:19,89)
//     kf.ExtrinsicEstEn() = extrinsic_est_en_;
//     kf.Update(&x, P_row_major);                       // x: propagated -> updated state_ikfom, P: 23 x 23 row-major in / out
class LioFilter {
public:
  explicit LioFilter(pcm_ctx* ctx) : ctx_(ctx) { pcm_lio_default_update_params(&params_); }
  double& R() { return params_.R; }
  int32_t& MaxIter() { return params_.max_iter; }
  int32_t& ExtrinsicEstEn() { return params_.extrinsic_est_en; }
  double* Limit() { return params_.limit; }
  // update_iterated_dyn_share_modified: every ObsModel call and the filter algebra on the device, one synchronisation
  const pcm_lio_update_result& Update(pcm_lio_filter_state* x, double* P) {
    const int rc = pcm_lio_update(ctx_, &params_, x, P, &last_);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_lio_update: ") + pcm_last_error(ctx_));
    return last_;
  }
  const pcm_lio_update_result& last() const { return last_; }
  // matching ObsModel launches since the context was made (or pcm_reset_stats): served by the lists kernel / by the tile kernel
  // (pcm_lio_search_path; the lists serve a context that set PCM_FLAG_FOLLOWING_LISTS or PCM_FLAG_NEIGHBOUR_LISTS)
  std::pair<uint64_t, uint64_t> searchPath() const {
    uint64_t n[2] = {0, 0};
    if (pcm_lio_search_path(ctx_, n) != PCM_OK) throw std::runtime_error("pcm_lio_search_path: bad argument");
    return {n[0], n[1]};
  }
  // the state ObsModel call `call` of the last update was evaluated at, its converge flag and n_eff
  bool Trace(int call, pcm_lio_filter_state* x, int32_t* converge, int32_t* n_eff, double* dx23 = nullptr) const {
    return pcm_lio_update_trace(ctx_, call, x, converge, n_eff, nullptr, dx23) == PCM_OK;
  }

  // ---- p_imu_->Process(measures_, kf_, scan_undistort_) (laser_mapping.cc:307) and the frame around the update -----------------------
  // the members of ImuProcess (SetExtrinsic / SetGyrCov / SetAccCov / SetGyrBiasCov / SetAccBiasCov write into it)
  pcm_lio_imu_state& Imu() { return imu_; }
  // the init branch of Process: one frame of IMUInit; true once the IMU is initialised (imu_need_init_ == false)
  bool imuInit(const pcm_imu_sample* imu, int n, pcm_lio_filter_state* x, double* P) {
    if (pcm_lio_imu_init(&imu_, imu, n, x, P) != PCM_OK) throw std::runtime_error("pcm_lio_imu_init: bad argument");
    return imu_.need_init == 0;
  }
  // the forward loop of UndistortPcl + esekf::predict on the device; the IMUpose_ list is kept for the frame entry
  const std::vector<pcm_imu_pose>& propagate(const pcm_imu_sample* imu, int n, double pcl_beg_time, double pcl_end_time, pcm_lio_filter_state* x, double* P) {
    poses_.resize((size_t)(n > 0 ? n : 0) + 1);
    int k = 0;
    const int rc = pcm_lio_propagate(ctx_, &imu_, imu, n, pcl_beg_time, pcl_end_time, x, P, poses_.data(), (int)poses_.size(), &k);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_lio_propagate: ") + pcm_last_error(ctx_));
    poses_.resize((size_t)k);
    return poses_;
  }
  enum class Frame { NoImu, Init, NoPoints, FirstScan, TooFewPoints, Updated };
  // LaserMapping::Run (laser_mapping.cc:301-356) for one synchronised package: a livox_ros_driver::CustomMsg (msg->points.data(),
  // n_points records), its IMU samples, lidar_bag_time_ and lidar_end_time_.  x, P: the filter's state and covariance, in / out.
  Frame processFrame(const void* custom_points, size_t n_points, const pcm_imu_sample* imu, int n_imu, double pcl_beg_time, double pcl_end_time,
                     const pcm_lio_frame_params& frame, float filter_size_map, pcm_lio_filter_state* x, double* P) {
    if (n_imu <= 0) return Frame::NoImu;
    if (imu_.need_init) { imuInit(imu, n_imu, x, P); return Frame::Init; }
    propagate(imu, n_imu, pcl_beg_time, pcl_end_time, x, P);
    pcm_lio_state st = poseOf(*x);
    pcm_lio_frame_params fp = frame;
    if (first_scan_) fp.leaf_size = 0.f;
    size_t n_scan = 0;
    int rc = pcm_lio_frame_begin(ctx_, custom_points, n_points, PCM_MEM_HOST, &fp, poses_.data(), (int)poses_.size(), &st, &n_scan);
    if (rc == PCM_ERR_NO_INPUT) return Frame::NoPoints;                       // "No point, skip this scan!"
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_lio_frame_begin: ") + pcm_last_error(ctx_));
    if (first_scan_) {                                                        // ivox_->AddPoints(scan_undistort_->points)
      std::vector<float> xyz(3 * n_scan);
      if (pcm_get_source(ctx_, xyz.data(), n_scan, &n_scan) != PCM_OK || pcm_target_insert(ctx_, xyz.data(), n_scan, 12, PCM_MEM_HOST) != PCM_OK)
        throw std::runtime_error(std::string("first scan: ") + pcm_last_error(ctx_));
      first_lidar_time_ = pcl_beg_time;
      first_scan_ = false;
      return Frame::FirstScan;
    }
    ekf_inited_ = (pcl_beg_time - first_lidar_time_) >= 0.1;                  // options::INIT_TIME
    if (n_scan < 5) return Frame::TooFewPoints;
    Update(x, P);
    st = poseOf(*x);
    size_t added = 0;
    rc = pcm_lio_frame_end(ctx_, &st, filter_size_map, ekf_inited_ ? 1 : 0, &added);
    if (rc != PCM_OK) throw std::runtime_error(std::string("pcm_lio_frame_end: ") + pcm_last_error(ctx_));
    return Frame::Updated;
  }
  bool EkfInited() const { return ekf_inited_; }

  // ---- the last block of Run (laser_mapping.cc:361-385) and Finish (:887-900) ----------------------------------------------------------
  // PointT: pcl::PointXYZINormal (PointType of jueying_lio).  The other fields are what the reference leaves in a fresh cloud:
  // data[3] = 1, normals and curvature 0.  x: the state the reference publishes with (state_point_ = kf_.get_x()).
  // PublishFrameWorld (:747-792): the cloud (dense_pub_en: scan_undistort_, else scan_down_world_); with pcd_save_en it is also appended
  // to the saved map on the device.  Returns true when the reference would write jueying_<*pcd_index>.pcd now: fetch the map with
  // finish(), write it, then clearSavedMap().
  template <typename PointT>
  bool publishFrameWorld(const pcm_lio_filter_state& x, bool dense_pub_en, pcl::PointCloud<PointT>* cloud, bool pcd_save_en = false, int pcd_save_interval = -1,
                         int* pcd_index = nullptr) {
    const pcm_lio_state st = poseOf(x);
    if (cloud) fetch(cloud, [&](void* out, size_t cap, size_t* n) { return pcm_lio_frame_world(ctx_, &st, dense_pub_en ? 1 : 0, out, cap, PCM_MEM_HOST, n); }, "pcm_lio_frame_world");
    if (!pcd_save_en) return false;
    pcm_lio_map_info info{};
    if (pcm_lio_map_append(ctx_, &st, dense_pub_en ? 1 : 0, pcd_save_interval, &info) != PCM_OK) throw std::runtime_error(std::string("pcm_lio_map_append: ") + pcm_last_error(ctx_));
    if (pcd_index) *pcd_index = info.pcd_index;
    return info.chunk_ready != 0;
  }
  // PublishFrameBody (:794-808)
  template <typename PointT>
  void publishFrameBody(const pcm_lio_filter_state& x, pcl::PointCloud<PointT>* cloud) {
    const pcm_lio_state st = poseOf(x);
    fetch(cloud, [&](void* out, size_t cap, size_t* n) { return pcm_lio_frame_body(ctx_, &st, out, cap, PCM_MEM_HOST, n); }, "pcm_lio_frame_body");
  }
  // PublishFrameEffectWorld (:810-823): the points of the last ObsModel call's rows, intensity = |z|
  template <typename PointT>
  void publishFrameEffectWorld(const pcm_lio_filter_state& x, pcl::PointCloud<PointT>* cloud) {
    const pcm_lio_state st = poseOf(x);
    fetch(cloud, [&](void* out, size_t cap, size_t* n) { return pcm_lio_frame_effect(ctx_, &st, out, cap, PCM_MEM_HOST, n); }, "pcm_lio_frame_effect");
  }
  // Finish: the cloud of jueying.pcd (false: the saved map is empty, the reference writes no file).  leaf_size > 0 and
  // z_min <= z_max add the filters of src/tool/pcd2map (VoxelGrid, then PassThrough on z).
  template <typename PointT>
  bool finish(pcl::PointCloud<PointT>* cloud, float leaf_size = 0.f, double z_min = 1.0, double z_max = 0.0) {
    fetch(cloud, [&](void* out, size_t cap, size_t* n) { return pcm_lio_map_export(ctx_, leaf_size, z_min, z_max, out, cap, PCM_MEM_HOST, n); }, "pcm_lio_map_export");
    pcm_lio_map_info info{};
    return pcm_lio_map_info_get(ctx_, &info) == PCM_OK && info.points > 0;
  }
  void clearSavedMap() { pcm_lio_map_clear(ctx_); }   // pcl_wait_save_->clear(); scan_wait_num = 0  (:788-789)

private:
  // count, then the (x, y, z, intensity) records into a cloud of PointT
  template <typename PointT, typename Call>
  void fetch(pcl::PointCloud<PointT>* cloud, Call call, const char* what) {
    size_t n = 0;
    int rc = call(nullptr, 0, &n);
    std::vector<float> rec(4 * n);
    if (rc == PCM_OK && n) rc = call(rec.data(), n, &n);
    if (rc != PCM_OK) throw std::runtime_error(std::string(what) + ": " + pcm_last_error(ctx_));
    cloud->points.resize(n);
    for (size_t i = 0; i < n; i++) {
      PointT p{};
      p.x = rec[4 * i]; p.y = rec[4 * i + 1]; p.z = rec[4 * i + 2]; p.data[3] = 1.f;
      p.intensity = rec[4 * i + 3];
      p.normal_x = p.normal_y = p.normal_z = 0.f; p.curvature = 0.f;
      cloud->points[i] = p;
    }
  }
  static pcm_lio_state poseOf(const pcm_lio_filter_state& x) {
    pcm_lio_state st{};
    for (int a = 0; a < 4; a++) { st.rot[a] = x.rot[a]; st.off_R[a] = x.off_R[a]; }
    for (int a = 0; a < 3; a++) { st.pos[a] = x.pos[a]; st.off_T[a] = x.off_T[a]; }
    return st;
  }
  pcm_ctx* ctx_ = nullptr;
  pcm_lio_update_params params_;
  pcm_lio_update_result last_{};
  pcm_lio_imu_state imu_ = [] { pcm_lio_imu_state s; pcm_lio_default_imu_state(&s); return s; }();
  std::vector<pcm_imu_pose> poses_;
  bool first_scan_ = true, ekf_inited_ = false;
  double first_lidar_time_ = 0.0;
};

}  // namespace pcm_amd

// The call sites spell the pclomp enumerators unqualified inside namespace pclomp (jueying_slam/src/localization.cpp:169-186:
// `ndt->setNeighborhoodSearchMethod(pclomp::DIRECT7)`).  Define PCM_AMD_PCLOMP_ALIASES before including this header, in a
// translation unit that no longer includes <pclomp/ndt_omp.h>, to keep those lines unchanged.
#ifdef PCM_AMD_PCLOMP_ALIASES
namespace pclomp {
using NeighborSearchMethod = pcm_amd::NeighborSearchMethodOmp;
using pcm_amd::KDTREE;
using pcm_amd::DIRECT26;
using pcm_amd::DIRECT7;
using pcm_amd::DIRECT1;
template <typename PointSource, typename PointTarget>
using NormalDistributionsTransform = pcm_amd::PclNdtRegistration<PointSource, PointTarget>;
}  // namespace pclomp
#endif

#endif  // __has_include(<pcl/registration/registration.h>)
