"""include/pcm_amd/registration.hpp -- the header-only pcl::Registration adapter a ROS / PCL workspace includes -- needs PCL and
Eigen, which the build container does not have.  This test lets it meet a compiler anyway: every adapter class is instantiated
and every member the reference's call sites use is called (jueying_slam/src/localization.cpp:162-189,317-340; fast_gicp/src/align.cpp:
51-104) against declaration-only stand-ins of the PCL / Eigen headers under tests/stubs/ (test infrastructure; nothing of the
reference is built with them), with g++ -fsyntax-only; then the translation unit is compiled and linked against libpcm_amd.so, which
checks every pcm_* call of the adapter against the exported symbols."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#define PCM_AMD_PCLOMP_ALIASES
#include <pcm_amd/registration.hpp>
#include <memory>
using P = pcl::PointXYZ;
using Cloud = pcl::PointCloud<P>;

template <typename Reg> static double common_surface(Reg& reg, const Cloud::ConstPtr& src, const Cloud::ConstPtr& tgt) {
  // the call order of localization.cpp:277,317-340 and align.cpp:61-99
  reg.setMaximumIterations(64);
  reg.setTransformationEpsilon(0.01);
  reg.setRotationEpsilon(2e-3);
  reg.setMaxCorrespondenceDistance(1.0);
  reg.setNumThreads(8);
  reg.setInputTarget(tgt);
  reg.setInputSource(src);
  Cloud aligned;
  reg.align(aligned, Eigen::Matrix4f::Identity());
  reg.swapSourceAndTarget();
  reg.clearSource();
  reg.clearTarget();
  Eigen::Matrix<double, 6, 6> H; Eigen::Matrix<double, 6, 1> b;
  double c = reg.evaluateCost(Eigen::Matrix4f::Identity(), &H, &b);
  return c + reg.getFitnessScore() + reg.getFitnessScore(1.0) + reg.getFinalHessian()(0, 0) + reg.getFinalTransformation()(0, 0) + (reg.hasConverged() ? 1 : 0) + reg.getFinalNumIteration();
}

int main() {
  auto src = std::make_shared<Cloud>(); auto tgt = std::make_shared<Cloud>();
  double s = 0;
  { pcm_amd::P2PlaneRegistration<P, P> r; r.setNumNeighborCells(27); r.setMaxRange(5.0); r.setOptimizer(pcm_amd::LSQ_OPTIMIZER_TYPE::GaussNewton); r.setInitialLambdaFactor(1e-9); r.setDebugPrint(false); s += common_surface(r, src, tgt); }
  { pcm_amd::GicpRegistration<P, P> r; r.setCorrespondenceRandomness(20); r.setRegularizationMethod(pcm_amd::RegularizationMethod::PLANE); s += common_surface(r, src, tgt); s += r.getSourceCovariances().size() + r.getTargetCovariances().size(); r.setSourceCovariances(r.getSourceCovariances()); r.setTargetCovariances(r.getTargetCovariances()); }
  { pcm_amd::VgicpRegistration<P, P> r; r.setResolution(1.0); r.setNeighborSearchMethod(pcm_amd::NeighborSearchMethod::DIRECT7); r.setVoxelAccumulationMode(pcm_amd::VoxelAccumulationMode::ADDITIVE); s += common_surface(r, src, tgt); }
  { pcm_amd::NdtRegistration<P, P> r; r.setDistanceMode(pcm_amd::NDTDistanceMode::D2D); r.setNeighborSearchMethod(pcm_amd::NeighborSearchMethod::DIRECT7, -1.0); s += common_surface(r, src, tgt); }
  { pcm_amd::VgicpCudaRegistration<P, P> r; r.setResolution(1.0); r.setCorrespondenceRandomness(20); r.setNeighborSearchMethod(pcm_amd::NeighborSearchMethod::DIRECT_RADIUS, 1.5); r.setNearestNeighborSearchMethod(pcm_amd::VgicpCudaRegistration<P, P>::NearestNeighborMethod::GPU_BRUTEFORCE); r.setKernelWidth(0.5, 3.0); s += common_surface(r, src, tgt); }
  { // jueying_slam/src/localization.cpp:162-189, through the pclomp spellings
    std::shared_ptr<pclomp::NormalDistributionsTransform<P, P>> ndt(new pclomp::NormalDistributionsTransform<P, P>());
    ndt->setTransformationEpsilon(0.01);
    ndt->setResolution(1.0);
    ndt->setNeighborhoodSearchMethod(pclomp::DIRECT7);
    ndt->setStepSize(0.1);
    ndt->setOutlierRatio(0.55); (void)ndt->getOutlierRatio(); (void)ndt->getStepSize(); (void)ndt->getResolution();
    s += common_surface(*ndt, src, tgt);
    s += ndt->getTransformationProbability() + ndt->getMaxEigen() + ndt->calculateScore();
  }
  return s > 0 ? 0 : 1;
}
'''


def test_adapter_header_compiles_against_stub_pcl_and_links_against_the_c_abi(tmp_path):
    inc = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-fsyntax-only", "-x", "c++", "-"] + inc, input=SRC.encode(), check=True)
    lib = os.path.join(ROOT, "pointcloud-slam_amd", "libpcm_amd.so")
    if os.path.exists(lib):   # every pcm_* symbol the adapter calls exists in the library (no GPU needed to link)
        subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-o", str(tmp_path / "pcm_adapter_link_check")] + inc +
                       ["-L", os.path.dirname(lib), "-lpcm_amd", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                       input=SRC.encode(), check=True)


def test_rccl_gather_example_compiles():
    """examples/gather_poses_rccl.cpp (the C++ caller's pcm_align_batch(device_out) -> ncclAllGather) against
    the image's RCCL and HIP headers."""
    import pytest
    if not os.path.exists("/opt/rocm/include/rccl/rccl.h"):
        pytest.skip("no RCCL headers")
    subprocess.run(["g++", "-std=c++17", "-Wall", "-fsyntax-only", "-D__HIP_PLATFORM_AMD__", "-I", os.path.join(ROOT, "include"), "-I", "/opt/rocm/include",
                    os.path.join(ROOT, "examples", "gather_poses_rccl.cpp")], check=True)
