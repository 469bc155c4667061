"""The two adapter additions of include/pcm_amd/registration.hpp -- pcm_amd::IterativeClosestPoint and
LoamKeyFrameMap::performSCLoopClosure -- against a compiler and the built library, over the stand-in PCL / Eigen headers of
tests/stubs.  No GPU: the program is linked, not run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ADAPTER_SRC = r'''
#include <pcm_amd/registration.hpp>
#include <memory>
using PointType = pcl::PointXYZI;
int main() {
  // mapOptmization.cpp:768-783 with the class swapped
  pcm_amd::IterativeClosestPoint<PointType, PointType> icp;
  icp.setMaxCorrespondenceDistance(150);
  icp.setMaximumIterations(100);
  icp.setTransformationEpsilon(1e-6);
  icp.setEuclideanFitnessEpsilon(1e-6);
  icp.setTransformationRotationEpsilon(0.999);
  icp.setRANSACIterations(0);
  icp.setResolution(1.0);
  pcl::PointCloud<PointType>::Ptr cure(new pcl::PointCloud<PointType>()), prev(new pcl::PointCloud<PointType>());
  icp.setInputSource(cure);
  icp.setInputTarget(prev);
  pcl::PointCloud<PointType> unused;
  icp.align(unused);
  int n = 0;
  if (icp.hasConverged() == false || icp.getFitnessScore() > 0.3) n++;
  Eigen::Matrix4f correction = icp.getFinalTransformation();
  n += icp.lastInfo().stop_reason == PCM_ICP_STOP_NO_CORRESPONDENCES;
  // performSCLoopClosure on the key-frame map
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  keyframes.setLoopLeafSize(0.2f); keyframes.setHistoryKeyframeSearchNum(25); keyframes.setHistoryKeyframeFitnessScore(0.3f);
  keyframes.scLoopParams().min_cur_points = 300;
  pcm_amd::LoamKeyFrameMap<PointType>::LoopFactor factor;
  if (keyframes.performSCLoopClosure(&factor)) n++;          // detectLoopClosureID + verification
  if (keyframes.performSCLoopClosure(12, 3, &factor)) n++;   // a pair the caller detected
  const float robustNoiseScore = factor.noise;
  return n + factor.index.first + (int)factor.between[15] + (int)robustNoiseScore + keyframes.scLoopResult().icp_iterations + (int)keyframes.scLoopResult().cauchy_k +
         (int)correction(0, 0);
}
'''


def test_icp_and_sc_loop_adapters_compile_and_link(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "icp_adapter.cpp"
    src.write_text(ADAPTER_SRC)
    exe = tmp_path / "icp_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
