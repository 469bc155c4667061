"""pcm_amd::LoamKeyFrameMap (include/pcm_amd/registration.hpp) meets a compiler: written the way mapOptmization.cpp calls it against
the declaration-only PCL / Eigen stand-ins of tests/stubs, compiled and linked against libpcm_amd.so (every pcm_loam_keyframe_* /
pcm_loam_submap_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <memory>
using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
int main() {
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  keyframes.setSurroundingKeyframeSearchRadius(50.0f); keyframes.setSurroundingKeyframeDensity(1.0f);
  keyframes.setMappingCornerLeafSize(0.2f); keyframes.setMappingSurfLeafSize(0.2f); keyframes.setLoopLeafSize(0.2f);
  auto corner = std::make_shared<Cloud>(), surf = std::make_shared<Cloud>();
  std::shared_ptr<const Cloud> cc = corner, cs = surf;
  float transformTobeMapped[6] = {0, 0, 0, 0, 0, 0};
  double timeLaserInfoCur = 1.0;
  const bool rebuilt = keyframes.extractSurroundingKeyFrames(timeLaserInfoCur);
  loam.setInputFeatures(cc, cs);
  const bool ran = loam.scan2MapOptimization(transformTobeMapped);
  keyframes.saveKeyFrame(transformTobeMapped, timeLaserInfoCur);
  keyframes.saveKeyFrame(transformTobeMapped, timeLaserInfoCur, cc, cs);
  keyframes.correctPoses(transformTobeMapped, 1);
  Cloud cure, prev;
  keyframes.loopFindNearKeyframes(cure, 0, 0);
  keyframes.loopFindNearKeyframesWithRespectTo(prev, 0, 25, 0);
  keyframes.clear();
  return keyframes.size() + (int)cure.size() + (int)prev.size() + keyframes.laserCloudCornerFromMapDSNum() + keyframes.laserCloudSurfFromMapDSNum() +
         keyframes.result().num_selected + (rebuilt ? 1 : 0) + (ran ? 1 : 0);
}
'''


def test_loam_submap_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_submap_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_submap_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
