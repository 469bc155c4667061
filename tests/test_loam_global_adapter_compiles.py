"""pcm_amd::LoamKeyFrameMap's publishGlobalMap / exportMap (include/pcm_amd/registration.hpp) meet a compiler: written the way
mapOptmization.cpp's visualizeGlobalMapThread calls them against the declaration-only PCL / Eigen stand-ins of tests/stubs, compiled
and linked against libpcm_amd.so (every pcm_loam_global_* / pcm_loam_map_export call of the adapter resolves to an exported
symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
int main() {
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  keyframes.setGlobalMapVisualizationSearchRadius(1000.0f); keyframes.setGlobalMapVisualizationPoseDensity(10.0f);
  keyframes.setGlobalMapVisualizationLeafSize(1.0f);
  Cloud globalMapKeyFramesDS, globalCornerCloud, globalSurfCloud, globalMapCloud;
  keyframes.publishGlobalMap(globalMapKeyFramesDS);
  const size_t on_device = keyframes.publishGlobalMap(static_cast<void*>(nullptr), 0);
  keyframes.exportMap(globalCornerCloud, 0);
  keyframes.exportMap(globalSurfCloud, 1);
  keyframes.exportMap(globalMapCloud);
  const size_t chunk = keyframes.exportMap(static_cast<void*>(nullptr), 0, 0, 0, 1);
  return (int)(globalMapKeyFramesDS.size() + globalCornerCloud.size() + globalSurfCloud.size() + globalMapCloud.size() + on_device + chunk) +
         keyframes.globalResult().num_used + (int)keyframes.globalParams().leaf;
}
"""


def test_loam_global_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_global_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_global_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
