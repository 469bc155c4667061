"""pcm_amd::LoamDynamicMap (include/pcm_amd/registration.hpp) meets a compiler: written the way localization.cpp calls it against the
declaration-only PCL / Eigen stand-ins of tests/stubs, compiled and linked against libpcm_amd.so (every pcm_loam_tile_* /
pcm_loam_dynmap_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
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
  loam.setLocalizationThresholds();
  pcm_amd::LoamDynamicMap<PointType> dynmap(loam);
  dynmap.setMaxRange(150.0f); dynmap.setMargin(100); dynmap.setAreaSize(50); dynmap.setCropX(false);
  Cloud tile;
  const double box[6] = {0, 0, 0, 100, 100, 10};
  const int ci = dynmap.addCornerArea(box, tile), si = dynmap.addSurfArea(box, tile);
  float transformTobeMapped[6] = {0, 0, 0, 0, 0, 0};
  bool changed = false;
  if (dynmap.needLoad(transformTobeMapped)) changed = dynmap.load(transformTobeMapped);
  const bool rebuilt = dynmap.dynamic_load_map(transformTobeMapped);
  auto corner = std::make_shared<Cloud>(), surf = std::make_shared<Cloud>();
  std::shared_ptr<const Cloud> cc = corner, cs = surf;
  loam.setInputFeatures(cc, cs);
  const bool ran = loam.scan2MapOptimization(transformTobeMapped);
  Cloud globalMap;
  dynmap.globalMap(globalMap);
  const size_t n_dev = dynmap.globalMap(nullptr, 0);
  dynmap.clear();
  return ci + si + dynmap.cornerAreas() + dynmap.surfAreas() + (int)globalMap.size() + (int)n_dev + dynmap.laserCloudCornerFromMapDSNum() +
         dynmap.laserCloudSurfFromMapDSNum() + dynmap.result().num_nonfinite + dynmap.loadResult().num_corner_selected + (changed ? 1 : 0) +
         (rebuilt ? 1 : 0) + (ran ? 1 : 0) + (loam.cornerFitnessScore() > 0.3 ? 1 : 0);
}
'''


def test_loam_dynmap_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_dynmap_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_dynmap_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
