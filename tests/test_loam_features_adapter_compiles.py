"""pcm_amd::LoamFeatureExtraction and LoamScanToMap::setInputScan (include/pcm_amd/registration.hpp) meet a compiler: instantiated
with a PointXYZIRT-shaped point against the declaration-only PCL / Eigen stand-ins of tests/stubs, compiled and linked against
libpcm_amd.so (every pcm_loam_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <cstdint>
#include <memory>
struct RingPoint { float x, y, z, pad; std::uint8_t intensity; double timestamp; std::uint16_t ring; };
using In = pcl::PointCloud<RingPoint>;
using Out = pcl::PointCloud<pcl::PointXYZI>;
int main() {
  auto scan = std::make_shared<In>();
  std::shared_ptr<const In> cscan = scan;
  pcm_amd::LoamFeatureExtraction<RingPoint> fe(0);
  fe.setNScan(16); fe.setHorizonScan(1800); fe.setDownsampleRate(1); fe.setAreaNum(6);
  fe.setMinRange(1.0f); fe.setMaxRange(150.0f); fe.setEdgeThreshold(1.0f); fe.setSurfThreshold(0.1f);
  fe.setOdometrySurfLeafSize(0.2f); fe.setMappingCornerLeafSize(0.2f); fe.setMappingSurfLeafSize(0.3f);
  Out corner, surf;
  fe.extract(cscan, corner, surf);
  pcm_amd::LoamScanToMap<pcl::PointXYZ> loam(0);
  loam.setInputScan(cscan, &fe.params());
  float x[6] = {0, 0, 0, 0, 0, 0};
  const bool ran = loam.scan2MapOptimization(x);
  return (int)corner.size() + (int)surf.size() + fe.result().num_corner + loam.featuresResult().num_surf + (ran ? 1 : 0);
}
'''


def test_loam_features_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_features_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_features_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
