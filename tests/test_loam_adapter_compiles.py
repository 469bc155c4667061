"""pcm_amd::LoamScanToMap (include/pcm_amd/registration.hpp) meets a compiler: instantiated with the call shape of
jueying_slam/src/mapOptmization.cpp:1560-1586 against the declaration-only PCL / Eigen stand-ins of tests/stubs, compiled and
linked against libpcm_amd.so (every pcm_loam_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <memory>
using P = pcl::PointXYZ;
using Cloud = pcl::PointCloud<P>;
int main() {
  auto corner = std::make_shared<Cloud>(); auto surf = std::make_shared<Cloud>();
  pcm_amd::LoamScanToMap<P> loam(0);
  loam.setIterNum(30);
  loam.setFeatureMinValidNum(10, 100);
  loam.setLocalizationThresholds();
  loam.setInputMaps(corner, surf, 1);
  loam.setInputFeatures(corner, surf);
  float transformTobeMapped[6] = {0, 0, 0, 0, 0, 0};
  const bool ran = loam.scan2MapOptimization(transformTobeMapped);
  return (ran ? 1 : 0) + (loam.isDegenerate() ? 1 : 0) + (int)loam.cornerFitnessScore() + (int)loam.surfFitnessScore() + loam.iterations()
         + loam.result().status + loam.params().iter_num;
}
'''


def test_loam_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
