"""pcm_amd::LoamScanContext (include/pcm_amd/registration.hpp) meets a compiler: written the way mapOptmization.cpp calls
scManager against the declaration-only PCL / Eigen stand-ins of tests/stubs (the adapter is free of Eigen), compiled and linked
against libpcm_amd.so (every pcm_loam_sc_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
#include <memory>
using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
int main() {
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  pcm_amd::LoamScanContext<PointType> scManager(loam);
  scManager.params().num_candidates = 10;
  Cloud thisRawCloudKeyFrame;
  scManager.makeAndSaveScancontextAndKeys(thisRawCloudKeyFrame);
  scManager.makeAndSaveScancontextAndKeysOfKeyFrame(0);
  const std::vector<double>& curr_scd = scManager.getConstRefRecentSCD();
  scManager.putScancontext(curr_scd);
  std::pair<int, float> detectResult = scManager.detectLoopClosureID();
  int loopKeyCur = -1, loopKeyPre = -1;
  const bool found = scManager.detectLoopClosureDistance(&loopKeyCur, &loopKeyPre, 1.0);
  std::pair<double, int> d = scManager.distanceBtnScanContext(0, 1);
  scManager.clear();
  return scManager.size() + detectResult.first + (int)detectResult.second + (found ? 1 : 0) + d.second + scManager.result().tree_size + (int)curr_scd.size();
}
"""


def test_loam_sc_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_sc_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_sc_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
