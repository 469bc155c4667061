"""pcm_amd::OccupancyMap2D (include/pcm_amd/registration.hpp) meets a compiler: written the way mapping_server.cc drives its
OccupancyMap2D, against the declaration-only PCL / Eigen stand-ins of tests/stubs (the adapter is free of Eigen), compiled and
linked against libpcm_amd.so (every pcm_occ_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
#include <memory>
using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
int main() {
  pcm_amd::OccupancyMap2D<PointType> online(0);
  online.params().max_radius = 15.0;
  online.initializeMap();
  Cloud initial_cloud;
  std::vector<double> robot_pose(6, 0.0);
  online.processCloud(initial_cloud, robot_pose);
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  pcm_amd::OccupancyMap2D<PointType> offline(loam);
  offline.initializeMap();
  offline.processKeyFrames(0, 0);
  std::vector<int8_t> data;
  std::vector<uint8_t> pgm;
  int width = 0, height = 0;
  double ox = 0, oy = 0, res = 0;
  offline.getGridMap(&data, &width, &height, &ox, &oy, &res);
  offline.getPgm(&pgm);
  return width + height + (int)data.size() + (int)pgm.size() + (int)ox + (int)oy + (int)res;
}
"""


def test_occ_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "occ_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "occ_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
