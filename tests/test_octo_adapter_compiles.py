"""pcm_amd::OccupancyMap3D of include/pcm_amd/registration.hpp against a compiler and the built library, over the stand-in PCL /
Eigen headers of tests/stubs.  No GPU: the program is linked, not run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ADAPTER_SRC = r'''
#include <pcm_amd/registration.hpp>
using PointType = pcl::PointXYZI;
int main() {
  // pcd2map/launch/octomap_server.launch and OctomapServer's constructor, with the node's parameter names
  pcm_amd::OccupancyMap3D<PointType> server(0);
  server.setResolution(0.1);
  server.setSensorModel(0.7, 0.4, 0.12, 0.97);
  server.setMaxRange(1000.0);
  server.setMinRange(-1.0);
  server.setPointcloudZ(-1.0, 3.0);
  server.setOccupancyZ(0.1, 2.0);
  server.setFilterSpeckles(true);
  server.setMinSize(0.0, 0.0);
  server.params().max_cells = 1u << 24;
  server.reset();
  pcl::PointCloud<PointType> cloud, ground, centers;
  Eigen::Matrix4f sensorToWorld = Eigen::Matrix4f::Identity();
  pcm_octo_insert_result r = server.insertCloud(cloud, sensorToWorld);
  r = server.insertCloud(ground, cloud, sensorToWorld);
  pcm_amd::OccupancyMap3D<PointType>::ProjectedMap map = server.projectedMap();
  server.occupiedCenters(&centers);
  int n = server.saveMap("/tmp/map") ? 1 : 0;
  // over a LOAM context: the key frames in place
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::OccupancyMap3D<PointType> fromKeyFrames(loam);
  fromKeyFrames.insertKeyFrames(0, 0);
  return n + (int)r.cells_touched + map.width + (int)map.data.size() + (int)centers.points.size() + (int)server.info().cells + (int)fromKeyFrames.info().epoch;
}
'''


def test_octo_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "octo_adapter.cpp"
    src.write_text(ADAPTER_SRC)
    exe = tmp_path / "octo_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
