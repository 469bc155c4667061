"""pcm_amd::ScanFusion (include/pcm_amd/registration.hpp) meets a compiler: written the way fusion_lidar_camera.cpp's callback
drives its conversion, against the declaration-only PCL / Eigen stand-ins of tests/stubs, compiled and linked against
libpcm_amd.so (every pcm_scan_* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
#include <cstdint>
#include <vector>
using PointType = pcl::PointXYZI;
struct RsPointXYZIRT { float x, y, z, pad; uint8_t intensity; uint16_t ring = 0; double timestamp = 0; };
struct RsPointXYZIRTf { float x, y, z, pad; float intensity; uint16_t ring = 0; double timestamp = 0; };
struct PointXYZRGB { float x, y, z, pad; uint32_t rgba; float p1, p2, p3; };
static int node_pitch_table[4] = {3, 2, 1, 0};
static int node_row_table[16] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 13, 14, 15};
int main() {
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::ScanFusion<PointType> fusion(loam);
  std::vector<std::vector<double>> camera_T(3, std::vector<double>(16, 0.0));
  fusion.setCameraT(camera_T);
  fusion.setDepthFilter(1.8);
  fusion.setPitchRingTable(node_pitch_table, 4);
  pcl::PointCloud<RsPointXYZIRT> pc_lidar;
  pcl::PointCloud<RsPointXYZIRTf> pc_lidar_f;
  pcl::PointCloud<pcl::PointXYZI> pc_xyzi;
  pcl::PointCloud<PointXYZRGB> pc_depth_0, pc_depth_1;
  fusion.begin();
  fusion.addLidar(pc_lidar);
  fusion.addDepth(pc_depth_0, 0, 0, 1000);
  fusion.addDepth(pc_depth_1, 1, -1, 999000000);
  const pcm_scan_fuse_result& r = fusion.fuseToFrontEnd(nullptr);
  pcm_amd::ScanFusion<PointType> converter(0);
  converter.setOutputType(PCM_SCAN_OUT_XYZIR);
  converter.begin();
  converter.addLidar(pc_lidar_f);
  converter.addLidarOrganised(pc_xyzi, 1800, 16, node_row_table, 16);
  std::vector<unsigned char> records;
  const pcm_scan_fuse_result& q = converter.fuseToHost(&records);
  return (int)r.n_out + (int)q.n_out + (int)records.size() + (int)loam.featuresResult().num_corner;
}
"""


def test_scan_fuse_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "scan_fuse_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "scan_fuse_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
