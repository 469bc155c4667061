"""pcm_amd::LoamFeatureExtraction's cachePointCloud / frameBegin / cloudDesc (include/pcm_amd/registration.hpp) meet a compiler:
instantiated with a message type that has sensor_msgs::PointCloud2's members, against the declaration-only PCL / Eigen stand-ins of
tests/stubs, compiled and linked against libpcm_amd.so (the pcm_loam_cloud_* calls of the adapter resolve to exported symbols).  Not run: no
GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <cstdint>
#include <string>
#include <vector>
namespace sensor_msgs {
struct PointField { std::string name; std::uint32_t offset; std::uint8_t datatype; std::uint32_t count; };
struct PointCloud2 { std::uint32_t height, width; std::vector<PointField> fields; bool is_bigendian; std::uint32_t point_step, row_step; std::vector<std::uint8_t> data; bool is_dense; };
}
struct RingPoint { float x, y, z, pad; std::uint8_t intensity; double timestamp; std::uint16_t ring; };
using FE = pcm_amd::LoamFeatureExtraction<RingPoint>;
int main() {
  sensor_msgs::PointCloud2 msg;
  msg.height = 16; msg.width = 1800; msg.point_step = 26; msg.is_dense = false; msg.is_bigendian = false; msg.row_step = 26 * 1800;
  msg.fields = {{"x", 0, 7, 1}, {"y", 4, 7, 1}, {"z", 8, 7, 1}, {"intensity", 12, 2, 1}, {"timestamp", 16, 8, 1}, {"ring", 24, 4, 1}};
  msg.data.resize((size_t)msg.point_step * msg.height * msg.width);
  FE fe(0);
  fe.setLidarType(PCM_LOAM_LIDAR_RSLIDAR_16);
  fe.setRecordKind(PCM_LOAM_CLOUD_MAPPING);
  fe.setTimeField("timestamp");
  const pcm_loam_cloud_desc d = fe.cloudDesc(msg);
  const pcm_loam_cloud_result& c = fe.cachePointCloud(msg);
  const pcm_loam_features_result& r = fe.frameBegin(msg);
  return (int)c.n_out + r.num_corner + (int)fe.cloudResult().n_nonfinite + (fe.context() != nullptr) + d.synth_ring;
}
'''


def test_loam_cloud_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_cloud_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_cloud_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
