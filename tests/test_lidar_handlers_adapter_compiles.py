"""pcm_amd::LidarPreprocess (include/pcm_amd/registration.hpp) meets a compiler: written the way a sensor_msgs::PointCloud2
callback would drive it -- a byte buffer, a point count and field offsets, no ROS type --, against the declaration-only PCL / Eigen
stand-ins of tests/stubs, compiled and linked against libpcm_amd.so (every pcm_lidar_* / pcm_lio_frame_begin_cloud call of the
adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
#include <cstdint>
#include <vector>
struct Msg { std::vector<uint8_t> data; uint32_t width = 0, height = 1, point_step = 32; };
int main() {
  Msg msg;
  pcm_amd::LidarPreprocess pre(PCM_LIDAR_RSLIDAR);
  pre.Blind() = 0.5; pre.NumScans() = 16; pre.PointFilterNum() = 1; pre.TimeScale() = 1000.f;
  pre.desc().stride_bytes = msg.point_step;
  std::vector<float> cloud_out;
  size_t m = pre.Process(msg.data.data(), (size_t)msg.width * msg.height, &cloud_out);
  pcm_ctx* ctx = pcm_create(0, nullptr);
  pcm_amd::LidarPreprocess frame(PCM_LIDAR_VELODYNE, ctx);
  frame.desc().time_offset_bytes = 20; frame.desc().time_kind = PCM_LIDAR_TIME_FLOAT;
  std::vector<pcm_imu_pose> IMUpose(2);
  pcm_lio_state end_state{};
  m += frame.FrameBegin(msg.data.data(), (size_t)msg.width * msg.height, 0.5f, IMUpose.data(), (int)IMUpose.size(), &end_state);
  pcm_lidar_desc d;
  m += (size_t)pcm_lidar_default_desc(PCM_LIDAR_OUSTER, &d) + (size_t)pcm_lidar_default_desc(PCM_LIDAR_LIVOX_STD, &d);
  pcm_destroy(ctx);
  return (int)m + (pre.GivenOffsetTime() ? 1 : 0);
}
"""


def test_lidar_preprocess_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "lidar_preprocess_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "lidar_preprocess_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
