"""pcm_amd::LoamFeatureExtraction's deskew (setDeskew / clearDeskew / the static deskewInfo) and LoamScanToMap::setInputScan with a
descriptor (include/pcm_amd/registration.hpp) meet a compiler: instantiated with a PointXYZIRT-shaped point against the
declaration-only PCL / Eigen stand-ins of tests/stubs, compiled and linked against libpcm_amd.so (every pcm_loam_* call of the adapter
resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <cstddef>
#include <cstdint>
#include <limits>
#include <memory>
#include <vector>
struct RingPoint { float x, y, z, pad; std::uint8_t intensity; double timestamp; std::uint16_t ring; };
using In = pcl::PointCloud<RingPoint>;
using Out = pcl::PointCloud<pcl::PointXYZI>;
using FE = pcm_amd::LoamFeatureExtraction<RingPoint>;
int main() {
  auto scan = std::make_shared<In>();
  std::shared_ptr<const In> cscan = scan;
  std::vector<pcm_loam_imu_sample> imu(20);
  std::vector<pcm_loam_odom_sample> odom(10);
  const double timeScanCur = 10.0, timeScanNext = std::numeric_limits<double>::infinity();
  pcm_amd::LoamDeskewTables tables;
  if (!FE::deskewInfo(timeScanCur, timeScanNext, imu.data(), imu.size(), odom.data(), odom.size(), &tables)) return 0;   // waiting for IMU data
  imu.erase(imu.begin(), imu.begin() + tables.info.imu_skipped);
  odom.erase(odom.begin(), odom.begin() + tables.info.odom_skipped);
  FE fe(0);
  fe.setDeskew(tables, offsetof(RingPoint, timestamp));
  Out corner, surf;
  fe.extract(cscan, corner, surf);
  fe.clearDeskew();
  fe.extract(cscan, corner, surf);
  fe.setDeskew(tables, offsetof(RingPoint, timestamp), PCM_LOAM_TIME_DOUBLE);
  pcm_amd::LoamScanToMap<pcl::PointXYZ> loam(0);
  tables.desc.time_offset_bytes = offsetof(RingPoint, timestamp);
  loam.setInputScan(cscan, &fe.params(), &tables.desc);
  loam.setInputScan(cscan, &fe.params());
  return (int)corner.size() + (int)surf.size() + fe.result().num_corner + loam.featuresResult().num_surf + tables.info.start_odom_index;
}
'''


def test_loam_deskew_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_deskew_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_deskew_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
