"""pcm_amd::LioFilter::imuInit / propagate / processFrame (include/pcm_amd/registration.hpp) meet a compiler: written the way
LaserMapping::Run would replace p_imu_->Process and the rest of the frame (laser_mapping.cc:301-356), against the declaration-only
PCL / Eigen stand-ins of tests/stubs, compiled and linked against libpcm_amd.so (pcm_lio_default_imu_state, pcm_lio_imu_init and
pcm_lio_propagate resolve to exported symbols).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
#include <vector>
int main() {
  pcm_ctx* ctx = pcm_create(0, nullptr);
  pcm_amd::LioFilter kf(ctx);
  kf.Imu().cov_acc_scale[0] = 0.1; kf.Imu().lidar_T_wrt_imu[0] = 0.04165;
  pcm_lio_filter_state x{};
  x.rot[3] = 1.0; x.off_R[3] = 1.0; x.grav[0] = 9.809;
  std::vector<double> P(23 * 23, 0.0);
  std::vector<pcm_imu_sample> imu(20);
  for (int i = 0; i < 20; i++) { imu[i].t = 0.005 * (i + 1); imu[i].acc[2] = 9.81; }
  std::vector<unsigned char> msg(20 * 100, 0);
  pcm_lio_frame_params fp{6, 2, 0.1, 0.5f, 0};
  int n = 0;
  try {
    while (!kf.imuInit(imu.data(), 20, &x, P.data())) n++;
    n += (int)kf.propagate(imu.data(), 20, 0.1, 0.2, &x, P.data()).size();
    pcm_amd::LioFilter::Frame f = kf.processFrame(msg.data(), 100, imu.data(), 20, 0.2, 0.3, fp, 0.5f, &x, P.data());
    n += f == pcm_amd::LioFilter::Frame::Updated ? kf.last().iterations : 0;
    n += kf.EkfInited() ? 1 : 0;
  } catch (const std::runtime_error&) { n = -1; }
  pcm_destroy(ctx);
  return n;
}
"""


def test_lio_propagate_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "lio_propagate_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "lio_propagate_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
