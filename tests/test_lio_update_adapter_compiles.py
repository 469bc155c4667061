"""pcm_amd::LioFilter (include/pcm_amd/registration.hpp) meets a compiler: written the way LaserMapping::Run would replace
kf_.update_iterated_dyn_share_modified (laser_mapping.cc:347), against the declaration-only PCL / Eigen stand-ins of tests/stubs,
compiled and linked against libpcm_amd.so (every pcm_lio_update* call of the adapter resolves to an exported symbol).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r"""
#include <pcm_amd/registration.hpp>
#include <vector>
int main() {
  pcm_ctx* ctx = pcm_create(0, nullptr);
  pcm_amd::LioFilter kf(ctx);
  kf.R() = 0.001; kf.MaxIter() = 4; kf.ExtrinsicEstEn() = 1; kf.Limit()[22] = 0.001;
  pcm_lio_filter_state x{};
  x.rot[3] = 1.0; x.off_R[3] = 1.0; x.grav[2] = -9.809;
  std::vector<double> P(23 * 23, 0.0);
  for (int i = 0; i < 23; i++) P[i * 23 + i] = 1.0;
  int n = 0;
  try {
    const pcm_lio_update_result& r = kf.Update(&x, P.data());
    n = r.iterations + r.rematches + r.valid_calls + r.t + kf.last().n_eff_last;
    int32_t converge = 0, n_eff = 0;
    double dx[23];
    if (kf.Trace(0, &x, &converge, &n_eff, dx)) n += converge + n_eff;
  } catch (const std::runtime_error&) { n = -1; }
  pcm_lio_state st{};
  size_t added = 0;
  pcm_lio_frame_end(ctx, &st, 0.5f, 1, &added);
  pcm_destroy(ctx);
  return n + (int)added;
}
"""


def test_lio_filter_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "lio_filter_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "lio_filter_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
