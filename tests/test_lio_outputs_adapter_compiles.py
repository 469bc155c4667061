"""pcm_amd::LioFilter's frame outputs (publishFrameWorld, publishFrameBody, publishFrameEffectWorld, finish, clearSavedMap) meet a
compiler against the declaration-only PCL / Eigen stand-ins of tests/stubs, with a point type laid out like pcl::PointXYZINormal
declared by the test itself, and link against libpcm_amd.so: every pcm_lio_* call of the adapter exists in the library."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
// the fields of pcl::PointXYZINormal (PointType of jueying_lio, common_lib.h)
struct PointXYZINormal {
  union { float data[4]; struct { float x, y, z; }; };
  union { float data_n[4]; struct { float normal_x, normal_y, normal_z; }; };
  float intensity, curvature, pad[2];
};
static_assert(sizeof(PointXYZINormal) == 48, "the layout of the frame records");
using Cloud = pcl::PointCloud<PointXYZINormal>;

int main() {
  pcm_ctx* ctx = pcm_create(0, nullptr);
  if (!ctx) return 0;                     // no device here: the link is what is checked
  pcm_amd::LioFilter kf(ctx);
  pcm_lio_filter_state x{};
  x.rot[3] = x.off_R[3] = 1.0;
  Cloud world, body, effect, map;
  int index = 0;
  try {
    const bool chunk = kf.publishFrameWorld(x, true, &world, true, 2, &index);   // laser_mapping.cc:362-365
    kf.publishFrameBody(x, &body);
    kf.publishFrameEffectWorld(x, &effect);
    if (chunk) { kf.finish(&map); kf.clearSavedMap(); }
  } catch (const std::runtime_error&) {}  // no frame on this context: PCM_ERR_NO_INPUT
  const bool any = kf.finish(&map, 0.1f, -1.0, 2.0);
  pcm_destroy(ctx);
  return any ? 1 : 0;
}
'''


def test_lio_output_adapter_compiles_and_links(tmp_path):
    inc = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-fsyntax-only", "-x", "c++", "-"] + inc, input=SRC.encode(), check=True)
    lib = os.path.join(ROOT, "pointcloud-slam_amd", "libpcm_amd.so")
    if os.path.exists(lib):
        subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-o", str(tmp_path / "lio_outputs_adapter_link_check")] + inc +
                       ["-L", os.path.dirname(lib), "-lpcm_amd", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                       input=SRC.encode(), check=True)
