"""pcm_amd::LoamDynamicMap::buildFromKeyFrames / tileInfo / getTile (include/pcm_amd/registration.hpp) meet a compiler: written the
way a node that has just finished mapping would call them, against the declaration-only PCL / Eigen stand-ins of tests/stubs,
compiled and linked against libpcm_amd.so (pcm_loam_tiles_build, pcm_loam_tile_info and pcm_loam_tile_get resolve to exported
symbols).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <memory>
using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
int main() {
  pcm_amd::LoamScanToMap<PointType> loam(0);
  pcm_amd::LoamKeyFrameMap<PointType> keyframes(loam);
  auto corner = std::make_shared<Cloud>(), surf = std::make_shared<Cloud>();
  std::shared_ptr<const Cloud> cc = corner, cs = surf;
  const float pose[6] = {0, 0, 0, 1, 2, 3};
  keyframes.saveKeyFrame(pose, 100.0, cc, cs);
  pcm_amd::LoamDynamicMap<PointType> dynmap(loam);
  pcm_loam_tiles_params p;
  pcm_loam_default_tiles_params(&p);
  p.tile_size = 25.0f;
  const pcm_loam_tiles_result& built = dynmap.buildFromKeyFrames(keyframes, &p);
  const pcm_loam_tiles_result& again = dynmap.buildFromKeyFrames(keyframes, nullptr, 0, 1);
  double box[6];
  int32_t ixy[2];
  size_t n = 0;
  Cloud tile;
  for (int i = 0; i < dynmap.surfAreas(); i++) {
    n += dynmap.tileInfo(1, i, box, ixy);
    dynmap.getTile(1, i, tile);
    n += dynmap.getTile(1, i, nullptr, 0);
  }
  float transformTobeMapped[6] = {0, 0, 0, 0, 0, 0};
  dynmap.load(transformTobeMapped);
  dynmap.dynamic_load_map(transformTobeMapped);
  return (int)n + built.num_corner_tiles + again.num_surf_tiles + (int)built.num_nonfinite + (int)tile.size() + ixy[0] + (int)box[0];
}
'''


def test_loam_tiles_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_tiles_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_tiles_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include"), str(src),
                    so, "-o", str(exe)], check=True)
    assert exe.exists()
