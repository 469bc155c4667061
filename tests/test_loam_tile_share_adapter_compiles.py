"""pcm_amd::LoamDynamicMap's fleet members (include/pcm_amd/registration.hpp: shareTilesWith, tileShareCount, cropBatch) meet a
compiler: written the way a fleet of localisation nodes would call them against the declaration-only PCL / Eigen stand-ins of
tests/stubs, compiled with warnings as errors and linked against libpcm_amd.so (pcm_loam_tile_share, pcm_loam_tile_share_count and
pcm_loam_dynmap_crop_batch resolve to exported symbols).  Not run: no GPU here."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <memory>
#include <vector>
using PointType = pcl::PointXYZI;
using Cloud = pcl::PointCloud<PointType>;
using Map = pcm_amd::LoamDynamicMap<PointType>;
int main() {
  // one site map, three robots: the first holds the areas, the others share them
  std::vector<std::unique_ptr<pcm_amd::LoamScanToMap<PointType>>> loams;
  std::vector<std::unique_ptr<Map>> maps;
  for (int i = 0; i < 3; i++) {
    loams.emplace_back(new pcm_amd::LoamScanToMap<PointType>(0));
    maps.emplace_back(new Map(*loams.back()));
    maps.back()->setMargin(100);
  }
  Cloud tile;
  const double box[6] = {0, 0, 0, 100, 100, 10};
  maps[0]->addCornerArea(box, tile); maps[0]->addSurfArea(box, tile);
  for (int i = 1; i < 3; i++) maps[i]->shareTilesWith(*maps[0]);
  int n = maps[0]->tileShareCount();
  std::vector<float> poses(6 * 3, 0.0f);
  std::vector<Map*> fleet;
  for (auto& m : maps) { m->load(&poses[0]); fleet.push_back(m.get()); }
  std::vector<pcm_loam_dynmap_crop_result> rec(3);
  int rc = Map::cropBatch(fleet, poses.data(), rec.data());
  rc += Map::cropBatch(fleet, poses.data());
  for (auto& m : maps) n += m->laserCloudCornerFromMapDSNum() + m->result().rebuilt;
  maps[2]->clear();                    // areas of its own again
  maps[0].reset(); loams[0].reset();   // the first holder goes, the areas stay with maps[1]
  return n + rc + rec[1].num_surf + maps[1]->tileShareCount() + maps[2]->tileShareCount() > 0 ? 0 : 1;
}
'''


def test_loam_tile_share_adapter_compiles_and_links(tmp_path, pcm):
    so = pcm.build_library()
    src = tmp_path / "loam_tile_share_adapter.cpp"
    src.write_text(SRC)
    exe = tmp_path / "loam_tile_share_adapter"
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-I", os.path.join(ROOT, "tests", "stubs"),
                    "-I", os.path.join(ROOT, "include"), str(src), so, "-o", str(exe)], check=True)
    assert exe.exists()
