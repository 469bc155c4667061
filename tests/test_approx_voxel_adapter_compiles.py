"""pcm_amd::ApproximateVoxelGrid of include/pcm_amd/registration.hpp meets a compiler: under the name pcl::ApproximateVoxelGrid it
is driven the way fast_gicp's gicp_align prepares its clouds (src/align.cpp:136-147: one filter object, setLeafSize with three
equal floats, setInputCloud with a non-const PointCloud::Ptr, filter into a fresh cloud, twice) and the way pygicp's downsample
does (double leaves), for two point types, against the declaration-only PCL / Eigen stand-ins of tests/stubs/ with g++
-fsyntax-only; then compiled and linked against libpcm_amd.so, which checks the pcm_* call against the exported symbols."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SRC = r'''
#include <pcm_amd/registration.hpp>
#include <memory>

namespace pcl { template <typename PointT> using ApproximateVoxelGrid = pcm_amd::ApproximateVoxelGrid<PointT>; }

template <typename P> static size_t prepare(double resolution) {
  typename pcl::PointCloud<P>::Ptr target_cloud(new pcl::PointCloud<P>());
  typename pcl::PointCloud<P>::Ptr source_cloud(new pcl::PointCloud<P>());
  target_cloud->points.resize(8);
  source_cloud->points.resize(5);

  pcl::ApproximateVoxelGrid<P> voxelgrid;
  voxelgrid.setLeafSize(0.1f, 0.1f, 0.1f);

  typename pcl::PointCloud<P>::Ptr filtered(new pcl::PointCloud<P>());
  voxelgrid.setInputCloud(target_cloud);
  voxelgrid.filter(*filtered);
  target_cloud = filtered;

  filtered.reset(new pcl::PointCloud<P>());
  voxelgrid.setInputCloud(source_cloud);
  voxelgrid.filter(*filtered);
  source_cloud = filtered;

  voxelgrid.setLeafSize(resolution, resolution, resolution);   // pygicp's downsample hands doubles over
  typename pcl::PointCloud<P>::ConstPtr again = target_cloud;
  voxelgrid.setInputCloud(again);
  voxelgrid.filter(*filtered);
  return target_cloud->size() + source_cloud->size() + filtered->size() + voxelgrid.dropped();
}

static bool unequal_leaves_throw() {
  pcm_amd::ApproximateVoxelGrid<pcl::PointXYZ> g;
  try { g.setLeafSize(0.1f, 0.1f, 0.2f); } catch (const std::invalid_argument&) { return true; }
  return false;
}

int main() { return prepare<pcl::PointXYZ>(0.25) + prepare<pcl::PointXYZI>(0.5) > 0 && unequal_leaves_throw() ? 0 : 1; }
'''


def test_approx_voxel_adapter_compiles_and_links(tmp_path):
    inc = ["-I", os.path.join(ROOT, "tests", "stubs"), "-I", os.path.join(ROOT, "include")]
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-Wno-unused-parameter", "-fsyntax-only", "-x", "c++", "-"] + inc, input=SRC.encode(), check=True)
    lib = os.path.join(ROOT, "pointcloud-slam_amd", "libpcm_amd.so")
    if os.path.exists(lib):   # the pcm_* symbol the adapter calls exists in the library (no GPU needed to link)
        subprocess.run(["g++", "-std=c++17", "-x", "c++", "-", "-o", str(tmp_path / "approx_voxel_adapter_link_check")] + inc +
                       ["-L", os.path.dirname(lib), "-lpcm_amd", "-Wl,-rpath," + os.path.dirname(lib), "-Wl,--unresolved-symbols=ignore-in-shared-libs"],
                       input=SRC.encode(), check=True)
