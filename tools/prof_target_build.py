"""The device work of the target and candidate-list builds, for a profiler run (profiles/target_build_*): one cold P2PLANE
registration with the lists asked for, one incremental map update with LRU eviction, one GICP registration.  Small clouds: the
run is about which kernels and which runtime calls are made, not how long they take.

  rocprofv3 --kernel-trace --stats -d OUT -- python tools/prof_target_build.py
  rocprofv3 --hip-trace --stats -d OUT -- python tools/prof_target_build.py       # a run of its own
PCM_AMD_LIBRARY names another build of the library (the parent commit's, for the comparison)."""
import importlib
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import pointcloud_slam_amd as pcm

synth = importlib.import_module("pointcloud-slam_amd.synth")
scan, submap, T = synth.corner_scene(5000, 20000, seed=3, noise=0.01)
rng = np.random.default_rng(4)

g = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27, flags=pcm.capi.PCM_FLAG_NEIGHBOUR_LISTS)
g.set_input_target(submap)
g.set_input_source(scan)
r = g.align(T)
print("cold P2PLANE with lists: converged %d, %d iterations" % (r.converged, r.iterations))

g = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27, map_capacity=400)
g.set_input_target(submap)
g.set_input_source(scan)
g.evaluate_cost(T)                                                  # the full build
new = (rng.uniform(0.0, 10.0, (3000, 3)) + [20.0, 4.0, -2.0]).astype(np.float32)   # new territory: more voxels than the capacity holds
g.target_insert(new)
g.evaluate_cost(T)                                                  # the incremental update, with eviction
print("incremental update: %d log points, %d voxels, %d batch hazards" % (len(g.get_target()), g.stats()["target_voxels"], g.stats()["lru_batch_hazards"]))

g = pcm.GicpRegistration(0)
g.set_input_target(submap[:6000])
g.set_input_source(scan[:3000])
r = g.align(T)
print("GICP: converged %d, %d iterations" % (r.converged, r.iterations))
