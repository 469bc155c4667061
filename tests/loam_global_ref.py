"""CPU restatement of jueying_slam's global map and saved map for the tests: publishGlobalMap (mapOptmization.cpp:547-590) and the
clouds visualizeGlobalMapThread saves (:524-542).

publishGlobalMap's selection (:555-583) is extractNearby's radius search and pose VoxelGrid followed by extractCloud's skip test,
with globalMapVisualizationSearchRadius / PoseDensity in place of the surrounding ones and without the window of recent key
frames: loam_submap_ref.select restates exactly those steps, so it is called with a window no key frame falls into.  Clouds go
through loam_submap_ref.transform (transformPointCloud), the VoxelGrid through the oracle.  Shares no code with csrc/loam_submap.h."""
from __future__ import annotations

import numpy as np

import loam_submap_ref as R
from oracle.loader import voxel_downsample

F = np.float32
# the general selections of tests/test_gpu_loam_global.py: synth_keyframes.make_keyframes(GENERAL_SEED, GENERAL_K) at
# (search radius, pose density, leaf)
GENERAL_SEED, GENERAL_K = 0, 120
GENERAL_CASES = ((15.0, 1.0, 0.4), (1000.0, 10.0, 1.0))


def select(poses, radius=1000.0, density=10.0) -> R.Selection:
    """:555-583; .keys = thisKeyInd of every leaf that passes :578, in globalMapKeyPosesDS order."""
    poses = np.asarray(poses, F)
    sel = R.select(poses, np.zeros(len(poses)), 0.0, radius, density, window=-np.inf)
    assert len(sel.window) == 0
    return sel


def concatenated(poses, corner, surf, keys):
    """:581-582 for every key: corner then surf cloud under the key frame's pose."""
    parts = []
    for k in keys:
        parts.append(R.transform(corner[k], poses[k]))
        parts.append(R.transform(surf[k], poses[k]))
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), F)


def global_map(poses, corner, surf, radius=1000.0, density=10.0, leaf=1.0):
    """publishGlobalMap -> (selection, globalMapKeyFrames, globalMapKeyFramesDS)."""
    sel = select(poses, radius, density)
    cloud = concatenated(poses, corner, surf, sel.keys)
    ds = voxel_downsample(cloud, leaf) if len(cloud) and leaf > 0 else cloud.copy()
    return sel, cloud, ds


def export(poses, corner, surf, which, first=0, n=None):
    """:530-541 over key frames [first, first + n): 0 globalCornerCloud, 1 globalSurfCloud, 2 globalMapCloud."""
    n = len(poses) - first if n is None else n
    ks = range(first, first + n)
    co = [R.transform(corner[k], poses[k]) for k in ks]
    su = [R.transform(surf[k], poses[k]) for k in ks]
    parts = {0: co, 1: su, 2: co + su}[which]
    return np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), F)


def voxel_grid_pinned(cloud, leaf):
    """The VoxelGrid as DESIGN.md sections 10 / 11 pin it on the device, in numpy: pcl's leaf index, leaves in index order, a leaf's
    points in input order, double sums, one rounding to float.  Independent of the oracle's C."""
    cloud = np.asarray(cloud, F)
    inv = F(1.0) / F(leaf)
    cell = np.floor(cloud[:, :3] * inv)
    mn = np.floor(cloud[:, :3].min(axis=0) * inv)
    dims = (np.floor(cloud[:, :3].max(axis=0) * inv) - mn).astype(np.int64) + 1
    ijk = (cell - mn).astype(np.int64)
    lin = ijk[:, 0] + ijk[:, 1] * dims[0] + ijk[:, 2] * dims[0] * dims[1]
    order = np.argsort(lin, kind="stable")
    starts = np.nonzero(np.diff(lin[order], prepend=-1))[0]
    sums = np.add.reduceat(cloud[order].astype(np.float64), starts, axis=0)
    counts = np.diff(np.append(starts, len(order))).astype(np.float64)
    return (sums / counts[:, None]).astype(F)
