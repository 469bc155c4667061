"""CPU restatement of jueying_slam's surrounding-key-frame submap for the tests: extractNearby / extractCloud
(mapOptmization.cpp:1153-1222), transformPointCloud (:447-470) and loopFindNearKeyframes[WithRespectTo] (:972-1018).

numpy float32 arithmetic in the reference's operation order; every pcl::VoxelGrid through the oracle (oracle.loader.voxel_downsample),
the pose matrix through loam_ref.pose_matrix.  Rules the reference tree does not pin: the radius search keeps
d2 < r2 with d2 = (dx^2 + dy^2) + dz^2 in float and returns ascending (d2, index).  It shares no code with csrc/loam_submap.h."""
from __future__ import annotations

import dataclasses

import numpy as np

import loam_ref
from oracle.loader import voxel_downsample

F = np.float32


@dataclasses.dataclass
class Selection:
    keys: np.ndarray          # key frame of every used entry, in list order
    num_near: int
    num_pose_leaves: int
    num_skipped: int
    near: np.ndarray          # (a) indices by ascending (d2, index)
    leaves: np.ndarray        # (b) (L, 4) averaged x y z index
    leaf_members: list        # (b) key indices of every leaf
    window: np.ndarray        # (c) indices, newest first


def select(poses, times, time_cur, radius=50.0, density=1.0, window=10.0) -> Selection:
    poses = np.asarray(poses, F)
    times = np.asarray(times, np.float64)
    K = poses.shape[0]
    xyz = poses[:, 3:6]
    last = xyz[K - 1]
    d = xyz - last[None, :]
    d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
    r = F(radius)
    inside = np.nonzero(d2 < r * r)[0]
    near = inside[np.lexsort((inside, d2[inside]))]
    cloud = np.concatenate([xyz[near], near.astype(F)[:, None]], axis=1).astype(F)
    leaves = voxel_downsample(cloud, density) if len(near) else np.zeros((0, 4), F)
    # which keys fell into which leaf (for the tests' conditions only): the grid of the VoxelGrid over `cloud`
    members = []
    if len(near):
        inv = F(1.0) / F(density)
        mn = np.floor(cloud[:, :3].min(axis=0) * inv)
        cell = (np.floor(cloud[:, :3] * inv) - mn).astype(np.int64)
        dims = (np.floor(cloud[:, :3].max(axis=0) * inv) - mn).astype(np.int64) + 1
        lin = cell[:, 0] + cell[:, 1] * dims[0] + cell[:, 2] * dims[0] * dims[1]
        for v in np.unique(lin):
            members.append(near[lin == v])
        assert len(members) == len(leaves)
    win = []
    for i in range(K - 1, -1, -1):
        if time_cur - times[i] < window:
            win.append(i)
        else:
            break
    win = np.asarray(win, np.int64)
    entries = np.concatenate([leaves, np.concatenate([xyz[win], win.astype(F)[:, None]], axis=1).astype(F).reshape(-1, 4)], axis=0)
    e = entries[:, :3] - last[None, :]
    dist = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1] + e[:, 2] * e[:, 2]).astype(F)
    skip = dist > r
    keys = entries[~skip, 3].astype(np.int32)   # (int) truncation; the values are >= 0
    return Selection(keys, len(near), len(leaves), int(skip.sum()), near, leaves, members, win)


def transform(cloud, pose6):
    """transformPointCloud: (N,4) body -> world under pose6 (roll, pitch, yaw, x, y, z), intensity copied."""
    cloud = np.asarray(cloud, F).reshape(-1, 4)
    T, _ = loam_ref.pose_matrix(pose6)
    out = cloud.copy()
    out[:, :3] = loam_ref.to_map(T, cloud[:, :3]) if len(cloud) else cloud[:, :3]
    return out


def _vg(cloud, leaf):
    if len(cloud) == 0 or not leaf > 0:
        return cloud.copy()
    return voxel_downsample(cloud, leaf)


def submap(poses, times, corner, surf, time_cur, radius=50.0, density=1.0, corner_leaf=0.2, surf_leaf=0.2, window=10.0):
    """extractSurroundingKeyFrames -> dict(sel, corner_in, surf_in, corner_map, surf_map)."""
    sel = select(poses, times, time_cur, radius, density, window)
    ci = [transform(corner[k], poses[k]) for k in sel.keys]
    si = [transform(surf[k], poses[k]) for k in sel.keys]
    corner_in = np.concatenate(ci, axis=0) if ci else np.zeros((0, 4), F)
    surf_in = np.concatenate(si, axis=0) if si else np.zeros((0, 4), F)
    return dict(sel=sel, corner_in=corner_in, surf_in=surf_in, corner_map=_vg(corner_in, corner_leaf), surf_map=_vg(surf_in, surf_leaf))


def near_keyframes(poses, corner, surf, key, search_num, wrt_key=-1, leaf=0.2):
    """loopFindNearKeyframes (wrt_key < 0) / loopFindNearKeyframesWithRespectTo."""
    K = len(poses)
    parts = []
    for i in range(-search_num, search_num + 1):
        k = key + i
        if k < 0 or k >= K:
            continue
        p = poses[k] if wrt_key < 0 else poses[wrt_key]
        parts.append(transform(corner[k], p))
        parts.append(transform(surf[k], p))
    cloud = np.concatenate(parts, axis=0) if parts else np.zeros((0, 4), F)
    return _vg(cloud, leaf)
