"""Synthetic loop-closing trajectory of full LiDAR scans for the Scan Context store.

``make_loop`` drives one ``synth.make_scene``: ``n_out`` frames out along a line, a detour of ``n_detour`` frames on a circle
beside it, and ``n_out`` frames back over the early poses, displaced by ``offset`` metres and with the heading turned by
``turn`` radians.  Every frame is one revolution of ``synth_spin.spin_points`` (xyz in the body frame), so a returning frame sees
what its early partner saw, rotated: its Scan Context matches the partner's under a column shift of
``num_sector - turn / (2 pi / num_sector)``."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import synth, synth_spin


@dataclasses.dataclass
class LoopFrames:
    poses: np.ndarray    # (K, 6) float32 roll, pitch, yaw, x, y, z
    clouds: list         # K arrays (N, 3) float32, body frame
    partner: np.ndarray  # (K,) int: the early frame a returning frame revisits, -1 elsewhere
    turn: float


def make_poses(n_out: int = 12, n_detour: int = 24, step: float = 1.5, offset: float = 0.3, turn: float = 2.5, origin=(14.0, 18.0, 1.5), radius: float = 7.0):
    K = 2 * n_out + n_detour
    poses = np.zeros((K, 6), np.float64)
    partner = np.full(K, -1, np.int64)
    for i in range(n_out):
        poses[i, 2:] = [0.05, origin[0] + i * step, origin[1], origin[2]]
    ex, ey = poses[n_out - 1, 3], poses[n_out - 1, 4]
    for j in range(n_detour):
        a = 2 * math.pi * (j + 0.5) / n_detour
        poses[n_out + j, 2:] = [a, ex + radius * math.sin(a), ey + radius * (1.0 - math.cos(a)), origin[2]]
    for i in range(n_out):
        k = n_out + n_detour + i
        poses[k] = poses[i]
        poses[k, 2] += turn
        poses[k, 4] += offset
        partner[k] = i
    return poses.astype(np.float32), partner


def make_loop(seed: int = 0, scale: float = 15.0, n_scan: int = 16, horizon_scan: int = 1800, **kw) -> LoopFrames:
    scene = synth.make_scene(seed, scale, n_boxes=60, n_cyls=12)
    turn = kw.get("turn", 2.5)
    poses, partner = make_poses(**kw)
    clouds = []
    for k in range(poses.shape[0]):
        rec = synth_spin.spin_points(scene, poses[k], n_scan, horizon_scan, seed=1000 * seed + k, empty_rings=0)
        clouds.append(np.ascontiguousarray(rec[:, :12]).view(np.float32).reshape(-1, 3).copy())
    return LoopFrames(poses, clouds, partner, turn)
