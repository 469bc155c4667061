"""Synthetic LOAM key-frame trajectories for the key-frame store and the surrounding-key-frame submap.

``make_keyframes`` drives a lawn-mower trajectory over one ``synth_loam`` scene: key frames about 0.6 m and 0.7 s apart on
straight lanes 0.4 m apart, driven back and forth.  Later lanes therefore revisit the 1 m pose leaves of earlier ones, which is
what makes jueying_slam's key-pose VoxelGrid average far-apart key indices (a leaf holding keys {10, 130} selects key frame 70);
the 10 s window of recent key frames reaches about 8 m back, so with a small search radius some of its entries are skipped.
Each key frame's corner / surf clouds are samples of the scene's edges / planes within ``scan_radius`` of the pose, in the key
frame's body frame, with a random intensity (x, y, z, intensity)."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import synth, synth_loam


@dataclasses.dataclass
class KeyFrames:
    poses: np.ndarray      # (K, 6) float32 roll, pitch, yaw, x, y, z
    times: np.ndarray      # (K,) float64 seconds
    corner: list           # K arrays (n_c, 4) float32, body frame, x y z intensity
    surf: list             # K arrays (n_s, 4)
    time_cur: float        # timeLaserInfoCur of the frame that follows the last key frame


def make_trajectory(seed: int, K: int, step: float = 0.6, dt: float = 0.7, lane_gap: float = 0.4, lane_len: float = 36.0,
                    origin=(12.0, 15.0, 1.5), jitter: float = 0.03):
    """(poses (K,6) float32, times (K,) float64) of the lawn-mower."""
    rng = np.random.default_rng(seed + 4242)
    per_lane = int(round(lane_len / step))
    poses = np.zeros((K, 6), np.float64)
    for i in range(K):
        lane, j = divmod(i, per_lane)
        fwd = lane % 2 == 0
        s = (j + 0.5) * step
        x = origin[0] + (s if fwd else lane_len - s)
        y = origin[1] + lane * lane_gap
        yaw = 0.0 if fwd else math.pi
        poses[i] = [rng.normal(0, 0.01), rng.normal(0, 0.01), yaw + rng.normal(0, 0.02), x + rng.normal(0, jitter), y + rng.normal(0, jitter),
                    origin[2] + rng.normal(0, jitter)]
    times = 100.0 + dt * np.arange(K) + rng.uniform(-0.05, 0.05, K)
    return poses.astype(np.float32), times.astype(np.float64)


def make_keyframes(seed: int, K: int, n_corner: int = 150, n_surf: int = 600, scan_radius: float = 20.0, scale: float = 15.0, noise: float = 0.01,
                   **traj) -> KeyFrames:
    scene = synth.make_scene(seed, scale, n_boxes=60, n_cyls=12)
    poses, times = make_trajectory(seed, K, **traj)
    rng = np.random.default_rng(seed + 99)
    segs = synth_loam._segments(scene)
    pool_c = synth_loam._sample_edges(segs, 40 * n_corner, rng, noise)
    pool_s = synth_loam._sample_planes(scene, 40 * n_surf, rng, noise)
    corner, surf = [], []
    for k in range(K):
        out = []
        for pool, n in ((pool_c, n_corner), (pool_s, n_surf)):
            d = np.linalg.norm(pool[:, :2] - poses[k, 3:5].astype(np.float64)[None], axis=1)
            idx = np.nonzero(d < scan_radius)[0]
            idx = idx[rng.permutation(idx.size)[:n]]
            b = synth_loam._to_body(pool[idx], poses[k])
            b[:, 3] = rng.integers(0, 256, b.shape[0]).astype(np.float32)
            out.append(b)
        corner.append(out[0])
        surf.append(out[1])
    return KeyFrames(poses, times, corner, surf, float(times[-1] + 0.1))
