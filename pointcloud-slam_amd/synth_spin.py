"""Synthetic spinning multi-beam LiDAR scans (PointXYZIRT records) for the LOAM front end.

``make_spin`` ray-casts ``synth.make_scene`` from a sensor pose with a VLP-16 shaped (16 x 1800, +-15 deg) or a 128 x 1800 beam
pattern: azimuth jitter, range noise, ranges quantised to 2 mm (so tied curvatures occur), random dropouts and whole empty rings,
duplicate returns that land in an occupied cell (the first point in input order owns it), in firing (column-major) or shuffled
order.  It also returns the ground-truth pose (roll, pitch, yaw, x, y, z) and LOAM corner / surf maps of the same scene from
synth_loam's samplers, so that a frame can be registered end to end."""
from __future__ import annotations

import dataclasses
import importlib
import math

import numpy as np

synth = importlib.import_module(__package__ + ".synth") if __package__ else importlib.import_module("synth")
synth_loam = importlib.import_module(__package__ + ".synth_loam") if __package__ else importlib.import_module("synth_loam")

SHAPES = {16: (-15.0, 15.0), 128: (-25.0, 15.0)}   # rings -> vertical field of view [deg]


@dataclasses.dataclass
class SpinFrame:
    records: np.ndarray      # (N, 48) uint8 PointXYZIRT
    x_gt: np.ndarray         # (6,) float32 body pose in the world (roll, pitch, yaw, x, y, z)
    corner_map: np.ndarray   # (M_c, 4) float32 world frame
    surf_map: np.ndarray     # (M_s, 4)
    n_scan: int
    horizon_scan: int


def spin_points(scene, x_gt, n_scan=16, horizon_scan=1800, seed=0, order="firing", dropout=0.05, empty_rings=1, duplicates=0.01,
                range_noise=0.005, quantum=0.002, max_range=120.0):
    """(N, 48) PointXYZIRT records of one revolution seen from x_gt."""
    from .registration import pack_xyzirt
    rng = np.random.default_rng(seed)
    lo, hi = SHAPES.get(n_scan, (-15.0, 15.0))
    elev = np.radians(np.linspace(lo, hi, n_scan))
    az = 2 * math.pi * (np.arange(horizon_scan) + 0.5) / horizon_scan
    # firing order: column-major (every ring of column 0, then column 1, ...)
    A, E = np.meshgrid(az, elev, indexing="ij")
    ring = np.broadcast_to(np.arange(n_scan)[None, :], A.shape).reshape(-1)
    A = A.reshape(-1) + rng.normal(0.0, 0.1 * 2 * math.pi / horizon_scan, A.size)
    E = E.reshape(-1)
    d_body = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=1)
    T = synth_loam.pose_matrix(x_gt)
    d_world = d_body @ T[:3, :3].T
    r = synth.raycast(scene, T[:3, 3], d_world, max_range)
    keep = np.isfinite(r)
    keep &= rng.uniform(size=r.size) >= dropout
    for e in rng.choice(n_scan, size=min(empty_rings, n_scan), replace=False):
        keep &= ring != e
    r = r + rng.normal(0.0, range_noise, r.size)
    r = np.round(r / quantum) * quantum
    pts = (d_body * r[:, None]).astype(np.float32)
    idx = np.nonzero(keep)[0]
    # duplicate returns right after their original, nudged within the same cell
    dup = idx[rng.uniform(size=idx.size) < duplicates]
    pts_d = pts[dup] * np.float32(1.0 + 1e-4)
    allp = np.concatenate([pts[idx], pts_d])
    allr = np.concatenate([ring[idx], ring[dup]])
    key = np.concatenate([idx.astype(np.float64), dup.astype(np.float64) + 0.5])
    o = np.argsort(key, kind="stable")
    allp, allr = allp[o], allr[o]
    if order == "shuffled":
        o = rng.permutation(allp.shape[0])
        allp, allr = allp[o], allr[o]
    inten = rng.integers(0, 256, allp.shape[0])
    stamp = np.linspace(0.0, 0.1, allp.shape[0])
    return pack_xyzirt(allp, inten, allr, stamp)


def make_spin(seed: int, n_scan: int = 16, horizon_scan: int = 1800, order: str = "firing", scale: float = 15.0, n_boxes: int = 60,
              n_cyls: int = 12, n_corner_map: int = 20000, n_surf_map: int = 100000, noise: float = 0.01, **kw) -> SpinFrame:
    scene = synth.make_scene(seed, scale, n_boxes=n_boxes, n_cyls=n_cyls)
    T = synth.sensor_pose(scene, seed + 11)
    yaw = math.atan2(T[1, 0], T[0, 0])
    rng = np.random.default_rng(seed + 7777)
    x_gt = np.array([rng.normal(0, 0.01), rng.normal(0, 0.01), yaw, T[0, 3], T[1, 3], T[2, 3]], np.float32)
    rec = spin_points(scene, x_gt, n_scan, horizon_scan, seed, order, **kw)
    segs = synth_loam._segments(scene)
    corner_map = synth_loam.voxel_downsample(synth_loam._sample_edges(segs, n_corner_map, rng, noise), synth_loam.CORNER_LEAF)
    surf_map = synth_loam.voxel_downsample(synth_loam._sample_planes(scene, n_surf_map, rng, noise), synth_loam.SURF_LEAF)
    return SpinFrame(rec, x_gt, corner_map, surf_map, n_scan, horizon_scan)
