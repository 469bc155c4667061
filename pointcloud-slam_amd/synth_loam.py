"""Synthetic LOAM frames: corner (edge) and surf (plane) feature maps and one scan of features at a perturbed pose.

Built on ``synth.make_scene`` (boxes on a ground plane inside four walls, vertical cylinders); what ``synth.py`` returns is not
changed.  Edge points lie on the box edges and the cylinder silhouettes (two vertical lines per cylinder), plane points on the
ground, the walls, the box faces and the cylinder sides.  Maps and scans are down-sampled with the reference's leaf sizes
(jueying_slam utility.h:271-272, localization.cpp:159-160: corner 0.2 m, surf 0.2 x 1.5 = 0.3 m).  ``make_corridor`` is a scene
with no structure along its axis (two walls and a floor) for the degeneracy path of LMOptimization.

Poses are transformTobeMapped vectors (roll, pitch, yaw, x, y, z); ``pose_matrix`` is pcl::getTransformation in double.
"""
from __future__ import annotations

import dataclasses
import math

import numpy as np

from . import synth

CORNER_LEAF = 0.2
SURF_LEAF = 0.2 * 1.5


@dataclasses.dataclass
class LoamFrame:
    corner_map: np.ndarray   # (M_c, 4) float32 x y z 1, world frame
    surf_map: np.ndarray     # (M_s, 4)
    corner: np.ndarray       # (N_c, 4) scan features, body frame
    surf: np.ndarray         # (N_s, 4)
    x_gt: np.ndarray         # (6,) float32 the pose the scan was taken at
    x_guess: np.ndarray      # (6,) float32 the perturbed start


def pose_matrix(x) -> np.ndarray:
    """4x4 of pcl::getTransformation(x, y, z, roll, pitch, yaw) = Rz(yaw) Ry(pitch) Rx(roll), double."""
    r, p, y = float(x[0]), float(x[1]), float(x[2])
    cr, sr, cp, sp, cy, sy = math.cos(r), math.sin(r), math.cos(p), math.sin(p), math.cos(y), math.sin(y)
    T = np.eye(4)
    T[:3, :3] = [[cy * cp, cy * sp * sr - sy * cr, sy * sr + cy * sp * cr],
                 [sy * cp, cy * cr + sy * sp * sr, sy * sp * cr - cy * sr],
                 [-sp, cp * sr, cp * cr]]
    T[:3, 3] = [float(x[3]), float(x[4]), float(x[5])]
    return T


def voxel_downsample(pts: np.ndarray, leaf: float) -> np.ndarray:
    """pcl::VoxelGrid-style: the centroid of every occupied leaf, leaves in index order; (N,3) -> (K,4) float32 with w = 1."""
    p = np.asarray(pts, np.float64)[:, :3]
    key = np.floor(p / leaf).astype(np.int64)
    key -= key.min(axis=0)
    dims = key.max(axis=0) + 1
    lin = (key[:, 2] * dims[1] + key[:, 1]) * dims[0] + key[:, 0]
    uniq, inv = np.unique(lin, return_inverse=True)
    cnt = np.bincount(inv, minlength=uniq.size).astype(np.float64)
    out = np.ones((uniq.size, 4), np.float32)
    for a in range(3):
        out[:, a] = (np.bincount(inv, weights=p[:, a], minlength=uniq.size) / cnt).astype(np.float32)
    return out


def _segments(scene: synth.Scene):
    """(S, 2, 3) edge segments of the scene: 12 edges per box (bottom ones on the ground), 2 silhouettes per cylinder."""
    segs = []
    for b in scene.boxes:
        x0, y0, z0, x1, y1, z1 = b
        c = np.array([[x, y, z] for z in (z0, z1) for y in (y0, y1) for x in (x0, x1)])
        for i, j in ((0, 1), (2, 3), (4, 5), (6, 7), (0, 2), (1, 3), (4, 6), (5, 7), (0, 4), (1, 5), (2, 6), (3, 7)):
            segs.append((c[i], c[j]))
    for cx, cy, r, h in scene.cyls:
        for ang in (0.0, math.pi):
            px, py = cx + r * math.cos(ang), cy + r * math.sin(ang)
            segs.append((np.array([px, py, 0.0]), np.array([px, py, h])))
    return np.asarray(segs, np.float64)


def _sample_edges(segs: np.ndarray, n: int, rng, noise: float) -> np.ndarray:
    length = np.linalg.norm(segs[:, 1] - segs[:, 0], axis=1)
    k = rng.choice(len(segs), size=n, p=length / length.sum())
    t = rng.uniform(0.0, 1.0, n)[:, None]
    return segs[k, 0] + t * (segs[k, 1] - segs[k, 0]) + rng.normal(0.0, noise, (n, 3))


def _planes(scene: synth.Scene):
    """(origin, u, v) rectangles of the plane surfaces: ground, four walls, box sides and tops."""
    rects = [(np.array([0.0, 0.0, 0.0]), np.array([scene.lx, 0, 0]), np.array([0, scene.ly, 0]))]
    h = scene.wall_h
    rects += [(np.array([0.0, 0.0, 0.0]), np.array([scene.lx, 0, 0]), np.array([0, 0, h])),
              (np.array([0.0, scene.ly, 0.0]), np.array([scene.lx, 0, 0]), np.array([0, 0, h])),
              (np.array([0.0, 0.0, 0.0]), np.array([0, scene.ly, 0]), np.array([0, 0, h])),
              (np.array([scene.lx, 0.0, 0.0]), np.array([0, scene.ly, 0]), np.array([0, 0, h]))]
    for x0, y0, z0, x1, y1, z1 in scene.boxes:
        dx, dy, dz = np.array([x1 - x0, 0, 0]), np.array([0, y1 - y0, 0]), np.array([0, 0, z1 - z0])
        rects += [(np.array([x0, y0, z0]), dx, dz), (np.array([x0, y1, z0]), dx, dz), (np.array([x0, y0, z0]), dy, dz),
                  (np.array([x1, y0, z0]), dy, dz), (np.array([x0, y0, z1]), dx, dy)]
    return rects


def _sample_planes(scene: synth.Scene, n: int, rng, noise: float) -> np.ndarray:
    rects = _planes(scene)
    area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in rects])
    ncyl = len(scene.cyls)
    cyl_area = np.array([2 * math.pi * r * hh for _, _, r, hh in scene.cyls]) if ncyl else np.zeros(0)
    w = np.concatenate([area, cyl_area])
    k = rng.choice(len(w), size=n, p=w / w.sum())
    out = np.empty((n, 3))
    s, t = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
    for j in np.unique(k):
        m = k == j
        if j < len(rects):
            o, u, v = rects[j]
            out[m] = o + s[m, None] * u + t[m, None] * v
        else:
            cx, cy, r, hh = scene.cyls[j - len(rects)]
            ang = 2 * math.pi * s[m]
            out[m] = np.stack([cx + r * np.cos(ang), cy + r * np.sin(ang), hh * t[m]], axis=1)
    return out + rng.normal(0.0, noise, (n, 3))


def _to_body(world: np.ndarray, x) -> np.ndarray:
    T = pose_matrix(x)
    b = (world[:, :3] - T[:3, 3]) @ T[:3, :3]
    out = np.ones((b.shape[0], 4), np.float32)
    out[:, :3] = b.astype(np.float32)
    return out


def _frame(scene, seg_sampler, plane_sampler, centre, seed, n_corner_map, n_surf_map, n_corner, n_surf, scan_radius, perturb, yaw):
    rng = np.random.default_rng(seed)
    corner_map = voxel_downsample(seg_sampler(n_corner_map, rng), CORNER_LEAF)
    surf_map = voxel_downsample(plane_sampler(n_surf_map, rng), SURF_LEAF)
    x_gt = np.array([rng.normal(0, 0.02), rng.normal(0, 0.02), yaw, centre[0], centre[1], 1.5], np.float32)

    def near(p, n):
        d = np.linalg.norm(p[:, :2] - np.asarray(centre)[None, :2], axis=1)
        p = p[d < scan_radius]
        return p[rng.permutation(len(p))[:n]]

    corner_w = voxel_downsample(near(seg_sampler(4 * n_corner_map, rng), 4 * n_corner), CORNER_LEAF)
    surf_w = voxel_downsample(near(plane_sampler(4 * n_surf_map, rng), 4 * n_surf), SURF_LEAF)
    corner = _to_body(corner_w[rng.permutation(len(corner_w))[:n_corner]], x_gt)
    surf = _to_body(surf_w[rng.permutation(len(surf_w))[:n_surf]], x_gt)
    dt, dr = perturb
    u = rng.normal(size=3)
    w = rng.normal(size=3)
    x_guess = x_gt.astype(np.float64).copy()
    x_guess[:3] += math.radians(dr) * w / np.linalg.norm(w)
    x_guess[3:] += dt * u / np.linalg.norm(u)
    return LoamFrame(corner_map, surf_map, corner, surf, x_gt, x_guess.astype(np.float32))


def make_frame(seed: int, scale: float = 15.0, n_corner_map: int = 20000, n_surf_map: int = 100000, n_corner: int = 1500,
               n_surf: int = 6000, scan_radius: float = 25.0, perturb=(0.3, 3.0), n_boxes: int = 60, n_cyls: int = 12,
               noise: float = 0.01) -> LoamFrame:
    """A mapping frame: maps of the whole scene, a scan of the features within ``scan_radius`` of the sensor (taken at a
    random yaw near the scene's centre), start pose perturbed by ``perturb`` = (metres, degrees)."""
    scene = synth.make_scene(seed, scale, n_boxes=n_boxes, n_cyls=n_cyls)
    segs = _segments(scene)
    rng = np.random.default_rng(seed + 7777)
    centre = (scene.lx * rng.uniform(0.4, 0.6), scene.ly * rng.uniform(0.4, 0.6))
    return _frame(scene, lambda n, r: _sample_edges(segs, n, r, noise), lambda n, r: _sample_planes(scene, n, r, noise), centre, seed,
                  n_corner_map, n_surf_map, n_corner, n_surf, scan_radius, perturb, float(rng.uniform(-math.pi, math.pi)))


def make_corridor(seed: int, length: float = 80.0, width: float = 4.0, height: float = 3.0, n_corner_map: int = 4000,
                  n_surf_map: int = 60000, n_corner: int = 150, n_surf: int = 700, perturb=(0.2, 1.0), noise: float = 0.01) -> LoamFrame:
    """Two walls and a floor along x, nothing across it: translation along the axis is unobservable (degenerate A^T A)."""
    segs = np.array([[[0, -width / 2, 0], [length, -width / 2, 0]], [[0, width / 2, 0], [length, width / 2, 0]],
                     [[0, -width / 2, height], [length, -width / 2, height]], [[0, width / 2, height], [length, width / 2, height]]], np.float64)
    rects = [(np.array([0.0, -width / 2, 0.0]), np.array([length, 0, 0]), np.array([0, width, 0])),
             (np.array([0.0, -width / 2, 0.0]), np.array([length, 0, 0]), np.array([0, 0, height])),
             (np.array([0.0, width / 2, 0.0]), np.array([length, 0, 0]), np.array([0, 0, height]))]

    def planes(n, rng):
        area = np.array([np.linalg.norm(np.cross(u, v)) for _, u, v in rects])
        k = rng.choice(len(rects), size=n, p=area / area.sum())
        s, t = rng.uniform(0, 1, n), rng.uniform(0, 1, n)
        o = np.stack([rects[j][0] for j in k]); u = np.stack([rects[j][1] for j in k]); v = np.stack([rects[j][2] for j in k])
        return o + s[:, None] * u + t[:, None] * v + rng.normal(0.0, noise, (n, 3))

    return _frame(None, lambda n, r: _sample_edges(segs, n, r, noise), planes, (length / 2, 0.0), seed, n_corner_map, n_surf_map,
                  n_corner, n_surf, 25.0, perturb, 0.0)
