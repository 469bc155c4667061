"""Synthetic inputs of the scan fusion: an organised LiDAR cloud as vendor records and depth-camera
clouds as pcl::PointXYZRGB records.

``lidar_cloud`` ray-casts ``synth.make_scene`` with a 16 x W (row-major: id / width is the row) or 128 x W (column-major: id %
height is the row) beam pattern; a beam without a return, and a random share of the others, is a NaN point, as the drivers of
organised clouds publish them.  ``pack_rs_f32`` / ``pack_rs_u8`` / ``pack_hesai`` / ``pack_xyzi`` lay the cloud out as the
records of rs_to_velodyne.cpp, fusion_lidar_camera.cpp, hesai_to_velodyne.cpp and pcl::PointXYZI, with increasing double time
stamps.  ``depth_cloud`` is a pinhole grid over a smooth depth field with NaN holes and points beyond the depth filter; its
first points are placed, through the inverse of the camera transform, on every branch of the node's pitch rule (below
pitch_min, inside the table, in the half-unit below pitch_max whose index leaves the table, at and above pitch_max, and at the
LiDAR origin).  Every camera point is kept ``margin`` away from the values of the pitch at which a last-bit difference of asin
could change its ring; a point that is not becomes a NaN hole.  The tables below are synthetic (a permutation, a reversal): the
reference's own tables are the caller's to pass."""
from __future__ import annotations

import importlib
import math

import numpy as np

synth = importlib.import_module(__package__ + ".synth") if __package__ else importlib.import_module("synth")
synth_loam = importlib.import_module(__package__ + ".synth_loam") if __package__ else importlib.import_module("synth_loam")

F, D = np.float32, np.float64
PITCH_SCALE, PITCH_MIN, PITCH_MAX, PITCH_OFFSET = 28.6478897565, -40.0, 12.0, 40.0
SHAPES = {16: (-15.0, 15.0), 128: (-25.0, 15.0)}


def ring_table(rows: int, seed: int = 0) -> np.ndarray:
    """A synthetic row -> ring table (int32, a fixed permutation of 0 .. rows - 1)."""
    return np.random.default_rng(1000 + seed + rows).permutation(rows).astype(np.int32)


def identity_table(rows: int) -> np.ndarray:
    return np.arange(rows, dtype=np.int32)


def pitch_table(n: int = 52) -> np.ndarray:
    """A synthetic pitch-index -> ring table of n entries (int32)."""
    return (np.arange(n, dtype=np.int32)[::-1] * 3) % 61


def lidar_cloud(seed: int, rows: int = 16, width: int = 40, nan_frac: float = 0.1, scale: float = 15.0):
    """(xyz (rows * width, 3) float32 with NaN rows, ring-row of every point, x_gt) in the cloud's own point order."""
    scene = synth.make_scene(seed, scale, n_boxes=40, n_cyls=8)
    T = synth.sensor_pose(scene, seed + 11)
    rng = np.random.default_rng(seed + 5)
    lo, hi = SHAPES.get(rows, (-15.0, 15.0))
    elev = np.radians(np.linspace(lo, hi, rows))
    az = 2 * math.pi * (np.arange(width) + 0.5) / width
    if rows == 128:   # column-major
        A, E = np.meshgrid(az, elev, indexing="ij")
        row = np.broadcast_to(np.arange(rows)[None, :], A.shape).reshape(-1)
    else:             # row-major
        E, A = np.meshgrid(elev, az, indexing="ij")
        row = np.broadcast_to(np.arange(rows)[:, None], A.shape).reshape(-1)
    A, E = A.reshape(-1), E.reshape(-1)
    d_body = np.stack([np.cos(E) * np.cos(A), np.cos(E) * np.sin(A), np.sin(E)], axis=1)
    r = synth.raycast(scene, T[:3, 3], d_body @ T[:3, :3].T, 120.0)
    r = np.round((r + rng.normal(0.0, 0.005, r.size)) / 0.002) * 0.002
    pts = (d_body * r[:, None]).astype(F)
    bad = ~np.isfinite(r) | (rng.uniform(size=r.size) < nan_frac)
    pts[bad] = np.nan
    # a NaN in one coordinate only is a NaN point too
    one = np.nonzero(bad)[0][::3]
    pts[one, (one % 3 + 1) % 3] = 1.0
    good = np.nonzero(~bad)[0]
    if good.size > 4:
        pts[good[3], 0] = np.inf                  # Inf is no NaN: the point passes
    yaw = math.atan2(T[1, 0], T[0, 0])
    x_gt = np.array([0.0, 0.0, yaw, T[0, 3], T[1, 3], T[2, 3]], F)
    return pts, row, x_gt, scene


def _put(rec, off, a):
    a = np.ascontiguousarray(a)
    rec[:, off:off + a.dtype.itemsize] = a.view(np.uint8).reshape(a.shape[0], a.dtype.itemsize)


def _stamps(n, t0=1670940000.25):
    return t0 + np.arange(n, dtype=D) * (0.1 / max(n, 1))


def pack_rs_f32(pts, ring, seed=0):
    """rs_to_velodyne.cpp's RsPointXYZIRT, 32 bytes: float intensity @16, uint16 ring @20, double timestamp @24."""
    n = pts.shape[0]
    rec = np.zeros((n, 32), np.uint8)
    _put(rec, 0, np.ascontiguousarray(pts[:, 0], F)); _put(rec, 4, np.ascontiguousarray(pts[:, 1], F)); _put(rec, 8, np.ascontiguousarray(pts[:, 2], F))
    _put(rec, 16, np.random.default_rng(seed).uniform(0, 255, n).astype(F))
    _put(rec, 20, np.asarray(ring).astype(np.uint16))
    _put(rec, 24, _stamps(n))
    return rec, dict(ioff=16, roff=20, toff=24, itype="f32")


def pack_rs_u8(pts, ring, seed=0):
    """fusion_lidar_camera.cpp's RsPointXYZIRT, 32 bytes: uint8 intensity @16, uint16 ring @18, double timestamp @24."""
    n = pts.shape[0]
    rec = np.zeros((n, 32), np.uint8)
    _put(rec, 0, np.ascontiguousarray(pts[:, 0], F)); _put(rec, 4, np.ascontiguousarray(pts[:, 1], F)); _put(rec, 8, np.ascontiguousarray(pts[:, 2], F))
    inten = np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8)
    if n:
        inten[n // 2] = 255
    _put(rec, 16, inten)
    _put(rec, 18, np.asarray(ring).astype(np.uint16))
    _put(rec, 24, _stamps(n))
    return rec, dict(ioff=16, roff=18, toff=24, itype="u8")


def pack_hesai(pts, ring, seed=0):
    """hesai_to_velodyne.cpp's HesaiPointXYZIRT, 48 bytes: uint8 intensity @16, double timestamp @24, uint16 ring @32."""
    n = pts.shape[0]
    rec = np.zeros((n, 48), np.uint8)
    _put(rec, 0, np.ascontiguousarray(pts[:, 0], F)); _put(rec, 4, np.ascontiguousarray(pts[:, 1], F)); _put(rec, 8, np.ascontiguousarray(pts[:, 2], F))
    _put(rec, 16, np.random.default_rng(seed).integers(0, 256, n).astype(np.uint8))
    _put(rec, 24, _stamps(n))
    _put(rec, 32, np.asarray(ring).astype(np.uint16))
    return rec, dict(ioff=16, roff=32, toff=24, itype="u8")


def pack_xyzi(pts, seed=0):
    """pcl::PointXYZI, 32 bytes: float intensity @16."""
    n = pts.shape[0]
    rec = np.zeros((n, 32), np.uint8)
    _put(rec, 0, np.ascontiguousarray(pts[:, 0], F)); _put(rec, 4, np.ascontiguousarray(pts[:, 1], F)); _put(rec, 8, np.ascontiguousarray(pts[:, 2], F))
    _put(rec, 16, np.random.default_rng(seed).uniform(0, 255, n).astype(F))
    return rec


def camera_T(k: int) -> np.ndarray:
    """The 16 doubles of a camera -> LiDAR transform as the node stores it (the transposed 4x4): camera z (depth) forward along
    LiDAR x, pitched down by 20 degrees, yawed k * 120 degrees, mounted 0.1 m ahead and 0.1 m below."""
    R0 = np.array([[0.0, 0.0, 1.0], [-1.0, 0.0, 0.0], [0.0, -1.0, 0.0]])     # optical frame -> x forward, y left, z up
    R = synth.rot_xyz(0.0, math.radians(20.0), math.radians(120.0 * k)) @ R0
    M = np.eye(4)
    M[:3, :3] = R
    M[:3, 3] = R @ np.array([0.0, 0.1, 0.1])
    return np.ascontiguousarray(M.T).reshape(16)


def _pitch(pts, T):
    """The node's pitch of camera points, with its own float / double casts (used only to keep the generator off the boundaries)."""
    T = np.asarray(T, D)
    X, Y, Z = pts[:, 0].astype(D), pts[:, 1].astype(D), pts[:, 2].astype(D)
    o = [(X * T[c] + Y * T[4 + c] + Z * T[8 + c] + T[12 + c]).astype(F) for c in range(3)]
    s = (o[0] * o[0] + o[1] * o[1]) + o[2] * o[2]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.arcsin(o[2].astype(D) / np.sqrt(s).astype(D)) * PITCH_SCALE


def _branch_points(T, rng):
    """Camera-frame points whose LiDAR-frame pitch lies well inside every branch of the rule, and one at the LiDAR origin."""
    M = np.asarray(T, D).reshape(4, 4).T
    want = [-43.5, -41.2, -39.7, -20.3, 0.2, 11.2, 11.7, 11.8, 12.4, 30.0, 44.0]
    out = []
    for p in want:
        el, az, r = p / PITCH_SCALE, rng.uniform(-math.pi, math.pi), rng.uniform(0.5, 1.5)
        q = r * np.array([math.cos(el) * math.cos(az), math.cos(el) * math.sin(az), math.sin(el)])
        out.append(np.linalg.solve(M[:3, :3], q - M[:3, 3]))
    out.append(np.linalg.solve(M[:3, :3], -M[:3, 3]))
    return np.asarray(out)


def depth_cloud(seed: int, T, n: int = 1025, width: int = 64, depth_filter: float = 1.8, nan_frac: float = 0.1, margin: float = 1e-5,
                branches: bool = True) -> np.ndarray:
    """(n, 32) uint8 pcl::PointXYZRGB records of the first n pixels of a `width`-wide pinhole grid."""
    rng = np.random.default_rng(seed)
    i = np.arange(n)
    u, v = i % width, i // width
    h = max(int(v.max()) + 1 if n else 1, 1)
    fx = 0.6 * width
    z = 1.1 + 0.9 * np.sin(0.37 * u + 0.011 * seed) * np.cos(0.23 * v) + rng.normal(0.0, 0.01, n)    # 0.2 .. 2.0: some beyond the filter
    pts = np.stack([(u - width / 2 + 0.5) / fx * z, (v - h / 2 + 0.5) / fx * z, z], axis=1)
    if branches and n:
        b = _branch_points(T, rng)[:n]
        pts[:b.shape[0]] = b
    pts = pts.astype(F)
    if n > 20:
        pts[14, 2] = F(depth_filter)              # z == depth_filter exactly: kept
        pts[15, 2] = np.nextafter(F(depth_filter), F(10))
    hole = rng.uniform(size=n) < nan_frac
    hole[:20] = False
    p = _pitch(pts, T)
    with np.errstate(invalid="ignore"):
        near = np.isfinite(p) & ((np.abs(p - PITCH_MIN) < margin) | (np.abs(p - PITCH_MAX) < margin) |
                                 (np.abs((p + PITCH_OFFSET) - np.floor(p + PITCH_OFFSET) - 0.5) < margin))
    pts[hole | near] = np.nan
    one = np.nonzero(hole)[0][::2]
    pts[one, 0] = 0.25                            # NaN in y and z only
    rec = np.zeros((n, 32), np.uint8)
    for a in range(3):
        _put(rec, 4 * a, np.ascontiguousarray(pts[:, a]))
    _put(rec, 12, np.ones(n, F))
    _put(rec, 16, rng.integers(0, 1 << 24, n).astype(np.uint32))   # rgb
    return rec
