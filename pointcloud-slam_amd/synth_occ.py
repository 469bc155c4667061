"""Synthetic world for the 2D occupancy map: a grid of rooms with vertical walls and door gaps, a floor,
a serpentine trajectory through the doors, and ring-structured scans in the sensor frame with yaw-only poses.  Seeded, no files.

Every ray's azimuth in the sensor frame is ``(k + 0.5 + u) * angle_increment - pi`` with ``|u| <= 0.3`` for an integer beam k,
so no point lies near a beam boundary of the virtual scan: the float ``atan2`` of the device and of the host may differ in the
last bits without moving a point to another beam (tests/test_occ_map.py asserts the margin on the restatement's own angles).
Floor returns lie below the tool's z band; wall returns above and below the band exist too (the walls are 2.5 m high)."""
from __future__ import annotations

import dataclasses
import math

import numpy as np


@dataclasses.dataclass
class World:
    segs: np.ndarray        # (M, 4) float64 wall segments x0 y0 x1 y1
    centres: np.ndarray     # (R, 2) room centres in serpentine order
    room: float
    sensor_height: float = 0.5
    wall_height: float = 2.5


@dataclasses.dataclass
class OccScans:
    poses: np.ndarray       # (S, 6) float32 roll, pitch, yaw, x, y, z (yaw, x, y only)
    clouds: list            # S arrays (n, 4) float32 x y z intensity, sensor frame
    world: World

    def keyframe_split(self, seed: int = 0, corner_share: float = 0.2):
        """Every cloud split into a 'corner' and a 'surf' cloud (the two files of the offline tool)."""
        rng = np.random.default_rng(seed + 77)
        corner, surf = [], []
        for c in self.clouds:
            m = rng.random(c.shape[0]) < corner_share
            corner.append(np.ascontiguousarray(c[m]))
            surf.append(np.ascontiguousarray(c[~m]))
        return corner, surf


def make_world(seed: int, nx: int = 3, ny: int = 2, room: float = 8.0, door: float = 2.0, centre=(0.0, 0.0)) -> World:
    """nx x ny rooms of `room` metres around `centre`; every interior wall has a door in its middle; a pillar in some rooms."""
    rng = np.random.default_rng(seed + 1313)
    x0, y0 = centre[0] - nx * room / 2, centre[1] - ny * room / 2
    segs = []
    for i in range(nx + 1):
        for j in range(ny):
            xa, ya, yb = x0 + i * room, y0 + j * room, y0 + (j + 1) * room
            if i in (0, nx):
                segs.append((xa, ya, xa, yb))
            else:
                m = (ya + yb) / 2
                segs += [(xa, ya, xa, m - door / 2), (xa, m + door / 2, xa, yb)]
    for j in range(ny + 1):
        for i in range(nx):
            ya, xa, xb = y0 + j * room, x0 + i * room, x0 + (i + 1) * room
            if j in (0, ny):
                segs.append((xa, ya, xb, ya))
            else:
                m = (xa + xb) / 2
                segs += [(xa, ya, m - door / 2, ya), (m + door / 2, ya, xb, ya)]
    centres = []
    for j in range(ny):
        cols = range(nx) if j % 2 == 0 else range(nx - 1, -1, -1)
        for i in cols:
            cx, cy = x0 + (i + 0.5) * room, y0 + (j + 0.5) * room
            centres.append((cx, cy))
            if rng.random() < 0.6:   # a square pillar off the centre line
                px, py, h = cx + rng.uniform(1.5, 2.5) * rng.choice([-1, 1]), cy + rng.uniform(1.5, 2.5) * rng.choice([-1, 1]), rng.uniform(0.2, 0.5)
                segs += [(px - h, py - h, px + h, py - h), (px + h, py - h, px + h, py + h), (px + h, py + h, px - h, py + h), (px - h, py + h, px - h, py - h)]
    return World(np.asarray(segs, np.float64), np.asarray(centres, np.float64), room)


def make_trajectory(world: World, seed: int, step: float = 1.0, jitter: float = 0.15):
    """(S, 6) float32 poses along the serpentine through the room centres, `step` metres apart."""
    rng = np.random.default_rng(seed + 2121)
    pts = world.centres
    out = []
    for a, b in zip(pts[:-1], pts[1:]):
        n = max(1, int(round(np.linalg.norm(b - a) / step)))
        head = math.atan2(b[1] - a[1], b[0] - a[0])
        for k in range(n):
            p = a + (b - a) * (k / n)
            out.append([0.0, 0.0, head + rng.normal(0, 0.2), p[0] + rng.uniform(-jitter, jitter), p[1] + rng.uniform(-jitter, jitter), 0.0])
    out.append([0.0, 0.0, 0.0, pts[-1][0], pts[-1][1], 0.0])
    return np.asarray(out, np.float64).astype(np.float32)


def _cast(world: World, px: float, py: float, ang: np.ndarray) -> np.ndarray:
    """Distance of the first wall along every world-frame direction (inf: none)."""
    dx, dy = np.cos(ang)[:, None], np.sin(ang)[:, None]
    s = world.segs
    ex, ey = (s[:, 2] - s[:, 0])[None], (s[:, 3] - s[:, 1])[None]
    ox, oy = (s[:, 0] - px)[None], (s[:, 1] - py)[None]
    den = dx * ey - dy * ex
    with np.errstate(divide="ignore", invalid="ignore"):
        t = (ox * ey - oy * ex) / den
        u = (ox * dy - oy * dx) / den
    ok = (np.abs(den) > 1e-12) & (t > 1e-6) & (u >= 0.0) & (u <= 1.0)
    return np.where(ok, t, np.inf).min(axis=1)


def make_scan(world: World, pose: np.ndarray, rng, rings: int = 16, n_az: int = 1800, angle_increment: float = 0.006, noise: float = 0.01,
              fov_deg: float = 15.0) -> np.ndarray:
    """One ring-structured cloud (n, 4) float32 in the sensor frame of a yaw-only pose."""
    beams = int(math.ceil(2 * 3.1415927 / angle_increment))
    k = np.minimum((np.arange(n_az) * beams) // n_az, beams - 2)   # the last, narrower beam is left out
    az = (k + 0.5 + rng.uniform(-0.3, 0.3, n_az)) * angle_increment - math.pi
    yaw, px, py = float(pose[2]), float(pose[3]), float(pose[4])
    d_wall = _cast(world, px, py, az + yaw)
    elev = np.deg2rad(np.linspace(-fov_deg, fov_deg, rings))
    out = []
    for e in elev:
        te = math.tan(e)
        z_wall = d_wall * te
        hit_wall = np.isfinite(d_wall) & (z_wall >= -world.sensor_height) & (z_wall <= world.wall_height - world.sensor_height)
        d = np.where(hit_wall, d_wall, np.inf)
        if te < 0:   # the floor in front of the wall, or where the ray passes over / beside it
            d_floor = world.sensor_height / -te
            d = np.where(hit_wall & (d_wall <= d_floor), d_wall, d_floor)
        keep = np.isfinite(d)
        dd = d[keep] + rng.normal(0, noise, int(keep.sum()))
        a = az[keep]
        out.append(np.stack([dd * np.cos(a), dd * np.sin(a), dd * te, rng.integers(0, 256, dd.size).astype(np.float64)], axis=1))
    return np.concatenate(out).astype(np.float32) if out else np.zeros((0, 4), np.float32)


def make_scans(seed: int, nx: int = 3, ny: int = 2, room: float = 8.0, step: float = 1.0, rings: int = 16, n_az: int = 1800, centre=(0.0, 0.0),
               max_scans: int | None = None, angle_increment: float = 0.006) -> OccScans:
    world = make_world(seed, nx, ny, room, centre=centre)
    poses = make_trajectory(world, seed, step)
    if max_scans is not None:
        poses = poses[:max_scans]
    rng = np.random.default_rng(seed + 555)
    clouds = [make_scan(world, p, rng, rings, n_az, angle_increment) for p in poses]
    return OccScans(poses, clouds, world)
