"""Synthetic localisation maps: a ``synth_loam`` corner / surf map cut into a grid of area tiles, as jueying_slam's map tool
saves them (one PCD per area and a CSV area list with its bounding box, include/dynamic_map.h:16-106).

``make_tiles`` cuts the two maps with different grids and stores the surf list in a shuffled order, so the two lists differ in
number, boxes and order.  A tile's box is the true bounding box of its points (float64 of the float32 coordinates), so the
extreme points of every tile lie exactly on its box; a grid cell without points becomes an empty tile with the cell's nominal
box, and ``n_emptied`` further tiles lose their points but keep their boxes.  ``make_sized_tiles`` lays tiles of prescribed sizes
on a line of cells (for tests that need tile boundaries at given positions of the concatenation).

Nothing here is read by the library: tile clouds go in as arrays (there is no PCD reader).
"""
from __future__ import annotations

import dataclasses

import numpy as np

from . import synth_loam


@dataclasses.dataclass
class TileSet:
    corner_boxes: np.ndarray   # (Tc, 6) float64: x_min, y_min, z_min, x_max, y_max, z_max
    corner_tiles: list         # Tc arrays (n, 4) float32: x y z intensity, map frame
    surf_boxes: np.ndarray     # (Ts, 6)
    surf_tiles: list
    lo: np.ndarray             # (2,) lower x, y corner of the map
    hi: np.ndarray             # (2,) upper corner
    corner: np.ndarray = None  # make_tiles: one scan's features in the body frame, as synth_loam.LoamFrame
    surf: np.ndarray = None
    x_gt: np.ndarray = None    # (6,) the pose the scan was taken at (near the map's centre)
    x_guess: np.ndarray = None

    def lists(self):
        return ((self.corner_boxes, self.corner_tiles), (self.surf_boxes, self.surf_tiles))


def cut(points: np.ndarray, nx: int, ny: int, lo, hi):
    """(boxes (nx * ny, 6), tiles) of ``points`` (N, 4) over the nx x ny grid on [lo, hi], row-major in (iy, ix); a tile keeps the
    points' order."""
    p = np.asarray(points, np.float32)
    size = (np.asarray(hi, np.float64) - np.asarray(lo, np.float64)) / np.array([nx, ny], np.float64)
    ix = np.clip(np.floor((p[:, 0].astype(np.float64) - lo[0]) / size[0]).astype(np.int64), 0, nx - 1)
    iy = np.clip(np.floor((p[:, 1].astype(np.float64) - lo[1]) / size[1]).astype(np.int64), 0, ny - 1)
    zmin, zmax = (float(p[:, 2].min()), float(p[:, 2].max())) if len(p) else (0.0, 0.0)
    boxes, tiles = [], []
    for j in range(ny):
        for i in range(nx):
            t = p[(ix == i) & (iy == j)]
            if len(t):
                q = t[:, :3].astype(np.float64)
                boxes.append(np.concatenate([q.min(axis=0), q.max(axis=0)]))
            else:
                boxes.append(np.array([lo[0] + i * size[0], lo[1] + j * size[1], zmin, lo[0] + (i + 1) * size[0], lo[1] + (j + 1) * size[1], zmax]))
            tiles.append(np.ascontiguousarray(t))
    return np.asarray(boxes, np.float64), tiles


def make_tiles(seed: int, grid_corner=(4, 3), grid_surf=(3, 5), n_corner_map: int = 3000, n_surf_map: int = 15000, n_emptied: int = 1, scale: float = 15.0) -> TileSet:
    """A synth_loam map of scene ``seed`` as two lists of area tiles."""
    f = synth_loam.make_frame(seed, scale=scale, n_corner_map=n_corner_map, n_surf_map=n_surf_map, n_corner=80, n_surf=500)
    rng = np.random.default_rng(seed + 4242)
    corner = f.corner_map.copy()
    surf = f.surf_map.copy()
    corner[:, 3] = rng.uniform(0.0, 255.0, len(corner)).astype(np.float32)
    surf[:, 3] = rng.uniform(0.0, 255.0, len(surf)).astype(np.float32)
    both = np.concatenate([corner[:, :2], surf[:, :2]]).astype(np.float64)
    lo, hi = both.min(axis=0), both.max(axis=0)
    cb, ct = cut(corner, grid_corner[0], grid_corner[1], lo, hi)
    sb, st = cut(surf, grid_surf[0], grid_surf[1], lo, hi)
    for boxes, tiles in ((cb, ct), (sb, st)):
        full = [k for k, t in enumerate(tiles) if len(t)]
        for k in rng.permutation(full)[:n_emptied]:
            tiles[int(k)] = np.zeros((0, 4), np.float32)   # the box stays
    perm = rng.permutation(len(st))   # the surf list is not in grid order
    sb, st = sb[perm], [st[int(k)] for k in perm]
    return TileSet(cb, ct, sb, st, lo, hi, f.corner, f.surf, f.x_gt, f.x_guess)


def make_sized_tiles(seed: int, sizes_corner, sizes_surf, cell: float = 20.0, z_range=(0.0, 4.0)) -> TileSet:
    """Tiles of the given point counts: tile k of a list fills cell k of a line of ``cell`` x ``cell`` squares along x (the two lists
    overlap the same squares), points uniform inside the square.  A tile of size 0 keeps its square as its box; the others
    get their true bounding box."""
    rng = np.random.default_rng(seed + 977)

    def build(sizes):
        boxes, tiles = [], []
        for k, n in enumerate(sizes):
            x0 = k * cell
            t = np.zeros((int(n), 4), np.float32)
            t[:, 0] = rng.uniform(x0, x0 + cell, n)
            t[:, 1] = rng.uniform(0.0, cell, n)
            t[:, 2] = rng.uniform(z_range[0], z_range[1], n)
            t[:, 3] = rng.uniform(0.0, 255.0, n)
            if n:
                q = t[:, :3].astype(np.float64)
                boxes.append(np.concatenate([q.min(axis=0), q.max(axis=0)]))
            else:
                boxes.append(np.array([x0, 0.0, z_range[0], x0 + cell, cell, z_range[1]]))
            tiles.append(t)
        return np.asarray(boxes, np.float64).reshape(-1, 6), tiles

    cb, ct = build(list(sizes_corner))
    sb, st = build(list(sizes_surf))
    n = max(len(ct), len(st), 1)
    return TileSet(cb, ct, sb, st, np.array([0.0, 0.0]), np.array([n * cell, cell]))
