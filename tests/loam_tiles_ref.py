"""numpy restatement of the key-frame map cut into localisation area tiles (pcm_loam_tiles_build), written
from the rules and not from the library:

  tile index   ix = (int32)floorf(x / tile_size) on float32 values, iy likewise: floor, not truncation (-0.0f lies in tile 0,
               -1e-7f in tile -1, a point exactly on k * tile_size in tile k); |ix| or |iy| >= 32768: OutOfRange
  key, order   (iy + 32768) << 16 | (ix + 32768); a list's tiles in ascending key order; a tile exists only where a point lies
  cloud        leaf == 0: the tile's points, a stable partition of the input order -- as one-point means (v + 0.0f: a negative zero
               is stored as zero); leaf > 0: the VoxelGrid of the tile's points alone (loam_global_ref.voxel_grid_pinned: pcl's
               leaf index from the tile's own min / max, leaves in index order, double sums, one rounding; a sum starts from +0.0,
               so a leaf of negative zeros alone is stored as zero here as well)
  box          x_min = float64(ix) * float64(tile_size), x_max = float64(ix + 1) * float64(tile_size), the same for y; z_min / z_max
               of the stored points, widened to float64
  a point with a non-finite x, y or z is dropped and counted

The input cloud of a list is loam_global_ref.export (transformPointCloud of every key frame's cloud, in key-frame order)."""
from __future__ import annotations

import dataclasses

import numpy as np

import loam_global_ref as GR

F = np.float32
LIMIT = 32768


class OutOfRange(Exception):
    pass


@dataclasses.dataclass
class Tile:
    ix: int
    iy: int
    box: np.ndarray       # (6,) float64 x_min, y_min, z_min, x_max, y_max, z_max
    points: np.ndarray    # (n, 4) float32


def tile_index(v, tile_size):
    """floorf(v / tile_size) in float32, as float32 (the caller tests the range before the cast)."""
    with np.errstate(over="ignore", invalid="ignore"):
        return np.floor(np.asarray(v, F) / F(tile_size)).astype(F)


def tile_key(ix, iy):
    return ((np.asarray(iy, np.int64) + LIMIT) << 16) | (np.asarray(ix, np.int64) + LIMIT)


def tile_box_xy(ix, iy, tile_size):
    t = np.float64(F(tile_size))
    return np.float64(ix) * t, np.float64(iy) * t, np.float64(ix + 1) * t, np.float64(iy + 1) * t


def cut(cloud, tile_size, leaf):
    """(tiles in ascending key order, number of non-finite points dropped) of one list's cloud (n, 4)."""
    cloud = np.asarray(cloud, F).reshape(-1, 4)
    finite = np.isfinite(cloud[:, :3]).all(axis=1)
    pts = cloud[finite]
    fx, fy = tile_index(pts[:, 0], tile_size), tile_index(pts[:, 1], tile_size)
    if ((np.abs(fx) >= LIMIT) | (np.abs(fy) >= LIMIT)).any():
        raise OutOfRange("a point lies 32768 tiles or more from the origin")
    ix, iy = fx.astype(np.int32), fy.astype(np.int32)
    keys = tile_key(ix, iy)
    tiles = []
    for k in np.unique(keys):             # ascending
        member = np.nonzero(keys == k)[0]   # ascending: the input order
        i, j = int(ix[member[0]]), int(iy[member[0]])
        p = pts[member]
        stored = ((GR.voxel_grid_pinned(p, leaf) if leaf > 0 else p) + F(0.0)).astype(F)
        x0, y0, x1, y1 = tile_box_xy(i, j, tile_size)
        box = np.array([x0, y0, np.float64(stored[:, 2].min()), x1, y1, np.float64(stored[:, 2].max())], np.float64)
        tiles.append(Tile(i, j, box, stored))
    return tiles, int((~finite).sum())


def build(poses, corner, surf, tile_size, leaf_corner, leaf_surf, first=0, n=None):
    """pcm_loam_tiles_build over key frames [first, first + n): ((corner tiles, surf tiles), non-finite points of both lists)."""
    tc, bad_c = cut(GR.export(poses, corner, surf, 0, first, n), tile_size, leaf_corner)
    ts, bad_s = cut(GR.export(poses, corner, surf, 1, first, n), tile_size, leaf_surf)
    return (tc, ts), bad_c + bad_s
