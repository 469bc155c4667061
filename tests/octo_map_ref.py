"""CPU restatement of the 3D occupancy map for the tests: octomap_server's insertCloudCallback / insertScan / publishAll projection
(src/tool/octomap_server/src/OctomapServer.cpp) and map_saver's files, with the rules of the octomap library underneath as DESIGN.md
section 38 declares them, in plain Python / numpy float32 + float64 with dictionaries and sets.  Imports neither the product nor
the oracle and shares no code with csrc/octo_map.h."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

F = np.float32
DBL_MAX = 1.7976931348623157e308
FLT_MAX = 3.4028234663852886e38
KEY0 = 32768
OK, REJECTED, BOUND = 0, 1, 2
SKIP_MIN_RANGE, END_NONE, END_OCCUPIED, END_FREE = 0, 1, 2, 3


@dataclasses.dataclass
class Params:
    resolution: float = 0.05
    prob_hit: float = 0.7
    prob_miss: float = 0.4
    clamp_min: float = 0.12
    clamp_max: float = 0.97
    max_range: float = -1.0
    min_range: float = -1.0
    pointcloud_min_x: float = -DBL_MAX
    pointcloud_max_x: float = DBL_MAX
    pointcloud_min_y: float = -DBL_MAX
    pointcloud_max_y: float = DBL_MAX
    pointcloud_min_z: float = -DBL_MAX
    pointcloud_max_z: float = DBL_MAX
    occupancy_min_z: float = -DBL_MAX
    occupancy_max_z: float = DBL_MAX
    min_x_size: float = 0.0
    min_y_size: float = 0.0
    filter_speckles: int = 0


def logodds(p: float):
    return F(math.log(p / (1 - p)))


def limit(v: float):
    """A PassThrough limit: the double rounded once to float, an infinity beyond FLT_MAX."""
    if v > FLT_MAX:
        return F(np.inf)
    if v < -FLT_MAX:
        return F(-np.inf)
    return F(v)


def key_d(c: float, res: float):
    """Key of a double coordinate, or None when it is not in [0, 65536)."""
    q = c / res
    if not math.isfinite(q):
        return None
    f = math.floor(q)
    if not (-32768 <= f < 32768):
        return None
    return int(f) + KEY0


def key(c, res):
    return key_d(float(F(c)), res)


def key3(p, res):
    k = tuple(key(p[a], res) for a in range(3))
    return None if None in k else k


def coord(k: int, res: float) -> float:
    return ((k - KEY0) + 0.5) * res


def pack(k) -> int:
    return (k[0] << 32) | (k[1] << 16) | k[2]


def norm(dx, dy, dz):
    with np.errstate(all="ignore"):
        s = F(F(F(dx) * F(dx)) + F(F(dy) * F(dy))) + F(F(dz) * F(dz))
        return F(math.sqrt(float(s))) if not math.isnan(float(s)) else F(np.nan)


def truncate(o, p, n, max_range):
    with np.errstate(all="ignore"):
        return np.array([F(o[a]) + F(F(F(p[a]) - F(o[a])) / F(n)) * F(max_range) for a in range(3)], F)


def point_rule(o, p, ground, max_range, min_range):
    """insertScan :373-439 for one point -> (rule, ray end, truncated)."""
    o, p = np.asarray(o, F), np.asarray(p, F)
    with np.errstate(all="ignore"):
        n = norm(p[0] - o[0], p[1] - o[1], p[2] - o[2])
    if min_range > 0 and float(n) < min_range:
        return SKIP_MIN_RANGE, p.copy(), False
    if ground:
        if max_range > 0.0 and float(n) > max_range:
            return END_NONE, truncate(o, p, n, max_range), True
        return END_NONE, p.copy(), False
    if max_range < 0.0 or float(n) <= max_range:
        return END_OCCUPIED, p.copy(), False
    return END_FREE, truncate(o, p, n, max_range), True


def walk(o, e, res):
    """computeRayKeys -> (status, keys, steps): the origin's key and every key up to, not including, the end's."""
    o, e = np.asarray(o, F), np.asarray(e, F)
    ko, ke = key3(o, res), key3(e, res)
    if ko is None or ke is None:
        return REJECTED, [], 0
    if ko == ke:
        return OK, [], 0
    keys = [ko]
    with np.errstate(all="ignore"):
        d = [F(e[a] - o[a]) for a in range(3)]
        n = norm(d[0], d[1], d[2])
        direction = [F(d[a] / n) for a in range(3)]
    step, tmax, tdelta = [0, 0, 0], [DBL_MAX] * 3, [DBL_MAX] * 3
    bound = 3
    for a in range(3):
        dr = float(direction[a])
        step[a] = 1 if dr > 0.0 else -1 if dr < 0.0 else 0
        if step[a]:
            with np.errstate(all="ignore"):
                tmax[a] = float(np.float64(coord(ko[a], res) + step[a] * 0.5 * res - float(o[a])) / np.float64(dr))
                tdelta[a] = float(np.float64(res) / np.float64(abs(dr)))
        bound += abs(ke[a] - ko[a])
    k = list(ko)
    length = float(n)
    steps = 0
    while True:
        if steps == bound:
            return BOUND, [], steps
        steps += 1
        if tmax[0] < tmax[1]:
            dim = 0 if tmax[0] < tmax[2] else 2
        else:
            dim = 1 if tmax[1] < tmax[2] else 2
        k[dim] += step[dim]
        tmax[dim] += tdelta[dim]
        if k[dim] < 0 or k[dim] >= 65536:
            return REJECTED, [], steps
        if tuple(k) == ke:
            break
        if min(tmax) > length:     # also false for a NaN length
            break
        keys.append(tuple(k))
    return OK, keys, steps


def transform(T, p):
    """Row-major 4x4 float matrix on a float point, the sum left to right."""
    T, p = np.asarray(T, F).reshape(4, 4), np.asarray(p, F)
    with np.errstate(all="ignore"):
        return np.array([F(F(F(T[a, 0] * p[0]) + F(T[a, 1] * p[1])) + F(T[a, 2] * p[2])) + T[a, 3] for a in range(3)], F)


def update(v, d, lo, hi):
    v = F(F(v) + F(d))
    if v < lo:
        v = lo
    if v > hi:
        v = hi
    return F(v)


def pgm_byte(v: int) -> int:
    if 0 <= v <= 25:
        return 254
    if v >= 65:
        return 0
    return 205


@dataclasses.dataclass
class Geometry:
    min_key: tuple
    width: int
    height: int
    origin_x: float
    origin_y: float
    metric_min: tuple
    metric_max: tuple


def geometry(kmin, kmax, res, min_x_size=0.0, min_y_size=0.0):
    """handlePreNodeTraversal :951-999 at full depth, in double; None where a padded key cannot be made (:973-980)."""
    mn = [coord(kmin[a], res) - res / 2.0 for a in range(3)]
    mx = [coord(kmax[a], res) + res / 2.0 for a in range(3)]
    metric_min, metric_max = tuple(mn), tuple(mx)
    hx, hy = 0.5 * min_x_size, 0.5 * min_y_size
    mn[0], mx[0] = min(mn[0], -hx), max(mx[0], hx)
    mn[1], mx[1] = min(mn[1], -hy), max(mx[1], hy)
    lo = [key_d(mn[a], res) for a in range(3)]
    hi = [key_d(mx[a], res) for a in range(3)]
    if None in lo or None in hi:
        return None
    return Geometry((lo[0], lo[1]), hi[0] - lo[0] + 1, hi[1] - lo[1] + 1, coord(lo[0], res) - res * 0.5, coord(lo[1], res) - res * 0.5,
                    metric_min, metric_max)


class Map:
    """The map as dictionaries: cells[key triple] = float32 log-odds."""

    def __init__(self, P: Params):
        self.P = P
        self.cells = {}
        self.hit, self.miss = logodds(P.prob_hit), logodds(P.prob_miss)
        self.lo, self.hi = logodds(P.clamp_min), logodds(P.clamp_max)
        self.win_lo = [limit(P.pointcloud_min_x), limit(P.pointcloud_min_y), limit(P.pointcloud_min_z)]
        self.win_hi = [limit(P.pointcloud_max_x), limit(P.pointcloud_max_y), limit(P.pointcloud_max_z)]

    def insert_scan(self, nonground=None, origin=(0.0, 0.0, 0.0), ground=None, sensor_to_world=None) -> dict:
        P, res = self.P, self.P.resolution
        o = np.asarray(origin, F).reshape(3)
        r = dict(points_in=0, dropped_nonfinite=0, skipped_window=0, skipped_min_range=0, truncated=0, rejected_rays=0, cells_touched=0, new_cells=0)
        free, occ = set(), set()
        for is_ground, cloud in ((True, ground), (False, nonground)):
            if cloud is None:
                continue
            for p in np.asarray(cloud, F).reshape(-1, np.asarray(cloud).shape[-1])[:, :3]:
                r["points_in"] += 1
                q = transform(sensor_to_world, p) if sensor_to_world is not None else p
                if not np.all(np.isfinite(q)):
                    r["dropped_nonfinite"] += 1
                    continue
                if not all(self.win_lo[a] <= q[a] <= self.win_hi[a] for a in range(3)):
                    r["skipped_window"] += 1
                    continue
                rule, e, truncated = point_rule(o, q, is_ground, P.max_range, P.min_range)
                if rule == SKIP_MIN_RANGE:
                    r["skipped_min_range"] += 1
                    continue
                r["truncated"] += int(truncated)
                status, keys, _ = walk(o, e, res)
                if status != OK:
                    r["rejected_rays"] += 1
                else:
                    free.update(keys)
                ke = key3(e, res)
                if rule == END_OCCUPIED and ke is not None:
                    occ.add(ke)
                elif rule == END_FREE and status == OK and ke is not None:
                    free.add(ke)
        for k in free - occ:
            r["new_cells"] += int(k not in self.cells)
            self.cells[k] = update(self.cells.get(k, F(0.0)), self.miss, self.lo, self.hi)
        for k in occ:
            r["new_cells"] += int(k not in self.cells)
            self.cells[k] = update(self.cells.get(k, F(0.0)), self.hit, self.lo, self.hi)
        r["cells_touched"] = len(free | occ)
        self.last_free, self.last_occ = free, occ
        return r

    # ---- outputs ----
    def sorted_cells(self):
        ks = sorted(self.cells, key=pack)
        return np.array(ks, np.int32).reshape(-1, 3), np.array([self.cells[k] for k in ks], F)

    def counts(self):
        occ = sum(1 for v in self.cells.values() if v >= F(0.0))
        return len(self.cells), occ, len(self.cells) - occ

    def key_box(self):
        ks = np.array(list(self.cells), np.int64).reshape(-1, 3)
        return tuple(int(v) for v in ks.min(axis=0)), tuple(int(v) for v in ks.max(axis=0))

    def in_z(self, kz: int) -> bool:
        z, half = coord(kz, self.P.resolution), self.P.resolution / 2.0
        return z + half > self.P.occupancy_min_z and z - half < self.P.occupancy_max_z

    def is_speckle(self, k) -> bool:
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    if (dx, dy, dz) != (0, 0, 0) and self.cells.get((k[0] + dx, k[1] + dy, k[2] + dz), F(-1.0)) >= F(0.0):
                        return False
        return True

    def published_occupied(self, k) -> bool:
        return self.cells[k] >= F(0.0) and self.in_z(k[2]) and not (self.P.filter_speckles and self.is_speckle(k))

    def occupied_points(self):
        res = self.P.resolution
        ks = [k for k in sorted(self.cells, key=pack) if self.published_occupied(k)]
        return np.array([[F(coord(k[0], res)), F(coord(k[1], res)), F(coord(k[2], res)), self.cells[k]] for k in ks], F).reshape(-1, 4)

    def project(self):
        """-> (Geometry, (height, width) int8 grid), or None where nothing is produced."""
        if len(self.cells) <= 1:
            return None
        kmin, kmax = self.key_box()
        G = geometry(kmin, kmax, self.P.resolution, self.P.min_x_size, self.P.min_y_size)
        if G is None:
            return None
        grid = np.full((G.height, G.width), -1, np.int8)
        for k in self.cells:
            if self.published_occupied(k):
                grid[k[1] - G.min_key[1], k[0] - G.min_key[0]] = 100
        for k, v in self.cells.items():
            if v < F(0.0) and self.in_z(k[2]) and grid[k[1] - G.min_key[1], k[0] - G.min_key[0]] == -1:
                grid[k[1] - G.min_key[1], k[0] - G.min_key[0]] = 0
        return G, grid


def pgm_body(grid) -> bytes:
    """map_saver.cpp:74-85: rows top-down."""
    h, w = grid.shape
    return bytes(pgm_byte(int(grid[h - y - 1, x])) for y in range(h) for x in range(w))


def map_files(prefix: str, G: Geometry, grid, res: float):
    """map_saver.cpp:72-73, :115 -> (pgm bytes, yaml bytes)."""
    pgm = ("P5\n# CREATOR: map_saver.cpp %.3f m/pix\n%d %d\n255\n" % (res, G.width, G.height)).encode() + pgm_body(grid)
    yaml = ("image: %s\nresolution: %f\norigin: [%f, %f, 0.00]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n\n"
            % (prefix + ".pgm", res, G.origin_x, G.origin_y)).encode()
    return pgm, yaml
