"""Literal numpy / python restatement of jueying_slam's 2D occupancy mapping tool (src/tool/occupancy_mapping): getScan,
processScan, TraceLine, ConvertWorld2GridIndex, updateGrid (as a dict of doubles added to in the reference's visit order instead
of the quadtree, whose shape does not reach the values), getGridMap's crop and values, saveMap's bytes.  Plus the rule the device
uses: a cell's value from its two integer counters."""
from __future__ import annotations

import dataclasses
import math

import numpy as np

F = np.float32
PI7 = 3.1415927   # the tool's own constant


@dataclasses.dataclass
class Params:   # config/rslidar.yaml, config/livox.yaml
    min_z: float = -0.15
    max_z: float = 1.5
    angle_increment: float = 0.006
    min_range: float = 0.5
    max_range: float = 200.0
    log_occ: float = 0.1
    log_free: float = -0.01
    resolution: float = 0.1
    max_radius: float = 20.0
    fill_with_white: bool = True
    use_nan: bool = False


def beam_size(P: Params) -> int:
    return int(math.ceil((PI7 - (-PI7)) / P.angle_increment))


def point_beams(cloud, P: Params):
    """Per point of getScan: (contributes, beam index, float range, float angle).  A non-finite point is skipped (pinned)."""
    x, y, z = (np.asarray(cloud[:, k], F) for k in range(3))
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(invalid="ignore", over="ignore"):
        rng = np.hypot(x, y)               # float overload
        ang = np.arctan2(y, x)             # float overload
        assert rng.dtype == F and ang.dtype == F
        idx = np.where(fin, (ang.astype(np.float64) - (-PI7)) / P.angle_increment, 0.0).astype(np.int64)   # (int): truncation, the value is >= 0
    zz = z.astype(np.float64)
    rr = rng.astype(np.float64)
    ok = fin & (zz >= P.min_z) & (zz <= P.max_z) & (idx >= 0) & (idx < beam_size(P)) & (rr >= P.min_range) & (rr <= P.max_range)
    return ok, idx, rng, ang


def get_scan(cloud, P: Params):
    """(ranges float32 with NaN for empty beams, angles float64)."""
    B = beam_size(P)
    ranges = np.full(B, F(P.max_range + 1), F)
    ok, idx, rng, _ = point_beams(cloud, P)
    np.minimum.at(ranges, idx[ok], rng[ok])   # if (range < ranges[index]) ranges[index] = range, over the points
    r64 = ranges.astype(np.float64)
    ranges[(r64 > P.max_range) | (r64 < P.min_range)] = np.nan
    i = np.arange(B, dtype=np.float64)
    angles = P.angle_increment * i + P.angle_increment / 2 - math.pi
    return ranges, angles


def world2grid(v: float, P: Params) -> int:
    return int(v / P.resolution)   # int(): towards zero


def trace_line(x0: int, y0: int, x1: int, y1: int):
    """TraceLine: the cells from (x0, y0) towards (x1, y1), the end cell left out."""
    x_end, y_end = x1, y1
    with np.errstate(divide="ignore", invalid="ignore"):
        steep = bool(np.abs((np.float64(y1) * 1.0 - np.float64(y0) * 1.0) / (np.float64(x1) * 1.0 - np.float64(x0) * 1.0)) >= 1)
    if steep:
        x0, y0 = y0, x0
        x1, y1 = y1, x1
    if x0 > x1:
        x0, x1 = x1, x0
        y0, y1 = y1, y0
    delta_x = x1 - x0
    delta_y = abs(y1 - y0)
    error = 0
    y = y0
    ystep = 1 if y0 < y1 else -1
    out = []
    for x in range(x0, x1 + 1):
        if steep:
            px, py = y, x
        else:
            px, py = x, y
        error += delta_y
        if 2 * error >= delta_x:
            y += ystep
            error -= delta_x
        if px == x_end and py == y_end:
            continue
        out.append((px, py))
    return out


def beam_end(rng: float, angle: float, pose, P: Params):
    """processScan for one beam: None when skipped, else (dist, occ cell, hit, trace)."""
    dist = float(rng)
    if math.isinf(dist) or math.isnan(dist):
        if math.isnan(dist) and P.use_nan:
            dist = P.max_radius + 0.1
        else:
            return None
    if dist > P.max_radius:
        dist = P.max_radius + 0.1
    theta = float(pose[2])
    laser_x = dist * math.cos(theta + angle)
    laser_y = dist * math.sin(theta + angle)
    world_x = laser_x + float(pose[3])
    world_y = laser_y + float(pose[4])
    occ = (world2grid(world_x, P), world2grid(world_y, P))
    return dist, occ, dist <= P.max_radius, (dist <= P.max_radius or P.fill_with_white), (world_x / P.resolution, world_y / P.resolution)


class Map:
    """The map of the tool without its quadtree: logit per touched cell in visit order, and the two counters per cell."""

    def __init__(self, P: Params):
        self.P = P
        self.logit = {}     # cell -> double, added to in visit order (updateGrid)
        self.n_occ = {}
        self.n_free = {}
        self.init_cell = None
        self.min_end_margin = 1.0   # smallest distance of an end point to a cell boundary, in cells (the GPU tests' precondition)

    def _update(self, cell, occ: bool):
        self.logit[cell] = self.logit.get(cell, 0.0) + (self.P.log_occ if occ else self.P.log_free)
        d = self.n_occ if occ else self.n_free
        d[cell] = d.get(cell, 0) + 1

    def insert(self, cloud, pose):
        P = self.P
        pose = [float(v) for v in np.asarray(pose, F)]
        robot = (world2grid(pose[3], P), world2grid(pose[4], P))
        if self.init_cell is None:   # initializeMap: a level-0 node with logit 0 from the start
            self.init_cell = robot
            self.logit.setdefault(robot, 0.0)
        ranges, angles = get_scan(cloud, P)
        for i in range(ranges.shape[0]):
            e = beam_end(ranges[i], float(angles[i]), pose, P)
            if e is None:
                continue
            dist, occ, hit, trace, frac = e
            for v in frac:
                self.min_end_margin = min(self.min_end_margin, abs(v - round(v)))
            if hit:
                self._update(occ, True)
            if trace:
                for cell in trace_line(robot[0], robot[1], occ[0], occ[1]):
                    if cell == occ:
                        continue
                    self._update(cell, False)
        return ranges, angles

    # ---- getGridMap ----
    def bounds(self):
        xs = [c[0] for c in self.logit]
        ys = [c[1] for c in self.logit]
        return min(xs), max(xs), min(ys), max(ys)

    def counts(self):
        """(n_occ, n_free) uint32 arrays over the crop, row-major [j, i]."""
        x0, x1, y0, y1 = self.bounds()
        a = np.zeros((y1 - y0 + 1, x1 - x0 + 1), np.uint32)
        b = np.zeros_like(a)
        for (x, y), n in self.n_occ.items():
            a[y - y0, x - x0] = n
        for (x, y), n in self.n_free.items():
            b[y - y0, x - x0] = n
        return a, b

    def grid(self, rule: str = "counts"):
        """int8 [height, width]: -1 unknown, else 100 / 0.  rule 'literal': the visit-order sum; 'counts': the count rule."""
        x0, x1, y0, y1 = self.bounds()
        g = np.full((y1 - y0 + 1, x1 - x0 + 1), -1, np.int8)
        for (x, y), l in self.logit.items():
            if rule == "counts":
                l = logit_from_counts(self.n_occ.get((x, y), 0), self.n_free.get((x, y), 0), self.P)
            g[y - y0, x - x0] = value_literal(l)
        return g

    def info(self):
        """width, height, origin_x, origin_y (first cell index * resolution: one product)."""
        x0, x1, y0, y1 = self.bounds()
        return x1 - x0 + 1, y1 - y0 + 1, float(x0) * self.P.resolution, float(y0) * self.P.resolution


def value_literal(logit: float) -> int:
    """getGridMap's leaf: the literal expression."""
    prob = 1.0 / (1.0 + math.exp(-1.0 * logit))
    prob = prob * 100.0
    return int(100.1) if prob >= 50 else int(0.1)


def logit_from_counts(n_occ: int, n_free: int, P: Params) -> float:
    """The device's definition: two products, one add."""
    return float(n_occ) * P.log_occ + float(n_free) * P.log_free


def sum_error_bound(n_occ: int, n_free: int, P: Params) -> float:
    """Bound on |visit-order sum - exact sum| of n = n_occ + n_free terms (and, with one more rounding each, of the count rule)."""
    n = n_occ + n_free
    return max(n - 1, 0) * 2.0 ** -53 * (n_occ * abs(P.log_occ) + n_free * abs(P.log_free))


def pgm_bytes(grid) -> bytes:
    """saveMap's body: rows top-down."""
    h, w = grid.shape
    out = bytearray()
    for y in range(h):
        row = grid[h - y - 1]
        for x in range(w):
            v = int(row[x])
            if 0 <= v <= 25:
                out.append(254)
            elif v >= 65:
                out.append(0)
            else:
                out.append(205)
    return bytes(out)


def pgm_file(grid, resolution: float) -> bytes:
    h, w = grid.shape
    return ("P5\n# CREATOR: occupancy_mapping %.3f m/pix\n%d %d\n255\n" % (resolution, w, h)).encode() + pgm_bytes(grid)


def yaml_file(image_path: str, resolution: float, origin_x: float, origin_y: float) -> bytes:
    return ("image: %s\nresolution: %f\norigin: [%f, %f, 0.00]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n\n"
            % (image_path, resolution, origin_x, origin_y)).encode()
