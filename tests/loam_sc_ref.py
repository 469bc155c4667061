"""numpy restatement of jueying_slam's Scan Context (src/Scancontext.cpp, include/Scancontext.h; ring-key metric of
include/nanoflann.hpp:274-298) and of detectLoopClosureDistance (mapOptmization.cpp:843-880), written from the reference line by
line with the rules DESIGN.md section 12 pins: double sums in index order for means, norms and dot products; a NaN angle is
sector 1; ring-key candidates in ascending (d2, index); candidates folded with strict <.  It never imports the library.

A descriptor here is a (num_ring, num_sector) float64 array whose entries are float32 values, as the reference's MatrixXd."""
import dataclasses
import math

import numpy as np

F = np.float32
LARGE = 10000000.0


@dataclasses.dataclass
class Params:
    lidar_height: float = 0.3      # Scancontext.h:80
    num_ring: int = 20             # :82
    num_sector: int = 60           # :83
    max_radius: float = 80.0       # :84
    num_exclude_recent: int = 30   # :89
    num_candidates: int = 3        # :90; 0 = every entry of the search set (the library's extension)
    search_ratio: float = 0.1      # :93
    dist_threshold: float = 0.3    # :95
    tree_making_period: int = 10   # :99


def xy2theta(x, y):
    """:23-36 on float32 arrays: float quotient, double atan, double degrees, one rounding to float."""
    x = np.asarray(x, F); y = np.asarray(y, F)
    k = 180.0 / math.pi
    out = np.zeros(x.shape, F)
    with np.errstate(all="ignore"):
        b1 = (x >= 0) & (y >= 0)
        b2 = (x < 0) & (y >= 0)
        b3 = (x < 0) & (y < 0)
        b4 = (x >= 0) & (y < 0)
        out[b1] = (k * np.arctan((y[b1] / x[b1]).astype(np.float64))).astype(F)
        out[b2] = (180.0 - k * np.arctan((y[b2] / (-x[b2])).astype(np.float64))).astype(F)
        out[b3] = (180.0 + k * np.arctan((y[b3] / x[b3]).astype(np.float64))).astype(F)
        out[b4] = (360.0 - k * np.arctan(((-y[b4]) / x[b4]).astype(np.float64))).astype(F)
    return out


def point_bins(pts, P: Params):
    """Per point of makeScancontext (:166-179): keep (bool), ring, sector (0-based int32), z' (float32); unkept entries are 0."""
    pts = np.asarray(pts, F)
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    fin = np.isfinite(x) & np.isfinite(y) & np.isfinite(z)
    with np.errstate(all="ignore"):
        zp = (z.astype(np.float64) + P.lidar_height).astype(F)
        rng = np.sqrt(x * x + y * y)
        ang = xy2theta(x, y)
        keep = fin & ~(rng.astype(np.float64) > P.max_radius)
        fr = np.ceil((rng.astype(np.float64) / P.max_radius) * P.num_ring)
        fs = np.ceil((ang.astype(np.float64) / 360.0) * P.num_sector)
    fr = np.where(keep, fr, 1.0)
    fs = np.where(keep & ~np.isnan(fs), fs, 1.0)   # NaN angle: int(NaN) is INT_MIN on x86-64, clamped to 1
    ring = np.clip(fr, 1, P.num_ring).astype(np.int32) - 1
    sector = np.clip(fs, 1, P.num_sector).astype(np.int32) - 1
    return keep, np.where(keep, ring, 0).astype(np.int32), np.where(keep, sector, 0).astype(np.int32), np.where(keep, zp, F(0)).astype(F)


def make_scancontext(pts, P: Params):
    keep, ring, sector, zp = point_bins(pts, P)
    desc = np.full((P.num_ring, P.num_sector), F(-1000.0), F)
    np.maximum.at(desc, (ring[keep], sector[keep]), zp[keep])   # desc < z ? desc = z, from NO_POINT
    desc[desc == F(-1000.0)] = F(0)
    desc[desc == F(0)] = F(0)   # one zero for both signs
    return desc.astype(np.float64)


def ring_key(desc):
    """Row means (in-order double sums), rounded to float as eig2stdvec does."""
    R, S = desc.shape
    acc = np.zeros(R)
    for s in range(S):
        acc = acc + desc[:, s]
    return (acc / float(S)).astype(F)


def sector_key(desc):
    R, S = desc.shape
    acc = np.zeros(S)
    for r in range(R):
        acc = acc + desc[r, :]
    return acc / float(R)


def col_norms(desc):
    R, S = desc.shape
    acc = np.zeros(S)
    for r in range(R):
        acc = acc + desc[r, :] * desc[r, :]
    return np.sqrt(acc)


def ring_d2(query, keys):
    """nanoflann L2_Adaptor<float>::evalMetric of `query` (R,) against every row of keys (K,R): float32 (K,)."""
    q = np.asarray(query, F); k = np.asarray(keys, F).reshape(-1, q.shape[0])
    R = q.shape[0]
    res = np.zeros(k.shape[0], F)
    d = 0
    while d + 3 < R:
        d0 = q[d] - k[:, d]; d1 = q[d + 1] - k[:, d + 1]; d2 = q[d + 2] - k[:, d + 2]; d3 = q[d + 3] - k[:, d + 3]
        res = res + (((d0 * d0 + d1 * d1) + d2 * d2) + d3 * d3)
        d += 4
    while d < R:
        d0 = q[d] - k[:, d]
        res = res + d0 * d0
        d += 1
    return res.astype(F)


def fast_align(v1, v2):
    """fastAlignUsingVkey (:93-113)."""
    S = v1.shape[0]
    j = np.arange(S)
    acc = np.zeros(S)   # one entry per shift
    for col in range(S):
        dcol = v1[col] - v2[(col - j) % S]   # circshift by shift j: column col comes from col - j
        acc = acc + dcol * dcol
    norms = np.sqrt(acc)
    arg, best = 0, LARGE
    for sh in range(S):
        if norms[sh] < best:
            arg, best = sh, norms[sh]
    return arg


def dist_direct(d1, n1, d2, n2, shift):
    """distDirectSC(_sc1, circshift(_sc2, shift)) (:69-90)."""
    R, S = d1.shape
    c = (np.arange(S) - shift) % S
    d2s, n2s = d2[:, c], n2[c]
    dot = np.zeros(S)
    for r in range(R):
        dot = dot + d1[r, :] * d2s[r, :]
    with np.errstate(all="ignore"):
        sim = dot / (n1 * n2s)
    skip = (n1 == 0) | (n2s == 0)
    total, eff = 0.0, 0
    for col in range(S):
        if skip[col]:
            continue
        total = total + float(sim[col])
        eff += 1
    if eff == 0:
        return float("nan")
    return 1.0 - total / eff


def c_round(v):
    return int(math.floor(abs(v) + 0.5)) * (1 if v >= 0 else -1)


def distance(d1, d2, search_ratio=0.1):
    """distanceBtnScanContext (:116-148) -> (distance, shift)."""
    S = d1.shape[1]
    arg = fast_align(sector_key(d1), sector_key(d2))
    radius = c_round(0.5 * search_ratio * S)
    space = [arg]
    for ii in range(1, radius + 1):
        space.append((arg + ii + S) % S)
        space.append((arg - ii + S) % S)
    space.sort()
    n1, n2 = col_norms(d1), col_norms(d2)
    best_shift, best = 0, LARGE
    for sh in space:
        cur = dist_direct(d1, n1, d2, n2, sh)
        if cur < best:
            best_shift, best = sh, cur
    return best, best_shift


def yaw(nn_align, S):
    deg = F(nn_align * (360.0 / S))
    return F(float(deg) * math.pi / 180.0)


class Manager:
    """SCManager: descriptors, ring keys, the stale tree and detectLoopClosureID (:253-344)."""

    def __init__(self, P: Params):
        self.P = P
        self.descs, self.rkeys = [], []
        self.counter = 0
        self.tree = None   # ring keys of the search set (a copy, as polarcontext_invkeys_to_search_)

    def add(self, desc):
        self.descs.append(np.asarray(desc, np.float64))
        self.rkeys.append(ring_key(self.descs[-1]))

    def add_cloud(self, pts):
        self.add(make_scancontext(pts, self.P))

    def detect(self):
        P = self.P
        out = {"loop_id": -1, "yaw": F(0.0), "early": True}
        if len(self.rkeys) < P.num_exclude_recent + 1:
            return out
        rebuilt = False
        if self.counter % P.tree_making_period == 0:
            self.tree = np.array(self.rkeys[:len(self.rkeys) - P.num_exclude_recent], F)
            rebuilt = True
        self.counter += 1
        T = self.tree.shape[0]
        d2 = ring_d2(self.rkeys[-1], self.tree)
        if P.num_candidates == 0:
            cand = list(range(T))
        else:
            cand = sorted(range(T), key=lambda i: (d2[i], i))[:P.num_candidates]
        min_dist, nn_align, nn_idx = LARGE, 0, 0
        rows = []
        for ci in cand:
            dist, align = distance(self.descs[-1], self.descs[ci], P.search_ratio)
            rows.append((ci, d2[ci], dist, align))
            if dist < min_dist:
                min_dist, nn_align, nn_idx = dist, align, ci
        return {"loop_id": nn_idx if min_dist < P.dist_threshold else -1, "yaw": yaw(nn_align, P.num_sector), "early": False, "min_dist": min_dist,
                "nn_idx": nn_idx, "nn_align": nn_align, "tree_size": T, "tree_rebuilt": rebuilt, "candidates": rows}


def loop_distance(poses, times, radius, time_diff, time_cur):
    """detectLoopClosureDistance without the loopIndexContainer test: key frame, or -1."""
    poses = np.asarray(poses, F)
    K = poses.shape[0]
    if K == 0:
        return -1
    cur = K - 1
    dx = poses[:, 3] - poses[cur, 3]; dy = poses[:, 4] - poses[cur, 4]; dz = F(1.1) - np.full(K, F(1.1), F)
    d2 = (dx * dx + dy * dy) + dz * dz
    r2 = F(radius) * F(radius)
    near = sorted((i for i in range(K) if d2[i] < r2), key=lambda i: (d2[i], i))
    for i in near:
        if abs(float(times[i]) - time_cur) > time_diff and cur - i > 10:
            return i
    return -1
