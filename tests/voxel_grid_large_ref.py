"""pcl::VoxelGridLarge::applyFilter (jueying_slam/include/voxel_grid_large.cpp:23-255) restated in numpy, recursively as the
reference has it, with the rules DESIGN section 22 pins: the box over the finite points, the extents as the float product
truncated plus one, their product in double, x where dx is strictly the largest, else y where dy is, else z, the cut at
mid = min + (max - min) / 2 in float32, first half min <= v <= mid, second half v > mid, both in input order, first half's cells
first.  A leaf piece is the plain VoxelGrid the tests already have (oracle.loader.voxel_downsample: double sums in input order).
An empty piece gives nothing; a cut with mid >= max, or one below MAX_DEPTH cuts, raises Stuck.

``independent`` states the same result without recursion: every point gets its depth-first path as a string of bits level by
level, then the cells are the groups of (path, lattice cell relative to the path's box), ordered by path, then by cell index."""
import numpy as np

F = np.float32
MAX_DEPTH = 64          # PCM_VOXEL_LARGE_MAX_DEPTH
LEAF, SPLIT, STUCK = 0, 1, 2


class Stuck(Exception):
    pass


def decide(mn, mx, leaf):
    """(kind, axis, mid) of a piece with the float32 box mn, mx: vg::split"""
    inv = F(1.0) / F(leaf)
    mn, mx = np.asarray(mn, F), np.asarray(mx, F)
    with np.errstate(over="ignore", invalid="ignore"):
        d = np.trunc(((mx - mn) * inv).astype(np.float64)) + 1.0
        if not (d[0] * d[1] * d[2] > 2147483647.0):
            return LEAF, -1, F(0)
        axis = 0 if (d[0] > d[1] and d[0] > d[2]) else 1 if (d[1] > d[0] and d[1] > d[2]) else 2
        mid = F(mn[axis] + F(F(mx[axis] - mn[axis]) / F(2)))
    return (SPLIT if mid < mx[axis] else STUCK), axis, mid


def apply_filter(points, leaf, depth=0, stats=None):
    """the cells of ``points`` (N, F) float32, in the reference's order; stats: {"pieces", "depth"} updated"""
    from oracle.loader import voxel_downsample
    points = np.ascontiguousarray(points, F)
    if stats is None:
        stats = {}
    stats.setdefault("pieces", 0)
    stats.setdefault("depth", 0)
    p = points[np.isfinite(points[:, :3]).all(axis=1)]
    if len(p) == 0:
        return np.zeros((0, points.shape[1]), F)
    mn, mx = p[:, :3].min(axis=0), p[:, :3].max(axis=0)
    kind, axis, mid = decide(mn, mx, leaf)
    if kind == LEAF:
        stats["pieces"] += 1
        stats["depth"] = max(stats["depth"], depth)
        return voxel_downsample(p, leaf)
    if kind == STUCK or depth >= MAX_DEPTH:
        raise Stuck("axis %d: [%r, %r], mid %r" % (axis, mn[axis], mx[axis], mid))
    v = p[:, axis]
    first = apply_filter(p[(v >= mn[axis]) & (v <= mid)], leaf, depth + 1, stats)
    second = apply_filter(p[v > mid], leaf, depth + 1, stats)
    return np.concatenate([first, second])


def independent(points, leaf):
    """The same cells without recursion and without the oracle: (cells, pieces, depth)."""
    points = np.ascontiguousarray(points, F)
    p = points[np.isfinite(points[:, :3]).all(axis=1)]
    width = points.shape[1]
    if len(p) == 0:
        return np.zeros((0, width), F), 0, 0
    inv = F(1.0) / F(leaf)
    path = np.array([""] * len(p), dtype=object)
    done = {}            # path -> (mn, mx) of a leaf piece
    depth = 0
    while True:
        cut = False
        for key in sorted(set(path) - set(done)):
            sel = path == key
            q = p[sel, :3]
            mn, mx = q.min(axis=0), q.max(axis=0)
            kind, axis, mid = decide(mn, mx, leaf)
            if kind == LEAF:
                done[key] = (mn, mx)
                continue
            if kind == STUCK or len(key) >= MAX_DEPTH:
                raise Stuck(key)
            path[sel] = np.where(q[:, axis] > mid, key + "1", key + "0")
            cut = True
        if not cut:
            break
        depth += 1
    out = []
    for key in sorted(done):        # "0" < "00" < "01" < "1": depth-first, first half first
        mn, mx = done[key]
        q = p[path == key]
        mb = np.floor(mn * inv).astype(np.int64)
        xb = np.floor(mx * inv).astype(np.int64)
        div = xb - mb + 1
        ijk = (np.floor(q[:, :3] * inv) - mb.astype(F)).astype(np.int64)
        idx = ijk[:, 0] + ijk[:, 1] * div[0] + ijk[:, 2] * div[0] * div[1]
        order = np.argsort(idx, kind="stable")
        _, first, count = np.unique(idx[order], return_index=True, return_counts=True)
        s = q[order].astype(np.float64)
        for b, n in zip(first, count):
            acc = np.zeros(width, np.float64)
            for row in s[b:b + n]:      # input order, one addition at a time, as the restatement sums
                acc += row
            out.append((acc / float(n)).astype(F))
    return np.array(out, F).reshape(-1, width), len(done), depth
