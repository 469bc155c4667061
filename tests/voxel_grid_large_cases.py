"""Inputs shared by tests/test_voxel_grid_large.py and tests/test_gpu_voxel_grid_large.py, and their references (computed once).

Dyadic clouds: every coordinate and every extra field is a multiple of 2^-8 with |v| < 2^20, so a double sum of a few thousand
of them is exact in any order and the device has to give the restatement's bits."""
import numpy as np

import voxel_grid_large_ref as VL

F = np.float32
LEAF = 0.05
_CACHE = {}


def dyadic_site(n, width=4, seed=0, origin=(0.0, 0.0, 0.0), extent=(3000.0, 3000.0, 100.0)):
    """n points over ``extent`` from ``origin``: n / 4 places (rounded up), up to four points within 0.03 m of each, shuffled"""
    rng = np.random.default_rng(seed)
    places = (n + 3) // 4
    base = np.stack([rng.integers(0, int(e * 256) - 8, places) for e in extent], axis=1)
    xyz = (np.repeat(base, 4, axis=0)[:n] + rng.integers(0, 8, (n, 3))) / 256.0 + np.asarray(origin)
    pts = np.zeros((n, width), F)
    pts[:, :3] = xyz
    if width > 3:
        pts[:, 3:] = rng.integers(-65536, 65536, (n, width - 3)) / 256.0
    assert (pts[:, :3].astype(np.float64) == xyz).all() and np.abs(pts).max() < 2 ** 20
    return pts[rng.permutation(n)]


def dyadic_cases():
    """name -> (points, leaf): all overflow the leaf index at 0.05 m"""
    if "dyadic" not in _CACHE:
        c = {"site_4096": (dyadic_site(4096), LEAF),
             "xyz_only": (dyadic_site(1500, width=3, seed=1), LEAF),
             "sixteen_floats": (dyadic_site(1500, width=16, seed=2), LEAF),
             "negative_octant": (dyadic_site(2048, seed=3, origin=(-3500.0, -3200.0, -150.0)), LEAF)}
        for n in (1, 63, 64, 65, 257):
            c["n_%d" % n] = (dyadic_site(n, seed=10 + n), LEAF)
        holes = dyadic_site(2000, seed=4)
        holes[::7, 0] = np.nan
        holes[3::11, 1] = np.inf
        holes[5::13, 2] = -np.inf
        c["non_finite"] = (holes, LEAF)
        c["many_pieces"] = (dyadic_site(12000, seed=6), 0.002)       # thousands of pieces: the piece tables grow
        c["only_non_finite"] = (np.full((300, 4), np.nan, F), LEAF)
        _CACHE["dyadic"] = c
    return _CACHE["dyadic"]


def reference(name):
    """(cells, pieces, depth) of the restatement for a dyadic case"""
    key = ("ref", name)
    if key not in _CACHE:
        pts, leaf = dyadic_cases()[name]
        stats = {}
        cells = VL.apply_filter(pts, leaf, stats=stats)
        cells.setflags(write=False)
        _CACHE[key] = (cells, stats["pieces"], stats["depth"])
    return _CACHE[key]


def straddle():
    """x is strictly the longest axis: x in [0, 120000] at leaf 0.05 is 2.4e6 leaves, y and z 1000 each -- 2.4e12 leaves.  mid =
    60000; the lattice cell [60000.0, 60000.05) holds one point on the cut plane (v <= mid: first piece) and one 1/64 m beyond it
    (second piece).  Two corner points give the box.  Returns (points, leaf, the two centroids of that cell in piece order)."""
    pts = np.array([[0.0, 0.0, 0.0, 1.0],
                    [60000.015625, 25.0, 25.0, 2.0],
                    [120000.0, 49.96875, 49.96875, 3.0],
                    [60000.0, 25.0, 25.0, 4.0]], F)
    return pts, LEAF, pts[3].copy(), pts[1].copy()


def tie_cloud(flat_z):
    """dx == dy > dz: 3000 x 3000 m, z over 100 m (cut along z, the reference's tie rule) or flat (z cannot be cut)"""
    pts = dyadic_site(1024, seed=5, extent=(3000.0, 3000.0, 100.0))
    pts[0, :3] = (0.0, 0.0, 0.0)
    pts[1, :3] = (2999.96875, 2999.96875, 99.96875)
    if flat_z:
        pts[:, 2] = 7.0
    return pts, LEAF


def general_float():
    """random float32 coordinates (not dyadic) that overflow: the VoxelGrid rule's case"""
    if "general" not in _CACHE:
        rng = np.random.default_rng(77)
        places = rng.uniform((-1500.0, -1500.0, -20.0), (1500.0, 1500.0, 80.0), (1200, 3))
        xyz = np.repeat(places, 4, axis=0) + rng.uniform(0.0, 0.12, (4800, 3))
        pts = np.concatenate([xyz, rng.uniform(0.0, 255.0, (4800, 1))], axis=1).astype(F)
        _CACHE["general"] = (pts[rng.permutation(len(pts))], 0.1)
    return _CACHE["general"]


def close_ulp_share(a, b):
    """The VoxelGrid rule (DESIGN sections 10 and 21): no value differs by more than 1 ulp, at least 99.99 % are equal."""
    assert a.shape == b.shape, (a.shape, b.shape)
    ulp = np.spacing(np.maximum(np.abs(a), 1e-3).astype(F))
    share = float((a == b).mean()) if a.size else 1.0
    print("max |a - b| / ulp = %g, equal share = %.6f" % (float((np.abs(a - b) / ulp).max()) if a.size else 0.0, share))
    assert (np.abs(a - b) <= ulp).all() and share >= 0.9999
