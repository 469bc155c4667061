"""pcl::ApproximateVoxelGrid as the per-point loop it is (the rules of include/pcm_amd.h), in Python: the
reference of tests/test_approx_voxel.py and tests/test_gpu_approx_voxel.py.  float32 arithmetic for x * inv; the history is a
dictionary of the 512 entries; every run keeps the input indices of its points, so a test can compare membership.  The cases the
two test files share are here as well."""
import numpy as np

F = np.float32
ENTRIES = 512


def keys(xyz, leaf):
    """-> (ijk (n,3) int64, h (n,) int64, valid (n,) bool); ijk and h of a dropped point are 0."""
    xyz = np.ascontiguousarray(xyz, F).reshape(-1, 3)
    inv = F(1.0) / F(leaf)
    with np.errstate(invalid="ignore", over="ignore"):
        f = np.floor(xyz * inv)                      # float32 product, then floorf
        valid = np.isfinite(xyz).all(axis=1) & (np.abs(f) < F(2.0 ** 31)).all(axis=1)
    ijk = np.where(valid[:, None], f, F(0)).astype(np.int64)
    # the low nine bits of the 32-bit wrapping sum are the low nine bits of the exact sum (two's complement)
    h = (ijk[:, 0] * 7171 + ijk[:, 1] * 3079 + ijk[:, 2] * 4231) & (ENTRIES - 1)
    return ijk, np.where(valid, h, 0), valid


def apply_filter(xyz, leaf):
    """The loop.  -> (runs, dropped): runs in output order, each the list of the input indices of its points."""
    ijk, h, valid = keys(xyz, leaf)
    history, runs, dropped = {}, [], 0
    for cp in range(len(valid)):
        if not valid[cp]:
            dropped += 1
            continue
        voxel, e = tuple(ijk[cp]), history.get(int(h[cp]))
        if e is not None and e[0] != voxel:          # flush
            runs.append(e[1])
            e = None
        if e is None:
            e = history[int(h[cp])] = (voxel, [])
        e[1].append(cp)
    for hh in sorted(history):                       # the final flush, in increasing h
        runs.append(history[hh][1])
    return runs, dropped


def means(records, runs):
    """float32(float64 mean) of every field of every run -> (len(runs), k) float32"""
    records = np.asarray(records, F)
    out = np.zeros((len(runs), records.shape[1]), F)
    for r, idx in enumerate(runs):
        out[r] = records[idx].astype(np.float64).sum(axis=0) / float(len(idx))
    return out


def slots(runs, n):
    """slot of every point (0xffffffff: dropped): what approx_voxel.h's emit_slots_host returns"""
    s = np.full(n, 0xffffffff, np.uint32)
    for r, idx in enumerate(runs):
        s[idx] = r
    return s


def distinct_voxels(xyz, leaf):
    ijk, _, valid = keys(xyz, leaf)
    return len(np.unique(ijk[valid], axis=0))


def ulp_apart(a, b):
    """distance in float32 steps (same-sign finite values; a zero of either sign is the same place)"""
    a, b = np.ascontiguousarray(a, F), np.ascontiguousarray(b, F)
    ia, ib = a.view(np.int32).astype(np.int64), b.view(np.int32).astype(np.int64)
    ia = np.where(ia < 0, -(ia & 0x7fffffff), ia)
    ib = np.where(ib < 0, -(ib & 0x7fffffff), ib)
    return np.abs(ia - ib)


def _centres(voxels):
    return (np.asarray(voxels, np.float64) + 0.5).astype(F)


def small_cases():
    """name -> (xyz (n,3) float32, leaf, expected runs or None).  3 ix + 7 iy + 135 iz = h (mod 512), and ix + 512 collides with ix."""
    c = {}
    # with leaf 1.0, x = 0.5, 512.5, 0.5 gives ix = 0 and ix = 512 in one entry: three outputs, two of them for voxel A
    c["collision_aba"] = (np.array([[0.5, 0.5, 0.5], [512.5, 0.5, 0.5], [0.5, 0.5, 0.5]], F), 1.0, [[0], [1], [2]])
    # three voxels first seen in decreasing h (9, 6, 3) leave in increasing h
    c["final_flush_order"] = (_centres([[3, 0, 0], [2, 0, 0], [1, 0, 0]]), 1.0, [[2], [1], [0]])
    # entry 7 flushed by point 3, entry 3 by points 5 and 6, entries 15, 18, 0 untouched: flushes by flusher index, then finals by h
    c["mixed_flushes"] = (_centres([[1, 0, 0], [0, 1, 0], [5, 0, 0], [512, 1, 0], [6, 0, 0], [513, 0, 0], [1, 0, 0], [0, 0, 0]]), 1.0,
                          [[1], [0], [5], [7], [6], [3], [2], [4]])
    # a run that goes on behind points of other entries, and one that a collision cuts
    c["interleaved_run"] = (_centres([[1, 0, 0], [2, 0, 0], [1, 0, 0], [513, 0, 0], [2, 0, 0], [1, 0, 0]]), 1.0, [[0, 2], [3], [5], [1, 4]])
    # negative coordinates, and indices whose hash product leaves 32 bits (400 000 * 7171 > 2^31)
    c["negative_and_wrap"] = (_centres([[-1, 0, 0], [400000, 0, 0], [-400000, 300000, -1], [-1, 0, 0], [400000, 0, 0], [-513, 0, 0], [-1, -1, -1]]), 1.0, None)
    c["single_point"] = (np.array([[0.25, -0.75, 3.5]], F), 0.1, [[0]])
    c["empty"] = (np.zeros((0, 3), F), 0.1, [])
    # a NaN, an Inf and a 1e30 coordinate between two points of one run: 3 dropped, the run unbroken
    c["invalid_points"] = (np.array([[0.5, 0.5, 0.5], [np.nan, 0.5, 0.5], [0.5, np.inf, 0.5], [0.5, 0.5, 1e30], [0.6, 0.4, 0.5]], F), 1.0, [[0, 4]])
    c["all_invalid"] = (np.array([[np.nan, 0, 0], [0, -np.inf, 0]], F), 1.0, [])
    c["limit_2p31"] = (np.array([[-2147483648.0, 0.5, 0.5], [2147483520.0, 0.5, 0.5], [-2147483520.0, 0.5, 0.5], [2147483648.0, 0.5, 0.5]], F), 1.0, [[1], [2]])
    return c


def random_cloud(seed, n, lo, hi):
    return np.random.default_rng(seed).uniform(lo, hi, (n, 3)).astype(F)


def long_runs():
    """a run of 65, one of 257 and one of 5 000 points, each in one voxel, the cloud arriving voxel by voxel (leaf 1.0)"""
    rng = np.random.default_rng(11)
    parts = [np.array(v, F) + rng.uniform(0.01, 0.99, (m, 3)).astype(F) for v, m in (((1, 0, 0), 65), ((-4, 2, 7), 257), ((30, -9, 1), 5000))]
    return np.concatenate(parts), 1.0


def short_runs():
    """20 000 random points in a 3 m cube at leaf 0.1: many short runs and real collisions"""
    return random_cloud(5, 20000, -1.5, 1.5), 0.1


def tagged(xyz, k, seed=3):
    """(n, k) records: x y z, then (k > 3) the input index, then random tags in [-8, 8)"""
    xyz = np.asarray(xyz, F)
    rec = np.zeros((len(xyz), k), F)
    rec[:, :3] = xyz
    if k > 3:
        rec[:, 3] = np.arange(len(xyz), dtype=F)
    if k > 4:
        rec[:, 4:] = np.random.default_rng(seed).uniform(-8, 8, (len(xyz), k - 4)).astype(F)
    return rec
