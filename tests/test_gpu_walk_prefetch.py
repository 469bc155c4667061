"""The pipelined keyed walk of k_linearize_lists (csrc/neighbour_lists.hip: the loads of a later trip are issued before the current
trip is consumed, without a bounds test, and the five fit gathers go out together): the places where a prefetching walk can go
wrong -- the last run of the array, runs of one, two and three trips, the longest keyed run next to an unkeyed one, waves whose
lanes disagree about everything, dead lanes, a range limit that excludes most candidates.  Sums, planes and poses of the lists
kernel against the tile kernel (PCM_FLAG_NO_NEIGHBOUR_LISTS), as equalities, with the harness of tests/test_gpu_padded_lists.py.

The map: the floor and wall of tests/test_gpu_keyed_walk.py (3 840 points) and a row of ISOLATED voxels (2 m apart, so the run of a
query in one of them is that voxel's points alone, for every neighbourhood) holding 1, 4, 5, 8, 9, 12, 118, 125, 128 and 130
points: runs of 1, 1, 2, 2, 3, 3, 30, 32, 32 trips and one of 132 entries, which the keyed walk leaves to best_offer_d2.  One more
isolated voxel lies beyond everything else in x, so the last run of the array is its.  The scan is a pattern of 16 lanes repeated,
so every wave -- the partial one of the last tile included -- holds every kind of lane.  Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest

from test_gpu_padded_lists import LISTS, TILE, RES, _bits, _in_range_counts, _reg, _same_linearize, _voxel
from test_gpu_keyed_walk import run_lengths, surface_queries, surfaces

pytestmark = pytest.mark.gpu

EYE = np.eye(4)
SIZES = (257, 300, 600)        # one live lane in the second tile; 44 live lanes and 20 dead ones in its first wave; a partial third tile
ROW = {"one": (-10.0, 1), "four": (-8.0, 4), "five": (-6.0, 5), "eight": (-4.0, 8), "nine": (-2.0, 9), "twelve": (0.0, 12),
       "thirty": (2.0, 118), "k125": (4.0, 125), "k128": (6.0, 128), "long": (8.0, 130)}     # name: (x of the voxel's centre, points); y = -6, z = 0
LAST_AT = np.array([20.0, 2.0, 0.0])
KEY_LIMIT = (1 << 20) - 32     # |voxel coordinate| below this: inside the key range (neighbour_lists.hip)
PATTERN = ("one", "thirty", "empty", "edge", "four", "five", "eight", "nine", "twelve", "k125", "k128", "long", "floor", "last", "floor", "nan")
_cache = {}


def _cluster(rng, c, n, spread=0.2, dz=0.01):
    return np.asarray(c) + np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.normal(0, dz, n)], 1)


def scene(last_count=7):
    """(submap f32, scan f32 (600, 3) at the identity pose, kind of every lane)."""
    if last_count in _cache:
        return _cache[last_count]
    rng = np.random.default_rng(40 + last_count)
    sub = [surfaces(rng)] + [_cluster(rng, (x, -6.0, 0.0), n) for x, n in ROW.values()] + [_cluster(rng, LAST_AT, last_count)]
    sub = np.concatenate(sub).astype(np.float32)
    sub = sub[rng.permutation(len(sub))]
    n = 600
    kinds = np.array([PATTERN[i % len(PATTERN)] for i in range(n)])
    scan = surface_queries(rng, n)
    for i, k in enumerate(kinds):
        if k in ROW:
            scan[i] = _cluster(rng, (ROW[k][0], -6.0, 0.0), 1, dz=0.03)[0]
        elif k == "last":      # the list voxel beyond the last occupied one in x, y and z: its run is the array's last (checked below)
            scan[i] = _cluster(rng, LAST_AT + RES, 1, spread=0.1, dz=0.03)[0]
        elif k == "empty":     # a voxel in the key range with nothing in its neighbourhood
            scan[i] = [-30.0 - (i % 5), 30.0, 3.0]
        elif k == "edge":      # the first voxel coordinate outside the key range, and the last one inside it
            scan[i] = [(KEY_LIMIT - (i // 16) % 2) * RES, 0.0, 0.0]
        elif k == "nan":
            scan[i] = [np.nan, 1.0, 1.0] if (i // 16) % 2 else [1e7, -1e7, 1e7]
    scan = scan.astype(np.float32)
    for a in (sub, scan):
        a.setflags(write=False)
    _cache[last_count] = (sub, scan, kinds)
    return _cache[last_count]


def _padded_runs(sub, scan):
    ok = np.isfinite(scan).all(1) & (np.abs(scan) < 1e5).all(1)
    L = np.zeros(len(scan), np.int64)
    L[ok] = run_lengths(sub, scan[ok])
    return (L + 3) // 4 * 4


def check(pcm, sub, scan, max_range, nn=27, sizes=SIZES):
    """Lists against tile at every size: planes (the plane-writing variant of the kernel), flags, cost, H, b and inliers, bit for bit."""
    out = []
    for n in sizes:
        a = _reg(pcm, sub, scan[:n], num_neighbors=nn, flags=LISTS)
        b = _reg(pcm, sub, scan[:n], num_neighbors=nn, flags=TILE)
        for g in (a, b):
            g.set_max_range(max_range)
        out.append(_same_linearize(a, b, EYE, n))
    print("nn %d max_range %g: (planes, inliers) per size %s" % (nn, max_range, out))
    return out


def check_aligns(pcm, sub, scan, max_range, nn=27):
    """GN (the kernel without plane writes) and LM (trial passes on the written planes), single and batched: every result field."""
    G = np.eye(4, dtype=np.float32); G[:3, 3] = np.float32([0.04, -0.03, 0.02])
    for optimizer in ("GN", "LM"):
        res = {}
        for flags in (LISTS, TILE):
            regs = [_reg(pcm, sub, scan[:n], optimizer, num_neighbors=nn, max_iterations=6, flags=flags) for n in (300, 600)]
            for g in regs:
                g.set_max_range(max_range)
            res[flags] = pcm.align_batch(regs, np.stack([G, G])) + [g.align(G) for g in regs]
        for r, base in zip(res[LISTS], res[TILE]):
            assert np.array_equal(r.T64, base.T64) and np.array_equal(r.T, base.T) and np.array_equal(r.H, base.H) and r.cost == base.cost
            assert r.iterations == base.iterations and r.num_inliers == base.num_inliers and r.num_linearize == base.num_linearize
            assert r.num_compute_error == base.num_compute_error and r.converged == base.converged and r.status == base.status
        print("%s: %d iterations, %d inliers" % (optimizer, res[TILE][0].iterations, res[TILE][0].num_inliers))


def test_scene_is_what_the_cases_need():
    """Run lengths and lane kinds as the docstring says, in every wave (CPU only arithmetic, but it guards the GPU cases below)."""
    sub, scan, kinds = scene()
    P = _padded_runs(sub, scan)
    want = {"one": 4, "four": 4, "five": 8, "eight": 8, "nine": 12, "twelve": 12, "thirty": 120, "k125": 128, "k128": 128, "long": 132, "last": 8,
            "empty": 0, "edge": 0, "nan": 0}
    for k, v in want.items():
        assert np.all(P[kinds == k] == v), (k, np.unique(P[kinds == k]))
    assert np.median(P[kinds == "floor"]) > 20 and P[kinds == "floor"].max() <= 128
    for w in range(0, 600, 64):
        assert set(PATTERN) <= set(kinds[w:w + 64]) or w + 64 > 600
    vx = _voxel(scan[kinds == "edge"])[:, 0]
    assert set(vx) == {KEY_LIMIT, KEY_LIMIT - 1}                   # one outside the key range, one at its last coordinate
    assert set(kinds[256:300]) >= {"one", "thirty", "long", "k125", "last", "empty"} and len(kinds[300:320]) == 20   # live next to dead lanes


@pytest.mark.parametrize("nn", [1, 27])
@pytest.mark.parametrize("last_count", [2, 7, 9])
def test_queries_in_the_last_run_of_the_array(pcm, nn, last_count):
    """The run that ends at num_candidates has 1, 2 or 3 trips; the walk's loads behind it read the zeroed tail.  Queries sit in its
    voxel (found from the read-back lists), results equal the tile kernel's and the lists are what they were afterwards."""
    sub, scan, kinds = scene(last_count)
    a = _reg(pcm, sub, scan, num_neighbors=nn, flags=LISTS)
    a.evaluate_cost(EYE)                                                  # builds the map and the lists
    centres, starts, xyz, idx = a.get_neighbour_lists()
    r = int(np.flatnonzero(np.diff(starts.astype(np.int64)) > 0)[-1])
    assert int(starts[r + 1]) == len(xyz) and int(starts[r + 1]) - int(starts[r]) == (last_count + 3) // 4 * 4
    real = idx[starts[r]:] != 0xffffffff
    assert real.sum() == last_count and np.all(np.abs(xyz[starts[r]:][real] - LAST_AT) < 0.25)
    scan = scan.copy()
    rng = np.random.default_rng(5)
    lanes = np.flatnonzero(kinds == "last")
    scan[lanes] = (centres[r] + rng.uniform(-0.1, 0.1, (len(lanes), 3))).astype(np.float32)
    assert np.all(_voxel(scan[lanes]) == _voxel(centres[r]))
    a.set_input_source(scan)
    a.evaluate_cost(EYE)
    pl = a.get_planes(len(scan))[lanes]
    print("last run: %d entries at %s, %d of its %d queries have a plane" % (starts[r + 1] - starts[r], centres[r], (~np.isnan(pl[:, 0])).sum(), len(lanes)))
    check(pcm, sub, scan, 5.0, nn=nn, sizes=(300, 600))
    if nn == 27:
        check_aligns(pcm, sub, scan, 5.0)
    a.align(EYE.astype(np.float32))
    c2, s2, x2, i2 = a.get_neighbour_lists()
    assert np.array_equal(_bits(c2), _bits(centres)) and np.array_equal(s2, starts) and np.array_equal(_bits(x2), _bits(xyz)) and np.array_equal(i2, idx)


@pytest.mark.parametrize("nn", [1, 27])
def test_runs_of_one_two_and_three_trips(pcm, nn):
    """An isolated map point: four entries, three of them pads; 4, 5, 8, 9 and 12 points: exactly the prefetch depth and one trip
    more, with and without pad entries, for a depth of one and of two."""
    sub, scan, kinds = scene()
    out = check(pcm, sub, scan, 5.0, nn=nn)
    assert all(sel > n // 4 for (sel, inl), n in zip(out, SIZES))
    a = _reg(pcm, sub, scan, num_neighbors=nn, flags=LISTS); a.evaluate_cost(EYE)
    have = ~np.isnan(a.get_planes(len(scan))[:, 0])
    assert not have[kinds == "one"].any()                                  # one candidate: below KMIN, the gathers are not for it
    assert have[kinds == "five"].any() and have[kinds == "nine"].any() and have[kinds == "four"].any()


def test_longest_keyed_run_next_to_an_unkeyed_one(pcm):
    """125 and 128 points (32 trips, the key's last position) and 130 points (132 entries: best_offer_d2) in every wave, beside
    lanes that finish after one trip."""
    sub, scan, kinds = scene()
    P = _padded_runs(sub, scan[:64])
    assert {4, 128, 132} <= set(P)
    check(pcm, sub, scan, 5.0)
    check_aligns(pcm, sub, scan, 5.0)


def test_mixed_wave(pcm):
    """One trip, thirty trips, no list, outside the key range, NaN and +-1e7 in one wave: the scalar position and the lanes' own
    lengths.  A scan of nothing but such lanes, so that no wave is carried by its ordinary ones."""
    sub, scan, kinds = scene()
    keep = np.flatnonzero(np.isin(kinds, ["one", "thirty", "empty", "edge", "nan"]))
    mixed = scan[np.resize(keep, 300)]
    assert set(_padded_runs(sub, mixed[:64])) == {0, 4, 120}
    out = check(pcm, sub, mixed, 5.0, sizes=(257, 300))
    assert all(sel > 20 for sel, inl in out)
    check(pcm, sub, mixed, 5.0, nn=1, sizes=(300,))


@pytest.mark.parametrize("max_range", [0.03, 0.1, 1e30])
def test_range_limit(pcm, max_range):
    """0.03 m and 0.1 m: most candidates are out of range, lanes with 0, 1-2 (below KMIN: no fit, whatever was gathered), 3-4 and 5
    in range share a wave.  1e30: max_range^2 is +inf, the value of a pad entry's distance, so the short runs are undecided."""
    sub, scan, kinds = scene()
    ok = np.flatnonzero(np.isfinite(scan[:128]).all(1) & (np.abs(scan[:128]) < 1e5).all(1))
    m = _in_range_counts(sub, scan[ok], 27, float(np.float32(max_range)))
    print("max_range %g: queries with 0 / 1-2 / 3-4 / >= 5 in range: %d %d %d %d" % (max_range, (m == 0).sum(), ((m > 0) & (m < 3)).sum(), ((m > 2) & (m < 5)).sum(), (m >= 5).sum()))
    if max_range < 1.0:
        assert (m == 0).sum() > 5 and ((m > 0) & (m < 3)).sum() > 5
    if max_range == 0.1:
        assert ((m > 2) & (m < 5)).sum() > 2 and (m >= 5).sum() > 5
    check(pcm, sub, scan, max_range)
    check_aligns(pcm, sub, scan, max_range)
