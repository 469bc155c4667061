"""The keyed walk of k_linearize_lists with its distances on plain f32 instructions (csrc/neighbour_lists.hip: walk_d2; the turn
of two trips holds no packed f32 instruction and no operand-pair move): every place where the turn can go wrong, in ONE launch.
Sums, planes and poses of the lists kernel against the tile kernel (PCM_FLAG_NO_NEIGHBOUR_LISTS) as equalities of bits, with the
harness of tests/test_gpu_padded_lists.py; k_lio_lists, which keeps the walk it had, against its tile-kernel twin with the harness
of tests/test_gpu_lio_lists.py.  No assertion on time or on the disassembly.

The map (4 413 points): the floor and wall of tests/test_gpu_keyed_walk.py, a row of ISOLATED voxels (2 m apart: the run of a query
in one of them is that voxel's points alone) holding 1, 5, 9, 12, 13, 118, 125, 128 and 130 points -- padded runs of exactly 1, 2,
3, 3 and 4 trips (the left-over trip behind the two-trip turn, one turn, a turn and the left-over trip, two turns), 30 and 32
trips, and 132 entries, which the keyed walk leaves to best_offer_d2 -- a lattice patch of 25 points whose queries are lattice
points (exact ties: the repeat path), and one cluster beyond everything else in x, whose run is the array's last.  The scan is a
pattern of 16 lanes repeated, so every wave -- the partial one of the last tile included -- holds every kind of lane: the 128- and
the 132-entry run, a lane with no list, one outside the key range and a NaN lane beside live ones.  Scans of 257, 300 and 600
points: one live lane in a tile, a wave of 44 live and 20 dead lanes, a partial third tile.  Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest

from test_gpu_padded_lists import LISTS, TILE, RES, _bits, _reg, _same_linearize, _voxel
from test_gpu_keyed_walk import _d2, run_lengths, surface_queries, surfaces

pytestmark = pytest.mark.gpu

EYE = np.eye(4)
SIZES = (257, 300, 600)
Q = 1.0 / 16
ROW = {"one": (-10.0, 1), "five": (-8.0, 5), "nine": (-6.0, 9), "twelve": (-4.0, 12), "thirteen": (-2.0, 13), "thirty": (0.0, 118),
       "k125": (2.0, 125), "k128": (4.0, 128), "long": (6.0, 130)}          # name: (x of the voxel's centre, points); y = -6, z = 0
PADDED = {"one": 4, "five": 8, "nine": 12, "twelve": 12, "thirteen": 16, "thirty": 120, "k125": 128, "k128": 128, "long": 132, "lattice": 28,
          "last": 8, "empty": 0, "edge": 0, "nan": 0}
LATTICE_AT = np.array([-14.0, -6.0, 0.0])     # a voxel centre; the patch lies inside that voxel
LAST_AT = np.array([20.0, 2.0, 0.0])
LAST_COUNT = 7
KEY_LIMIT = (1 << 20) - 32                    # |voxel coordinate| below this: inside the key range (neighbour_lists.hip)
PATTERN = ("one", "thirty", "empty", "edge", "thirteen", "five", "lattice", "nine", "twelve", "k125", "k128", "long", "floor", "last", "floor", "nan")
_cache = {}


def _cluster(rng, c, n, spread=0.2, dz=0.01):
    return np.asarray(c) + np.stack([rng.uniform(-spread, spread, n), rng.uniform(-spread, spread, n), rng.normal(0, dz, n)], 1)


def _lattice_patch():
    """5 x 5 lattice points of step 1/16 around LATTICE_AT, z off the plane by -1 .. 1 steps so that the fits are not degenerate."""
    return np.array([LATTICE_AT + [i * Q, j * Q, ((i + 2 * j) % 3 - 1) * Q] for i in range(-2, 3) for j in range(-2, 3)])


def scene():
    """(submap f32, scan f32 (600, 3) at the identity pose, kind of every lane); computed once, read-only."""
    if "scene" in _cache:
        return _cache["scene"]
    rng = np.random.default_rng(62)
    sub = [surfaces(rng)] + [_cluster(rng, (x, -6.0, 0.0), n) for x, n in ROW.values()] + [_lattice_patch(), _cluster(rng, LAST_AT, LAST_COUNT)]
    sub = np.concatenate(sub).astype(np.float32)
    sub = sub[rng.permutation(len(sub))]
    n = 600
    kinds = np.array([PATTERN[i % len(PATTERN)] for i in range(n)])
    scan = surface_queries(rng, n)
    for i, k in enumerate(kinds):
        if k in ROW:
            scan[i] = _cluster(rng, (ROW[k][0], -6.0, 0.0), 1, dz=0.03)[0]
        elif k == "lattice":   # a lattice point of the patch's plane, one step inside the patch: its neighbours come in tied pairs
            scan[i] = LATTICE_AT + [((i // 16) % 3 - 1) * Q, ((i // 48) % 3 - 1) * Q, 0.0]
        elif k == "last":      # the list voxel beyond the last occupied one in x, y and z: its run is among the array's last (test_last_run_of_the_array finds the very last)
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
    _cache["scene"] = (sub, scan, kinds)
    return _cache["scene"]


def _padded_runs(sub, scan):
    ok = np.isfinite(scan).all(1) & (np.abs(scan) < 1e5).all(1)
    L = np.zeros(len(scan), np.int64)
    L[ok] = run_lengths(sub, scan[ok])
    return (L + 3) // 4 * 4


def _check(pcm, sub, scan, max_range, nn=27, sizes=SIZES):
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


def test_scene_is_what_the_cases_need():
    """Run lengths, lane kinds and ties as the docstring says, in every wave (CPU arithmetic only; it guards the GPU cases below)."""
    sub, scan, kinds = scene()
    P = _padded_runs(sub, scan)
    for k, v in PADDED.items():
        assert np.all(P[kinds == k] == v), (k, np.unique(P[kinds == k]))
    assert np.median(P[kinds == "floor"]) > 20 and P[kinds == "floor"].max() <= 128
    for w in range(0, 600, 64):
        assert set(PATTERN) <= set(kinds[w:w + 64]) or w + 64 > 600
    assert {128, 132} <= set(P[:64]) and {128, 132} <= set(P[256:300])      # the keyed limit and the repeat path in one wave
    vx = _voxel(scan[kinds == "edge"])[:, 0]
    assert set(vx) == {KEY_LIMIT, KEY_LIMIT - 1}
    assert set(kinds[256:300]) >= {"one", "thirteen", "long", "k128", "last", "empty", "lattice"} and len(kinds[300:320]) == 20   # live next to dead lanes
    lat = scan[kinds == "lattice"]
    assert np.all(_voxel(lat) == _voxel(LATTICE_AT))
    d = np.sort(_d2(sub[None, :, :], lat[:, None, :]), axis=1)[:, :6]
    assert (np.diff(d, axis=1) == 0).any(1).all()                             # every lattice query has an exact tie among its six nearest


def test_last_run_of_the_array(pcm):
    """The "last" lanes are moved into the list voxel whose run ends at num_candidates (found in the lists read back): the loads ahead
    of its left-over trip read the zeroed tail.  The lists are what they were after the passes."""
    sub, scan, kinds = scene()
    a = _reg(pcm, sub, scan, num_neighbors=27, flags=LISTS)
    a.evaluate_cost(EYE)                                                      # builds the map and the lists
    centres, starts, xyz, idx = a.get_neighbour_lists()
    r = int(np.flatnonzero(np.diff(starts.astype(np.int64)) > 0)[-1])
    assert int(starts[r + 1]) == len(xyz) and int(starts[r + 1]) - int(starts[r]) == PADDED["last"]
    real = idx[starts[r]:] != 0xffffffff
    assert real.sum() == LAST_COUNT and np.all(np.abs(xyz[starts[r]:][real] - LAST_AT) < 0.25)
    scan = scan.copy()
    lanes = np.flatnonzero(kinds == "last")
    scan[lanes] = (centres[r] + np.random.default_rng(5).uniform(-0.1, 0.1, (len(lanes), 3))).astype(np.float32)
    assert np.all(_voxel(scan[lanes]) == _voxel(centres[r]))
    _check(pcm, sub, scan, 5.0)
    a.set_input_source(scan)
    a.align(EYE.astype(np.float32))
    c2, s2, x2, i2 = a.get_neighbour_lists()
    assert np.array_equal(_bits(c2), _bits(centres)) and np.array_equal(s2, starts) and np.array_equal(_bits(x2), _bits(xyz)) and np.array_equal(i2, idx)


@pytest.mark.parametrize("max_range", [0.03, 5.0, 1e30])
def test_planes_and_sums_equal_the_tile_kernel(pcm, max_range):
    """Every kind of lane in one launch, at three range limits.  0.03 m: most candidates are out of range, lanes with 0, 1-2 (below
    KMIN), 3-4 and 5 in range share a wave.  1e30: max_range^2 is +inf, the distance of a pad entry, so every short run is undecided
    and repeats its walk."""
    sub, scan, kinds = scene()
    out = _check(pcm, sub, scan, max_range)
    a = _reg(pcm, sub, scan, num_neighbors=27, flags=LISTS); a.set_max_range(max_range); a.evaluate_cost(EYE)
    have = ~np.isnan(a.get_planes(len(scan))[:, 0])
    assert not have[np.isin(kinds, ["one", "empty", "edge", "nan"])].any()     # one candidate is below KMIN; the others have no list
    if max_range >= 5.0:
        assert all(sel > n // 4 for (sel, inl), n in zip(out, SIZES))
        for k in ("five", "nine", "thirteen", "k128", "long", "lattice"):      # ("last": half a metre off its cluster's plane, never selected)
            assert have[kinds == k].any(), k


def test_single_neighbourhood(pcm):
    """num_neighbors = 1: a run is one voxel's points, the same lanes through shorter runs."""
    sub, scan, kinds = scene()
    _check(pcm, sub, scan, 5.0, nn=1, sizes=(300, 600))


@pytest.mark.parametrize("optimizer", ["GN", "LM"])
@pytest.mark.parametrize("max_range", [0.03, 5.0, 1e30])
def test_aligns_equal_the_tile_kernel(pcm, optimizer, max_range):
    """GN (the kernel without plane writes) and LM (trial passes on the written planes), a batch of two and the single aligns: every
    result field."""
    sub, scan, kinds = scene()
    G = np.eye(4, dtype=np.float32); G[:3, 3] = np.float32([0.04, -0.03, 0.02])
    res = {}
    for flags in (LISTS, TILE):
        regs = [_reg(pcm, sub, scan[:n], optimizer, num_neighbors=27, max_iterations=6, flags=flags) for n in (300, 600)]
        for g in regs:
            g.set_max_range(max_range)
        res[flags] = pcm.align_batch(regs, np.stack([G, G])) + [g.align(G) for g in regs]
    for r, base in zip(res[LISTS], res[TILE]):
        assert np.array_equal(r.T64, base.T64) and np.array_equal(r.T, base.T) and np.array_equal(r.H, base.H) and r.cost == base.cost
        assert r.iterations == base.iterations and r.num_inliers == base.num_inliers and r.num_linearize == base.num_linearize
        assert r.num_compute_error == base.num_compute_error and r.converged == base.converged and r.status == base.status
    print("%s max_range %g: %d iterations, %d inliers" % (optimizer, max_range, res[TILE][0].iterations, res[TILE][0].num_inliers))
    assert res[TILE][0].iterations > 0


@pytest.mark.parametrize("flags_a", [16, 128])
def test_lio_lists_equal_the_tile_kernel(pcm, flags_a):
    """k_lio_lists (contiguous lists, pooled following lists) on the finite lanes of the same scene against k_linearize<.., LIO>: HTH,
    HTh, the counts and the planes, bit for bit; the harness asserts that the lists kernel served the call."""
    from test_gpu_lio_lists import Pair, _state
    sub, scan, kinds = scene()
    keep = ~np.isin(kinds, ["nan", "edge"])
    pr = Pair(pcm, sub, flags_a=flags_a, sort_source=0)
    for n in (300, 600):
        pr.source(np.ascontiguousarray(scan[:n][keep[:n]]))
        pr.obs(_state(EYE, (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)), False, True, min_eff=20)
    assert pr.a.lio_search_path() == (2, 0) and pr.b.lio_search_path() == (0, 2)
