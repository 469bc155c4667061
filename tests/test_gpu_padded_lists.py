"""The padded candidate lists (build_neighbour_lists: every run a multiple of four entries on a 64-byte boundary, pad entry = +inf with
index 0xffffffff) and the walk of k_linearize_lists that takes whole trips without a bounds test: bit for bit against the tile kernel
(PCM_FLAG_NO_NEIGHBOUR_LISTS) and the oracle, on small lattice corners whose voxels hold 1 .. 9 points, so that runs of every length
mod 4 occur -- with num_neighbors = 1 a run IS one voxel's points -- and a query meets fewer than five candidates, ties, voxel
boundaries and negative coordinates.  The second half reads the lists back (pcm_get_neighbour_lists) and compares them with a numpy
construction of the reference's visit order (ivox3d.h:211-235).  Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LISTS, TILE = 16, 64
RES, Q = 0.5, 1.0 / 16
ORIGIN = np.array([-9.0, -6.5, 2.0])               # lattice point; the scene lies at negative x and y
T_T = np.array([1.75, -0.5, 0.25])                 # lattice translation of the pose under test
NEARBY = np.array([(0, 0, 0), (-1, 0, 0), (1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, -1), (0, 0, 1), (1, 1, 0), (-1, 1, 0), (1, -1, 0), (-1, -1, 0),
                   (1, 0, 1), (-1, 0, 1), (1, 0, -1), (-1, 0, -1), (0, 1, 1), (0, -1, 1), (0, 1, -1), (0, -1, -1), (1, 1, 1), (-1, 1, 1), (1, -1, 1),
                   (1, 1, -1), (-1, -1, 1), (-1, 1, -1), (1, -1, -1), (-1, -1, -1)], np.int64)
# in-plane offsets of a voxel's points in units of Q: -4 is exactly the voxel's lower boundary (roundf ties), the rest inside
SLOTS = [(-4, 0), (0, 0), (3, -3), (-3, 3), (2, 2), (-2, -1), (1, -4), (-1, 1), (3, 3)]
COUNTS = {"all": (1, 2, 3, 4, 5, 6, 7, 8, 9), "ragged": (1, 2, 3, 5, 6, 7, 9)}   # ragged: no voxel holds a multiple of four (corner())

_scene = {}


def _voxel(p):
    """roundf(p * inv_res) in float32, half away from zero: the iVox key (ivox3d.h:283-286)."""
    x = np.asarray(p, np.float32) * np.float32(1.0 / RES)
    return (np.sign(x) * np.floor(np.abs(x) + np.float32(0.5))).astype(np.int64)


def corner(kind):
    """(submap (M,3) f32, scan in the body frame (600,3) f32, T (4,4) f64): a floor and two walls of 8 x 6 voxels each on a lattice
    of step Q; voxel (i, j) of a face holds COUNTS[kind][(3 i + 5 j + face) mod len] points, their third coordinate off the face by
    -1 .. 1 lattice steps so that the fits are not degenerate.  The scan is made of lattice points next to the faces."""
    if kind in _scene:
        return _scene[kind]
    counts = COUNTS[kind]
    pts = []
    for face in range(3):
        for i in range(8):
            for j in range(6):
                c = counts[(3 * i + 5 * j + face) % len(counts)]
                for k in range(c):
                    a, b = SLOTS[k]
                    w = ((i + 2 * j + 3 * k + face) % 3 - 1) * Q
                    u, v = (i + 1) * RES + a * Q, (j + 1) * RES + b * Q
                    pts.append(((u, v, w), (u, w, v), (w, u, v))[face])
    rng = np.random.default_rng(11)
    submap = np.asarray(pts)[rng.permutation(len(pts))] + ORIGIN       # input order: shuffled, the lists keep it inside a voxel
    if kind == "ragged":   # the faces share voxels and a boundary point belongs to the neighbour: drop a point where a multiple of four remains
        keys, inv, cnt = np.unique(_voxel(submap), axis=0, return_inverse=True, return_counts=True)
        drop = [int(np.flatnonzero(inv.ravel() == k)[0]) for k in np.flatnonzero(cnt % 4 == 0)]
        submap = np.delete(submap, drop, axis=0)
        assert np.all(np.unique(_voxel(submap), axis=0, return_counts=True)[1] % 4 != 0)
    n = 600
    face = rng.integers(0, 3, n)
    u = rng.integers(2, 8 * 8 + 6, n) * Q; v = rng.integers(2, 6 * 8 + 6, n) * Q; w = rng.integers(-2, 3, n) * Q
    world = np.where((face == 0)[:, None], np.stack([u, v, w], 1), np.where((face == 1)[:, None], np.stack([u, w, v], 1), np.stack([w, u, v], 1))) + ORIGIN
    scan = world - T_T
    T = np.eye(4); T[:3, 3] = T_T
    sub32, scan32 = submap.astype(np.float32), scan.astype(np.float32)
    assert np.array_equal(sub32.astype(np.float64), submap) and np.array_equal((scan32 + T_T.astype(np.float32)).astype(np.float64), world)
    for a in (sub32, scan32):
        a.setflags(write=False)
    _scene[kind] = (sub32, scan32, T)
    return _scene[kind]


def _reg(pcm, submap, scan, optimizer="GN", **kw):
    kw.setdefault("sort_source", 0)
    g = pcm.P2PlaneRegistration(0, optimizer=optimizer, voxel_resolution=RES, **kw)
    g.set_input_target(submap); g.set_input_source(scan)
    return g


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same_linearize(a, b, T, n):
    ra, rb = a.evaluate_cost(T), b.evaluate_cost(T)
    pa, pb = a.get_planes(n), b.get_planes(n)
    assert np.array_equal(np.isnan(pa[:, 0]), np.isnan(pb[:, 0]))
    ok = ~np.isnan(pa[:, 0])
    assert np.array_equal(_bits(pa[ok]), _bits(pb[ok]))
    assert ra[3] == rb[3] and ra[0] == rb[0] and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2])
    return int(ok.sum()), ra[3]


def _in_range_counts(submap, world, nn, max_range):
    """Per query: candidates of its nn-neighbourhood within max_range (double compare, as ivox3d_node.hpp:162)."""
    vm, vq = _voxel(submap), _voxel(world)
    out = np.zeros(len(world), np.int64)
    for i in range(len(world)):
        near = (vm[None, :, :] == (vq[i] + NEARBY[:nn])[:, None, :]).all(2).any(0)
        d = submap[near].astype(np.float32) - world[i].astype(np.float32)
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        out[i] = int((d2.astype(np.float64) < max_range * max_range).sum())
    return out


@pytest.mark.parametrize("kind", ["all", "ragged"])
@pytest.mark.parametrize("nn", [1, 7, 27])
@pytest.mark.parametrize("max_range", [5.0, 1e30])
def test_planes_equal_the_tile_kernel(pcm, kind, nn, max_range):
    """n = 257: the second tile's first lane is its only live lane; 300, 513, 600: one or two full tiles and a partial one.  max_range
    1e30: max_range^2 rounds to +inf in float, the threshold a pad entry's +inf is compared with.  Queries with fewer than five (and
    fewer than three) candidates in range are there, and no pad entry is counted: flags, planes, inliers and sums equal."""
    submap, scan, T = corner(kind)
    world = scan + T_T.astype(np.float32)
    m = _in_range_counts(submap, world, nn, max_range)
    print("queries with 0 / 1-2 / 3-4 / >= 5 candidates: %d %d %d %d" % ((m == 0).sum(), ((m > 0) & (m < 3)).sum(), ((m >= 3) & (m < 5)).sum(), (m >= 5).sum()))
    if nn == 1:
        assert (m == 0).sum() > 10 and ((m > 0) & (m < 3)).sum() > 10 and ((m >= 3) & (m < 5)).sum() > 10 and (m >= 5).sum() > 10
    for n in (257, 300, 513, 600):
        a = _reg(pcm, submap, scan[:n], num_neighbors=nn, flags=LISTS)
        b = _reg(pcm, submap, scan[:n], num_neighbors=nn, flags=TILE)
        for g in (a, b):
            g.set_max_range(max_range)
        sel, inl = _same_linearize(a, b, T, n)
        print("n %d: %d planes, %d inliers" % (n, sel, inl))
        assert sel > 0 or nn == 1


@pytest.mark.parametrize("nn", [1, 27])
def test_planes_equal_the_oracle(pcm, nn):
    """As tests/test_gpu_neighbour_lists.py::test_sparse_and_ragged_tiles: selection flags and planes of every point, bit for bit."""
    from oracle import Oracle
    submap, scan, T = corner("all")
    n = len(scan)
    a = _reg(pcm, submap, scan, num_neighbors=nn, flags=LISTS)
    o = Oracle("P2PLANE", "GN", voxel_resolution=RES, num_neighbors=nn); o.set_input_target(submap); o.set_input_source(scan)
    G = T.copy(); G[:3, 3] += [0.03, -0.02, 0.04]
    for X in (T, G):
        o.linearize(X)
        c1, H1, b1, inl = a.evaluate_cost(X)
        po, so = o.get_planes(n)
        pg = a.get_planes(n)
        sg = ~np.isnan(pg[:, 0])
        print("selected %d (oracle %d), inliers %d / %d" % (sg.sum(), so.sum(), inl, o.num_inliers))
        assert np.array_equal(so, sg) and np.array_equal(_bits(po[so]), _bits(pg[sg])) and inl == o.num_inliers and so.sum() > 100


@pytest.mark.parametrize("optimizer", ["GN", "LM"])
def test_aligns_equal_the_tile_kernel(pcm, optimizer):
    """Single registrations and a batch of three with unequal scan sizes; LM reads the written planes back for its trial passes."""
    submap, scan, T = corner("all")
    ragged = corner("ragged")[0]
    jobs = [(submap, scan[:600]), (ragged, scan[:257]), (submap, scan[100:549])]
    G = T.astype(np.float32).copy(); G[:3, 3] += np.float32([0.05, -0.03, 0.04])
    guesses = np.stack([G] * len(jobs))
    res = {}
    for flags in (LISTS, TILE):
        regs = [_reg(pcm, m, s, optimizer, num_neighbors=27, sort_source=1, flags=flags) for m, s in jobs]
        res[flags] = (pcm.align_batch(regs, guesses), [g.align(G) for g in regs])
    for k in range(len(jobs)):
        base = res[TILE][0][k]
        print("job %d: %d iterations, %d inliers, converged %s" % (k, base.iterations, base.num_inliers, base.converged))
        assert base.num_inliers > 50
        for r in (res[LISTS][0][k], res[LISTS][1][k], res[TILE][1][k]):
            assert np.array_equal(r.T64, base.T64) and np.array_equal(r.H, base.H) and r.cost == base.cost
            assert r.iterations == base.iterations and r.num_inliers == base.num_inliers and r.num_linearize == base.num_linearize
            assert r.num_compute_error == base.num_compute_error and r.converged == base.converged


def _expected_lists(submap, nn):
    """{list voxel: xyz rows in visit order}: for every voxel u of the occupied set dilated by the neighbourhood, the points of
    u + NEARBY[g] for g = 0 .. nn - 1, a voxel's points in the map's input order."""
    vm = _voxel(submap)
    by_voxel = {}
    for i, v in enumerate(map(tuple, vm)):
        by_voxel.setdefault(v, []).append(i)
    lists = {}
    for v in by_voxel:
        for g in range(nn):
            u = tuple(np.asarray(v) - NEARBY[g])
            if u not in lists:
                idx = [i for h in range(nn) for i in by_voxel.get(tuple(np.asarray(u) + NEARBY[h]), [])]
                lists[u] = submap[idx]
    return lists


@pytest.mark.parametrize("kind", ["all", "ragged"])
@pytest.mark.parametrize("nn", [1, 7, 27])
def test_list_layout(pcm, kind, nn):
    """Starts are multiples of four, a run's real entries are the reference's visit order, everything up to the padded end is the pad
    pattern, and the runs tile the array: with `ragged` and nn = 1 the array's final entries are pad entries of its last run."""
    submap, scan, T = corner(kind)
    g = _reg(pcm, submap, scan, num_neighbors=nn, flags=LISTS)
    g.evaluate_cost(T)                                   # builds the map and the lists
    centres, starts, xyz, idx = g.get_neighbour_lists()
    want = _expected_lists(submap, nn)
    assert len(centres) == len(want) and len(starts) == len(centres) + 1
    assert starts[0] == 0 and starts[-1] == len(xyz) and np.all(starts % 4 == 0) and np.all(np.diff(starts.astype(np.int64)) >= 0)
    seen_len = set()
    point_of = {}
    for r, c in enumerate(centres):
        u = tuple(_voxel(c))
        real = want[u]
        s, e = int(starts[r]), int(starts[r + 1])
        assert e - s == (len(real) + 3) // 4 * 4, (u, s, e, len(real))
        assert np.array_equal(_bits(xyz[s:s + len(real)]), _bits(real))
        assert np.all(np.isposinf(xyz[s + len(real):e])) and np.all(idx[s + len(real):e] == 0xffffffff)
        assert np.all(idx[s:s + len(real)] < len(submap))
        for i, p in zip(idx[s:s + len(real)], map(tuple, real)):      # an index names one map point wherever it appears
            assert point_of.setdefault(int(i), p) == p
        seen_len.add(len(real))
    assert len(point_of) == len(submap)
    print("run lengths:", sorted(seen_len)[:12], "...", max(seen_len), "entries", len(xyz), "of them pad", int((idx == 0xffffffff).sum()))
    if nn == 1 and kind == "all":
        assert {1, 2, 3, 4, 5, 8} <= seen_len
    elif nn == 1:                                        # whichever run is the last, it ends in pad entries
        assert all(x % 4 for x in seen_len) and idx[-1] == 0xffffffff and np.all(np.isposinf(xyz[-1]))
    else:
        assert {x % 4 for x in seen_len} == {0, 1, 2, 3}


def test_lists_hook_needs_point_lists(pcm):
    submap, scan, T = corner("all")
    g = _reg(pcm, submap, scan, num_neighbors=27, flags=TILE)
    g.evaluate_cost(T)
    with pytest.raises(pcm.PcmError):
        g.get_neighbour_lists()
