"""The keyed walk of k_linearize_lists (csrc/keyed_best.h: six sorted (distance, position) keys, an ambiguous lane repeats its walk
with best_offer_d2): planes, sums and aligned poses of the lists kernel against the tile kernel (PCM_FLAG_NO_NEIGHBOUR_LISTS) and
the oracle, bit for bit, with the harness of tests/test_gpu_padded_lists.py.  Scans of 257, 300 and 600 points, maps of a few
thousand.  The scenes put lanes of both kinds into the same waves: a random cloud (runs below 128 entries, no ties: the keyed list
decides), a lattice (ties everywhere: every lane repeats), one crowded voxel neighbourhood (runs beyond 128), a query whose 5th and
6th distances are 1 or 200 ulp apart, a range limit within an ulp of a candidate's distance, +inf as the limit, and queries with
0, 3 and 4 candidates in range.  Run on the MI355X box with ``-m gpu``.
"""
import numpy as np
import pytest

from test_gpu_padded_lists import LISTS, TILE, RES, T_T, _bits, _in_range_counts, _reg, _same_linearize, _voxel, corner

pytestmark = pytest.mark.gpu

SIZES = (257, 300, 600)
EYE = np.eye(4)
_cache = {}


def _d2(p, q):
    """float32 squared distances in the kernel's operation order (list_d2 / best_offer)."""
    d = np.asarray(p, np.float32) - np.asarray(q, np.float32)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def surfaces(rng, density=20.0):
    """A floor (x, y in 2 .. 14, z ~ 0) and a wall (y = 14, z in 0 .. 4) with 1 cm noise: ~ 20 points per m^2, so a 27-voxel run of
    a query on one surface holds ~ 45 candidates and random reals never tie.  Nothing within 1.25 m of the origin."""
    nf, nw = int(144 * density), int(48 * density)
    floor = np.stack([rng.uniform(2, 14, nf), rng.uniform(2, 14, nf), rng.normal(0, 0.01, nf)], 1)
    wall = np.stack([rng.uniform(2, 14, nw), 14 + rng.normal(0, 0.01, nw), rng.uniform(0, 4, nw)], 1)
    return np.concatenate([floor, wall])


def surface_queries(rng, n):
    k = n // 4
    f = np.stack([rng.uniform(2.5, 13.5, n - k), rng.uniform(2.5, 13.5, n - k), rng.normal(0, 0.03, n - k)], 1)
    w = np.stack([rng.uniform(2.5, 13.5, k), 14 + rng.normal(0, 0.03, k), rng.uniform(0.5, 3.5, k)], 1)
    return np.concatenate([f, w])


def scene(kind):
    """(submap f32, scan f32) at the identity pose; `kind`: random | crowded | sparse."""
    if kind in _cache:
        return _cache[kind]
    rng = np.random.default_rng({"random": 1, "crowded": 2, "sparse": 3}[kind])
    sub = [surfaces(rng)]
    scan = [surface_queries(rng, 600)]
    if kind == "crowded":   # 400 points inside one voxel neighbourhood of the floor: runs of > 128 entries next to runs of ~ 45
        c = np.array([8.1, 8.1, 0.0])
        sub.append(c + np.stack([rng.uniform(-0.3, 0.3, 400), rng.uniform(-0.3, 0.3, 400), rng.normal(0, 0.01, 400)], 1))
        near = c + np.stack([rng.uniform(-1.2, 1.2, 200), rng.uniform(-1.2, 1.2, 200), rng.normal(0, 0.03, 200)], 1)
        scan[0][rng.permutation(600)[:200]] = near          # every wave holds some of them
    if kind == "sparse":    # clusters of 3 and of 4 points far from everything, queries at them and 0.6 m away
        c3, c4 = np.array([-4.0, -4.0, 0.0]), np.array([-4.0, 4.0, 0.0])
        sub.append(c3 + np.array([[0.05, 0.0, 0.0], [-0.04, 0.07, 0.01], [0.0, -0.08, 0.0]]))
        sub.append(c4 + np.array([[0.05, 0.0, 0.0], [-0.04, 0.07, 0.01], [0.0, -0.08, 0.0], [0.09, 0.09, -0.01]]))
        extra = []
        for c in (c3, c4):
            extra.append(c + rng.uniform(-0.03, 0.03, (40, 3)))                                  # all of the cluster within 0.3 m
            extra.append(c + np.array([0.6, 0.0, 0.0]) + rng.uniform(-0.03, 0.03, (40, 3)))      # in a list voxel, nothing within 0.3 m
        extra = np.concatenate(extra)
        scan[0][rng.permutation(600)[:len(extra)]] = extra
    sub, scan = np.concatenate(sub).astype(np.float32), np.concatenate(scan).astype(np.float32)
    sub = sub[rng.permutation(len(sub))]
    for a in (sub, scan):
        a.setflags(write=False)
    _cache[kind] = (sub, scan)
    return _cache[kind]


def run_lengths(submap, queries):
    """Candidates of each query's 27-voxel neighbourhood (the length of its run before padding)."""
    vm, vq = _voxel(submap), _voxel(queries)
    keys, cnt = np.unique(vm, axis=0, return_counts=True)
    table = {tuple(k): int(c) for k, c in zip(keys, cnt)}
    return np.array([sum(table.get((v[0] + a, v[1] + b, v[2] + c), 0) for a in (-1, 0, 1) for b in (-1, 0, 1) for c in (-1, 0, 1)) for v in vq])


def check(pcm, submap, scan, max_range, sizes=SIZES, nn=27, T=EYE):
    """Lists against tile at every size (planes, flags, cost, H, b, inliers: bit for bit), lists against the oracle at the largest."""
    from oracle import Oracle
    out = []
    for n in sizes:
        a = _reg(pcm, submap, scan[:n], num_neighbors=nn, flags=LISTS)
        b = _reg(pcm, submap, scan[:n], num_neighbors=nn, flags=TILE)
        for g in (a, b):
            g.set_max_range(max_range)
        out.append(_same_linearize(a, b, T, n))
    o = Oracle("P2PLANE", "GN", voxel_resolution=RES, num_neighbors=nn, max_range=float(np.float32(max_range)))
    o.set_input_target(submap); o.set_input_source(scan[:n])
    o.linearize(T)
    po, so = o.get_planes(n)
    pg = a.get_planes(n)
    sg = ~np.isnan(pg[:, 0])
    assert np.array_equal(so, sg) and np.array_equal(_bits(po[so]), _bits(pg[sg])) and a.evaluate_cost(T)[3] == o.num_inliers
    print("max_range %g: (planes, inliers) per size %s" % (max_range, out))
    return out


def test_random_cloud(pcm):
    """a) runs well below 128 entries and no ties: the keyed list decides (nearly) every lane."""
    sub, scan = scene("random")
    L = run_lengths(sub, scan)
    print("run lengths: min %d median %d max %d" % (L.min(), np.median(L), L.max()))
    assert L.max() <= 128 and np.median(L) > 20
    out = check(pcm, sub, scan, 5.0)
    assert all(sel > n // 2 for (sel, inl), n in zip(out, SIZES))


@pytest.mark.parametrize("kind", ["all", "ragged"])
def test_lattice_cloud(pcm, kind):
    """b) a lattice (tests/test_gpu_padded_lists.py's corner): about every other query has an exact tie among its six nearest and
    repeats its walk with best_offer_d2, in every wave."""
    sub, scan, T = corner(kind)
    world = scan + T_T.astype(np.float32)
    d = np.sort(_d2(sub[None, :, :], world[:64, None, :]), axis=1)[:, :6]
    share = (np.diff(d, axis=1) == 0).any(1).mean()
    print("queries with a tie among their six nearest: %.2f" % share)
    assert share > 0.4
    out = check(pcm, sub, scan, 5.0, T=T)
    assert out[-1][0] > 100


def test_crowded_voxel_next_to_sparse_ones(pcm):
    """c) runs beyond 128 entries (left to best_offer_d2) and runs of ~ 45 in the same waves."""
    sub, scan = scene("crowded")
    L = run_lengths(sub, scan)
    long_ = L > 128
    print("queries with a run > 128: %d of %d (max %d)" % (long_.sum(), len(L), L.max()))
    assert long_.sum() > 60 and (~long_).sum() > 300
    for w in range(0, 256, 64):                              # mixed waves in the first tile
        assert long_[w:w + 64].any() and not long_[w:w + 64].all()
    out = check(pcm, sub, scan, 5.0)
    assert all(sel > n // 2 for (sel, inl), n in zip(out, SIZES))


H_STAR = np.float32(0.125)     # the star of test d) lies in the plane z = 1/8 (a plane through the query itself has no A n = -1 fit)
T_STAR = np.eye(4); T_STAR[0, 3] = 8.0      # its query is the body point (-8, 0, 0): a point at the sensor itself is never selected


def _axis_pair(delta, rng):
    """a, b with bits(d2 of Y = (0, b, h + c)) - bits(d2 of X = (a, 0, h)) == delta for a query at the origin (h = 1/8, c = 1/32, so
    every difference the kernel forms is exact): searched among the floats next to 0.3."""
    h, c = H_STAR, np.float32(1.0 / 32)
    a = np.float32(0.3) + np.arange(400, dtype=np.float32) * np.float32(2.0 ** -25)
    b0 = np.sqrt(0.3 ** 2 + float(h) ** 2 - float(h + c) ** 2)
    b = np.float32(b0) + np.arange(-400, 400, dtype=np.float32) * np.float32(2.0 ** -25)
    da = ((a * a) + h * h).view(np.uint32).astype(np.int64)
    db = ((b * b) + (h + c) * (h + c)).view(np.uint32).astype(np.int64)
    hit = np.argwhere(db[None, :] - da[:, None] == delta)
    assert len(hit)
    i, j = hit[rng.integers(len(hit))]
    return a[i], b[j], c


def _star(delta):
    a, b, c = _axis_pair(delta, np.random.default_rng(abs(delta)))
    h = H_STAR
    return np.float32([[0.125, 0.0, h], [0.0, 0.125, h], [-0.125, 0.0, h], [0.0, -0.15625, h], [a, 0.0, h], [0.0, b, h + c]])


@pytest.mark.parametrize("delta", [1, -1, 200, -200])
def test_fifth_and_sixth_distance_apart_by_ulps(pcm, delta):
    """d) the origin query sees four near points and two more, X and Y, whose distances differ by |delta| ulp (sign: which of them is
    the nearer); X lies in the plane of the four, Y 1/32 m above it, so the plane tells which was taken."""
    sub, scan = scene("random")
    sub = np.concatenate([_star(delta), sub]).astype(np.float32)
    scan = scan - np.float32([8.0, 0.0, 0.0]); scan[5] = scan[70] = np.float32([-8.0, 0.0, 0.0])      # 1 * -8 + 0 + 0 + 8 = 0 exactly
    d2 = _d2(sub, np.zeros(3, np.float32))
    d = np.sort(d2.view(np.uint32).astype(np.int64))
    assert d[5] - d[4] == abs(delta) and d[4] - d[3] > 1000 and d[6] - d[5] > 1000 and (d2[5] > d2[4]) == (delta > 0)
    check(pcm, sub, scan, 5.0, T=T_STAR)
    g = _reg(pcm, sub, scan[:257], num_neighbors=27, flags=LISTS); g.evaluate_cost(T_STAR)
    pl = g.get_planes(257)[5]
    print("delta %d: plane of the origin query %s" % (delta, pl))
    assert not np.isnan(pl[0]) and (abs(pl[1]) < 1e-3) == (delta > 0)      # X taken: the plane is z = 1/8, normal (0, 0, -1); Y taken: tilted about x


@pytest.mark.parametrize("which", ["below", "equal", "inf"])
def test_range_limit_next_to_a_candidate(pcm, which):
    """e) max_range = the very distance a of candidates on the axes: max_r2f is the smallest float >= a^2, so their float distance
    fl(a^2) is 1 ulp below it (in range) or equal to it (out, the compare is strict), whichever way a^2 rounds; and 1e30, whose square
    is +inf.  The limit also leaves most floor queries with fewer than five candidates."""
    a = np.float32(0.4)
    while which != "inf" and (float(a * a) < float(a) * float(a)) != (which == "below"):     # fl(a^2) rounded down: max_r2f is the float above it
        a = np.nextafter(a, np.float32(1.0))
    # six candidates at distance exactly a around the origin, three well inside
    star = np.float32([[a, 0, 0], [-a, 0, 0], [0, a, 0], [0, -a, 0], [0, 0, a], [0, 0, -a], [0.125, 0.0, 0.0], [0.0, 0.125, 0.0], [-0.125, -0.125, 0.03125]])
    sub, scan = scene("random")
    sub = np.concatenate([star, sub]).astype(np.float32)
    scan = scan.copy(); scan[3] = 0.0; scan[130] = 0.0
    r = 1e30 if which == "inf" else float(a)
    m2 = float(np.float32(r)) ** 2 if which != "inf" else np.inf
    max_r2f = np.float32(m2) if float(np.float32(m2)) >= m2 else np.nextafter(np.float32(m2), np.float32(np.inf))
    gap = int(np.float32(max_r2f).view(np.uint32)) - int(np.float32(a * a).view(np.uint32))
    print("%s: a = %.9g, max_r2f - fl(a^2) = %d ulp" % (which, a, gap))
    assert which == "inf" or gap == (1 if which == "below" else 0)
    want = {"below": 9, "equal": 3, "inf": 9}[which]
    assert _in_range_counts(sub, np.zeros((1, 3), np.float32), 27, float(np.float32(r)))[0] == want
    check(pcm, sub, scan, r)


def test_zero_three_and_four_candidates_in_range(pcm):
    """f) clusters of three and of four points: queries at them find 3 / 4 within 0.3 m, queries 0.6 m off find none although their
    list voxel exists; at 5 m the latter find 3 / 4 as well."""
    sub, scan = scene("sparse")
    m = _in_range_counts(sub, scan, 27, float(np.float32(0.3)))
    print("queries with 0 / 3 / 4 candidates within 0.3 m: %d %d %d" % ((m == 0).sum(), (m == 3).sum(), (m == 4).sum()))
    assert (m == 0).sum() >= 80 and (m == 3).sum() >= 40 and (m == 4).sum() >= 40
    assert all((m[:257] == k).any() for k in (0, 3, 4))
    check(pcm, sub, scan, 0.3)
    check(pcm, sub, scan, 5.0)


@pytest.mark.parametrize("optimizer", ["GN", "LM"])
def test_align_batch_equals_the_tile_kernel(pcm, optimizer):
    """g) a batch of three pairs -- random, crowded, lattice -- and the single aligns: every result field equal to the tile kernel's."""
    lat_sub, lat_scan, lat_T = corner("all")
    jobs = [(scene("random")[0], scene("random")[1][:600], EYE), (scene("crowded")[0], scene("crowded")[1][:300], EYE), (lat_sub, lat_scan[:257], lat_T)]
    guesses = []
    for _, _, T in jobs:
        G = T.astype(np.float32).copy(); G[:3, 3] += np.float32([0.05, -0.03, 0.04])
        guesses.append(G)
    guesses = np.stack(guesses)
    res = {}
    for flags in (LISTS, TILE):
        regs = [_reg(pcm, m, s, optimizer, num_neighbors=27, sort_source=1, flags=flags) for m, s, _ in jobs]
        res[flags] = (pcm.align_batch(regs, guesses), [g.align(G) for g, G in zip(regs, guesses)])
    for k in range(len(jobs)):
        base = res[TILE][0][k]
        print("job %d: %d iterations, %d inliers, converged %s" % (k, base.iterations, base.num_inliers, base.converged))
        assert base.num_inliers > 50
        for r in (res[LISTS][0][k], res[LISTS][1][k], res[TILE][1][k]):
            assert np.array_equal(r.T64, base.T64) and np.array_equal(r.T, base.T) and np.array_equal(r.H, base.H) and r.cost == base.cost
            assert r.iterations == base.iterations and r.num_inliers == base.num_inliers and r.num_linearize == base.num_linearize
            assert r.num_compute_error == base.num_compute_error and r.converged == base.converged and r.status == base.status
