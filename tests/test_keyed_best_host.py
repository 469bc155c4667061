"""CPU checks of the keyed 5-best list of k_linearize_lists (pointcloud-slam_amd/csrc/keyed_best.h, compiled with g++ through
tests/keyed_best_hooks.cpp: the very functions the kernel runs) against a plain restatement of best_offer_d2 over the same candidate
sequences.  Wherever the keyed list calls itself unambiguous its result must be best_offer_d2's: the count m and the positions
i[0 .. m) in order (entries at and behind m are free slots; the plane fit reads j < m only).  The ambiguity flag itself is compared
with a numpy statement of the rule on every sequence, and the cases state where a list MUST be ambiguous (equal truncated distances
among the in-range five and the key behind them, a truncated distance equal to the range limit's) and where it must NOT be (so that
the fast path is not vacuously safe)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ID_BITS = 7
LOW = np.uint32((1 << ID_BITS) - 1)
INF_BITS = 0x7F800000


@pytest.fixture(scope="module")
def hooks(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("keyed_best") / "pcm_keyed_best_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "keyed_best_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    fp, up, ip = C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.POINTER(C.c_int)
    L.kb_keyed.argtypes = [fp, C.c_int, C.c_float, up, ip]; L.kb_keyed.restype = C.c_int
    L.kb_plain.argtypes = [fp, C.c_int, C.c_float, up, ip]; L.kb_plain.restype = None
    L.kb_keys.argtypes = [fp, C.c_int, up]; L.kb_keys.restype = None
    return L


def f2u(x):
    return np.asarray(x, np.float32).view(np.uint32)


def u2f(x):
    return np.asarray(x, np.uint32).view(np.float32)


def rule(d2, max_r2f):
    """The ambiguity rule of keyed_best.h in numpy: (ambiguous, m, positions)."""
    d2 = np.asarray(d2, np.float32)
    keys = (f2u(d2) & ~LOW) | np.arange(len(d2), dtype=np.uint32)
    k = np.concatenate([np.sort(keys), np.full(6, 0xFFFFFFFF, np.uint32)])[:6]
    t = (k & ~LOW).astype(np.int64)
    rb = int(f2u(np.float32(max_r2f)))
    R = rb & ~int(LOW)
    amb = rb > INF_BITS
    for j in range(5):
        amb = amb or t[j] == R or (t[j] < R and t[j] == t[j + 1])
    return bool(amb), int((t[:5] < R).sum()), (k[:5] & LOW).astype(np.int64)


def run(L, d2, max_r2f):
    """Both lists over one sequence; asserts the contract and returns (unambiguous, m of best_offer_d2)."""
    d2 = np.ascontiguousarray(d2, np.float32)
    n = len(d2)
    assert n <= 128
    pos, idx = (C.c_uint32 * 5)(), (C.c_uint32 * 5)()
    mk, mp = C.c_int(), C.c_int()
    p = d2.ctypes.data_as(C.POINTER(C.c_float))
    ok = L.kb_keyed(p, n, C.c_float(max_r2f), pos, C.byref(mk))
    L.kb_plain(p, n, C.c_float(max_r2f), idx, C.byref(mp))
    amb, m_rule, pos_rule = rule(d2, max_r2f)
    assert bool(ok) == (not amb), (d2, max_r2f)
    if ok:
        assert mk.value == mp.value == m_rule, (d2, max_r2f, mk.value, mp.value)
        assert list(pos)[:mk.value] == list(idx)[:mk.value] == list(pos_rule[:mk.value]), (d2, max_r2f, list(pos), list(idx))
    return bool(ok), mp.value


def spread(n, rng, lo=0.01, hi=4.0):
    """n distances whose truncated values are pairwise distinct (a geometric ladder, shuffled)."""
    d = (lo * (hi / lo) ** (np.arange(n) / max(n - 1, 1))).astype(np.float32)
    assert len(np.unique(f2u(d) >> ID_BITS)) == n
    return d[rng.permutation(n)]


@pytest.mark.parametrize("n", [1, 4, 5, 6, 17, 127, 128])
def test_random_distances(hooks, n):
    rng = np.random.default_rng(100 + n)
    fast = 0
    for it in range(300):
        d2 = (rng.random(n, dtype=np.float32) * np.float32(2.0)) ** 2
        r = [0.5, 1.0, 4.0, 25.0, np.inf][it % 5]
        ok, m = run(hooks, d2, np.float32(r))
        fast += ok
    print("n %d: %d of 300 unambiguous" % (n, fast))
    assert fast >= (150 if n >= 5 else 100)    # random floats rarely tie in 25 bits: the fast path is the common one


@pytest.mark.parametrize("n", [6, 9, 128])
def test_exact_ties(hooks, n):
    """A pair of equal distances at ranks (r, r + 1): ambiguous for r <= 4 (the pair reaches into the five best), decided for r = 5
    (sixth and seventh).  Both visit orders of the pair; a triple; everything equal."""
    rng = np.random.default_rng(7)
    for r in range(6):
        for rep in range(8):
            d2 = np.sort(spread(n, rng))
            if r + 1 >= n:
                continue
            d2[r + 1] = d2[r]
            d2 = d2[rng.permutation(n)]
            ok, m = run(hooks, d2, np.float32(25.0))
            assert ok == (r == 5), (r, d2)
    d2 = np.sort(spread(n, rng)); d2[2] = d2[3] = d2[4]
    assert not run(hooks, d2[rng.permutation(n)], np.float32(25.0))[0]
    assert not run(hooks, np.full(n, 0.25, np.float32), np.float32(25.0))[0]
    # a tie out of range decides nothing and costs nothing: three in range, the tie behind them
    d2 = np.float32([0.1, 0.2, 0.3, 30.0, 30.0, 30.0, 41.0])
    ok, m = run(hooks, d2, np.float32(25.0))
    assert ok and m == 3


@pytest.mark.parametrize("delta", [1, 127, 128, 129])
def test_near_ties_at_every_rank(hooks, delta):
    """Two distances `delta` ulp apart at ranks (r, r + 1), r = 0 .. 5, the lower one at every offset inside its 128-ulp bucket that
    matters (0, 1, 64, 126, 127).  The pair shares a bucket iff (a + delta) < 128: then and only then, and only for r <= 4, the list is
    ambiguous.  128 and 129 ulp never share one."""
    rng = np.random.default_rng(delta)
    n = 12
    for r in range(6):
        for a in (0, 1, 64, 126, 127):
            base = np.sort(spread(n, rng))
            lo = (int(f2u(base[r])) & ~int(LOW)) + a
            hi = lo + delta
            base[r] = u2f(np.uint32(lo)); base[r + 1] = u2f(np.uint32(hi))
            assert np.all(np.diff(base) > 0)
            share = (lo >> ID_BITS) == (hi >> ID_BITS)
            assert share == (a + delta < 128)
            for rep in range(3):
                ok, m = run(hooks, base[rng.permutation(n)], np.float32(25.0))
                assert ok == (not (share and r <= 4)), (r, a, delta)
                assert m == 5


def test_zero_denormal_and_pads(hooks):
    inf = np.float32(np.inf)
    tiny = u2f(np.uint32([1, 2, 127, 128, 300, 0x007FFFFF]))        # denormals: the first three share the bucket of 0
    # distance 0 and denormals in distinct buckets, pads behind: decided
    d2 = np.float32([0.0, tiny[3], tiny[4], tiny[5], 1.0, 2.0, inf, inf])
    ok, m = run(hooks, d2, np.float32(25.0))
    assert ok and m == 5
    # 0 and a denormal below 128 ulp: one bucket
    assert not run(hooks, np.float32([0.0, tiny[0], 1.0, 2.0, 3.0, 4.0, inf, inf]), np.float32(25.0))[0]
    assert not run(hooks, np.float32([tiny[1], tiny[2], 1.0, 2.0, 3.0, 4.0, 5.0, inf]), np.float32(25.0))[0]
    # pads only / pads among fewer than five real candidates: the pads tie with each other OUT of range, which decides nothing
    for real in ([], [0.5], [0.5, 0.7, 0.9], [0.5, 0.7, 0.9, 1.1]):
        d2 = np.float32(real + [np.inf] * (4 - len(real) % 4 if len(real) % 4 else (4 if not real else 0)))
        ok, m = run(hooks, d2, np.float32(25.0))
        assert ok and m == len(real), (real, ok, m)
    # a pad key is 0x7F800000 | position and the list stays sorted
    keys = (C.c_uint32 * 6)()
    d2 = np.float32([inf, 0.5, inf, 0.25])
    hooks.kb_keys(d2.ctypes.data_as(C.POINTER(C.c_float)), 4, keys)
    assert list(keys) == [int(f2u(np.float32(0.25))) | 3, int(f2u(np.float32(0.5))) | 1, INF_BITS | 0, INF_BITS | 2, 0xFFFFFFFF, 0xFFFFFFFF]
    # NaN distances are never inserted by best_offer_d2 and sort behind the pads here
    ok, m = run(hooks, np.float32([0.5, np.nan, 0.7, 0.9, 1.0, 1.5, 2.0, inf]), np.float32(25.0))
    assert ok and m == 5
    ok, m = run(hooks, np.float32([0.5, np.nan, 0.7, inf]), np.float32(25.0))
    assert ok and m == 2


@pytest.mark.parametrize("n_in", [0, 1, 2, 3, 4, 5, 6])
def test_fewer_than_five_in_range(hooks, n_in):
    rng = np.random.default_rng(n_in)
    for n in (8, 127, 128):
        for rep in range(20):
            d2 = np.sort(spread(n, rng, 0.01, 100.0))
            limit = np.float32(np.sqrt(float(d2[n_in - 1]) * float(d2[n_in]))) if n_in else np.float32(0.005)
            ok, m = run(hooks, d2[rng.permutation(n)], limit)
            assert ok and m == min(n_in, 5)


def test_range_limit_boundary(hooks):
    """Distances within +-130 ulp of max_r2f at every rank: undecided iff the distance shares the limit's bucket; decided, and
    decided right (strict `<`, as best_offer_d2), everywhere else.  max_r2f itself sits at several offsets inside its bucket."""
    rng = np.random.default_rng(3)
    n = 10
    seen = {True: 0, False: 0}
    for a in (0, 1, 64, 127):
        rb = (int(f2u(np.float32(1.0))) & ~int(LOW)) + a
        limit = u2f(np.uint32(rb))
        for off in (-130, -129, -128, -127, -64, -2, -1, 0, 1, 2, 64, 127, 128, 129, 130):
            for r in range(6):
                base = np.sort(spread(n, rng, 0.01, 0.5))                    # r of them below the limit ...
                base[r:] = np.sort(spread(n - r, rng, 2.0, 9.0))             # ... the rest above
                base[r] = u2f(np.uint32(rb + off))                           # rank r sits at the boundary
                shares = ((rb + off) >> ID_BITS) == (rb >> ID_BITS)
                ok, m = run(hooks, base[rng.permutation(n)], limit)
                assert ok == (not (shares and r <= 4)), (a, off, r)
                seen[ok] += 1
                if ok and r <= 4:
                    assert m == r + (1 if off < 0 else 0)
    assert seen[True] > 100 and seen[False] > 50
    # a negative or NaN limit: left to best_offer_d2
    assert not run(hooks, np.float32([0.1, 0.2, 0.3, 0.4]), np.float32(-1.0))[0]
    assert not run(hooks, np.float32([0.1, 0.2, 0.3, 0.4]), np.float32(np.nan))[0]


def test_infinite_range_limit(hooks):
    """max_r2f = +inf (max_range 1e30): R is the pads' bucket.  Five finite candidates or more: decided, m = 5; fewer: a pad or a
    free slot among the five sits at or behind R -- a pad AT it, so the list is left to best_offer_d2."""
    rng = np.random.default_rng(5)
    inf = np.float32(np.inf)
    for n in (5, 6, 8, 127, 128):
        ok, m = run(hooks, spread(n, rng), inf)
        assert ok and m == 5
    d2 = np.concatenate([spread(6, rng), np.float32([np.inf, np.inf])])
    ok, m = run(hooks, d2, inf)
    assert ok and m == 5
    for real in (1, 3, 4):
        d2 = np.concatenate([spread(real, rng), np.full(4 - real % 4, np.inf, np.float32)])
        ok, m = run(hooks, d2, inf)
        assert not ok and m == real                  # m: what best_offer_d2 itself says


@pytest.mark.parametrize("n", [1, 4, 127, 128])
def test_run_lengths(hooks, n):
    """Every position 0 .. n - 1 comes back: the best sits at each place of the run in turn (position 127 is the last that fits)."""
    rng = np.random.default_rng(n)
    for at in sorted({0, n // 2, n - 1}):
        d2 = spread(n, rng, 1.0, 9.0) if n > 1 else np.float32([2.0])
        d2[at] = np.float32(0.125)
        pos, m = (C.c_uint32 * 5)(), C.c_int()
        ok = hooks.kb_keyed(np.ascontiguousarray(d2).ctypes.data_as(C.POINTER(C.c_float)), n, C.c_float(25.0), pos, C.byref(m))
        assert ok and pos[0] == at and m.value == min(n, 5)
        run(hooks, d2, np.float32(25.0))
