"""The inputs of the ICP tests (tests/test_icp.py checks their conditions on the CPU, tests/test_gpu_icp.py runs them on the
device): the smallest clouds at which the pair kernel and the step can still go wrong.  Every case is (source, target, guess,
params); ``reference(name)`` is the numpy restatement's result (tests/icp_ref.py), computed once per process and shared."""
import functools

import numpy as np

import icp_ref as R


def se3(rx, ry, rz, t):
    M = np.eye(4)
    M[:3, :3] = R.rzryrx(rx, ry, rz)
    M[:3, 3] = t
    return M


def apply(M, p):
    return (p.astype(np.float64) @ M[:3, :3].T + M[:3, 3]).astype(np.float32)


T_LATTICE = se3(0.02, -0.015, 0.03, [0.3, -0.2, 0.1])
T_CLOUD = se3(0.03, -0.02, 0.035, [0.15, -0.1, 0.05])


def lattice(seed=11):
    """n = 7 against m = 9 on a 10 m lattice, perturbations below 1 m: the pairs are i <-> i from the first iteration on"""
    rng = np.random.default_rng(seed)
    g = np.array([[x, y, 0.0] for x in (-10.0, 0.0, 10.0) for y in (-10.0, 0.0, 10.0)])
    tgt = (g + rng.uniform(-0.9, 0.9, g.shape)).astype(np.float32)
    src = apply(np.linalg.inv(T_LATTICE), tgt[:7])
    guess = se3(0.01, 0.0, 0.02, [0.2, -0.1, 0.0]).astype(np.float32)
    return src, tgt, guess


def cloud(n, seed, noise=0.02):
    """n source points against m = 3000 in a 20 m box: a subset of the target moved by a known pose, plus noise"""
    rng = np.random.default_rng(seed)
    tgt = rng.uniform(-10.0, 10.0, (3000, 3)).astype(np.float32)
    pick = rng.permutation(3000)[:n]
    src = apply(np.linalg.inv(T_CLOUD), tgt[pick]) + rng.normal(0.0, noise, (n, 3)).astype(np.float32)
    return src.astype(np.float32), tgt, np.eye(4, dtype=np.float32)


def mirrored():
    """four coplanar points and their mirror image: the step takes S(2) = -1 (a half turn about y maps one onto the other)"""
    tgt = np.array([[0.3, 0.0, 0.0], [-0.2, 5.0, 0.0], [0.25, 10.0, 0.0], [-0.35, 15.0, 0.0]], np.float32)
    src = tgt * np.array([-1.0, 1.0, 1.0], np.float32)
    return src, tgt, np.eye(4, dtype=np.float32)


def threshold():
    """(0, 0, 0) -> (3, 4, 0): d2 = 25 exactly in float; three more pairs at d2 = 1"""
    src = np.array([[0, 0, 0], [100, 0, 0], [100, 10, 0], [100, 0, 10]], np.float32)
    tgt = np.array([[3, 4, 0], [101, 0, 0], [101, 10, 0], [101, 0, 10]], np.float32)
    return src, tgt, np.eye(4, dtype=np.float32)


def two_pairs():
    src, tgt, g = threshold()
    return src[:3].copy(), tgt[:3].copy(), se3(0.0, 0.0, 0.0, [0.125, 0.0, 0.0]).astype(np.float32)


def with_bad_points():
    src, tgt, g = cloud(63, 5)
    src = src.copy()
    src[3] = [np.nan, 0.0, 0.0]
    src[17] = [1.0, np.inf, 2.0]
    src[40] = [-np.inf, np.nan, 0.0]
    return src, tgt, g


def _c(maker, **params):
    return (maker, params)


CASES = {
    "lattice": _c(lattice),
    "lattice_transform_stop": _c(lattice, transformation_epsilon=1e-6),
    "lattice_abs_mse_stop": _c(lattice, mse_absolute=1e-6),
    "n63_rel_mse_stop": _c(lambda: cloud(63, 5), mse_absolute=0.0, euclidean_fitness_epsilon=1e-3, max_iterations=30),
    "lattice_no_pairs": _c(lattice, max_correspondence_distance=1e-3),
    "n63": _c(lambda: cloud(63, 5), max_iterations=12),
    "n64": _c(lambda: cloud(64, 6), max_iterations=12),
    "n257": _c(lambda: cloud(257, 7), max_iterations=12),
    "n1000": _c(lambda: cloud(1000, 8), max_iterations=20),
    "n257_three_iterations": _c(lambda: cloud(257, 7), max_iterations=3),
    "mirrored": _c(mirrored, transformation_epsilon=1e-6),   # an exact fit: against the default 0 the second step's |t|^2 is rounding residue
    "threshold_kept": _c(threshold, max_correspondence_distance=5.0, max_iterations=1),
    "threshold_dropped": _c(threshold, max_correspondence_distance=4.999, max_iterations=1),
    "two_pairs": _c(two_pairs, max_correspondence_distance=1.5, max_iterations=4),
    "bad_points": _c(with_bad_points, max_iterations=12),
}
MIN_GAP, MIN_MARGIN = 1e-4, 1e-9   # what every case must keep: relative NN gap, distance of every threshold comparison from equality


@functools.lru_cache(maxsize=None)
def inputs(name):
    maker, params = CASES[name]
    src, tgt, guess = maker()
    for a in (src, tgt, guess):
        a.setflags(write=False)
    return src, tgt, guess, dict(params)


@functools.lru_cache(maxsize=None)
def reference(name):
    src, tgt, guess, params = inputs(name)
    return R.align(src, tgt, guess, **params)
