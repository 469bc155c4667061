"""The window sequences of the device plane fit (plane_fit.h: fsqrt_fast, fdiv_recip + fdiv_fast) against IEEE float results:
sqrt over every finite non-negative float inside its window, division over every denominator significand at several exponents
with many numerators each, the window test on its boundaries (zero, denormals, huge values, inf, NaN take the full sequences),
and the per-point planes of k_linearize_lists against the oracle on full-size bench pairs.  Run on the MI355X box with ``-m gpu``.
"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "pointcloud-slam_amd", "csrc")


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    hipcc = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
    out = str(tmp_path_factory.mktemp("fdc") / "fast_divsqrt_check.so")
    subprocess.check_call([hipcc, "-O3", "-std=c++17", "-fPIC", "-shared", "--offload-arch=gfx950", "-ffp-contract=off", "-I" + CSRC,
                           os.path.join(HERE, "fast_divsqrt_check.hip"), "-o", out])
    L = C.CDLL(out)
    L.check_sqrt_range.argtypes = [C.c_uint32, C.c_uint64, C.c_void_p]
    L.check_div.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p]
    L.eval.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    return L


def _eval(lib, a, b):
    a = np.ascontiguousarray(a, np.float32); b = np.ascontiguousarray(b, np.float32)
    n = len(a)
    q, sq, win = np.empty(n, np.float32), np.empty(n, np.float32), np.empty(n, np.int32)
    assert lib.eval(a.ctypes.data, b.ctypes.data, n, q.ctypes.data, sq.ctypes.data, win.ctypes.data) == 0
    return q, sq, win


def test_sqrt_exhaustive(lib):
    cnt = np.zeros(2, np.uint64)
    assert lib.check_sqrt_range(0, 0x7F800000, cnt.ctypes.data) == 0   # +0 .. the largest finite float
    assert cnt[0] == 0x7F800000 - 0x0F800000 and cnt[1] == 0, cnt    # every float in [2^-96, inf) is in the window and exact


def test_sqrt_against_host(lib):
    rng = np.random.default_rng(1)
    bits = rng.integers(0x0F800000, 0x7F800000, 1 << 20, dtype=np.uint32)
    x = bits.view(np.float32)
    _, sq, win = _eval(lib, x, np.ones_like(x))
    assert np.all(win & 4)
    assert np.array_equal(sq.view(np.uint32), np.sqrt(x).view(np.uint32))


@pytest.mark.parametrize("eb", [-40, -17, -1, 0, 1, 6, 22, 39])
def test_div_every_significand(lib, eb):
    ea = np.array([-40, -23, -3, 0, 2, 7, 25, 39], np.int32)
    cnt = np.zeros(2, np.uint64)
    assert lib.check_div(eb, ea.ctypes.data, len(ea), 8, 12345 + eb, cnt.ctypes.data) == 0
    assert cnt[0] == len(ea) * 8 * (1 << 23) and cnt[1] == 0, cnt


def test_div_against_host(lib):
    rng = np.random.default_rng(2)
    n = 1 << 20
    a = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    b = (rng.uniform(1, 2, n) * np.exp2(rng.integers(-40, 40, n))).astype(np.float32) * rng.choice([-1, 1], n).astype(np.float32)
    q, _, win = _eval(lib, a, b)
    assert np.all(win & 3 == 3)
    assert np.array_equal(q.view(np.uint32), (a / b).view(np.uint32))
    assert np.array_equal(q.view(np.uint32), (a.astype(np.float64) / b.astype(np.float64)).astype(np.float32).view(np.uint32))


def test_window_boundaries(lib):
    f = np.float32
    edge = np.array([0.0, -0.0, 1e-45, 1.1754942e-38, 1.17549435e-38, 2.0 ** -96, np.nextafter(f(2.0 ** -96), f(0)), 2.0 ** -40,
                     np.nextafter(f(2.0 ** -40), f(0)), 2.0 ** 40, np.nextafter(f(2.0 ** 40), f(0)), 3.4028235e38, np.inf, -np.inf, np.nan,
                     -1.0, -2.0 ** -40, -2.0 ** 40], np.float32)
    _, _, win = _eval(lib, edge, edge)
    div_in = (win & 1) != 0
    sqrt_in = (win & 4) != 0
    expect_div = np.array([abs(float(v)) >= 2.0 ** -40 and abs(float(v)) < 2.0 ** 40 for v in edge])
    expect_sqrt = np.array([float(v) >= 2.0 ** -96 and float(v) < np.inf for v in edge])
    assert np.array_equal(div_in, expect_div) and np.array_equal(sqrt_in, expect_sqrt)
    # zero, denormals, inf, NaN and negatives are outside the sqrt window; zero, denormals, huge, inf, NaN outside the division's
    for v in (0.0, -0.0, 1e-45, 1.1754942e-38, np.inf, np.nan, -1.0):
        assert not sqrt_in[np.where((edge == np.float32(v)) | (np.isnan(edge) & np.isnan(v)))[0][0]]
    for v in (0.0, 1e-45, 1.1754942e-38, 3.4028235e38, np.inf, np.nan):
        assert not div_in[np.where((edge == np.float32(v)) | (np.isnan(edge) & np.isnan(v)))[0][0]]


@pytest.mark.parametrize("pair_id", [0, 1])
def test_fullsize_lists_planes_equal_oracle(pcm, synth, pair_id):
    """Per-point planes of k_linearize_lists (its WRITE_PLANES instance) on full-size bench pairs, bit-equal to the oracle's."""
    from oracle import Oracle
    p = synth.make_pair(pair_id, 100000, 1000000)
    n = len(p.scan)
    g = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=0.5, num_neighbors=27, sort_source=0, flags=16)
    g.set_input_target(p.submap); g.set_input_source(p.scan)
    o = Oracle("P2PLANE", "GN", voxel_resolution=0.5, num_neighbors=27)
    o.set_input_target(p.submap); o.set_input_source(p.scan)
    for X in (p.guess.astype(np.float64), p.T_gt):
        o.linearize(X); g.evaluate_cost(X)
        po, so = o.get_planes(n)
        pg = g.get_planes(n)
        sg = ~np.isnan(pg[:, 0])
        assert so.sum() > n // 2
        assert np.array_equal(so, sg) and np.array_equal(po[so], pg[sg])
        assert np.array_equal(np.signbit(po[so]), np.signbit(pg[sg]))
