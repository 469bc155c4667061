"""CPU checks of the iterated-Kalman-update arithmetic of pcm_lio_update (pointcloud-slam_amd/csrc/lio_iekf.h, compiled with g++ through
tests/lio_iekf_hooks.cpp: the very functions k_iekf_step runs, with one lane) against the numpy restatement of the reference
(tests/lio_iekf_ref.py), and of the pcm_lio_* struct layouts against the ctypes binding.  No GPU.

Every tolerance below is 10 x the worst difference measured between the g++ build and numpy on the inputs of the test (the margin is
for libm and summation-order differences); the measured figures are in the docstrings and in DESIGN.md section 17."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_iekf_ref as R  # noqa: E402

N = 23


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("iekf_hooks") / "lio_iekf_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "lio_iekf_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.iekf_hook_op.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iekf_hook_inverse.argtypes = [C.c_void_p, C.c_void_p]
    L.iekf_hook_run.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.iekf_hook_run.restype = C.c_int
    L.iekf_hook_pose.argtypes = [C.c_void_p, C.c_void_p]
    L.iekf_hook_layout.argtypes = [C.c_void_p]
    return L


def _op(H, op, a, b, n_out):
    a = np.ascontiguousarray(a, np.float64); b = np.ascontiguousarray(b if b is not None else np.zeros(1), np.float64)
    out = np.zeros(n_out)
    H.iekf_hook_op(op, _p(a), _p(b), _p(out))
    return out


def _rel(a, b):
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    return float(np.max(np.abs(a - b)) / max(np.max(np.abs(b)), 1e-300))


def _rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def _deltas(rng, dim):
    """Zero, both sides of the 1e-11 tolerance branches (1e-12, 1e-10), both sides of the Taylor bound of cos_sinc_sqrt, generic."""
    out = [np.zeros(dim)]
    for mag in (1e-12, 1e-10, 1e-3, 3e-2, 0.5, 2.0):
        for _ in range(3):
            d = rng.normal(size=dim)
            out.append(mag * d / np.linalg.norm(d))
    return out


def _grav_vectors(rng):
    out = [np.array([R.LENGTH, 0, 0]), np.array([0, 0, -R.LENGTH]), np.array([-R.LENGTH, 0.0, 0.0]),      # the last: vec[0] + length == 0, degenerate S2_Bx
           np.array([-R.LENGTH + 1e-12, 4.4e-6, 0.0])]
    for _ in range(6):
        v = rng.normal(size=3)
        out.append(R.LENGTH * v / np.linalg.norm(v))
    return out


MANIFOLD_TOL = 10 * 0.0


def test_manifold_pieces_match_restatement(H):
    """boxplus / boxminus round trips on SO3 and S2, A_matrix, S2_Bx, S2_Nx_yy, S2_Mx and cos_sinc_sqrt, header vs numpy.
    Measured worst relative difference (max |a - b| / max |b| per output): 0.0 -- the pieces are the same IEEE operations in the same
    order (-ffp-contract=off) and the restatement calls the process's libm through `math`, as the g++ build does.  Asserted: 10 x that,
    i.e. equality."""
    rng = np.random.default_rng(7)
    worst = 0.0
    for x2 in (0.0, 1e-20, 1.2e-4, 1.3e-4, 1e-2, 2.5, 9.0):
        worst = max(worst, _rel(_op(H, 8, [x2], None, 2), R.cos_sinc_sqrt(x2)))
    for d in _deltas(rng, 3):
        worst = max(worst, _rel(_op(H, 4, d, None, 9), R.A_matrix(d)))
        for _ in range(2):
            q = _rand_quat(rng)
            got = _op(H, 0, q, d, 4); want = R.so3_boxplus(q, d)
            worst = max(worst, _rel(got, want))
            back = _op(H, 1, got, q, 3)
            worst = max(worst, _rel(back, R.so3_boxminus(want, q)))
            if 1e-9 < np.linalg.norm(d) < 1.0:
                assert np.allclose(back, d, rtol=1e-6, atol=1e-15)            # a round trip, whatever the implementation
    for v in _grav_vectors(rng):
        worst = max(worst, _rel(_op(H, 5, v, None, 6), R.s2_Bx(v)))
        worst = max(worst, _rel(_op(H, 6, v, None, 6), R.s2_Nx_yy(v)))
        for d in _deltas(rng, 2):
            worst = max(worst, _rel(_op(H, 7, v, d, 6), R.s2_Mx(v, d)))
            got = _op(H, 2, v, d, 3); want = R.s2_boxplus(v, d)
            worst = max(worst, _rel(got, want))
            assert abs(np.linalg.norm(got) - R.LENGTH) < 1e-12
            back = _op(H, 3, got, v, 2); wback = R.s2_boxminus(want, v)
            worst = max(worst, float(np.max(np.abs(back - wback)) / max(np.max(np.abs(wback)), np.linalg.norm(d), 1e-300)))
            if 1e-6 < np.linalg.norm(d) < 1.0 and v[0] + R.LENGTH > 1e-3:
                assert np.allclose(back, d, rtol=1e-6, atol=1e-12)
    # antipodal vectors: the 3.1415926 of S2.hpp:146
    v = np.array([0.0, R.LENGTH, 0.0])
    assert np.array_equal(_op(H, 3, v, -v, 2), [3.1415926, 0.0]) and np.array_equal(R.s2_boxminus(v, -v), [3.1415926, 0.0])
    assert np.array_equal(_op(H, 3, v, v, 2), [0.0, 0.0])
    # S2_Mx: scalar(1 / 2) == 0 makes exp_delta the identity -> -hat(vec) * A(Bu)^T * Bx
    d = np.array([0.3, -0.2]); B = R.s2_Bx(v)
    assert np.allclose(_op(H, 7, v, d, 6).reshape(3, 2), -R.hat(v) @ R.A_matrix(B @ d).T @ B, rtol=1e-14, atol=1e-15)
    print("manifold worst rel", worst)
    assert worst <= MANIFOLD_TOL


def _state_vec(rng):
    x = R.make_state(pos=rng.normal(size=3) * 10, rot=_rand_quat(rng), off_R=_rand_quat(rng), off_T=rng.normal(size=3) * 0.1, vel=rng.normal(size=3),
                     bg=rng.normal(size=3) * 0.01, ba=rng.normal(size=3) * 0.01, grav=R.LENGTH * np.array([0.1, -0.3, -0.948683298]) / np.linalg.norm([0.1, -0.3, -0.948683298]))
    return x


def test_state_boxplus_boxminus_and_pose(H):
    """state_ikfom's boxplus / boxminus over the eight sub-manifolds, and the float pose an ObsModel call reads, header vs numpy:
    same tolerance as the pieces; the float pose is compared bit for bit with the casts pcm_obs_model makes."""
    rng = np.random.default_rng(11)
    worst = 0.0
    for k in range(20):
        x = _state_vec(rng)
        d = rng.normal(size=N) * (1e-3 if k % 2 else 0.2)
        y = R.state_boxplus(x, d)
        got = _op(H, 9, R.state_to_vec(x), d, 26)
        worst = max(worst, _rel(got, R.state_to_vec(y)))
        back = _op(H, 10, got, R.state_to_vec(x), N)
        worst = max(worst, _rel(back, R.state_boxminus(y, x)))
        assert np.allclose(back, d, rtol=1e-7, atol=1e-12)
        pose = np.zeros(32, np.float32)
        H.iekf_hook_pose(_p(np.ascontiguousarray(R.state_to_vec(x))), _p(pose))
        qwl = R.quat_mul(x["rot"], x["off_R"]).astype(np.float32)
        assert np.array_equal(pose[:4], qwl)
        assert np.array_equal(pose[7:10], x["off_T"].astype(np.float32))
        assert np.array_equal(pose[10:19].reshape(3, 3), R.quat_to_rot(x["off_R"]).astype(np.float32))
        assert np.array_equal(pose[19:28].reshape(3, 3), R.quat_to_rot(x["rot"]).T.astype(np.float32))
    print("state worst rel", worst)
    assert worst <= MANIFOLD_TOL


def _fixture_sums():
    a = np.load(os.path.join(ROOT, "tests", "golden", "lio_iekf_hth.npy"))
    return a[:144].reshape(12, 12), a[144:156], int(a[156])


INV_TOL = 10 * 2.5e-13


def test_lu_inverse_matches_numpy(H):
    """The 23 x 23 partial-pivot LU inverse against numpy.linalg.inv on filter-shaped matrices: P / R with P diagonal 1e-5 .. 1 and
    R = 1e-3, the reference's initial covariance, a dense SPD P, and each of them after inversion and `+= HTH` (HTH of a recorded ObsModel
    call, tests/golden/lio_iekf_hth.npy).  Measured worst max |a - b| / max |b|: 2.5e-13 (the post-HTH matrices, the worst conditioned
    of the set).  Asserted: 10 x that.  The product with the input is the identity to 1e-6."""
    rng = np.random.default_rng(3)
    HTH, _, _ = _fixture_sums()
    mats = []
    d = 10.0 ** rng.uniform(-5, 0, N)
    mats.append(np.diag(d) / 1e-3)
    mats.append(np.diag(R.INIT_P_DIAG) / 1e-3)
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    mats.append((Q * d) @ Q.T / 1e-3)
    for M in list(mats):
        T = np.linalg.inv(M)
        T[:12, :12] += HTH
        mats.append(T)
    Pm = rng.normal(size=(N, N)); Pm[0, 0] = 1e-9        # a first pivot that partial pivoting must move away from
    mats.append(Pm)
    worst = 0.0
    for M in mats:
        M = np.ascontiguousarray(M); inv = np.zeros((N, N))
        H.iekf_hook_inverse(_p(M), _p(inv))
        worst = max(worst, _rel(inv, np.linalg.inv(M)))
        assert np.allclose(inv @ M, np.eye(N), atol=1e-6)
    print("inverse worst rel", worst)
    assert worst <= INV_TOL


def _run(H, x, P, sums_rows, max_iter=4, R_=0.001, limit=None):
    xv = np.ascontiguousarray(R.state_to_vec(x)); Pm = np.ascontiguousarray(np.array(P, np.float64).reshape(N, N).copy())
    lim = np.ascontiguousarray(np.full(N, 0.001) if limit is None else np.asarray(limit, np.float64))
    s = np.ascontiguousarray(np.array(sums_rows, np.float64).reshape(-1, 96))
    ctl = np.zeros(8, np.int32); tdx = np.zeros((len(s), N)); tfl = np.zeros((len(s), 2), np.int32); poses = np.zeros((len(s), 32), np.float32)
    made = H.iekf_hook_run(_p(xv), _p(Pm), R_, max_iter, _p(lim), _p(s), len(s), _p(ctl), _p(tdx), _p(tfl), _p(poses))
    return dict(x=R.vec_to_state(xv), P=Pm, made=made, i=ctl[0], t=ctl[1], converge=ctl[2], done=ctl[3], iterations=ctl[4], rematches=ctl[5],
                valid_calls=ctl[6], n_eff_last=ctl[7], dx=tdx[:made], flags=tfl[:made], poses=poses[:made])


def _scripted(rows):
    """Measurement callback replaying recorded sums, whatever the state."""
    it = iter(rows)

    def h(x, converge):
        HTH, HTh, n_eff = next(it)
        return dict(valid=n_eff >= 1, HTH=HTH, HTh=HTh, n_eff=n_eff, sum_h2=0.0)
    return h


STEP_TOL = 10 * 3.1e-10


def test_full_step_matches_restatement(H):
    """Whole updates of the header against the restatement on the same sums (information form in both): a valid call, an invalid one
    (n_eff = 0 leaves state, P and t untouched, bit for bit) and the exit call with the closing covariance block.  Measured worst
    max |a - b| / max |b| over dx_, the state and P: 3.1e-10 (two inverses of matrices of condition ~1e9 per call, LU here against LAPACK
    there).  Asserted: 10 x that; the final P is symmetric to the same figure times its largest entry."""
    rng = np.random.default_rng(5)
    HTH, HTh, n_eff = _fixture_sums()
    x0 = _state_vec(rng)
    d = 10.0 ** rng.uniform(-5, 0, N)
    Q, _ = np.linalg.qr(rng.normal(size=(N, N)))
    worst = 0.0
    for P0 in (np.diag(R.INIT_P_DIAG), (Q * d) @ Q.T):
        rows = [(HTH, HTh, n_eff), (np.zeros((12, 12)), np.zeros(12), 0), (HTH * 0.9, HTh * 0.1, n_eff - 7), (HTH * 1.1, HTh * 0.01, n_eff), (HTH, HTh * 1e-3, n_eff)]
        want = R.update(x0, P0, _scripted(rows), max_iter=4, dense=False)
        got = _run(H, x0, P0, [R.sums_of(a, b, 0.0, c) for a, b, c in rows], max_iter=4)
        assert got["done"] and got["iterations"] == want["iterations"] == 5 and got["valid_calls"] == want["valid_calls"] == 4
        assert (got["t"], got["rematches"]) == (want["t"], want["rematches"])
        for k, tr in enumerate(want["trace"]):
            assert bool(got["flags"][k, 0]) == tr["converge"] and got["flags"][k, 1] == tr["n_eff"]
            if tr["n_eff"]:
                worst = max(worst, _rel(got["dx"][k], tr["dx_"]))
            else:
                assert not got["dx"][k].any()
        worst = max(worst, _rel(R.state_to_vec(got["x"]), R.state_to_vec(want["x"])), _rel(got["P"], want["P"]))
        assert np.abs(got["P"] - got["P"].T).max() <= STEP_TOL * np.abs(got["P"]).max()
        # an update whose every call is invalid: state and P come back bit for bit
        none = _run(H, x0, P0, [R.sums_of(np.zeros((12, 12)), np.zeros(12), 0.0, 0)] * 5, max_iter=4)
        assert none["done"] and none["iterations"] == 5 and none["valid_calls"] == 0 and none["t"] == 0
        assert np.array_equal(R.state_to_vec(none["x"]), R.state_to_vec(x0)) and np.array_equal(none["P"], P0)
        # a loop that ends on an invalid call keeps the re-projected P_ of the last valid call (P_ is a member): as the restatement
        rows2 = [(HTH, HTh, n_eff), (np.zeros((12, 12)), np.zeros(12), 0)]
        w2 = R.update(x0, P0, _scripted(rows2), max_iter=1, dense=False)
        g2 = _run(H, x0, P0, [R.sums_of(a, b, 0.0, c) for a, b, c in rows2], max_iter=1)
        assert g2["done"] and g2["iterations"] == 2
        worst = max(worst, _rel(g2["P"], w2["P"]), _rel(R.state_to_vec(g2["x"]), R.state_to_vec(w2["x"])))
    print("step worst rel", worst)
    assert worst <= STEP_TOL


@pytest.mark.parametrize("max_iter", [1, 3, 4])
@pytest.mark.parametrize("script", ["converge_first", "never", "early_exit", "invalid_mixed"])
def test_loop_control_matches_restatement(H, max_iter, script):
    """iterations, rematches, t, the exit call and every call's converge flag, header vs restatement, on scripted measurements:
    converging on the first call, never converging (the forced re-match at i == max_iter - 2), t > 1 early exit, invalid calls between
    valid ones; max_iter 1, 3 and 4."""
    rng = np.random.default_rng(max_iter)
    x0 = _state_vec(rng)
    P0 = np.diag(R.INIT_P_DIAG)
    big, small = 0.05, 1e-5
    mags = {"converge_first": [small, big, big, big, big], "never": [big, -big, big, -big, big], "early_exit": [big, small, small, big, big],
            "invalid_mixed": [big, None, small, None, small]}[script]
    rows = []
    sign = 1.0
    for m in mags:
        if m is None:
            rows.append((np.zeros((12, 12)), np.zeros(12), 0))
        else:
            # the state has moved by the earlier updates; a measurement that asks for `m` more from where the state is now needs
            # HTh = HTH (m + dx) -- approximated by alternating the sign, which keeps |dx_| at the scripted size
            HTH = np.eye(12) * 1e6
            HTh = np.zeros(12); HTh[0] = sign * m * 1e6
            rows.append((HTH, HTh, 500))
    rows = rows[:max_iter + 1]
    want = R.update(x0, P0, _scripted(rows), max_iter=max_iter, dense=False)
    got = _run(H, x0, P0, [R.sums_of(a, b, 0.0, c) for a, b, c in rows], max_iter=max_iter)
    assert got["done"] == 1
    assert (got["iterations"], got["rematches"], got["t"], got["valid_calls"]) == (want["iterations"], want["rematches"], want["t"], want["valid_calls"])
    assert got["made"] == want["iterations"]
    assert [bool(f) for f in got["flags"][:, 0]] == [tr["converge"] for tr in want["trace"]]
    if script == "never" and max_iter >= 3:
        assert want["t"] == 0 and want["iterations"] == max_iter + 1 and want["trace"][max_iter]["converge"]     # forced re-match before the last call
    if script == "converge_first" and max_iter >= 3:
        assert want["trace"][1]["converge"]
    if script == "early_exit" and max_iter == 4:
        assert want["t"] == 2 and want["iterations"] == 3                                                         # left at t > 1
    # the pose handed to the next call carries the next converge flag
    flags = got["poses"][:, 28].view(np.int32)
    nxt = [tr["converge"] for tr in want["trace"][1:]]
    assert [bool(f) for f in flags[:len(nxt)]] == nxt


def test_struct_layouts_match_header(H, pcm):
    from pointcloud_slam_amd import capi
    o = np.zeros(9, np.int64)
    H.iekf_hook_layout(_p(o))
    P, Rs = capi.PcmLioUpdateParams, capi.PcmLioUpdateResult
    assert list(o[:7]) == [C.sizeof(capi.PcmLioFilterState), C.sizeof(P), C.sizeof(Rs), P.limit.offset, P.reserved.offset, Rs.sum_h2_last.offset,
                           Rs.reserved.offset]
    assert C.sizeof(capi.PcmLioFilterState) == 26 * 8 and o[7] == 120 and o[8] == 16
