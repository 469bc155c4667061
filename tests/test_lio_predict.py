"""CPU checks of the IMU forward-propagation arithmetic of pcm_lio_imu_init / pcm_lio_propagate (pointcloud-slam_amd/csrc/lio_predict.h,
compiled with g++ through tests/lio_predict_hooks.cpp: the very functions k_imu_propagate runs, with one lane) against the numpy
restatement of the reference (tests/lio_predict_ref.py), and of the new struct layouts against the ctypes binding.  No GPU.

Every tolerance is 10 x the worst difference measured between the g++ build and numpy on the inputs of the test.  Measured: 0.0 in
every test below -- the header and the restatement perform the same IEEE operations in the same order (-ffp-contract=off there, no
fused multiply-add and term-by-term sums here) on the same libm -- so the assertions are equalities."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_iekf_ref as R  # noqa: E402
import lio_predict_case as case  # noqa: E402
import lio_predict_ref as PR  # noqa: E402

N = 23
TOL = 10 * 0.0          # measured worst relative difference, header vs restatement: 0.0
GXX = ["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"), "-I", os.path.join(ROOT, "include"),
       os.path.join(ROOT, "tests", "lio_predict_hooks.cpp")]


def _p(a):
    return a.ctypes.data_as(C.c_void_p)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    so = str(tmp_path_factory.mktemp("predict_hooks") / "lio_predict_hooks.so")
    subprocess.run(GXX + ["-fPIC", "-shared", "-o", so], check=True)
    L = C.CDLL(so)
    L.pred_hook_f.argtypes = [C.c_void_p] * 5
    L.pred_hook_predict.argtypes = [C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pred_hook_propagate.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_double, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    L.pred_hook_propagate.restype = C.c_int
    L.pred_hook_default.argtypes = [C.c_void_p]
    L.pred_hook_imu_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    L.pred_hook_layout.argtypes = [C.c_void_p]
    return L


# ---- the caller's pcm_lio_imu_state as raw doubles (49 = 38 doubles + 7 of last_imu + 4 of the eight int32) -------------------------
def _pack_state(s):
    d = np.concatenate([np.asarray(s[k], np.float64) for k, _ in PR.IMU_KEYS] + [[s["last_lidar_end_time"]], s["last_imu"]])
    i = np.array([s["init_iter_num"], s["first_frame"], s["need_init"], 0, 0, 0, 0, 0], np.int32)
    return np.concatenate([d, i.view(np.float64)])


def _unpack_state(buf):
    s, o = {}, 0
    for k, n in PR.IMU_KEYS:
        s[k] = buf[o:o + n].copy(); o += n
    s["last_lidar_end_time"] = float(buf[o]); o += 1
    s["last_imu"] = buf[o:o + 7].copy(); o += 7
    i = buf[o:o + 4].view(np.int32)
    s["init_iter_num"], s["first_frame"], s["need_init"] = int(i[0]), int(i[1]), int(i[2])
    return s


def _same_imu_state(a, b):
    return all(np.array_equal(a[k], b[k]) for k in a)


def _predict(H, x, P, dt, q, inp):
    xv = np.ascontiguousarray(R.state_to_vec(x)); Pm = np.ascontiguousarray(np.array(P, np.float64).reshape(N, N).copy())
    F = np.zeros((N, N)); W = np.zeros((N, 12))
    in6 = np.concatenate([inp["acc"], inp["gyro"]])
    H.pred_hook_predict(_p(xv), _p(Pm), dt, _p(np.ascontiguousarray(q, np.float64)), _p(in6), _p(F), _p(W))
    return dict(state=xv, P=Pm, F=F, W=W)


def _propagate(H, c):
    buf = _pack_state(c["s"])
    n = len(c["imu"])
    xv = np.ascontiguousarray(R.state_to_vec(c["x"])); Pm = c["P"].copy(); poses = np.zeros((n + 1, 22))
    k = H.pred_hook_propagate(_p(buf), _p(np.ascontiguousarray(c["imu"])), n, c["beg"], c["end"], _p(xv), _p(Pm), _p(poses))
    return dict(s=_unpack_state(buf), state=xv, P=Pm, poses=poses[:k])


Q0 = np.array([0.09, 0.1, 0.08, 0.1, 0.11, 0.12, 1e-4, 2e-4, 1e-4, 1e-4, 1e-4, 3e-4])


def test_f_and_jacobians_match_restatement(H):
    """get_f, df_dx, df_dw in the flatted 24-row layout, header vs numpy, on random states and at the degenerate S2_Bx point."""
    rng = np.random.default_rng(2)
    worst = 0.0
    for k in range(8):
        x = case.filter_state(rng, grav=(-1.0, 0.0, 0.0) if k == 7 else None)
        if k == 7:
            x["grav"] = np.array([-R.LENGTH, 0.0, 0.0])
        inp = PR.make_input(acc=rng.normal(size=3) * 3 + [0, 0, 9.8], gyro=rng.normal(size=3) * 0.5)
        f = np.zeros(24); fx = np.zeros((24, N)); fw = np.zeros((24, 12))
        H.pred_hook_f(_p(np.ascontiguousarray(R.state_to_vec(x))), _p(np.concatenate([inp["acc"], inp["gyro"]])), _p(f), _p(fx), _p(fw))
        worst = max(worst, PR.rel(f, PR.get_f(x, inp)), PR.rel(fx, PR.df_dx(x, inp)), PR.rel(fw, PR.df_dw(x, inp)))
        assert not f[6:12].any() and not f[15:24].any() and not fx[21:24].any()          # the rows the reference leaves zero
    print("f / df_dx / df_dw worst rel", worst)
    assert worst <= TOL


def _predict_inputs():
    rng = np.random.default_rng(4)
    out = []
    x = case.filter_state(rng)
    gen = PR.make_input(acc=[0.3, -0.2, 9.7], gyro=[0.3, -0.2, 0.1])
    out.append(("generic", x, case.covariance(rng), 0.005, gen))
    out.append(("generic_init_P", case.filter_state(rng), case.covariance(rng, False), 0.01, PR.make_input(acc=[-1.0, 2.0, 8.0], gyro=[-1.0, 0.5, 2.0])))
    out.append(("dt_zero", x, case.covariance(rng), 0.0, gen))
    out.append(("gyro_equals_bg", x, case.covariance(rng), 0.005, PR.make_input(acc=[0.3, -0.2, 9.7], gyro=x["bg"])))
    for name, mag in (("below_tol", 5e-12), ("above_tol", 2e-11)):         # |f dt| either side of the 1e-11 of A_matrix, dt = 0.005
        w = mag / 0.005 * np.array([2.0, -1.0, 2.0]) / 3.0
        out.append((name, x, case.covariance(rng), 0.005, PR.make_input(acc=[0.3, -0.2, 9.7], gyro=x["bg"] + w)))
    xd = case.filter_state(rng)
    xd["grav"] = np.array([-R.LENGTH, 0.0, 0.0])
    out.append(("degenerate_Bx", xd, case.covariance(rng), 0.005, gen))
    return out


@pytest.mark.parametrize("name", ["generic", "generic_init_P", "dt_zero", "gyro_equals_bg", "below_tol", "above_tol", "degenerate_Bx"])
def test_predict_matches_restatement(H, name):
    """One esekf::predict, header vs numpy: the state, P, F_x1 and dt * f_w_final.  Generic inputs, dt = 0, gyro == bg (zero rotation,
    the identity branch of A_matrix), |f dt| either side of 1e-11, grav at the degenerate S2_Bx point (-length, 0, 0)."""
    _, x, P, dt, inp = next(t for t in _predict_inputs() if t[0] == name)
    parts = {}
    x2, P2 = PR.predict(x, P, dt, Q0, inp, parts=parts)
    got = _predict(H, x, P, dt, Q0, inp)
    worst = max(PR.rel(got["state"], R.state_to_vec(x2)), PR.rel(got["P"], P2), PR.rel(got["F"], parts["F_x1"]), PR.rel(got["W"], parts["W"]))
    print(name, "worst rel", worst)
    assert worst <= TOL
    assert np.isfinite(got["P"]).all() and np.isfinite(got["state"]).all()
    if name == "dt_zero":
        assert np.array_equal(got["state"], R.state_to_vec(x)) and not got["W"].any()
    if name in ("gyro_equals_bg", "below_tol"):
        assert np.array_equal(got["F"][3:6, 15:18], -np.eye(3) * dt)           # A_matrix == I: the rows pass through unrotated
    if name == "dt_zero":
        # F_x1 is the identity but for its S2 block; P moves in rows / columns 21-22 only
        assert np.array_equal(got["P"][:21, :21], np.array(P)[:21, :21])


FRAMES = [(b, n) for b in case.BRANCHES for n in (1, 2, 3, 20) if not (b == "skipped_pair" and n < 2)]


@pytest.mark.parametrize("branch,n", FRAMES)
def test_forward_loop_matches_restatement(H, branch, n):
    """The forward loop of UndistortPcl and the closing predict, header vs numpy, n = 1, 2, 3, 20 in every branch: a shortened first
    dt, a skipped pair, every pair skipped, pcl_end_time < imu_end_time; the pose list, the state, P and the members left behind."""
    c = case.frame(branch, n)
    want = case.restate(c)
    got = _propagate(H, c)
    assert got["poses"].shape == want["poses"].shape
    expect = {"plain": n + 1, "short_dt": n + 1, "end_before_imu": n + 1, "skipped_pair": n, "all_skipped": 1}[branch]
    assert len(got["poses"]) == expect
    worst = max(PR.rel(got[g], want[g]) for g in ("state", "P", "poses"))
    print(branch, n, "worst rel", worst)
    assert worst <= TOL
    assert _same_imu_state(got["s"], want["s"])
    assert got["s"]["last_lidar_end_time"] == c["end"] and np.array_equal(got["s"]["last_imu"], c["imu"][-1])
    assert np.array_equal(got["poses"][0, 1:7], np.concatenate([c["s"]["acc_s_last"], c["s"]["angvel_last"]]))
    if branch == "short_dt":       # the first pose sits at tail.t, the state moved by tail.t - last_lidar_end_time only
        full = case.restate(dict(c, s=dict(c["s"], last_lidar_end_time=case.T0 - 0.001)))
        assert not np.array_equal(full["state"], want["state"])
    if branch == "end_before_imu":
        later = case.restate(dict(c, end=2 * c["imu"][-1, 0] - c["end"]))      # the mirrored end time: the same |dt|
        assert np.array_equal(later["state"], want["state"])


def test_imu_init_matches_restatement(H):
    """IMUInit and the init branch of Process over 3 frames of 8 samples: init_iter_num 1 -> 9 -> 17 -> 25 crosses MAX_INI_COUNT in the
    third, which rescales cov_acc and then overwrites cov_acc / cov_gyr by the configured scales and drops need_init."""
    rng = np.random.default_rng(6)
    buf = np.zeros(49)
    H.pred_hook_default(_p(buf))
    s = PR.default_imu_state()
    assert _same_imu_state(_unpack_state(buf), s)
    over = dict(cov_acc_scale=[0.2, 0.3, 0.4], cov_gyr_scale=[0.05, 0.06, 0.07], lidar_T_wrt_imu=[0.04165, 0.02326, -0.0284], lidar_R_wrt_imu=case.rand_quat(rng))
    s = PR.default_imu_state(**over)
    buf = _pack_state(s)
    x = case.filter_state(rng); P = case.covariance(rng)
    xv = np.ascontiguousarray(R.state_to_vec(x)); Pm = P.copy()
    t = 10.0
    for f in range(3):
        imu = case.samples(rng, 8, t0=t); t = imu[-1, 0]
        s, x, P = PR.imu_init(s, imu, x, P)
        H.pred_hook_imu_init(_p(buf), _p(np.ascontiguousarray(imu)), 8, _p(xv), _p(Pm))
        got = _unpack_state(buf)
        assert _same_imu_state(got, s), f
        assert PR.rel(xv, R.state_to_vec(x)) <= TOL and np.array_equal(Pm, P)
        assert got["init_iter_num"] == 1 + 8 * (f + 1) and got["need_init"] == (1 if f < 2 else 0) and got["first_frame"] == 0
        if f < 2:
            assert not np.array_equal(got["cov_acc"], over["cov_acc_scale"])
    assert np.array_equal(got["cov_acc"], over["cov_acc_scale"]) and np.array_equal(got["cov_gyr"], over["cov_gyr_scale"])
    assert abs(np.linalg.norm(xv[23:26]) - R.LENGTH) < 1e-14 and np.array_equal(xv[7:11], over["lidar_R_wrt_imu"])     # the S2 length, not 9.81
    assert np.array_equal(np.diag(Pm), R.INIT_P_DIAG)


def test_struct_layouts_match_header(H, pcm):
    from pointcloud_slam_amd import capi
    o = np.zeros(12, np.int64)
    H.pred_hook_layout(_p(o))
    S = capi.PcmLioImuState
    assert list(o[:9]) == [C.sizeof(capi.PcmImuSample), C.sizeof(S), S.cov_acc_scale.offset, S.lidar_R_wrt_imu.offset, S.last_lidar_end_time.offset,
                           S.last_imu.offset, S.init_iter_num.offset, S.reserved.offset, 22 * 8]
    assert C.sizeof(capi.PcmImuSample) == 56 and C.sizeof(S) == 49 * 8 and o[11] == 1024
    for name in ("pcm_lio_default_imu_state", "pcm_lio_imu_init", "pcm_lio_propagate"):
        assert name in capi.SYMBOLS


# ---- one test per quirk and pinned rule: the header sides with the literal restatement and against a "corrected" one ---------------
def _quirk_case():
    rng = np.random.default_rng(8)
    return case.filter_state(rng), case.covariance(rng), 0.005, PR.make_input(acc=[0.3, -0.2, 9.7], gyro=[0.8, -0.6, 0.4])


def test_quirk_a_exponentials_scaled_by_integer_half(H):
    """(a) scalar_type(1 / 2) == 0: the SO3 diagonal blocks of F_x1 before `+= f_x_final dt` are the identity and the S2 block is
    Nx(x_after) Mx(x_before, 0).  A restatement that scales by 0.5 puts R(exp(-f dt / 2)) there and fails."""
    x, P, dt, inp = _quirk_case()
    got = _predict(H, x, P, dt, Q0, inp)
    lit, fixed = {}, {}
    _, P_lit = PR.predict(x, P, dt, Q0, inp, parts=lit)
    _, P_fix = PR.predict(x, P, dt, Q0, inp, fix={"a": 1}, parts=fixed)
    assert np.array_equal(got["F"], lit["F_x1"]) and np.array_equal(got["P"], P_lit)
    assert np.array_equal(got["F"][3:6, 3:6], np.eye(3))                       # f_x_final has no entry in that block: the base block shows
    assert PR.rel(got["F"][3:6, 3:6], fixed["F_x1"][3:6, 3:6]) > 1e-4 and PR.rel(got["P"], P_fix) > 1e-6


def test_quirk_b_mx_takes_its_hat_branch(H):
    """(b) S2_Mx with a zero delta: the S2 block of F_x1 is Nx(x_after) (-hat(x_before) Bx(x_before)).  The rows of f_ that would move
    grav are zero, so no state-derived delta exists; the variant passes a non-zero one to show the test sees the branch."""
    x, P, dt, inp = _quirk_case()
    got = _predict(H, x, P, dt, Q0, inp)
    x_after, _ = PR.predict(x, P, dt, Q0, inp)
    want = PR._mm3(R.s2_Nx_yy(x_after["grav"]), PR._mm3(-R.hat(x["grav"]), R.s2_Bx(x["grav"])))
    assert np.allclose(got["F"][21:23, 21:23], want, rtol=1e-14, atol=1e-16)
    fixed = {}
    PR.predict(x, P, dt, Q0, inp, fix={"b": [0.3, -0.2]}, parts=fixed)
    assert PR.rel(got["F"][21:23, 21:23], fixed["F_x1"][21:23, 21:23]) > 1e-3


def test_quirk_c_a_matrix_identity_below_tolerance(H):
    """(c) |f dt| = 5e-12 < 1e-11: A_matrix is exactly the identity, so rows 3-5 of f_x_final are those of f_x_.  A series A_matrix
    (I + hat / 2 + ...) leaves 2.5e-12-sized off-diagonal entries and fails the equality."""
    x, P, dt, _ = _quirk_case()
    w = 5e-12 / dt * np.array([2.0, -1.0, 2.0]) / 3.0
    inp = PR.make_input(acc=[0.3, -0.2, 9.7], gyro=x["bg"] + w)
    got = _predict(H, x, P, dt, Q0, inp)
    fixed = {}
    PR.predict(x, P, dt, Q0, inp, fix={"c": 1}, parts=fixed)
    assert np.array_equal(got["F"][3:6, 15:18], -np.eye(3) * dt)
    assert not np.array_equal(fixed["F_x1"][3:6, 15:18], -np.eye(3) * dt)


def test_quirk_d_q_is_the_callers_diagonals(H):
    """(d) Q_ carries cov_gyr, cov_acc, cov_bias_gyr, cov_bias_acc of the caller on its diagonal and nothing else: P differs from a
    restatement that keeps the constructor's process_noise_cov(), and the noise term has no cross terms between the four groups."""
    c = case.frame("plain", 3)
    got = _propagate(H, c)
    assert np.array_equal(got["P"], case.restate(c)["P"])
    assert PR.rel(got["P"], case.restate(c, fix={"d": 1})["P"]) > 1e-6
    x, P, dt, inp = _quirk_case()
    a = _predict(H, x, np.zeros((N, N)), dt, Q0, inp)["P"]                      # P = 0: the noise term alone
    W = _predict(H, x, np.zeros((N, N)), dt, Q0, inp)["W"]
    assert np.allclose(a, (W * Q0) @ W.T, rtol=1e-13, atol=1e-30) and a[15:18, 18:21].any() is np.False_


def test_pinned_acc_s_last_starts_at_zero(H):
    """acc_s_last_ is never initialised by the reference's constructor: zero here, so the first pose of the first propagated frame
    carries acc = 0.  A variant that starts it from the incoming state fails."""
    buf = np.zeros(49)
    H.pred_hook_default(_p(buf))
    assert not _unpack_state(buf)["acc_s_last"].any()
    c = case.frame("plain", 3)
    c["s"]["acc_s_last"] = _unpack_state(buf)["acc_s_last"]
    got = _propagate(H, c)
    assert not got["poses"][0, 1:4].any()
    assert np.array_equal(got["poses"], case.restate(c)["poses"])
    assert case.restate(c, fix={"acc_s": 1})["poses"][0, 1:4].any()


def test_pinned_all_skipped_closing_predict_uses_zero_input(H):
    """Every pair skipped: the closing predict runs with in = 0 (the reference reads a default-constructed input_ikfom).  A variant
    that uses last_imu instead moves the state elsewhere."""
    c = case.frame("all_skipped", 3)
    got = _propagate(H, c)
    want = case.restate(c)
    assert np.array_equal(got["state"], want["state"]) and np.array_equal(got["P"], want["P"]) and len(got["poses"]) == 1
    dt = abs(c["end"] - c["imu"][-1, 0])
    x1, _ = PR.predict(c["x"], c["P"], dt, Q0, PR.make_input())
    assert np.array_equal(got["state"], R.state_to_vec(x1))
    assert not np.array_equal(case.restate(c, fix={"in": 1})["state"], want["state"])


def test_standalone_program_replays_the_frames(H, tmp_path):
    """tests/lio_predict_hooks.cpp with its main (the program the host-code sanitizer check builds): replays every forward-loop frame
    and the init frames from a file and prints the sums the library build gives."""
    exe = str(tmp_path / "lio_predict_replay")
    subprocess.run(GXX + ["-DLIO_PREDICT_HOOKS_MAIN", "-o", exe], check=True)
    path = str(tmp_path / "cases.bin")
    want = []
    with open(path, "wb") as fp:
        for branch, n in FRAMES + [("plain", 1024)]:
            c = case.frame(branch, n)
            fp.write(np.array([0, n], np.int32).tobytes() + np.array([c["beg"], c["end"]]).tobytes() + _pack_state(c["s"]).tobytes() +
                     R.state_to_vec(c["x"]).tobytes() + c["P"].tobytes() + np.ascontiguousarray(c["imu"]).tobytes())
            g = _propagate(H, c)
            want.append((0, n, len(g["poses"]), g["state"], g["P"]))
        rng = np.random.default_rng(6)
        s = PR.default_imu_state(); x = case.filter_state(rng); P = case.covariance(rng)
        imu = case.samples(rng, 8)
        fp.write(np.array([1, 8], np.int32).tobytes() + np.zeros(2).tobytes() + _pack_state(s).tobytes() + R.state_to_vec(x).tobytes() + P.tobytes() + imu.tobytes())
        _, x2, P2 = PR.imu_init(s, imu, x, P)
        want.append((1, 8, 0, R.state_to_vec(x2), P2))
    out = subprocess.run([exe, path], check=True, capture_output=True, text=True).stdout.strip().splitlines()
    assert len(out) == len(want)
    for line, (kind, n, k, xs, Ps) in zip(out, want):
        f = line.split()
        assert (int(f[0]), int(f[1]), int(f[2])) == (kind, n, k)
        sx = 0.0
        for v in xs:
            sx += float(v)
        sp = 0.0
        for v in Ps.ravel():
            sp += float(v)
        assert float.fromhex(f[3]) == sx and float.fromhex(f[4]) == sp
