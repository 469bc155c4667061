"""Inputs the CPU and GPU tests of the IMU forward propagation share (tests/test_lio_predict.py, tests/test_gpu_lio_propagate.py,
tools/measure_lio_propagate_tol.py): an initialised ImuProcess, a filter state, a covariance and a frame of IMU samples, one per
branch of the forward loop of ImuProcess::UndistortPcl."""
import numpy as np

import lio_iekf_ref as R
import lio_predict_ref as PR

RATE = 200.0        # IMU samples per second
T0 = 100.0          # stamp of last_imu
BRANCHES = ("plain", "short_dt", "skipped_pair", "all_skipped", "end_before_imu")


def rand_quat(rng):
    q = rng.normal(size=4)
    return q / np.linalg.norm(q)


def filter_state(rng, grav=None):
    g = np.array([0.1, -0.3, -0.948683298]) if grav is None else np.asarray(grav, np.float64)
    return R.make_state(pos=rng.normal(size=3) * 10, rot=rand_quat(rng), off_R=rand_quat(rng), off_T=rng.normal(size=3) * 0.1, vel=rng.normal(size=3),
                        bg=rng.normal(size=3) * 0.01, ba=rng.normal(size=3) * 0.01, grav=R.LENGTH * g / np.linalg.norm(g))


def covariance(rng, dense=True):
    if not dense:
        return np.diag(R.INIT_P_DIAG)
    d = 10.0 ** rng.uniform(-5, 0, 23)
    Q, _ = np.linalg.qr(rng.normal(size=(23, 23)))
    P = (Q * d) @ Q.T
    return 0.5 * (P + P.T)


def samples(rng, n, t0=T0):
    """(n, 7) rows t, acc, gyr: a sensor at rest up to noise, slowly turning."""
    t = t0 + (np.arange(n) + 1) / RATE
    acc = np.array([0.1, -0.2, 9.8]) + 0.05 * rng.normal(size=(n, 3))
    gyr = np.array([0.02, -0.01, 0.05]) + 0.1 * rng.normal(size=(n, 3))
    return np.column_stack([t, acc, gyr])


def imu_state(rng, **overrides):
    """An ImuProcess past its init frames, with every member the forward loop reads set."""
    last = np.concatenate([[T0], np.array([0.1, -0.2, 9.8]) + 0.05 * rng.normal(size=3), 0.1 * rng.normal(size=3)])
    kw = dict(mean_acc=[0.1, -0.2, 9.8], mean_gyr=[0.001, -0.002, 0.0005], cov_acc=[0.1, 0.11, 0.12], cov_gyr=[0.09, 0.1, 0.08],
              cov_bias_gyr=[0.0001, 0.0002, 0.0001], cov_bias_acc=[0.0001, 0.0001, 0.0003], angvel_last=0.1 * rng.normal(size=3),
              acc_s_last=0.2 * rng.normal(size=3), last_lidar_end_time=T0 - 0.001, last_imu=last, init_iter_num=25, first_frame=0, need_init=0)
    kw.update(overrides)
    return PR.default_imu_state(**kw)


def frame(branch, n, seed=0, dense_P=True):
    """-> dict(s, imu, beg, end, x, P) for one branch of the loop:
      plain           every pair kept, dt = tail.t - head.t, pcl_end_time > imu_end_time
      short_dt        head.t < last_lidar_end_time <= tail.t on the first pair: dt = tail.t - last_lidar_end_time
      skipped_pair    the first tail lies before last_lidar_end_time: that pair is skipped, the next one is shortened (n >= 2)
      all_skipped     every tail lies before last_lidar_end_time: only the closing predict runs, with in = 0
      end_before_imu  pcl_end_time < imu_end_time: dt = -(pcl_end_time - imu_end_time)"""
    rng = np.random.default_rng(1000 * BRANCHES.index(branch) + 10 * n + seed)
    imu = samples(rng, n)
    s = imu_state(rng)
    beg, end = T0 + 0.0007, imu[-1, 0] + 0.3 / RATE
    if branch == "short_dt":
        s["last_lidar_end_time"] = T0 + 0.4 / RATE
    elif branch == "skipped_pair":
        assert n >= 2
        s["last_lidar_end_time"] = T0 + 1.4 / RATE
    elif branch == "all_skipped":
        s["last_lidar_end_time"] = imu[-1, 0] + 0.1 / RATE
    elif branch == "end_before_imu":
        end = imu[-1, 0] - 0.3 / RATE
    return dict(s=s, imu=imu, beg=beg, end=end, x=filter_state(rng), P=covariance(rng, dense_P))


def restate(c, fix=None):
    """The restatement on a frame -> dict(s, x, P, poses, state (26-vector))."""
    s, x, P, poses = PR.propagate(c["s"], c["imu"], c["beg"], c["end"], c["x"], c["P"], fix)
    return dict(s=s, x=x, P=P, poses=poses, state=R.state_to_vec(x))


def groups(r):
    """The three output groups the tolerances are kept for."""
    return dict(state=r["state"], P=r["P"], poses=r["poses"])
