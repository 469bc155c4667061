"""GPU parity of pcm_lio_propagate -- the forward loop of ImuProcess::UndistortPcl with esekf::predict per IMU sample, one wave on the
device -- against the numpy restatement of the reference (tests/lio_predict_ref.py), and of LioOdometry (LaserMapping::Run composed
from the existing frame calls) against the same sequence with the propagation done by the restatement on the host.

The bounds are not taken from the device.  tools/measure_lio_propagate_tol.py restates every frame below once as is and 20 times
with every sin / cos / sqrt / atan result moved by +-1 ulp at random; MEASURED holds the worst relative difference (max |a - b| /
max |b|) of those runs per output group, and a device result must stay within 10 x that of the unperturbed restatement (the margin
is for the device's libm; the products are summed in the restatement's order, without fused multiply-adds)."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_iekf_ref as ref  # noqa: E402
import lio_predict_case as case  # noqa: E402
import lio_predict_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = [("plain", 1), ("plain", 2), ("plain", 3), ("plain", 20), ("plain", 64), ("plain", 65), ("plain", 1024),
         ("short_dt", 20), ("skipped_pair", 20), ("all_skipped", 20), ("end_before_imu", 20)]

# worst relative difference between the restatement and its 20 +-1 ulp libm runs (tools/measure_lio_propagate_tol.py)
MEASURED = {
    ('plain', 1): dict(state=2.8e-18, P=2.5e-15, poses=2.3e-16),
    ('plain', 2): dict(state=2.2e-18, P=1.5e-15, poses=7.0e-17),
    ('plain', 3): dict(state=4.8e-18, P=1.9e-15, poses=1.5e-16),
    ('plain', 20): dict(state=4.8e-17, P=6.4e-15, poses=2.3e-16),
    ('plain', 64): dict(state=7.2e-17, P=2.4e-15, poses=2.9e-16),
    ('plain', 65): dict(state=9.5e-17, P=5.9e-15, poses=4.0e-16),
    ('plain', 1024): dict(state=2.1e-16, P=1.5e-14, poses=2.1e-16),
    ('short_dt', 20): dict(state=4.8e-17, P=3.5e-15, poses=4.1e-16),
    ('skipped_pair', 20): dict(state=3.6e-17, P=4.8e-15, poses=3.4e-16),
    ('all_skipped', 20): dict(state=0.0e+00, P=8.0e-15, poses=0.0e+00),
    ('end_before_imu', 20): dict(state=2.4e-17, P=3.7e-15, poses=2.2e-16),
    'two_calls': dict(state=4.8e-17, P=4.3e-15, poses=4.5e-16),
}


def make_case(key):
    return case.frame(key[0], key[1])


def two_frames():
    """Two consecutive frames of 20 samples: the second starts where the first ended (its last_imu / last_lidar_end_time are the first's)."""
    c1 = case.frame("plain", 20, seed=3)
    rng = np.random.default_rng(77)
    t_last = c1["imu"][-1, 0]
    imu2 = case.samples(rng, 20, t0=t_last)
    c2 = dict(imu=imu2, beg=c1["end"] + 0.0004, end=imu2[-1, 0] + 0.2 / case.RATE)
    return c1, c2


def bound(key, group):
    return 10 * MEASURED[key][group]


def _state_of(pcm, s):
    from pointcloud_slam_amd.registration import lio_imu_state
    return lio_imu_state(**s)


@pytest.fixture(scope="module")
def reg(pcm):
    return pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)


@pytest.fixture(scope="module")
def restated():
    """Every frame restated once, shared by the tests."""
    return {key: case.restate(make_case(key)) for key in CASES}


def _run(pcm, reg, c, st=None, capacity=None):
    st = _state_of(pcm, c["s"]) if st is None else st
    x, P, poses = reg.lio_propagate(st, c["imu"], c["beg"], c["end"], c["x"], c["P"], capacity=capacity)
    return st, dict(x=x, P=P, poses=poses, state=ref.state_to_vec(x))


def _check(key, got, want):
    figs = {g: PR.rel(got[g], want[g]) for g in ("state", "P", "poses")}
    print(key, " ".join("%s %.2e (bound %.1e)" % (g, figs[g], bound(key, g)) for g in figs))
    assert got["poses"].shape == want["poses"].shape
    for g in figs:
        assert figs[g] <= bound(key, g), (key, g, figs[g], bound(key, g))


@pytest.mark.parametrize("key", CASES, ids=lambda k: "%s-%d" % k)
def test_propagate_matches_restatement(pcm, reg, restated, key):
    """State, covariance and the IMUpose_ list within the measured bound; the members the reference leaves behind (last_imu,
    last_lidar_end_time, angvel_last, acc_s_last) as the restatement leaves them; P symmetric to the bound with a positive diagonal."""
    c, want = make_case(key), restated[key]
    st, got = _run(pcm, reg, c)
    _check(key, got, want)
    ws = want["s"]
    assert st.last_lidar_end_time == ws["last_lidar_end_time"] == c["end"]
    assert np.array_equal([st.last_imu.t] + list(st.last_imu.acc) + list(st.last_imu.gyr), c["imu"][-1])
    tol = bound(key, "poses")
    assert PR.rel(np.array(st.angvel_last[:]), ws["angvel_last"]) <= tol and PR.rel(np.array(st.acc_s_last[:]), ws["acc_s_last"]) <= tol
    P = got["P"]
    assert np.abs(P - P.T).max() <= bound(key, "P") * np.abs(P).max()
    assert (np.diag(P) > 0).all()
    if key[0] == "all_skipped":
        assert len(got["poses"]) == 1
    if key[0] == "skipped_pair":
        assert len(got["poses"]) == key[1]


def test_capacity_and_sample_limits(pcm, reg):
    """capacity == n + 1 is enough; n + 0 and n = 1025 are errors that leave the IMU state, x and P untouched."""
    c = make_case(("plain", 20))
    _run(pcm, reg, c, capacity=21)
    for imu, cap, code in ((c["imu"], 20, -1), (case.samples(np.random.default_rng(5), 1025), 1026, -5), (c["imu"][:0], 4, -1)):
        st = _state_of(pcm, c["s"])
        before = bytes(st)
        x0 = {k: v.copy() for k, v in c["x"].items()}; P0 = c["P"].copy()
        with pytest.raises(pcm.PcmError) as e:
            reg.lio_propagate(st, imu, c["beg"], c["end"], c["x"], c["P"], capacity=cap)
        assert e.value.code == code and len(str(e.value)) > 20
        assert bytes(st) == before and np.array_equal(P0, c["P"]) and all(np.array_equal(x0[k], c["x"][k]) for k in x0)
    st = _state_of(pcm, dict(c["s"], need_init=1))
    with pytest.raises(pcm.PcmError, match="initialised"):
        reg.lio_propagate(st, c["imu"], c["beg"], c["end"], c["x"], c["P"])


def test_two_calls_carry_the_state(pcm, reg):
    """Two frames on one IMU state: the second call reads the last_imu, last_lidar_end_time, angvel_last and acc_s_last the first
    left, as the restatement doing the same."""
    c1, c2 = two_frames()
    a = case.restate(c1)
    want = case.restate(dict(c2, s=a["s"], x=a["x"], P=a["P"]))
    st, g1 = _run(pcm, reg, c1)
    _, g2 = _run(pcm, reg, dict(c2, s=None, x=g1["x"], P=g1["P"]), st=st)
    assert np.array_equal(g2["poses"][0, 1:7], np.concatenate([g1["poses"][-1, 1:4], g1["poses"][-1, 4:7]]))   # the first pose carries the last acc / gyr
    _check("two_calls", g2, want)


def test_run_to_run_identity(pcm, reg):
    c = make_case(("plain", 65))
    a = _run(pcm, reg, c)[1]; b = _run(pcm, reg, c)[1]
    for g in ("state", "P", "poses"):
        assert np.array_equal(a[g].view(np.uint64), b[g].view(np.uint64))


def test_poses_feed_undistort(pcm, reg, restated):
    """The device's pose list and the restatement's through the same pcm_undistort on a 256-point scan: the same compensated scan."""
    key = ("plain", 20)
    c, want = make_case(key), restated[key]
    _, got = _run(pcm, reg, c)
    rng = np.random.default_rng(9)
    pts = np.zeros((256, 12), np.float32)
    pts[:, :3] = rng.normal(size=(256, 3)) * 10
    pts[:, 9] = np.sort(rng.uniform(0, (c["end"] - c["beg"]) * 1000.0, 256)).astype(np.float32)    # curvature: ms after the first point
    out = []
    for r in (got, want):
        x = r["x"]
        out.append(reg.undistort(pts.copy(), 9, r["poses"], x["rot"], x["pos"], x["off_R"], x["off_T"])[:, :3])
    moved = np.abs(out[1] - pts[:, :3]).max()
    assert moved > 1e-3                                                   # the compensation does something on this frame
    assert np.abs(out[0] - out[1]).max() <= 4 * np.finfo(np.float32).eps * np.abs(out[1]).max()   # float32 outputs of double inputs 1e-13 apart


def _room(synth):
    """A room seen from an upright sensor: rot = identity, so a sensor at rest measures acc = (0, 0, 9.81) and the state IMUInit leaves
    (grav along -mean_acc) is consistent with the pose."""
    scene = synth.scene_for_points(4321, 20000, 8.0)
    T = np.eye(4)
    T[:3, 3] = synth.sensor_pose(scene, 12)[:3, 3]
    return scene, T


def test_lio_odometry_matches_restatement_driven_sequence(pcm, synth):
    """LioOdometry over 3 init frames + the first scan + 3 frames in a synthetic room (scans <= 2 k points, the map grows from the
    first scan; 20 IMU samples per propagated frame, 8 per init frame so that MAX_INI_COUNT is crossed in the third) against the same
    sequence with the propagation done by the restatement on the host: the same stages, scan sizes, loop counters and map size.  The
    two runs hand lio_update states that differ in the last bits (the bounds above); the update answers last-bit differences of its
    input by at most FRAME_TOL of tests/test_gpu_lio_update.py (that figure is its measured response to the last-bit differences of LU
    against LAPACK), so the final state and covariance may differ by that much per updated frame: 3 x 2.8e-10."""
    scene, T = _room(synth)
    rng = np.random.default_rng(31)
    frames = []
    t = 50.0
    for f in range(7):
        n = 8 if f < 3 else 20
        imu = case.samples(rng, n, t0=t)
        imu[:, 1:4] = np.array([0.0, 0.0, 9.81]) + 0.01 * rng.normal(size=(n, 3))
        imu[:, 4:7] = 0.002 * rng.normal(size=(n, 3))
        sc, ex = synth.livox_scan(scene, T, 2000, 900 + f, point_filter_num=1)
        frames.append((synth.custom_msg(sc, ex), imu, t + 0.001, imu[-1, 0] + 0.001))
        t = imu[-1, 0]

    def host_propagate(st, imu, t_beg, t_end, x, P):
        s = PR.default_imu_state(**{k: np.array(getattr(st, k)[:]) for k in pcm.registration.IMU_STATE_VECTORS},
                                 last_lidar_end_time=st.last_lidar_end_time, init_iter_num=st.init_iter_num, first_frame=st.first_frame, need_init=st.need_init,
                                 last_imu=[st.last_imu.t] + list(st.last_imu.acc) + list(st.last_imu.gyr))
        s2, x2, P2, poses = PR.propagate(s, imu, t_beg, t_end, x, P)
        st.angvel_last[:] = list(s2["angvel_last"]); st.acc_s_last[:] = list(s2["acc_s_last"])
        st.last_lidar_end_time = s2["last_lidar_end_time"]
        st.last_imu.t = s2["last_imu"][0]; st.last_imu.acc[:] = list(s2["last_imu"][1:4]); st.last_imu.gyr[:] = list(s2["last_imu"][4:7])
        return x2, P2, poses

    x0 = ref.make_state()        # the world frame is the first body frame, as in the reference (the first scan enters the map untransformed)
    runs = []
    for prop in (None, host_propagate):
        g = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)
        od = pcm.LioOdometry(g, x=x0, filter_size_map=0.5, propagate=prop, num_scans=6, point_filter_num=1, blind=0.1, leaf_size=0.5)
        stages, counters = [], []
        for msg, imu, tb, te in frames:
            stages.append(od.process(msg, imu, tb, te))
            if stages[-1] == "updated":
                r = od.last_update
                counters.append((r.iterations, r.rematches, r.valid_calls, r.t, r.n_eff_last))
        runs.append((stages, counters, ref.state_to_vec(od.x), od.P, len(g.get_target()), od.ekf_inited))
    a, b = runs
    assert a[0] == b[0] == ["init"] * 3 + ["first_scan"] + ["updated"] * 3
    assert a[1] == b[1] and all(c[2] >= 1 for c in a[1]) and a[4] == b[4] > 1000 and a[5] and b[5]
    print("odometry counters", a[1], "state rel %.2e P rel %.2e" % (PR.rel(a[2], b[2]), PR.rel(a[3], b[3])))
    assert PR.rel(a[2], b[2]) <= 3 * 2.8e-10 and PR.rel(a[3], b[3]) <= 3 * 2.8e-10
