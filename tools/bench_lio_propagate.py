"""pcm_lio_propagate (the forward loop of ImuProcess::UndistortPcl on the device) beside the numpy restatement of the same step
(tests/lio_predict_ref.py) on the same inputs: medians of 7 after a warm-up at n = 20, 100 and 1000 IMU samples, and one 100 k-point
frame end to end (propagate + lio_frame_begin + lio_update + lio_frame_end) with the propagation on the device and with the
restatement on the host.  No host C++ / Eigen build of the reference exists to compare with: the host column is interpreted numpy,
not what a compiled filter would take.  Writes profiles/lio_propagate_bench.json."""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
ap = argparse.ArgumentParser()
ap.add_argument("--map", type=int, default=1_000_000)
ap.add_argument("--scan", type=int, default=100_000)
ap.add_argument("--repeats", type=int, default=7)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lio_propagate_bench.json"))
a = ap.parse_args()
synth = importlib.import_module("pointcloud-slam_amd.synth")
import lio_iekf_ref as ref
import lio_predict_case as case
import lio_predict_ref as PR
import torch
import pointcloud_slam_amd as pcm
from pointcloud_slam_amd.registration import lio_imu_state


def median_ms(fn, repeats):
    fn()                                                    # warm-up
    ts = []
    for _ in range(repeats):
        t = time.perf_counter(); fn(); ts.append(time.perf_counter() - t)
    return 1e3 * float(np.median(ts))


g = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)
out = {"repeats": a.repeats, "propagate_ms": {}, "restatement_ms": {}}
for n in (20, 100, 1000):
    c = case.frame("plain", n)
    out["propagate_ms"][str(n)] = median_ms(lambda: g.lio_propagate(lio_imu_state(**c["s"]), c["imu"], c["beg"], c["end"], c["x"], c["P"]), a.repeats)
    out["restatement_ms"][str(n)] = median_ms(lambda: PR.propagate(c["s"], c["imu"], c["beg"], c["end"], c["x"], c["P"]), a.repeats if n < 1000 else 3)

# one frame end to end: a sensor at rest in the room, 20 IMU samples, the map on the device
scene = synth.scene_for_points(1234, a.map, 8.0)
submap = synth.sample_submap(scene, a.map, 4321)
T = synth.sensor_pose(scene, 77)
sc, ex = synth.livox_scan(scene, T, a.scan, 555, point_filter_num=1)
msg = synth.custom_msg(sc, ex)
from scipy.spatial.transform import Rotation
x0 = ref.make_state(pos=T[:3, 3], rot=Rotation.from_matrix(T[:3, :3]).as_quat())
P0 = np.diag(ref.INIT_P_DIAG)
rng = np.random.default_rng(3)
imu = case.samples(rng, 20)
acc_body = T[:3, :3].T @ np.array([0.0, 0.0, 9.81])
imu[:, 1:4] = acc_body + 0.01 * rng.normal(size=(20, 3)); imu[:, 4:7] = 0.002 * rng.normal(size=(20, 3))
s0 = case.imu_state(rng, mean_acc=acc_body, angvel_last=[0, 0, 0], acc_s_last=[0, 0, 0])
beg, end = case.T0 + 0.001, imu[-1, 0] + 0.001
kw = dict(num_scans=6, point_filter_num=1, blind=0.1, leaf_size=0.5)


def frame(device):
    f = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27, map_capacity=1_000_000)
    f.set_input_target(torch.from_numpy(submap).cuda())
    pose = lambda x: (x["rot"], x["pos"], x["off_R"], x["off_T"])   # noqa: E731

    def once():
        if device:
            x, P, poses = f.lio_propagate(lio_imu_state(**s0), imu, beg, end, x0, P0)
        else:
            _, x, P, poses = PR.propagate(s0, imu, beg, end, x0, P0)
        f.lio_frame_begin(msg, poses, *pose(x), **kw)
        r = f.lio_update(x, P)
        f.lio_frame_end(*pose(r.x), 0.5, True)
    once()                                                  # builds the map's tables: not a steady-state frame
    return median_ms(once, a.repeats)


out["frame_points"] = a.scan
out["map_points"] = a.map
out["frame_ms_device_propagate"] = frame(True)
out["frame_ms_host_restatement"] = frame(False)
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out, indent=1))
