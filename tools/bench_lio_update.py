"""jueying_lio frame loop with the iterated Kalman update in the path: the synthetic stream of tools/bench_lio_loop.py (20 Hz scans
against a sliding submap), every frame's propagated state = ground truth + the survey's guess perturbation (synth.perturb_pose), P = the
reference's initial covariance (imu_processing.hpp:154-161).  Two drivers of the same frames, each on its own registration object:
  device   pcm_lio_frame_begin -> pcm_lio_update (every ObsModel call and the 23 x 23 algebra on the device, one synchronisation)
           -> pcm_lio_frame_end
  host     pcm_lio_frame_begin -> pcm_obs_model x k with the numpy restatement of the filter (tests/lio_iekf_ref.py) between the calls
           -> pcm_lio_frame_end
Reports the median per-frame time of the update step of each and writes profiles/lio_update_bench.json."""
import argparse, importlib, json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
from scipy.spatial.transform import Rotation as R
ap = argparse.ArgumentParser()
ap.add_argument("--map", type=int, default=5_000_000)
ap.add_argument("--scan", type=int, default=100_000)
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--capacity", type=int, default=1_000_000)
ap.add_argument("--leaf", type=float, default=0.0)
ap.add_argument("--max-iter", type=int, default=4)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lio_update_bench.json"))
a = ap.parse_args()
synth = importlib.import_module("pointcloud-slam_amd.synth")
import lio_iekf_ref as ref
scene = synth.scene_for_points(1234, a.map, 8.0)
submap = synth.sample_submap(scene, a.map, 4321)
T0 = synth.sensor_pose(scene, 77)
msgs, truth, guesses = [], [], []
for f in range(a.frames):
    T = T0.copy(); T[:3, 3] += T[:3, 0] * 0.25 * f        # 5 m/s at 20 Hz
    sc, ex = synth.livox_scan(scene, T, a.scan, 555 + f, point_filter_num=1)
    msgs.append(synth.custom_msg(sc, ex))
    truth.append(T)
    G = synth.perturb_pose(T, 99 + f)
    guesses.append(ref.make_state(pos=G[:3, 3], rot=R.from_matrix(G[:3, :3]).as_quat(), grav=(0.0, 0.0, -ref.LENGTH)))
P0 = np.diag(ref.INIT_P_DIAG)
import torch
import pointcloud_slam_amd as pcm
kw = dict(num_scans=6, point_filter_num=1, blind=0.1, leaf_size=a.leaf)


def pose4(x):
    return x["rot"], x["pos"], x["off_R"], x["off_T"]


def err(x, T):
    return float(np.linalg.norm(x["pos"] - T[:3, 3]))


def run(mode):
    g = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27, map_capacity=a.capacity)
    g.set_input_target(torch.from_numpy(submap).cuda())
    per = {k: [] for k in ("update", "frame", "iterations", "rematches", "n_eff_last", "pos_err_before", "pos_err_after")}
    for f in range(a.frames):
        x0 = guesses[f]
        tf = time.perf_counter()
        g.lio_frame_begin(msgs[f], None, *pose4(x0), **kw)
        t = time.perf_counter()
        if mode == "device":
            r = g.lio_update(x0, P0, max_iter=a.max_iter)
            x, it, rm, ne = r.x, r.iterations, r.rematches, r.n_eff_last
        else:
            def h(xx, converge):
                HTH, HTh, n_eff, s2, valid = g.obs_model(*pose4(xx), False, converge)
                return dict(valid=valid, HTH=HTH, HTh=HTh, n_eff=n_eff, sum_h2=s2)
            w = ref.update(x0, P0, h, max_iter=a.max_iter, dense=False)
            x, it, rm, ne = w["x"], w["iterations"], w["rematches"], w["n_eff_last"]
        dt = time.perf_counter() - t
        g.lio_frame_end(*pose4(x), 0.5, True)
        if f:                                               # frame 0 builds the map: not a steady-state frame
            per["update"].append(dt); per["frame"].append(time.perf_counter() - tf); per["iterations"].append(it); per["rematches"].append(rm)
            per["n_eff_last"].append(ne); per["pos_err_before"].append(err(x0, truth[f])); per["pos_err_after"].append(err(x, truth[f]))
    return {k: float(np.median(v)) for k, v in per.items()}


out = {"scan_points": a.scan, "map_points": a.map, "frames_timed": a.frames - 1, "max_iter": a.max_iter,
       "device_loop": run("device"), "host_loop": run("host")}
out["update_ms_device"] = 1e3 * out["device_loop"]["update"]
out["update_ms_host"] = 1e3 * out["host_loop"]["update"]
out["host_over_device"] = out["update_ms_host"] / out["update_ms_device"]
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as fh:
    json.dump(out, fh, indent=1)
print(json.dumps(out, indent=1))
