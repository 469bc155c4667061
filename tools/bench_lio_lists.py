"""The jueying_lio frame loop of tools/bench_lio_loop.py (BASELINE configs[4]) with and without PCM_FLAG_FOLLOWING_LISTS, i.e. with the
measurement model on k_lio_lists or on the tile kernel, in three settings:
  leaf05      0.5 m voxels, the reference's 0.5 m scan filter (filter_size_surf)
  unfiltered  0.5 m voxels, every point of the 100 k-point frame is matched
  livox02     the Livox parameters of the reference (config/livox.yaml:42-47): 0.2 m voxels, NEARBY26 = num_neighbors 27, 0.5 m scan filter
One frame = lio_frame_begin, obs_model(rematch) -- which also brings the map and, with the flag, the lists up to date --, three
obs_model without matching, lio_frame_end.  Per setting: median ms per stage with [min, max], the last list update by stage from HIP
events (pcm_neighbour_list_update_ms; a pass of its own over the last frames), the pool's bytes, lio_search_path.
  python tools/bench_lio_lists.py --label parent --root <checkout of the parent commit>      (the yardstick; it knows no flag path)
  python tools/bench_lio_lists.py --label new
  python tools/bench_lio_lists.py --label new_flag --flag
Each run adds (or, with --append-run, appends a further run to) its label in --out (default profiles/lio_lists_bench.json).  Reads
nothing outside the repository; --time-limit bounds the whole run (checked between frames)."""
import argparse
import importlib
import json
import os
import sys
import time

ap = argparse.ArgumentParser()
ap.add_argument("--label", required=True)
ap.add_argument("--flag", action="store_true", help="PCM_FLAG_FOLLOWING_LISTS")
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout whose package and library are measured")
ap.add_argument("--out", default=None)
ap.add_argument("--settings", default="leaf05,unfiltered,livox02")
ap.add_argument("--map", type=int, default=5_000_000)
ap.add_argument("--scan", type=int, default=100_000)
ap.add_argument("--frames", type=int, default=40)
ap.add_argument("--capacity", type=int, default=1_000_000)
ap.add_argument("--time-limit", type=float, default=540.0, help="seconds for the whole run")
a = ap.parse_args()
T_START = time.perf_counter()
sys.path.insert(0, os.path.abspath(a.root))
import numpy as np  # noqa: E402
from scipy.spatial.transform import Rotation as R  # noqa: E402
import torch  # noqa: E402
import pointcloud_slam_amd as pcm  # noqa: E402

synth = importlib.import_module("pointcloud-slam_amd.synth")
FOLLOWING_LISTS = 128
SETTINGS = {"leaf05": dict(res=0.5, leaf=0.5), "unfiltered": dict(res=0.5, leaf=0.0), "livox02": dict(res=0.2, leaf=0.5)}

scene = synth.scene_for_points(1234, a.map, 8.0)
submap = synth.sample_submap(scene, a.map, 4321)
T0 = synth.sensor_pose(scene, 77)
msgs, states = [], []
for f in range(a.frames):
    T = T0.copy(); T[:3, 3] += T[:3, 0] * 0.25 * f        # 5 m/s at 20 Hz
    sc, ex = synth.livox_scan(scene, T, a.scan, 555 + f, point_filter_num=1)
    msgs.append(synth.custom_msg(sc, ex))
    states.append((R.from_matrix(T[:3, :3]).as_quat(), T[:3, 3].copy(), np.array([0, 0, 0, 1.0]), np.zeros(3)))
K = 11
poses = np.zeros((K, 22)); vel = T0[:3, 0] * 5.0
for k in range(K):
    poses[k, 0] = 0.01 * k; poses[k, 7:10] = vel; poses[k, 10:13] = vel * 0.01 * k; poses[k, 13:22] = np.eye(3).ravel()
d_submap = torch.from_numpy(submap).cuda()


def spread(v):
    v = np.asarray(v, np.float64) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "n": len(v)}


def out_of_time():
    return time.perf_counter() - T_START > a.time_limit


def run(name):
    s = SETTINGS[name]
    g = pcm.P2PlaneRegistration(0, voxel_resolution=s["res"], num_neighbors=27, map_capacity=a.capacity, flags=FOLLOWING_LISTS if a.flag else 0)
    kw = dict(num_scans=6, point_filter_num=1, blind=0.1, leaf_size=s["leaf"])
    t0 = time.perf_counter()
    g.set_input_target(d_submap)
    g.lio_frame_begin(msgs[0], poses, *states[0], **kw); g.obs_model(*states[0], False, True); torch.cuda.synchronize()
    t_first = time.perf_counter() - t0
    g.lio_frame_end(*states[0], 0.5, True)
    per = {k: [] for k in ("frame_begin", "match", "update", "frame_end", "frame")}
    cnt = {k: [] for k in ("added", "n_eff", "scan_points")}
    stages = {}
    timed_tail = 3 if a.flag else 0          # the last frames run under set_profiling(1) and are not part of the stage medians
    done = 0
    for f in range(1, a.frames):
        if out_of_time():
            break
        prof = a.flag and f >= a.frames - timed_tail
        g.set_profiling(1 if prof else 0)
        tf = time.perf_counter()
        t = time.perf_counter(); n = g.lio_frame_begin(msgs[f], poses, *states[f], **kw); tb = time.perf_counter() - t
        t = time.perf_counter(); H, h, ne, s2, ok = g.obs_model(*states[f], False, True); tm = time.perf_counter() - t   # includes the map and list update
        t = time.perf_counter()
        for _ in range(3):
            g.obs_model(*states[f], False, False)
        tu = time.perf_counter() - t
        t = time.perf_counter(); added = g.lio_frame_end(*states[f], 0.5, True); te = time.perf_counter() - t
        tfr = time.perf_counter() - tf
        if prof:
            for key, v in g.neighbour_list_update_ms().items():
                stages.setdefault(key, []).append(v * 1e-3)
            continue
        for key, v in (("frame_begin", tb), ("match", tm), ("update", tu), ("frame_end", te), ("frame", tfr)):
            per[key].append(v)
        cnt["added"].append(added); cnt["n_eff"].append(ne); cnt["scan_points"].append(n)
        done += 1
    g.set_profiling(0)
    res = {"voxel_resolution": s["res"], "leaf_size": s["leaf"], "num_neighbors": 27, "frames_timed": done, "first_frame_s": t_first}
    res.update({k: spread(v) for k, v in per.items() if v})
    res.update({k: float(np.median(v)) for k, v in cnt.items() if v})
    st = g.stats()
    res["target_voxels"] = int(st["target_voxels"]); res["map_points_end"] = int(len(g.get_target()))
    if hasattr(g, "lio_search_path"):
        res["lio_search_path"] = list(g.lio_search_path())
    if a.flag:
        info = g.neighbour_list_info()
        res["list_info_end"] = info
        res["pool_bytes"] = info["capacity"] * 16
        res["list_update_by_stage"] = {k: spread(v) for k, v in stages.items()}
    return res


doc_run = {"flag": bool(a.flag), "map_points": a.map, "scan_points": a.scan, "frames": a.frames, "capacity": a.capacity, "settings": {}}
for name in a.settings.split(","):
    if out_of_time():
        doc_run["settings"][name] = "not run: time limit"
        continue
    doc_run["settings"][name] = run(name)
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "lio_lists_bench.json")
doc = {}
if os.path.exists(out_path):
    with open(out_path) as f:
        doc = json.load(f)
doc.setdefault(a.label, []).append(doc_run)
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps({a.label: doc_run}))
