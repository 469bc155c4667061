"""Scan-to-submap mapping against a target that grows: PCM_FLAG_FOLLOWING_LISTS against the tile kernel a growing
target runs without it.  bench.py's sizes -- a 1 M-point submap, a 100 k-point scan -- and 7 000-point insert batches (the scan's own
points in the world frame, jittered: the voxels a frame touches).  One cycle = pcm_target_insert of a batch + k x pcm_align:
  leg (i)   k = 1   one align per insert
  leg (ii)  k = 10  the key-frame regime
Medians of 7 cycles after 2 warm-up cycles, with min and max.  The run without the flag uses only calls every earlier build has:
  python tools/bench_following_lists.py --label parent --root <checkout of the parent commit>     (the yardstick)
  python tools/bench_following_lists.py --label this_no_flag
  python tools/bench_following_lists.py --label this_flag --flag
Each run adds its label to --out (default profiles/following_lists_bench.json).  With --flag the run also records the update
alone from HIP events by stage (pcm_neighbour_list_update_ms, a pass of its own), the share of runs rewritten in place against
relocated, and the pool's memory."""
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
ap.add_argument("--map", type=int, default=1_000_000)
ap.add_argument("--scan", type=int, default=100_000)
ap.add_argument("--batch", type=int, default=7000)
ap.add_argument("--cycles", type=int, default=7)
ap.add_argument("--warmup", type=int, default=2)
a = ap.parse_args()
sys.path.insert(0, os.path.abspath(a.root))
import numpy as np  # noqa: E402
import pointcloud_slam_amd as pcm  # noqa: E402

synth = importlib.import_module("pointcloud-slam_amd.synth")
FOLLOWING_LISTS = 128
p = synth.make_pair(0, a.scan, a.map)
world = (p.scan[:, :3].astype(np.float64) @ p.T_gt[:3, :3].T + p.T_gt[:3, 3]).astype(np.float32)
rng = np.random.default_rng(1)
order = rng.permutation(len(world))


def batch(j):
    idx = order[(j * a.batch) % len(order):][:a.batch]
    b = np.ones((len(idx), 4), np.float32)
    b[:, :3] = world[idx] + rng.normal(0.0, 0.01, (len(idx), 3)).astype(np.float32)
    return b


def spread(v):
    v = np.asarray(v) * 1e3
    return {"median_ms": float(np.median(v)), "min_ms": float(v.min()), "max_ms": float(v.max()), "cycles": len(v)}


def leg(k):
    """a fresh context per leg: target, one align (the lists of a flagged context are built here), then the cycles"""
    g = pcm.P2PlaneRegistration(0, optimizer="GN", voxel_resolution=0.5, num_neighbors=27, flags=FOLLOWING_LISTS if a.flag else 0)
    g.set_input_target(p.submap); g.set_input_source(p.scan)
    g.align(p.guess)
    t_cycle, t_first, j = [], [], 0
    for c in range(a.warmup + a.cycles):
        b = batch(j); j += 1
        t0 = time.perf_counter()
        g.target_insert(b)
        r = g.align(p.guess)          # the map's merge (and the lists' update) is part of the first align after an insert
        t1 = time.perf_counter()
        for _ in range(k - 1):
            r = g.align(p.guess)
        t2 = time.perf_counter()
        if c >= a.warmup:
            t_cycle.append(t2 - t0); t_first.append(t1 - t0)
    out = {"aligns_per_insert": k, "cycle": spread(t_cycle), "insert_and_first_align": spread(t_first), "iterations_last": int(r.iterations), "inliers_last": int(r.num_inliers)}
    if a.flag:
        out["list_info"] = g.neighbour_list_info()
    return g, out, j


res = {"flag": bool(a.flag), "map_points": a.map, "scan_points": a.scan, "batch_points": a.batch}
g1, res["leg_i"], _ = leg(1)
del g1
g, res["leg_ii"], j = leg(10)
if a.flag:   # the update alone, by stage, from HIP events: a pass of its own (the events cost a synchronisation)
    g.set_profiling(1)
    stages = {}
    for c in range(a.cycles):
        g.target_insert(batch(j)); j += 1
        g.evaluate_cost(p.T_gt)
        for name, v in g.neighbour_list_update_ms().items():
            stages.setdefault(name, []).append(v * 1e-3)
    g.set_profiling(0)
    info = g.neighbour_list_info()
    moved = info["in_place"] + info["relocated"]
    res["update_by_stage"] = {name: spread(v) for name, v in stages.items()}
    res["in_place_share"] = info["in_place"] / moved if moved else None
    res["list_info_end"] = info
    res["pool_bytes"] = info["capacity"] * 16
    res["host_syncs_per_update"] = "1 (the totals); +3 (the index merge's own) when the batch makes new list voxels"
out_path = a.out or os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "following_lists_bench.json")
doc = {}
if os.path.exists(out_path):
    with open(out_path) as f:
        doc = json.load(f)
doc[a.label] = res
os.makedirs(os.path.dirname(out_path), exist_ok=True)
with open(out_path, "w") as f:
    json.dump(doc, f, indent=1)
print(json.dumps({a.label: res}))
