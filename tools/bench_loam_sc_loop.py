#!/usr/bin/env python3
"""Point-to-point ICP and the Scan Context loop verification on the device, timed.

    python tools/bench_loam_sc_loop.py            # writes profiles/loam_sc_loop_bench.json

1. One ICP (PCM_MODEL_ICP, PCL's defaults but 30 iterations): 10 k source points against a 250 k-point target, host buffers.
2. An SC verification (pcm_loam_sc_loop_verify) on the workload of section 19: K = 100 key frames of 10 000 features,
   history_search_num 25 -- against the host composition it replaces: submap_near to the host twice, then the same ICP from
   host buffers in a separate context, then its fitness score.
Medians of 7 after one warm-up.  Nothing is promised about the ratio: the figures are what was measured."""
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPS = 7


def median_ms(f):
    import torch
    f()
    ts = []
    for _ in range(REPS):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        f()
        torch.cuda.synchronize()
        ts.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ts), ts


def rigid(rz, t):
    c, s = np.cos(rz), np.sin(rz)
    M = np.eye(4)
    M[:2, :2] = [[c, -s], [s, c]]
    M[:3, 3] = t
    return M


def main():
    import pointcloud_slam_amd as pcm
    from pointcloud_slam_amd import icp, loam
    synth_keyframes = importlib.import_module("pointcloud-slam_amd.synth_keyframes")
    out = {"reps": REPS}
    # ---- 1. one ICP, 10 k against 250 k ----
    rng = np.random.default_rng(1)
    tgt = rng.uniform(-50.0, 50.0, (250000, 3)).astype(np.float32)
    tgt[:, 2] *= 0.1
    M = np.linalg.inv(rigid(0.01, [0.2, -0.1, 0.05]))
    src = (tgt[rng.permutation(len(tgt))[:10000]].astype(np.float64) @ M[:3, :3].T + M[:3, 3] + rng.normal(0, 0.02, (10000, 3))).astype(np.float32)
    g = icp.IterativeClosestPoint(0, max_iterations=30)
    g.set_input_target(tgt)
    g.set_input_source(src)
    med, ts = median_ms(lambda: g.align())
    r = g.align()
    out["icp_10k_vs_250k"] = {"align_ms": med, "all_ms": ts, "iterations": r.iterations, "stop_reason": r.stop_reason, "num_pairs": r.num_pairs, "mse": r.mse}
    med, ts = median_ms(lambda: g.get_fitness_score())
    out["icp_10k_vs_250k"]["fitness_ms"] = med
    # ---- 2. SC verification, K = 100 key frames of 10 000 features ----
    kf = synth_keyframes.make_keyframes(0, 100, 2000, 8000)   # tools/bench_loam_loop.py's store
    L = pcm.LoamRegistration(0)
    for k in range(len(kf.times)):
        L.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k])
    cur_key, pre_key = len(kf.times) - 1, len(kf.times) // 2
    params = dict(history_search_num=25)
    first = loam.loam_sc_loop_verify(L, cur_key, pre_key, **params)
    med, ts = median_ms(lambda: loam.loam_sc_loop_verify(L, cur_key, pre_key, **params))
    out["sc_loop_verify"] = {"device_ms": med, "all_ms": ts, "status": first.status, "num_cur_points": first.num_cur_points, "num_prev_points": first.num_prev_points,
                             "icp_iterations": first.icp_iterations, "fitness": first.fitness}
    v = icp.IterativeClosestPoint(0, voxel_resolution=1.0, max_iterations=100, max_correspondence_distance=150.0, transformation_epsilon=1e-6,
                                  euclidean_fitness_epsilon=1e-6)

    def host_composition():
        cur = L.near_keyframes(cur_key, 0, 0, 0.2)
        prev = L.near_keyframes(pre_key, 25, 0, 0.2)
        v.set_input_target(prev)
        v.set_input_source(cur)
        rr = v.align()
        return rr, v.get_fitness_score()

    rr, fit = host_composition()
    med, ts = median_ms(host_composition)
    out["sc_loop_verify"].update({"host_composition_ms": med, "host_all_ms": ts, "same_correction": bool(np.array_equal(rr.T, first.correction)), "same_fitness": fit == first.fitness})
    path = os.path.join(ROOT, "profiles", "loam_sc_loop_bench.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(out))


if __name__ == "__main__":
    main()
