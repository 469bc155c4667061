"""Loop-verification benchmark (pcm_loam_loop_verify / pcm_loam_submap_near_dev): K key frames of n_corner / n_surf points on the
synth_keyframes lawn-mower, the pair (K - 1, K // 2), search_num 25, default leaf (0.2 m) and NDT settings.  Times, in one process
on the same context, alternating the two paths run by run:
  (i)   verify_ms               loop_verify (both near clouds, gates, NDT, fitness, pose algebra; one call)
  (ii)  host_composition_ms     the path it replaces: near_keyframes x 2 (host) -> PclNdtRegistration.set_input_target / source ->
                                align -> get_fitness_score -> the restatement's pose algebra
  (iii) near_dev_ms / near_host_ms   submap_near_device into a device tensor against near_keyframes, for the previous cloud; both
                                are the same device pass, so near_host_ms is that pass plus the copy of the result to the host
                                (and near_keyframes' count queries)
Every timed call ends in a wait on the device (the count read-back, the NDT result or the fitness score), so the host clock is
the call's time.  Medians of --runs after a warm-up of every path.  Also checks that both paths give the same correction and
fitness.  Prints one JSON line.
Usage: python tools/bench_loam_loop.py [--runs 7] [--keyframes 100] [--out FILE]"""
import argparse
import importlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=100)
    ap.add_argument("--n-corner", type=int, default=2000, help="corner features per key frame (a 16 x 1800 scan gives about this many)")
    ap.add_argument("--n-surf", type=int, default=8000)
    ap.add_argument("--search-num", type=int, default=25)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import loam_loop_ref as R
    synth_keyframes = importlib.import_module("pointcloud-slam_amd.synth_keyframes")
    K = a.keyframes
    kf = synth_keyframes.make_keyframes(0, K, a.n_corner, a.n_surf)
    g = pcm.LoamRegistration(0)
    for k in range(K):
        g.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k])
    key_cur, key_pre = K - 1, K // 2
    params = dict(history_search_num=a.search_num)
    ndt = pcm.PclNdtRegistration(0, translation_eps=R.DEFAULTS["ndt_epsilon"])

    def verify():
        return g.loop_verify(key_cur, key_pre, **params)

    def composition():
        cur = g.near_keyframes(key_cur, 0, -1, R.DEFAULTS["near_leaf"])
        prev = g.near_keyframes(key_pre, a.search_num, -1, R.DEFAULTS["near_leaf"])

        def run():
            ndt.set_input_target(prev)
            ndt.set_input_source(cur)
            r = ndt.align()
            return r.converged, r.iterations, r.T, ndt.get_fitness_score()

        return R.perform_loop_closure(len(cur), len(prev), run, kf.poses[key_cur], kf.poses[key_pre], params)

    n_in = sum(len(kf.corner[k]) + len(kf.surf[k]) for k in range(max(0, key_pre - a.search_num), min(K, key_pre + a.search_num + 1)))
    dev = torch.empty((n_in, 4), dtype=torch.float32, device="cuda:0")

    def near_dev():
        return g.submap_near_device(key_pre, a.search_num, -1, R.DEFAULTS["near_leaf"], dev)

    def near_host():
        return len(g.near_keyframes(key_pre, a.search_num, -1, R.DEFAULTS["near_leaf"]))

    for _ in range(2):   # warm-up of every path
        v = verify(); c = composition(); nd = near_dev(); nh = near_host()
    assert nd == nh
    same = bool(np.array_equal(v.correction, c["correction"]) and v.fitness == c["fitness"] and v.iterations == c["iterations"]
                and R.STATUS_NAMES[c["status"]] == v.status)
    ts = {"verify_ms": [], "host_composition_ms": [], "near_dev_ms": [], "near_host_ms": []}
    for _ in range(a.runs):   # alternating, so that drift of the shared host hits both alike
        for name, f in (("verify_ms", verify), ("host_composition_ms", composition), ("near_dev_ms", near_dev), ("near_host_ms", near_host)):
            t = time.perf_counter()
            f()
            ts[name].append((time.perf_counter() - t) * 1e3)
    out = {"runs": a.runs, "keyframes": K, "n_corner": a.n_corner, "n_surf": a.n_surf, "search_num": a.search_num, "pair": [key_cur, key_pre],
           "status": v.status, "num_cur_points": v.num_cur_points, "num_prev_points": v.num_prev_points, "prev_points_in": n_in,
           "ndt_iterations": v.iterations, "fitness": v.fitness, "same_result_as_host_composition": same}
    for name, v_ in ts.items():
        out[name] = float(np.median(v_))
        out[name.replace("_ms", "_min_ms")] = float(np.min(v_))
        out[name.replace("_ms", "_max_ms")] = float(np.max(v_))
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
