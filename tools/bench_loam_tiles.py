"""Localisation-tile benchmark (pcm_loam_tiles_build): K key frames of n_corner / n_surf points on the lawn-mower of
tools/bench_loam_global.py (12 m between key frames and between lanes).  Per leaf pair, on one store in one process:
  (i)  build_tiles: device events around the call and the host clock (the call ends in a synchronise), and the per-stage split
       of build_tiles_ms (device events at the stage boundaries inside the call; workspace_host is host time);
  (ii) the route a caller had without it: export_map of each list to the host, the numpy partition and per-tile VoxelGrid of
       tests/loam_tiles_ref.py, add_tile per tile.
Medians of --runs after a warm-up (the host route: --host-runs).  Prints one JSON line; --out writes it to a file as well.
Usage: python tools/bench_loam_tiles.py [--runs 7] [--host-runs 3] [--keyframes 2000] [--points 10000] [--tile 50] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F = np.float32


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--host-runs", type=int, default=3)
    ap.add_argument("--keyframes", type=int, default=2000)
    ap.add_argument("--points", type=int, default=10000)
    ap.add_argument("--tile", type=float, default=50.0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import bench_loam_global as BG
    import loam_tiles_ref as TR

    n_corner = a.points // 5
    poses, clouds = BG.make_store(a.keyframes, n_corner, a.points - n_corner)
    g = pcm.LoamRegistration(0)
    for k in range(a.keyframes):
        g.add_keyframe(poses[k], 100.0 + 0.7 * k, clouds[k % 8][0], clouds[k % 8][1])
    out = {"bench": "loam_tiles", "keyframes": a.keyframes, "points_per_keyframe": a.points, "tile_size": a.tile, "runs": a.runs, "host_runs": a.host_runs,
           "device": torch.cuda.get_device_name(0), "cases": []}
    for leaf in (0.0, 0.2):
        kw = dict(tile_size=a.tile, leaf_corner=leaf, leaf_surf=leaf)
        r = g.build_tiles(**kw)   # warm-up
        wall, dev = [], []
        for _ in range(a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            t = time.perf_counter()
            e0.record()
            g.build_tiles(**kw)
            e1.record()
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t) * 1e3)
            dev.append(e0.elapsed_time(e1))

        def host_route():
            h_times = {}
            t0 = time.perf_counter()
            clouds_h = [g.export_map(w) for w in (0, 1)]
            t1 = time.perf_counter()
            cut = [TR.cut(c, a.tile, leaf)[0] for c in clouds_h]
            t2 = time.perf_counter()
            g.clear_tiles()
            for w in (0, 1):
                for t in cut[w]:
                    g.add_tile(w, t.box, t.points)
            t3 = time.perf_counter()
            h_times.update(export_ms=(t1 - t0) * 1e3, cut_ms=(t2 - t1) * 1e3, upload_ms=(t3 - t2) * 1e3, total_ms=(t3 - t0) * 1e3)
            return h_times

        host_route()
        hs = [host_route() for _ in range(a.host_runs)]
        splits = [g.build_tiles_ms(**kw) for _ in range(a.runs)]

        def med(f):
            return float(np.median([f(x) for x in splits]))

        split = {name: {k: med(lambda x, name=name, k=k: x[name][k]) for k in splits[0][name]} for name in ("corner", "surf")}
        split["gather"], split["arena_copy"] = med(lambda x: x["gather"]), med(lambda x: x["arena_copy"])
        case = {"leaf": leaf, "stage_ms": split, "tiles": [r.num_corner_tiles, r.num_surf_tiles], "points_in": r.corner_points_in + r.surf_points_in,
                "points_out": r.corner_points_out + r.surf_points_out, "build_tiles_wall_ms": float(np.median(wall)), "build_tiles_device_ms": float(np.median(dev)),
                "host_route_ms": {k: float(np.median([h[k] for h in hs])) for k in hs[0]}}
        case["host_over_device"] = case["host_route_ms"]["total_ms"] / case["build_tiles_wall_ms"]
        out["cases"].append(case)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(json.dumps(out, indent=1) + "\n")


if __name__ == "__main__":
    main()
