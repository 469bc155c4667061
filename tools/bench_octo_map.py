"""3D occupancy map benchmark (pcm_octo_*).  On one device in one process:
  (i)   the reference's cloud_to_map route: the synthetic mapping session of tools/bench_loam_global.py (K key frames of 2 000 + 8 000
        points on a lawn-mower), exported, down-sampled at 0.1 m and cut to pcd2map's z window, then inserted as one scan from the
        world origin at resolution 0.1 with max_range 1000 out of a device buffer: the insert with a table that is large enough
        (mark + apply + fold, one wait), the insert that starts from the default table (growth included), the projection, the
        sorted cells;
  (ii)  key-frame insertion in place: 100 key frames of 10 000 points;
  (iii) the host restatement (tests/octo_map_ref.py) on a 1/100 sample of (i), once, for scale only.
  (iv)  the phases of (i) by device events (pcm_octo_debug / pcm_octo_phase_ms): mark and apply + fold apart, for the mark kernel
        with one ray per lane, with one ray per wave, and, to price the dry walk, one ray per lane without it; and the phases of
        the insert that grows the table from the default.
Medians of --runs after a warm-up; host clocks around calls that end in a synchronise.  Prints one JSON line.
Usage: python tools/bench_octo_map.py [--runs 7] [--keyframes 100] [--out profiles/octo_map_bench.json]"""
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


def timed(f):
    t = time.perf_counter()
    r = f()
    return (time.perf_counter() - t) * 1e3, r


def note(*a):
    print(*a, file=sys.stderr, flush=True)


def median_ms(f, runs):
    f()
    return float(np.median([timed(f)[0] for _ in range(runs)]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=100)
    ap.add_argument("--z-window", type=float, nargs=2, default=[-1.0, 3.0])
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    from pointcloud_slam_amd import octo
    import octo_map_ref as R
    from bench_loam_global import make_store
    out = {"runs": a.runs}

    # (i) the saved map
    poses, clouds = make_store(a.keyframes, 2000, 8000)
    g = pcm.LoamRegistration(0)
    for k in range(a.keyframes):
        g.add_keyframe(poses[k], 100.0 + 0.7 * k, *clouds[k % 8])
    whole = g.export_map("both")
    ds = pcm.P2PlaneRegistration(0).voxel_downsample(whole, 0.1)
    z = ds[:, 2] - F(5.0)                                    # the session runs 5 m above the world origin
    cloud = np.ascontiguousarray(np.concatenate([ds[:, :2], z[:, None], np.zeros((len(ds), 1), F)], axis=1)[(z >= a.z_window[0]) & (z <= a.z_window[1])])
    dev = torch.from_numpy(cloud).to("cuda:0")
    row = {"keyframes": a.keyframes, "points_exported": int(len(whole)), "points_inserted": int(len(cloud))}
    P = dict(resolution=0.1, max_range=1000.0, max_cells=1 << 28)
    m = octo.OccupancyMap3D(0, initial_cells=1 << 16, **P)
    first_ms, r = timed(lambda: m.insert_scan(dev, (0.0, 0.0, 0.0)))
    runs = a.runs if first_ms < 4000.0 else 3
    note("first insert", first_ms, "ms", r)
    row.update(runs_used=runs, cells=int(r["cells_touched"]), table_growths_from_default=int(r["table_growths"]), rejected_rays=int(r["rejected_rays"]))
    room = 1 << int(np.ceil(np.log2(max(2, r["cells_touched"]))))

    def insert(initial):
        m.reset(initial_cells=initial, **P)
        return m.insert_scan(dev, (0.0, 0.0, 0.0))

    row["insert_no_growth_ms"] = median_ms(lambda: insert(room), runs)
    row["insert_from_default_table_ms"] = median_ms(lambda: insert(1 << 16), runs)
    note("inserts", row)
    row["growth_ms"] = row["insert_from_default_table_ms"] - row["insert_no_growth_ms"]
    row["reset_ms"] = median_ms(lambda: m.reset(initial_cells=room, **P), runs)

    def phases(variant, initial):
        m.debug(variant, timed=True)
        rows = []
        for _ in range(runs + 1):
            insert(initial)
            rows.append(m.phase_ms())
        m.debug("lane", timed=False)
        return {k: float(np.median([r[k] for r in rows[1:]])) for k in ("mark_ms", "apply_ms", "growth_ms", "mark_passes")}

    row["phases_no_growth"] = {v: phases(v, room) for v in ("lane", "wave", "lane_no_dry_walk")}
    note("phases", row["phases_no_growth"])
    row["phases_from_default_table"] = phases("lane", 1 << 16)
    row["mark_kernel_kept"] = "one ray per lane" if row["phases_no_growth"]["lane"]["mark_ms"] <= row["phases_no_growth"]["wave"]["mark_ms"] else "one ray per wave is faster here"
    insert(room)
    row["cells_per_second"] = row["cells"] / (row["insert_no_growth_ms"] * 1e-3)

    def project():
        m.insert_scan(dev[:1], (0.0, 0.0, 0.0))            # invalidates the cached projection
        return m.project()

    row["one_point_insert_ms"] = median_ms(lambda: m.insert_scan(dev[:1], (0.0, 0.0, 0.0)), runs)
    row["project_ms"] = median_ms(project, runs) - row["one_point_insert_ms"]
    grid = m.project()
    row.update(grid_width=grid.width, grid_height=grid.height)
    cells_dev = torch.zeros((m.info()["cells"], 4), dtype=torch.float32, device="cuda:0")
    row["sorted_cells_device_ms"] = median_ms(lambda: m.cells(out=cells_dev), runs)
    out["saved_map"] = row
    note("saved map", row)
    del cells_dev

    # (iii) the restatement on a 1/100 sample, once
    sample = cloud[::100]
    ref = R.Map(R.Params(resolution=0.1, max_range=1000.0))
    ms, rr = timed(lambda: ref.insert_scan(sample, (0.0, 0.0, 0.0)))
    ms_dev = median_ms(lambda: (m.reset(initial_cells=room, **P), m.insert_scan(sample, (0.0, 0.0, 0.0))), runs)
    out["host_restatement_sample"] = {"points": int(len(sample)), "cells": int(rr["cells_touched"]), "restatement_ms": ms, "device_ms": ms_dev}

    note("restatement", out["host_restatement_sample"])
    # (ii) key frames in place
    K = 100
    poses, clouds = make_store(K, 2000, 8000, seed=1)
    g2 = pcm.LoamRegistration(0)
    for k in range(K):
        g2.add_keyframe(poses[k], 100.0 + 0.7 * k, *clouds[k % 8])

    def keyframes():
        octo.octo_reset(g2, resolution=0.1, initial_cells=1 << 23)
        octo.octo_insert_keyframes(g2, 0, K)

    kms = median_ms(keyframes, runs)
    info = octo.octo_info(g2)
    out["keyframes"] = {"keyframes": K, "points": K * 10000, "insert_ms": kms, "cells": info["cells"], "ms_per_keyframe": kms / K}
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
