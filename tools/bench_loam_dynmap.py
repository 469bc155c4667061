"""LOAM localisation map benchmark (pcm_loam_dynmap_load / pcm_loam_dynmap_crop): a 7 x 7 grid of 40 m area tiles per list, of which the
margin selects 5 x 5 around the pose; the working set (points of the selected tiles) is about 2 M corner + 8 M surf points, and a
second, smaller one a tenth of that.  A rebuild is forced by moving pose_y by a centimetre, which moves the window and changes
no work.  Per size: crop_ms (rebuilt), crop_unchanged_ms, crop_plus_grids_1iter_ms (the crop, the grid build and one scan2map
iteration), load_ms; beside them, on the same inputs in the same process, the frame a caller has without the feature: a numpy mask
over the host-held working set, set_input_target with a new tag, the same grid build and iteration (parent_path_plus_grids_1iter_ms,
and its parts), and the numpy restatement's time.  Medians of --runs after a warm-up.  The reference's PCL node cannot be built here
(no PCL), so no reference time is reported.  Prints one JSON line.
Usage: python tools/bench_loam_dynmap.py [--runs 7] [--out FILE]; --trace runs nothing but rebuilt crops of the large working set,
for a kernel trace whose rows all belong to this path."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

CELL, GRID = 40.0, 7
F = np.float32


def median_ms(f, runs, before=None):
    ts = []
    for _ in range(runs):
        if before:
            before()
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def make_grid(rng, per_tile):
    boxes, tiles = [], []
    for j in range(GRID):
        for i in range(GRID):
            t = np.empty((per_tile, 4), F)
            t[:, 0] = rng.uniform(i * CELL, (i + 1) * CELL, per_tile)
            t[:, 1] = rng.uniform(j * CELL, (j + 1) * CELL, per_tile)
            t[:, 2] = rng.uniform(0.0, 6.0, per_tile)
            t[:, 3] = rng.uniform(0.0, 255.0, per_tile)
            boxes.append(np.array([i * CELL, j * CELL, 0.0, (i + 1) * CELL, (j + 1) * CELL, 6.0]))
            tiles.append(t)
    return np.asarray(boxes), tiles


def bench(pcm, R, runs, n_corner, n_surf, no_cpu, trace):
    rng = np.random.default_rng(0)
    lists = (make_grid(rng, n_corner // 25), make_grid(rng, n_surf // 25))
    g = pcm.LoamRegistration(0)
    for which, (boxes, tiles) in enumerate(lists):
        for b, t in zip(boxes, tiles):
            g.add_tile(which, b, t)
    centre = 0.5 * GRID * CELL
    p = dict(margin=80, area_size=50, max_range=50.0)
    k = [0]

    def pose():
        return np.array([0, 0, 0, centre, centre + 0.01 * (k[0] % 50), 1.5], F)

    def move():
        k[0] += 1

    ld = g.load_map(pose(), **p)
    assert ld.num_corner_selected == 25 and ld.num_surf_selected == 25
    if trace:
        for _ in range(runs + 2):
            move()
            assert g.crop_map(pose(), **p).rebuilt
        return None
    sels = (R.select(lists[0][0], centre, centre, 80), R.select(lists[1][0], centre, centre, 80))
    host_c, host_s = R.concat(lists[0][1], sels[0]), R.concat(lists[1][1], sels[1])   # what the caller keeps on the host today
    near_c = host_c[np.abs(host_c[:, :2] - centre).max(axis=1) < 25.0][:1500].copy()
    near_s = host_s[np.abs(host_s[:, :2] - centre).max(axis=1) < 25.0][:6000].copy()
    near_c[:, :3] -= np.array([centre, centre, 1.5], F); near_s[:, :3] -= np.array([centre, centre, 1.5], F)
    g.set_input_source(near_c, near_s)
    for _ in range(2):   # warm-up
        move(); g.crop_map(pose(), **p); g.scan2map(pose(), iter_num=1)
    move()
    r = g.crop_map(pose(), **p)
    assert r.rebuilt
    row = {"points_in": r.num_corner_in + r.num_surf_in, "points_kept": r.num_corner + r.num_surf}
    row["crop_ms"] = median_ms(lambda: g.crop_map(pose(), **p), runs, before=move)
    row["crop_plus_grids_1iter_ms"] = median_ms(lambda: (g.crop_map(pose(), **p), g.scan2map(pose(), iter_num=1)), runs, before=move)
    g.crop_map(pose(), **p)
    row["crop_unchanged_ms"] = median_ms(lambda: g.crop_map(pose(), **p), runs)
    row["scan2map_1iter_ms"] = median_ms(lambda: g.scan2map(pose(), iter_num=1), runs)
    row["load_ms"] = median_ms(lambda: g.load_map(pose(), **p), runs)
    # the caller's frame without the feature
    h = pcm.LoamRegistration(0)
    h.set_input_source(near_c, near_s)
    tag = [1]
    parts = {"mask": [], "upload": []}

    def parent():
        tag[0] += 1
        x = pose()
        t0 = time.perf_counter()
        lo, hi = R.limits(x[4], 50.0)
        c = host_c[(lo <= host_c[:, 1]) & (host_c[:, 1] <= hi)]
        s = host_s[(lo <= host_s[:, 1]) & (host_s[:, 1] <= hi)]
        t1 = time.perf_counter()
        h.set_input_target(c, s, tag=tag[0])
        t2 = time.perf_counter()
        h.scan2map(x, iter_num=1)
        parts["mask"].append((t1 - t0) * 1e3); parts["upload"].append((t2 - t1) * 1e3)

    move(); parent(); move(); parent()
    parts = {"mask": [], "upload": []}
    row["parent_path_plus_grids_1iter_ms"] = median_ms(parent, runs, before=move)
    row["parent_numpy_mask_ms"] = float(np.median(parts["mask"]))
    row["parent_set_input_target_ms"] = float(np.median(parts["upload"]))
    row["parent_over_new"] = row["parent_path_plus_grids_1iter_ms"] / row["crop_plus_grids_1iter_ms"]
    if not no_cpu:
        t = time.perf_counter()
        R.crop(lists, sels, pose(), 50.0, 80, 0)
        row["numpy_restatement_ms"] = (time.perf_counter() - t) * 1e3
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--trace", action="store_true", help="only rebuilt crops of the large working set (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pointcloud_slam_amd as pcm
    import loam_dynmap_ref as R
    if a.trace:
        bench(pcm, R, a.runs, 2000000, 8000000, True, True)
        return
    out = {"runs": a.runs, "tile_grid": GRID, "tile_size_m": CELL, "selected": "5 x 5"}
    for name, (nc, ns) in (("large", (2000000, 8000000)), ("small", (200000, 800000))):
        out[name] = bench(pcm, R, a.runs, nc, ns, a.no_cpu, False)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
