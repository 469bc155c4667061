"""Fleet benchmark of the LOAM localisation map: one tile store shared by B contexts (pcm_loam_tile_share) and their per-frame crops in
one call (pcm_loam_dynmap_crop_batch).  The map is tools/bench_loam_dynmap.py's: a 7 x 7 grid of 40 m area tiles per list, of which the
margin selects 5 x 5 around a pose; the working set (points of the selected tiles) is about 2 M corner + 8 M surf points, and a second
one a tenth of that.  For B in 1, 8, 32, in one process:
  set-up   B owners (each uploads the whole map: what a fleet pays without sharing) against 1 owner + B - 1 sharers: wall time and
           device memory in use afterwards (hipMemGetInfo through torch);
  crop     B forced-rebuild crops (every robot at its own pose, moved by a centimetre per sample, which moves the windows and changes
           no work) as a loop of single crop_map calls against one loam_crop_map_batch, on the same shared fleet, samples
           interleaved: median, minimum and maximum of --runs after a warm-up.  Both are one code path (a single crop is a round of
           one context): the loop pays the round's upload, four launches, read-back and wait once per context, the batch once;
  identity every target of the two ways at one pose, compared on the device bit for bit; a difference fails the run.
Prints one JSON line (and writes it to --out).  --trace runs nothing but batched crops of --trace-size at B = 32, for a kernel trace
whose rows all belong to this path."""
import argparse
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CELL, GRID = 40.0, 7
F = np.float32
SIZES = {"large": (2000000, 8000000), "small": (200000, 800000)}
P = dict(margin=80, area_size=50, max_range=50.0)
loam = None   # pointcloud_slam_amd.loam, imported by main()


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


def used(torch):
    torch.cuda.synchronize()
    free, total = torch.cuda.mem_get_info()
    return total - free


def owner(pcm, lists):
    g = pcm.LoamRegistration(0)
    for which, (boxes, tiles) in enumerate(lists):
        for b, t in zip(boxes, tiles):
            g.add_tile(which, b, t)
    return g


def destroy(regs):
    for r in regs:
        r.__del__()
    gc.collect()


def poses(B, k):
    """robot i at sample k: the centre, 0.37 m apart in y, moved by a centimetre per sample"""
    centre = 0.5 * GRID * CELL
    x = np.zeros((B, 6), F)
    x[:, 3] = centre
    x[:, 4] = centre + 0.37 * np.arange(B) + 0.01 * (k % 50)
    x[:, 5] = 1.5
    return x


def stats(ts):
    return {"median_ms": float(np.median(ts)), "min_ms": float(np.min(ts)), "max_ms": float(np.max(ts))}


def shared_fleet(pcm, lists, B):
    o = owner(pcm, lists)
    fleet = [o]
    for _ in range(B - 1):
        g = pcm.LoamRegistration(0)
        loam.loam_share_tiles(g, o)
        fleet.append(g)
    return fleet


def load_all(fleet):
    for g, x in zip(fleet, poses(len(fleet), 0)):
        ld = g.load_map(x, **P)
        assert ld.num_corner_selected == 25 and ld.num_surf_selected == 25


def targets(torch, fleet, cap):
    out = []
    for g in fleet:
        t = torch.empty((cap, 4), dtype=torch.float32, device="cuda:0")
        n = g.global_map(t)
        out.append(t[:n].view(torch.int32).clone())
    return out


def point(pcm, torch, lists, B, runs):
    row = {}
    # set-up: B owners, then 1 owner + B - 1 sharers
    u0 = used(torch)
    t = time.perf_counter()
    owners = [owner(pcm, lists) for _ in range(B)]
    torch.cuda.synchronize()
    row["owners_setup_s"] = time.perf_counter() - t
    row["owners_device_bytes"] = used(torch) - u0
    destroy(owners)
    u1 = used(torch)
    t = time.perf_counter()
    fleet = shared_fleet(pcm, lists, B)
    torch.cuda.synchronize()
    row["shared_setup_s"] = time.perf_counter() - t
    row["shared_device_bytes"] = used(torch) - u1
    assert loam.loam_tile_share_count(fleet[0]) == B
    load_all(fleet)
    # crops: a loop of single calls against one batch call, interleaved
    k = 0

    def loop(x):
        for g, xi in zip(fleet, x):
            assert g.crop_map(xi, **P).rebuilt

    def batch(x):
        assert all(r.rebuilt and r.status == 0 for r in loam.loam_crop_map_batch(fleet, x, **P))

    for _ in range(2):   # warm-up: workspaces, targets
        k += 1; loop(poses(B, k)); k += 1; batch(poses(B, k))
    t_loop, t_batch = [], []
    for _ in range(runs):
        for f, ts in ((loop, t_loop), (batch, t_batch)):
            k += 1
            x = poses(B, k)
            torch.cuda.synchronize()
            t = time.perf_counter()
            f(x)
            ts.append((time.perf_counter() - t) * 1e3)
    row["loop_of_single_crops"], row["crop_batch"] = stats(t_loop), stats(t_batch)
    row["loop_over_batch"] = row["loop_of_single_crops"]["median_ms"] / row["crop_batch"]["median_ms"]
    spread = max(row["crop_batch"]["max_ms"] - row["crop_batch"]["min_ms"], row["loop_of_single_crops"]["max_ms"] - row["loop_of_single_crops"]["min_ms"])
    row["batch_slower_than_loop_by_more_than_the_spread"] = bool(row["crop_batch"]["median_ms"] - row["loop_of_single_crops"]["median_ms"] > spread)
    # identity at one pose
    x = poses(B, 7)
    loop(x)
    r = fleet[0].crop_map(x[0], **P)
    row["points_in"], row["points_kept"] = r.num_corner_in + r.num_surf_in, r.num_corner + r.num_surf
    single = targets(torch, fleet, row["points_in"])
    batch(poses(B, 8))
    batch(x)
    both = targets(torch, fleet, row["points_in"])
    for i, (a, b) in enumerate(zip(single, both)):
        if a.shape != b.shape or not torch.equal(a, b):
            raise SystemExit("target %d of the batched crop differs from the single crop's" % i)
    row["targets_bit_identical"] = True
    del single, both
    destroy(fleet)
    torch.cuda.empty_cache()
    return row


def trace(pcm, lists, runs):
    fleet = shared_fleet(pcm, lists, 32)
    load_all(fleet)
    for k in range(runs + 2):
        assert all(r.rebuilt for r in loam.loam_crop_map_batch(fleet, poses(32, k + 1), **P))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--batches", default="1,8,32")
    ap.add_argument("--trace", action="store_true", help="only batched crops at B = 32 (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--trace-size", default="small", choices=sorted(SIZES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    global loam
    from pointcloud_slam_amd import loam as loam_module
    loam = loam_module
    if a.trace:
        nc, ns = SIZES[a.trace_size]
        rng = np.random.default_rng(0)
        trace(pcm, (make_grid(rng, nc // 25), make_grid(rng, ns // 25)), a.runs)
        return
    out = {"runs": a.runs, "tile_grid": GRID, "tile_size_m": CELL, "selected": "5 x 5", "baseline": "loop of single pcm_loam_dynmap_crop calls; B owners"}
    for name, (nc, ns) in SIZES.items():
        rng = np.random.default_rng(0)
        lists = (make_grid(rng, nc // 25), make_grid(rng, ns // 25))
        warm = owner(pcm, lists)   # what a process pays once (runtime, code objects) is paid here
        destroy([warm])
        out[name] = {"store_points": GRID * GRID * (nc // 25 + ns // 25), "B": {}}
        for B in [int(v) for v in a.batches.split(",")]:
            out[name]["B"][str(B)] = point(pcm, torch, lists, B, a.runs)
            print(name, B, json.dumps(out[name]["B"][str(B)]), file=sys.stderr, flush=True)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
