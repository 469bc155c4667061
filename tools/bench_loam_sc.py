"""Scan Context benchmark (pcm_loam_sc_add / pcm_loam_sc_detect).  sc_add of a 16 x 1800 and a 128 x 1800 synth_spin scan from
device memory, with the VoxelGrid of 0.5 m and without, and of a stored surf key frame; beside it, in the same process, what a
caller pays for the same descriptor without the feature: reading that cloud back to the host plus the numpy restatement
(tests/loam_sc_ref.py: descriptor and both keys).  sc_detect at K = 1 000 / 10 000 / 100 000 stored descriptors (sc_put of random
column rotations and perturbations of the scans' own descriptors; the search set is rebuilt on every call, so it holds K entries)
with the reference parameters (3 candidates) and with num_candidates = 0 (every entry), against the restatement's time at
K = 1 000.  Medians of --runs after a warm-up.  The reference cannot be built here (no PCL / Eigen), so no reference time is
reported.  Prints one JSON line.
Usage: python tools/bench_loam_sc.py [--runs 9] [--out FILE]; --trace-k K fills a store of K descriptors and runs nothing but
detect calls (half with 3 candidates, half with num_candidates = 0), for a kernel trace (the fill's k_sc_finish rows aside, every
row belongs to the detection)."""
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
F = np.float32


def median_ms(f, runs):
    ts = []
    for _ in range(runs):
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def perturbed_pool(bases, n, rng):
    """n descriptors: a base, its columns rotated, its occupied bins moved by a few centimetres (float-representable)."""
    pool = []
    for i in range(n):
        d = np.roll(bases[i % len(bases)], int(rng.integers(0, bases[0].shape[1])), axis=1).copy()
        occ = d != 0
        d[occ] = (d[occ] + rng.normal(0.0, 0.05, int(occ.sum()))).astype(F).astype(np.float64)
        pool.append(d)
    return pool


def fill(g, pool, upto, rng):
    S = pool[0].shape[1]
    while g.sc_count < upto:
        g.sc_put(np.roll(pool[int(rng.integers(0, len(pool)))], int(rng.integers(0, S)), axis=1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=9)
    ap.add_argument("--sizes", default="1000,10000,100000")
    ap.add_argument("--trace-k", type=int, default=0, help="only detect calls on a store of this many descriptors (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import pointcloud_slam_amd as pcm
    import loam_sc_ref as R
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    synth_spin = importlib.import_module("pointcloud-slam_amd.synth_spin")
    rng = np.random.default_rng(0)
    P = R.Params()
    scene = synth.make_scene(0, 15.0, n_boxes=60, n_cyls=12)
    pose = np.array([0, 0, 0.05, 14.0, 18.0, 1.5], F)
    scans = {}
    for n_scan in (16,) if a.trace_k else (16, 128):
        rec = synth_spin.spin_points(scene, pose, n_scan, 1800, seed=n_scan, empty_rings=0)
        scans[n_scan] = np.ascontiguousarray(rec[:, :12]).view(F).reshape(-1, 3).copy()
    bases = [R.make_scancontext(scans[16], P)]
    for dx in (1.5, 3.0, 4.5):   # the same scene seen from a few more places
        rec = synth_spin.spin_points(scene, pose + np.array([0, 0, 0, dx, 0, 0], F), 16, 1800, seed=int(10 * dx), empty_rings=0)
        bases.append(R.make_scancontext(np.ascontiguousarray(rec[:, :12]).view(F).reshape(-1, 3), P))
    pool = perturbed_pool(bases, 256, rng)
    det = dict(tree_making_period=1)

    if a.trace_k:
        g = pcm.LoamRegistration(0)
        fill(g, pool, a.trace_k + 30, rng)
        for _ in range(a.runs + 2):
            g.sc_detect(**det)
            g.sc_detect(num_candidates=0, **det)
        return

    out = {"runs": a.runs}
    g = pcm.LoamRegistration(0)
    for n_scan, xyz in scans.items():
        d = torch.from_numpy(xyz).cuda()
        row = {"points": int(xyz.shape[0])}
        for name, leaf in (("leaf_0.5", 0.5), ("no_voxelgrid", 0.0)):
            for _ in range(3):
                g.sc_add(points=d, leaf=leaf)
            row["sc_add_%s_ms" % name] = median_ms(lambda: g.sc_add(points=d, leaf=leaf), a.runs)
            row["points_%s" % name] = int(g._sc_last_add.num_points)
        # without the feature: the cloud comes back to the host and the descriptor and its keys are made there

        def caller():
            h = d.cpu().numpy()
            desc = R.make_scancontext(h, P)
            return R.ring_key(desc), R.sector_key(desc)

        caller()
        row["readback_ms"] = median_ms(lambda: d.cpu().numpy(), a.runs)
        row["readback_plus_numpy_restatement_ms"] = median_ms(caller, a.runs)
        out["scan_%dx1800" % n_scan] = row
        g.sc_clear()
    # a stored surf key frame: 8 000 points of the 16-ring scan (what matters here is the count)
    surf = np.zeros((8000, 4), F)
    surf[:, :3] = scans[16][rng.permutation(scans[16].shape[0])[:8000]]
    g.add_keyframe(pose, 0.0, surf[:100], surf)
    for _ in range(3):
        g.sc_add(keyframe=0)
    out["keyframe_surf"] = {"points": 8000, "sc_add_ms": median_ms(lambda: g.sc_add(keyframe=0), a.runs),
                            "get_keyframe_plus_numpy_restatement_ms": median_ms(lambda: R.ring_key(R.make_scancontext(g.get_keyframe(0)[1][:, :3], P)), a.runs)}
    g.sc_clear()

    for K in [int(v) for v in a.sizes.split(",")]:
        t = time.perf_counter()
        fill(g, pool, K + 30, rng)
        row = {"fill_s": time.perf_counter() - t}
        for name, nc in (("reference_3_candidates", 3), ("all_entries", 0)):
            for _ in range(2):
                r = g.sc_detect(num_candidates=nc, **det)
            assert r.tree_size == K and r.num_evaluated == (nc or K)
            row["detect_%s_ms" % name] = median_ms(lambda: g.sc_detect(num_candidates=nc, **det), a.runs)
            row["min_dist_%s" % name] = r.min_dist
        row["detect_64_candidates_ms"] = median_ms(lambda: g.sc_detect(num_candidates=64, **det), a.runs)
        if K <= 1000:   # the restatement on the same descriptors
            M = R.Manager(R.Params(tree_making_period=1))
            for i in range(g.sc_count):
                M.add(g.sc_get(i)[0])
            for name, nc in (("reference_3_candidates", 3), ("all_entries", 0)):
                M.P.num_candidates = nc
                t = time.perf_counter()
                ref = M.detect()
                row["numpy_restatement_%s_ms" % name] = (time.perf_counter() - t) * 1e3
                assert ref["min_dist"] == row["min_dist_%s" % name]
        out["K_%d" % K] = row
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
