"""LOAM key-frame submap benchmark (pcm_loam_submap_update / pcm_loam_keyframe_add): K key frames of n_corner / n_surf points on the
synth_keyframes lawn-mower, search radius 50 m (every key frame inside) and 15 m, all at the default leaves (0.2 m); a rebuild
is forced by a correctPoses of one key frame to its own value, which changes no work.  Per radius: update_ms (rebuilt),
update_plus_grids_ms (the update and the grid build of the next scan2map's first pass), update_unchanged_ms, keyframe_add_ms (device
copy of the source), points in / out; beside them, on the same inputs in the same process, the path a caller has without the
feature: the host-transformed concatenation (not timed) through two voxel_downsample calls and set_input_target with a new tag plus
the same grid build (timed), and the numpy restatement's time.  Medians of --runs after a warm-up.  The reference's PCL node cannot
be built here (no PCL), so no reference time is reported.  Prints one JSON line.
Usage: python tools/bench_loam_submap.py [--runs 7] [--keyframes 200] [--out FILE]; --trace-radius R runs nothing but rebuilt updates
at radius R, for a kernel trace whose rows all belong to this path."""
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


def median_ms(f, runs, before=None):
    ts = []
    for _ in range(runs):
        if before:
            before()
        t = time.perf_counter()
        f()
        ts.append((time.perf_counter() - t) * 1e3)
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--keyframes", type=int, default=200)
    ap.add_argument("--n-corner", type=int, default=2000)
    ap.add_argument("--n-surf", type=int, default=8000)
    ap.add_argument("--no-cpu", action="store_true", help="skip the numpy restatement")
    ap.add_argument("--trace-radius", type=float, default=0.0, help="only rebuilt updates at this radius (run under rocprofv3 --kernel-trace --stats)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import pointcloud_slam_amd as pcm
    import loam_submap_ref as R
    synth_keyframes = importlib.import_module("pointcloud-slam_amd.synth_keyframes")
    kf = synth_keyframes.make_keyframes(0, a.keyframes, a.n_corner, a.n_surf)
    K = a.keyframes
    g = pcm.LoamRegistration(0)
    for k in range(K):
        g.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k])
    scan_c, scan_s = kf.corner[-1], kf.surf[-1]
    x0 = kf.poses[-1]
    out = {"runs": a.runs, "keyframes": K, "n_corner": a.n_corner, "n_surf": a.n_surf}

    def touch():   # correctPoses of one key frame to its own value: the pose generation moves, so the next update rebuilds the same work
        g.set_keyframe_poses(kf.poses[:1], 0)

    if a.trace_radius:   # for a kernel trace: nothing but rebuilt updates at one radius (after the key-frame uploads)
        for _ in range(a.runs + 2):
            touch()
            assert g.update_submap(kf.time_cur, search_radius=a.trace_radius).rebuilt
        return
    for radius in (50.0, 15.0):
        p = dict(search_radius=radius)
        g.set_input_source(scan_c, scan_s)
        for _ in range(2):   # warm-up
            touch(); g.update_submap(kf.time_cur, **p); g.scan2map(x0, iter_num=1)
        touch()
        r = g.update_submap(kf.time_cur, **p)
        assert r.rebuilt
        row = {"num_selected": r.num_selected, "points_in": r.num_corner_in + r.num_surf_in, "points_out": r.num_corner_map + r.num_surf_map}
        row["update_ms"] = median_ms(lambda: g.update_submap(kf.time_cur, **p), a.runs, before=touch)
        # one iteration of scan2map on the fresh target: the grid build and one correspondence pass
        row["update_plus_grids_ms"] = median_ms(lambda: (g.update_submap(kf.time_cur, **p), g.scan2map(x0, iter_num=1)), a.runs, before=touch)
        g.update_submap(kf.time_cur, **p)
        info = g.submap_info()
        row["update_unchanged_ms"] = median_ms(lambda: g.update_submap(kf.time_cur, **p), a.runs)
        row["scan2map_1iter_ms"] = median_ms(lambda: g.scan2map(x0, iter_num=1), a.runs)
        # the caller's path without the feature: the concatenated clouds are on the host already (not timed)
        h = pcm.LoamRegistration(0)
        h.set_input_source(scan_c, scan_s)
        vg = pcm.P2PlaneRegistration(0)
        cin, sin = info["corner_in"], info["surf_in"]
        tag = [1]

        def parent():
            tag[0] += 1
            h.set_input_target(vg.voxel_downsample(cin, 0.2), vg.voxel_downsample(sin, 0.2), tag=tag[0])
            h.scan2map(x0, iter_num=1)

        parent(); parent()
        row["parent_path_plus_grids_ms"] = median_ms(parent, a.runs)
        if not a.no_cpu:
            t = time.perf_counter()
            R.submap(kf.poses, kf.times, kf.corner, kf.surf, kf.time_cur, radius)
            row["numpy_restatement_ms"] = (time.perf_counter() - t) * 1e3
        out["radius_%d" % int(radius)] = row
    # set_input_source of the 10 k-point scan (it also keeps the records' fourth float for a later key frame)
    out["set_input_source_ms"] = median_ms(lambda: g.set_input_source(scan_c, scan_s), 5 * a.runs)
    # keyframe_add with the features staying on the device
    g.set_input_source(scan_c, scan_s)
    g.add_keyframe(x0, kf.time_cur)
    out["keyframe_add_ms"] = median_ms(lambda: g.add_keyframe(x0, kf.time_cur), a.runs)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
