"""One map, N registration contexts: owning against shared (pcm_share_target).

One process builds N point-to-plane contexts against one map of --map-points points twice: "owning" -- every context is given the
map through set_input_target, today's way and the baseline of this run -- and "shared" -- the first context is given the map and
the others share its target.  For each way it records
  * the device memory taken: used memory (hipMemGetInfo) after the warm-up batches minus before the first context, so the lazily
    built structures (voxel map, candidate lists) are in;
  * the set-up time: creating the contexts and giving them the map and their scans, and the first batch, which holds whatever is
    still built lazily;
  * registrations/s of a pcm_align_batch over the N contexts: median of --runs batches after --warmup.
The ways run one after the other with everything of the first destroyed before the second starts; both compute the same results
(checked bit for bit).  Temporary scratch of the builds stays in the device's memory pool after the first way, so the second
way's memory figure holds persistent allocations only; the order is owning first, which can only favour owning.
The scans are not ray casts: scan k is every (map_points / scan_points)-th map point from offset k, moved into a body frame by a
small rigid motion, registered from the identity -- the same construction the GPU tests use, sized like the headline workload.
Usage: python tools/bench_shared_target.py [--contexts 64] [--map-points 1000000] [--scan-points 100000] [--runs 7] [--out FILE]"""
import argparse
import ctypes as C
import gc
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def make_inputs(synth, n_map, n_scan, n_ctx):
    tgt = synth.sample_submap(synth.scene_for_points(1234, n_map, 8.0), n_map, 4321)
    stride = max(1, n_map // n_scan)
    rng = np.random.default_rng(7)
    scans = []
    for k in range(n_ctx):
        pts = tgt[k % stride::stride][:n_scan].astype(np.float64)
        T = np.eye(4)
        T[:3, :3] = synth.rot_xyz(*(np.deg2rad(1.0) * rng.uniform(-1, 1, 3)))
        T[:3, 3] = rng.uniform(-0.1, 0.1, 3)
        body = pts.copy()
        body[:, :3] = (pts[:, :3] - T[:3, 3]) @ T[:3, :3]        # inverse motion: the registration finds T from the identity
        scans.append(np.ascontiguousarray(body, dtype=np.float32))
    return tgt, scans


def one_way(pcm, torch, way, tgt, scans, a):
    L = pcm.load_library()
    n = len(scans)

    def used():
        torch.cuda.synchronize()
        free, total = torch.cuda.mem_get_info()
        return total - free

    def batch(regs):
        arr = (C.c_void_p * n)(*[r.handle for r in regs])
        out = (pcm.capi.PcmResult * n)()
        g = np.ascontiguousarray(np.stack([np.eye(4, dtype=np.float32)] * n))
        t = time.perf_counter()
        rc = L.pcm_align_batch(arr, n, g.ctypes.data, out, None)
        dt = time.perf_counter() - t
        if rc not in (0, pcm.capi.PCM_ERR_NOT_CONVERGED):
            raise pcm.PcmError(rc, (L.pcm_last_error(regs[0].handle) or b"").decode())
        return dt, out

    before = used()
    t0 = time.perf_counter()
    regs = [pcm.P2PlaneRegistration(0, optimizer="GN", max_iterations=a.max_iterations, flags=a.flags) for _ in range(n)]
    for k, r in enumerate(regs):
        if way == "owning" or k == 0:
            r.set_input_target(tgt)
        else:
            r.share_target(regs[0])
        r.set_input_source(scans[k])
    torch.cuda.synchronize()
    setup_s = time.perf_counter() - t0
    first_batch_s, _ = batch(regs)
    for _ in range(max(a.warmup - 1, 1)):       # the second batch builds the owning contexts' lists (default policy)
        batch(regs)
    taken = used() - before
    times, out = [], None
    for _ in range(a.runs):
        dt, out = batch(regs)
        times.append(dt)
    res = {"way": way, "device_memory_taken_bytes": int(taken), "device_memory_taken_per_context_bytes": taken / n, "setup_s": setup_s,
           "first_batch_s": first_batch_s, "batch_s_median": float(np.median(times)), "batch_s_min_max": [min(times), max(times)],
           "registrations_per_s": n / float(np.median(times)), "share_counts": sorted({r.target_share_count for r in regs}),
           "converged": int(sum(o.converged for o in out)), "iterations_total": int(sum(o.iterations for o in out))}
    bits = b"".join(bytes(out[i]) for i in range(n))
    for r in regs:
        r.__del__()
    del regs
    gc.collect()
    torch.cuda.synchronize()
    return res, bits


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--contexts", type=int, default=64)
    ap.add_argument("--map-points", type=int, default=1000000)
    ap.add_argument("--scan-points", type=int, default=100000)
    ap.add_argument("--max-iterations", type=int, default=64)
    ap.add_argument("--flags", type=int, default=0)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "shared_target_bench.json"))
    a = ap.parse_args()
    import importlib
    import torch
    import pointcloud_slam_amd as pcm
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    tgt, scans = make_inputs(synth, a.map_points, a.scan_points, a.contexts)
    # what a process pays once (runtime, code objects, the first launch of the tile kernel and of the lists kernel, which the
    # second registration against a target runs) is paid before either way is measured
    warm = pcm.P2PlaneRegistration(0, optimizer="GN", max_iterations=2)
    warm.set_input_target(tgt[:20000]); warm.set_input_source(scans[0][:2000])
    for _ in range(3):
        warm.align()
    warm.__del__()
    ways, bits = [], []
    for way in ("owning", "shared"):
        res, b = one_way(pcm, torch, way, tgt, scans, a)
        print("%s: %.2f GB, set-up %.2f s + first batch %.2f s, %.0f registrations/s" % (way, res["device_memory_taken_bytes"] / 1e9, res["setup_s"], res["first_batch_s"],
                                                                                         res["registrations_per_s"]), file=sys.stderr, flush=True)
        ways.append(res)
        bits.append(b)
    own, sh = ways
    out = {"bench": "shared_target", "device": torch.cuda.get_device_name(0), "contexts": a.contexts, "map_points": a.map_points,
           "scan_points": a.scan_points, "max_iterations": a.max_iterations, "flags": a.flags, "warmup": a.warmup, "runs": a.runs, "ways": ways,
           "results_equal_bit_for_bit": bits[0] == bits[1],
           "memory_ratio_owning_over_shared": own["device_memory_taken_bytes"] / max(sh["device_memory_taken_bytes"], 1),
           "setup_ratio_owning_over_shared": (own["setup_s"] + own["first_batch_s"]) / (sh["setup_s"] + sh["first_batch_s"]),
           "throughput_ratio_shared_over_owning": sh["registrations_per_s"] / own["registrations_per_s"]}
    print(json.dumps(out))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
