"""How often the keyed walk of k_linearize_lists (csrc/keyed_best.h) must repeat a lane's walk with best_offer_d2 (host only, numpy):
the bench pairs 0-7, the scan in the order sort_sources_batched gives it, at the initial guess and at the ground-truth pose.  For
every scan point: the candidates of its 27-voxel run, float32 d2 in the kernel's operation order, the six smallest truncated
distances (d2 bits without the low kKeyIdBits), and the ambiguity rule of the header -- a truncated distance among the five best
equal to the range limit's, or an in-range one equal to its successor's.  Reported: the share of ambiguous lanes, of lanes whose run
is longer than 128 entries, of waves with at least one such lane, and the trips the repeated walks add to the trips of the keyed
walk (a wave runs its longest lane's count in either loop).
usage: keyed_walk_model.py [--pairs 8] [--id-bits 7] [--max-range 5.0] [--out profiles/keyed_walk_model.json]"""
import argparse, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import numpy as np
from uniform_wave_share import RES, key, morton_order, rnd

OFFS = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int64)


def transform(T, pts):
    """transform() of linearize_common.h: (r0 x + r1 y) + r2 z + t in float32."""
    T = T.astype(np.float32); p = pts[:, :3].astype(np.float32)
    return np.stack([(T[a, 0] * p[:, 0] + T[a, 1] * p[:, 1]) + T[a, 2] * p[:, 2] + T[a, 3] for a in range(3)], 1)


def six_smallest(pts, uniq, start, count, q, bits, chunk=4096):
    """(n, 6) truncated distances of the six nearest candidates (free slots: all ones), (n,) run length before padding."""
    n = len(q)
    top = np.full((n, 6), 0xFFFFFFFF >> bits, np.int64)
    length = np.zeros(n, np.int64)
    qv = rnd(q * np.float32(1.0 / RES)).astype(np.int64)
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk); m = hi - lo
        k = key((qv[lo:hi, None, :] + OFFS[None, :, :]).reshape(-1, 3))
        idx = np.minimum(np.searchsorted(uniq, k), len(uniq) - 1)
        hit = uniq[idx] == k
        s = np.where(hit, start[idx], 0); c = np.where(hit, count[idx], 0)
        length[lo:hi] = c.reshape(m, 27).sum(1)
        tot = int(c.sum())
        if tot == 0:
            continue
        first = np.cumsum(c) - c
        flat = np.repeat(s - first, c) + np.arange(tot)
        qid = np.repeat(np.repeat(np.arange(m), 27), c)
        d = pts[flat] - q[lo:hi][qid]
        d2 = (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]
        t = (d2.view(np.uint32) >> np.uint32(bits)).astype(np.int64)
        order = np.sort((qid.astype(np.int64) << 32) | t)
        qs = order >> 32
        seg = np.searchsorted(qs, np.arange(m))
        for j in range(6):
            at = seg + j
            ok = (at < tot) & (length[lo:hi] > j)
            top[lo:hi, j][ok] = order[at[ok]] & 0xFFFFFFFF
    return top, length


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--id-bits", type=int, default=7)
    ap.add_argument("--max-range", type=float, default=5.0)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    bits, max_run = a.id_bits, 1 << a.id_bits
    m2 = float(np.float32(a.max_range)) ** 2
    r2f = np.float32(m2) if float(np.float32(m2)) >= m2 else np.nextafter(np.float32(m2), np.float32(np.inf))
    R = int(np.float32(r2f).view(np.uint32)) >> bits
    rows = []
    for pid in range(a.pairs):
        p = synth.make_pair(pid, 100000, 1000000)
        sub = p.submap[:, :3].astype(np.float32)
        mk = key(rnd(sub * np.float32(1.0 / RES)).astype(np.int64))
        o = np.argsort(mk, kind="stable")
        pts, mk = sub[o], mk[o]
        uniq, start, count = np.unique(mk, return_index=True, return_counts=True)
        scan = p.scan[morton_order(p.guess.astype(np.float64), p.scan)]
        row = {"pair": pid}
        for name, T in (("guess", p.guess.astype(np.float64)), ("gt", p.T_gt)):
            q = transform(np.asarray(T), scan)
            top, length = six_smallest(pts, uniq, start, count, q, bits)
            walks = length > 0
            trips = (length + 3) // 4
            long_ = trips * 4 > max_run
            t5, t6 = top[:, :5], top[:, 1:6]
            amb = walks & ~long_ & ((t5 == R) | ((t5 < R) & (t5 == t6))).any(1)
            slow = amb | long_
            n = len(q); nw = (n + 63) // 64
            def waves(x, fill=0):
                y = np.full(nw * 64, fill, x.dtype); y[:n] = x
                return y.reshape(nw, 64)
            w_walk, w_slow = waves(walks).any(1), waves(slow).any(1)
            fast_trips = waves(np.where(long_, 0, trips)).max(1).sum()
            slow_trips = waves(np.where(slow, trips, 0)).max(1).sum()
            old_trips = waves(trips).max(1).sum()
            row[name] = {"walking_lanes": int(walks.sum()), "ambiguous_lane_share": float(amb.sum() / walks.sum()), "long_run_lane_share": float(long_.sum() / walks.sum()),
                         "waves_with_a_walk": int(w_walk.sum()), "slow_wave_share": float(w_slow.sum() / w_walk.sum()),
                         "trips_per_wave_before": float(old_trips / w_walk.sum()), "keyed_trips_per_wave": float(fast_trips / w_walk.sum()),
                         "repeated_trips_per_wave": float(slow_trips / w_walk.sum()), "median_run": float(np.median(length[walks])), "max_run": int(length.max())}
        rows.append(row)
        print(json.dumps(row), flush=True)
    out = {"id_bits": bits, "max_range": a.max_range}
    for name in ("guess", "gt"):
        out[name] = {k: float(np.mean([r[name][k] for r in rows])) for k in ("ambiguous_lane_share", "long_run_lane_share", "slow_wave_share", "trips_per_wave_before",
                                                                           "keyed_trips_per_wave", "repeated_trips_per_wave")}
    out["pairs"] = rows
    print(json.dumps({k: v for k, v in out.items() if k != "pairs"}))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
