"""Share of the waves of k_linearize_lists whose live lanes all walk ONE run (host only, numpy): the bench pairs 0-7, the scan in the
order sort_sources_batched gives it (32-bit [scan | Morton] keys of a 64-pair batch, cell = the voxel at the initial guess, stable),
list voxel of every point at the initial guess and at the ground-truth pose.  A lane walks iff one of the 27 voxels around its own
holds a map point.  Also the list entries of the target with and without the padding of a run to a multiple of four.
usage: uniform_wave_share.py [--pairs 8] [--out FILE]"""
import argparse, importlib, json, os, sys
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

RES, BIAS = 0.5, 1 << 20


def rnd(x):   # roundf: half away from zero
    return np.sign(x) * np.floor(np.abs(x) + np.float32(0.5))


def voxels(T, pts):
    T = T.astype(np.float32)
    q = (pts[:, :3].astype(np.float32) @ T[:3, :3].T + T[:3, 3]).astype(np.float32)
    return rnd(q * np.float32(1.0 / RES)).astype(np.int64)


def key(v):
    return ((v[:, 0] + BIAS) << 42) | ((v[:, 1] + BIAS) << 21) | (v[:, 2] + BIAS)


def spread(v, bits):
    out = np.zeros_like(v)
    for b in range(bits):
        out |= ((v >> b) & 1) << (3 * b)
    return out


def morton_order(T, pts, mb=26):
    bz = mb // 3; rem = mb - 3 * bz
    nb = [bz + (rem >= 1), bz + (rem >= 2), bz]
    v = voxels(T, pts) - rnd(T[:3, 3].astype(np.float32) * np.float32(1.0 / RES)).astype(np.int64)
    c = [np.clip(v[:, a], -(1 << (nb[a] - 1)), (1 << (nb[a] - 1)) - 1) + (1 << (nb[a] - 1)) for a in range(3)]
    low = (1 << bz) - 1
    m = spread(c[0] & low, bz) | (spread(c[1] & low, bz) << 1) | (spread(c[2] & low, bz) << 2)
    m |= ((c[0] >> bz) | ((c[1] >> bz) << (nb[0] - bz))) << (3 * bz)
    return np.argsort(m, kind="stable")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=8)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    synth = importlib.import_module("pointcloud-slam_amd.synth")
    offs = np.array([(x, y, z) for x in (-1, 0, 1) for y in (-1, 0, 1) for z in (-1, 0, 1)], np.int64)
    rows = []
    for pid in range(a.pairs):
        p = synth.make_pair(pid, 100000, 1000000)
        mv = voxels(np.eye(4), p.submap)
        occ, cnt = np.unique(key(mv), return_counts=True)
        # candidates of every list voxel = sum of the counts of its 27 neighbours
        uv = np.stack([(occ >> 42) - BIAS, ((occ >> 21) & 0x1fffff) - BIAS, (occ & 0x1fffff) - BIAS], 1)
        lk = np.concatenate([key(uv - o) for o in offs]); lc = np.tile(cnt, 27)
        lists, inv = np.unique(lk, return_inverse=True)
        n_list = np.bincount(inv, weights=lc).astype(np.int64)
        entries, padded = int(n_list.sum()), int(((n_list + 3) & ~3).sum())
        order = morton_order(p.guess.astype(np.float64), p.scan)
        scan = p.scan[order]
        row = {"pair": pid, "list_voxels": int(len(lists)), "list_entries": entries, "list_entries_padded": padded}
        for name, T in (("guess", p.guess.astype(np.float64)), ("gt", p.T_gt)):
            k = key(voxels(T, scan))
            walks = np.isin(k, lists)
            n = len(k); nw = (n + 63) // 64
            kk = np.full(nw * 64, -1, np.int64); kk[:n] = np.where(walks, k, -1)
            kk = kk.reshape(nw, 64)
            live = kk >= 0
            hi = np.where(live, kk, -1).max(1); lo = np.where(live, kk, np.iinfo(np.int64).max).min(1)
            has = live.any(1)
            uniform = has & (hi == lo)
            distinct = np.array([len(np.unique(r[r >= 0])) for r in kk[has]])
            row[name] = {"waves_with_a_walk": int(has.sum()), "uniform": int(uniform.sum()), "uniform_share": float(uniform.sum() / max(1, has.sum())),
                         "median_distinct_runs_per_wave": float(np.median(distinct))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    tot = {n: sum(r[n]["uniform"] for r in rows) / sum(r[n]["waves_with_a_walk"] for r in rows) for n in ("guess", "gt")}
    e, ep = sum(r["list_entries"] for r in rows) / len(rows), sum(r["list_entries_padded"] for r in rows) / len(rows)
    out = {"uniform_wave_share": tot, "mean_list_bytes_per_target": 16 * e, "mean_list_bytes_per_target_padded": 16 * ep, "padding_growth": ep / e - 1, "pairs": rows}
    print(json.dumps({k: v for k, v in out.items() if k != "pairs"}))
    if a.out:
        json.dump(out, open(a.out, "w"), indent=1)


if __name__ == "__main__":
    main()
