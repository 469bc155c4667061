#!/usr/bin/env python3
"""Records tests/golden/target_build_parent.json on the GPU, and names the cases it holds for tests/test_gpu_target_build_pins.py.

The file pins what the target build (build_target_map, voxel_hash.hip) and the candidate-list build (build_neighbour_lists,
neighbour_lists.hip) computed on the commit before both became runs of named stages over one scoped scratch: per case the SHA-256
of the raw bytes of every output that depends on the build order -- the point log, the list index, the list entries with their
map indices, covariances, correspondences, and the sums of the passes that read them.  The pins are equalities, so the anchor
lies outside the code under test.  Everything goes through the C ABI.  It also holds a SHA-256 of the generated inputs: when a
generator changes, the tests say so instead of reporting a mismatch of the builds.  PCM_AMD_LIBRARY names the build to record.
Re-recording with a later commit pins that commit, not the original.

  python tests/make_golden_target_build.py [out.json]     # rewrites tests/golden/target_build_parent.json (needs the GPU)
"""
import hashlib
import importlib
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

PATH = os.path.join(ROOT, "tests", "golden", "target_build_parent.json")
RES = 0.5
NEIGHBOURHOODS = (1, 7, 19, 27)
_CACHE = {}
_LOAM = []


def _synth():
    return importlib.import_module("pointcloud-slam_amd.synth")


def _state(T):
    """the LIO state of a sensor at T with the identity extrinsic: (rot xyzw, pos, off_R xyzw, off_T)"""
    from scipy.spatial.transform import Rotation
    return Rotation.from_matrix(T[:3, :3]).as_quat(), T[:3, 3].copy(), np.array([0.0, 0.0, 0.0, 1.0]), np.zeros(3)


def inputs():
    """name -> tuple of arrays.  Few hundred to few thousand points each."""
    if _CACHE:
        return _CACHE
    S = _synth()
    rng = np.random.default_rng(23)
    f32 = np.float32
    scan, submap, T = S.corner_scene(300, 2000, seed=1, noise=0.01)
    # full builds: (target, source); the sources of the degenerate targets are a few of their points, nudged
    one_voxel = rng.uniform(1.05, 1.20, (257, 3)).astype(f32)   # one 0.5 m voxel under every voxel convention, across a 256-thread block
    bricks = np.stack([rng.uniform(-4.6, -3.4, 600), rng.uniform(-1.0, 1.0, 600), np.full(600, -0.3) + rng.normal(0, 0.005, 600)], 1).astype(f32)   # a floor across the brick face x = -4 m
    _CACHE["full/one_point"] = (np.array([[0.3, -1.2, 2.5]], f32), np.array([[0.31, -1.2, 2.5]], f32))
    _CACHE["full/one_voxel_257"] = (one_voxel, one_voxel[:40] + f32(0.003))
    _CACHE["full/two_bricks_negative"] = (bricks, bricks[::7] + f32(0.004))
    _CACHE["full/scattered_2000"] = (submap[:, :3].copy(), (scan[:, :3] @ T[:3, :3].T + T[:3, 3]).astype(f32))
    # incremental merge: 300 points, then 40 twice (some in old voxels, some in new ones)
    base = rng.uniform(0.0, 4.0, (300, 3)).astype(f32)
    base[:, 2] = (0.2 + rng.normal(0, 0.004, 300)).astype(f32)
    adds = []
    for k in range(2):
        a = rng.uniform(0.0, 5.5, (40, 3)).astype(f32)
        a[:, 2] = (0.2 + rng.normal(0, 0.004, 40)).astype(f32)
        adds.append(a)
    _CACHE["incremental"] = (base, adds[0], adds[1], base[::5] + f32(0.002))
    # LRU: capacity 6 voxels; 4 voxels first, then three inserts of which the last two overflow (one re-touches an old voxel)
    def cells(cs, per):
        return np.concatenate([(np.array(c, np.float64) * RES + rng.uniform(-0.2, 0.2, (per, 3))).astype(f32) for c in cs])
    _CACHE["lru"] = (cells([(0, 0, 0), (1, 0, 0), (2, 0, 0), (3, 0, 0)], 9), cells([(4, 0, 0)], 5), cells([(0, 0, 0), (5, 0, 0), (6, 0, 0), (7, 1, 0)], 4),
                     cells([(8, 0, 0), (9, 0, 0), (10, 0, 0), (2, 0, 0), (11, 0, 0)], 3))
    # MapIncremental: the corner scene, the scan in the sensor frame, the sensor's pose
    _CACHE["map_incremental"] = (submap[:, :3].copy(), scan[:, :3].copy(), T)
    # GICP and the voxel models: ~600 points each side
    gs, gm, gT = S.corner_scene(600, 600, seed=2, noise=0.01)
    _CACHE["gicp"] = (gm[:, :3].copy(), gs[:, :3].copy(), gT)
    # the voxel models at 1 m: three 3 m faces, ~50 points per voxel (a leaf needs 6), a scan of 300 in the sensor frame
    def faces(n):
        q = rng.uniform(0.0, 3.0, (n, 3))
        q[np.arange(n), rng.integers(0, 3, n)] = rng.normal(0, 0.01, n)
        return q + np.array([3.0, 4.0, -2.0])
    Ti = np.linalg.inv(gT)
    _CACHE["voxel_models"] = (faces(1500).astype(f32), (faces(300) @ Ti[:3, :3].T + Ti[:3, 3]).astype(f32), gT)
    return _CACHE


def loam_frame():
    if not _LOAM:
        SL = importlib.import_module("pointcloud-slam_amd.synth_loam")
        _LOAM.append(SL.make_frame(5, n_corner_map=400, n_surf_map=2000, n_corner=80, n_surf=400))
    return _LOAM[0]


def sha(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


def input_digest():
    h = hashlib.sha256()
    fr = loam_frame()
    named = dict(inputs())
    named["loam"] = (fr.corner_map, fr.surf_map, fr.corner, fr.surf, np.asarray(fr.x_guess), np.asarray(fr.x_gt))
    for k in sorted(named):
        for a in named[k]:
            a = np.ascontiguousarray(a)
            h.update(("%s%s%s" % (k, a.dtype.str, a.shape)).encode())
            h.update(a.tobytes())
    return h.hexdigest()


def linearize_digest(g, T, planes=0):
    cost, H, b, inl = g.evaluate_cost(T)
    out = {"linearize": sha(H, b, np.float64([cost]), np.int64([inl])), "inliers": int(inl)}
    if planes:
        out["planes"] = sha(g.get_planes(planes))
    return out


def compute_full(pcm):
    """P2PLANE with the lists asked for: linearize, planes and the three arrays of the lists"""
    out = {}
    for name, (tgt, src) in ((k, v) for k, v in inputs().items() if k.startswith("full/")):
        for nn in NEIGHBOURHOODS:
            g = pcm.P2PlaneRegistration(0, voxel_resolution=RES, num_neighbors=nn, flags=pcm.capi.PCM_FLAG_NEIGHBOUR_LISTS)
            g.set_input_target(tgt)
            g.set_input_source(src)
            d = linearize_digest(g, np.eye(4), planes=len(src))
            centres, starts, xyz, idx = g.get_neighbour_lists()
            d.update(lists=len(centres), entries=len(idx), list_centres=sha(centres), list_starts=sha(starts), list_entries=sha(xyz, idx))
            out["%s/nn%d" % (name, nn)] = d
    return out


def compute_incremental(pcm):
    base, add1, add2, src = inputs()["incremental"]
    g = pcm.P2PlaneRegistration(0, voxel_resolution=RES, num_neighbors=27)
    g.set_input_target(base)
    g.set_input_source(src)
    out = {"step0": linearize_digest(g, np.eye(4))}
    for k, a in enumerate((add1, add2)):
        g.target_insert(a)
        d = linearize_digest(g, np.eye(4))
        t = g.get_target()
        d.update(target=sha(t), points=len(t))
        out["step%d" % (k + 1)] = d
    return out


def compute_lru(pcm):
    first, *batches = inputs()["lru"]
    g = pcm.P2PlaneRegistration(0, voxel_resolution=RES, num_neighbors=27, map_capacity=6)
    g.set_input_target(first)
    g.set_input_source(first[:5])
    out = {}
    for k, a in enumerate(batches):
        g.target_insert(a)
        t = g.get_target()
        out["insert%d" % k] = {"target": sha(t), "points": len(t), "lru_batch_hazards": int(g.stats()["lru_batch_hazards"])}
    return out


def compute_map_incremental(pcm):
    submap, scan, T = inputs()["map_incremental"]
    out = {}
    for sort_source in (0, 1):
        g = pcm.P2PlaneRegistration(0, voxel_resolution=RES, num_neighbors=27, sort_source=sort_source)
        g.set_input_target(submap)
        g.set_input_source(scan)
        st = _state(T)
        g.obs_model(*st, False, True)
        added = g.map_incremental(*st, 0.5, True)
        t = g.get_target()
        out["sort_source%d" % sort_source] = {"num_added": int(added), "target": sha(t), "points": len(t)}
    return out


def compute_gicp(pcm):
    tgt, src, T = inputs()["gicp"]
    g = pcm.GicpRegistration(0, regularization="PCLOMP", max_corr_dist=0.6)
    g.set_input_target(tgt)
    g.set_input_source(src)
    m = g.gicp_bfgs_update_correspondences(np.eye(4, dtype=np.float32), T.astype(np.float32))
    isrc, itgt, M = g.gicp_bfgs_get_correspondences()
    return {"source_covariances": sha(g.get_covariances(False)), "target_covariances": sha(g.get_covariances(True)), "correspondences": int(m),
            "correspondence_indices": sha(isrc, itgt), "correspondence_mahalanobis": sha(M)}


def compute_voxel_models(pcm):
    """Gauss voxels (NDT_D2D), leaf lists (NDT_OMP, kind 1) and voxel-slot rows (VGICP_CUDA, kind 2)"""
    tgt, src, T = inputs()["voxel_models"]
    out = {}
    g = pcm.NdtRegistration(0, flags=pcm.capi.PCM_FLAG_NEIGHBOUR_LISTS)
    g.set_input_target(tgt); g.set_input_source(src)
    out["ndt_d2d"] = linearize_digest(g, T)
    for nn in (0, 1, 7, 27):
        g = pcm.PclNdtRegistration(0, num_neighbors=nn, flags=pcm.capi.PCM_FLAG_NEIGHBOUR_LISTS)
        g.set_input_target(tgt); g.set_input_source(src)
        score, grad, H = g.ndt_derivatives(np.array([0.05, -0.04, 0.03, 0.02, -0.015, 0.03]))
        out["ndt_omp/nn%d" % nn] = {"derivatives": sha(np.float64([score]), grad, H)}
    g = pcm.VgicpCudaRegistration(0, flags=pcm.capi.PCM_FLAG_NEIGHBOUR_LISTS)
    g.set_input_target(tgt); g.set_input_source(src)
    out["vgicp_cuda"] = linearize_digest(g, T)
    return out


def compute_loam(pcm):
    fr = loam_frame()
    g = pcm.LoamRegistration(0)
    g.set_input_target(fr.corner_map, fr.surf_map)
    g.set_input_source(fr.corner, fr.surf)
    out = {}
    for name, x in (("at_guess", fr.x_guess), ("at_truth", fr.x_gt)):
        co, su, AtA, AtB, cnt = g.coefficients(x)
        cn, sn = g.neighbours(x)
        out[name] = {"corner": sha(co), "surf": sha(su), "sums": sha(AtA, AtB), "counts": [int(v) for v in cnt], "neighbours": sha(cn, sn)}
    return out


GROUPS = {"full": compute_full, "incremental": compute_incremental, "lru": compute_lru, "map_incremental": compute_map_incremental, "gicp": compute_gicp,
          "voxel_models": compute_voxel_models, "loam": compute_loam}


def load():
    with open(PATH) as f:
        return json.load(f)


def check_inputs(golden):
    assert input_digest() == golden["inputs"], (
        "the generators no longer produce the inputs that tests/golden/target_build_parent.json was recorded with: "
        "the recorded digests do not apply to these inputs")


def main():
    import pointcloud_slam_amd as pcm
    out = {"inputs": input_digest()}
    for name, fn in GROUPS.items():
        out[name] = fn(pcm)
    with open(sys.argv[1] if len(sys.argv) > 1 else PATH, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print("recorded " + ", ".join("%d %s" % (len(out[k]), k) for k in GROUPS))


if __name__ == "__main__":
    main()
