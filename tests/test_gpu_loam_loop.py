"""GPU checks of loop verification on the device (pcm_loam_submap_near_dev, pcm_loam_loop_verify, pcm_loam_loop_closure):

* the near cloud -- pcm_loam_submap_near's host cloud and pcm_loam_submap_near_dev's, which are one device pass -- equals, bit for
  bit, the cloud of the two-segment pass that pcm_loam_submap_near ran before the two became one (the digests recorded in
  tests/golden/loam_near_parent.json; tests/make_golden_loam_near.py);
* a verification equals the composition it replaces on the same context state -- near_keyframes x 2 -> a fresh PclNdtRegistration
  with the same settings -> align -> get_fitness_score -> the numpy restatement of performLoopClosure (tests/loam_loop_ref.py):
  correction, fitness and iterations as equalities, and `between` with the CPU tolerance of tests/test_loam_loop.py, which is 0
  (the header and the restatement perform the same IEEE operations on the same libm);
* the context's target, source, key frames and Scan Context store are untouched.

Case (d) of the issue, rejected_not_converged, has no pair: pclomp's loop sets converged_ when the iteration cap is passed
(ndt_omp_impl.hpp:137-138), so hasConverged() is false only after a NaN step norm (:119-122), which no finite pair of clouds with
occupied leaves produces -- on the CPU oracle (orc_pclndt) as on the device.  The status is covered on the CPU
(tests/test_loam_loop.py::test_gates_and_acceptance)."""
import importlib
import math

import numpy as np
import pytest

import loam_loop_ref as R
import make_golden_loam_near as G

pytestmark = pytest.mark.gpu

synth = importlib.import_module("pointcloud-slam_amd.synth")
synth_keyframes = importlib.import_module("pointcloud-slam_amd.synth_keyframes")
synth_loam = importlib.import_module("pointcloud-slam_amd.synth_loam")
_CACHE = {}


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


near_keyframes = G.near_keyframes
_CACHE["golden"] = G.load()


def recorded(K, case, cloud):
    """whether `cloud` is the cloud recorded for the case: same rows, same SHA-256 of its float32 bytes"""
    return G.digest(cloud) == _CACHE["golden"]["near"][G.case_id(K, *case)]


def filled(pcm, kf):
    g = pcm.LoamRegistration(0)
    for k in range(len(kf.times)):
        assert g.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k]) == k
    return g


def window_points(kf, key, search_num):
    K = len(kf.times)
    return sum(len(kf.corner[k]) + len(kf.surf[k]) for k in range(max(0, key - search_num), min(K, key + search_num + 1)))


# ---- the device near cloud --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", [1, 2, 7])
def test_device_near_cloud_equals_host_near_cloud(pcm, K):
    import torch
    kf = near_keyframes(K)
    G.check_inputs(_CACHE["golden"], K)
    g = filled(pcm, kf)
    n_checked = 0
    for case in G.near_cases(K):
        key, search_num, wrt_key, leaf = case
        want = g.near_keyframes(key, search_num, wrt_key, leaf)
        assert recorded(K, case, want), case
        N, m = window_points(kf, key, search_num), len(want)
        assert m <= N and (leaf > 0 or m == N)
        # host buffer
        out = np.full((N + 1, 4), np.nan, np.float32)
        assert g.submap_near_device(key, search_num, wrt_key, leaf, out) == m
        assert recorded(K, case, out[:m]) and np.array_equal(bits(out[:m]), bits(want)) and np.all(np.isnan(out[m:]))
        # device buffers: room for every input point (written in place), and exactly the result's size
        for cap in sorted({N, m}):
            if cap == 0:
                continue
            dev = torch.full((cap, 4), float("nan"), dtype=torch.float32, device="cuda:0")
            assert g.submap_near_device(key, search_num, wrt_key, leaf, dev) == m
            torch.cuda.synchronize()
            got = dev.cpu().numpy()
            assert recorded(K, case, got[:m]) and np.array_equal(bits(got[:m]), bits(want)), (case, cap)
            if leaf == 0.0 or cap == m:
                assert np.all(np.isnan(got[m:]))
        # one short: PCM_ERR_INVALID_ARGUMENT with the count set
        if m > 0:
            for short in (np.zeros((m - 1, 4), np.float32), torch.zeros((max(m - 1, 1), 4), dtype=torch.float32, device="cuda:0")[:m - 1]):
                with pytest.raises(pcm.capi.PcmError) as e:
                    g.submap_near_device(key, search_num, wrt_key, leaf, short)
                assert e.value.code == -1 and g._near_count == m
        n_checked += 1
    assert n_checked == len({0, K // 2, K - 1}) * (14 if K == 7 else 12)
    # the host entry still gives what it gave, after all the device passes
    assert recorded(K, (K - 1, 25, -1, 0.4), g.near_keyframes(K - 1, 25, -1, 0.4))


def test_near_entries_share_a_workspace(pcm):
    """pcm_loam_submap_near runs in the workspace of pcm_loam_submap_near_dev: a device result left un-waited -- in place without
    a leaf, and as a queued copy out of the workspace's cell array with one -- survives a host call with other arguments."""
    import torch
    K = 7
    kf = near_keyframes(K)
    G.check_inputs(_CACHE["golden"], K)
    g = filled(pcm, kf)
    # the first result is written in place (no leaf: as many rows as input points); the other two are fewer rows than points
    for first, second in (((3, 25, -1, 0.0), (6, 1, 0, 0.4)), ((3, 25, -1, 0.4), (0, 25, 0, 0.0)), ((6, 25, 0, G.BIG_LEAF), (3, 1, -1, 0.4))):
        rows = _CACHE["golden"]["near"][G.case_id(K, *first)]["rows"]
        assert (rows == window_points(kf, first[0], first[1])) == (first[3] == 0.0)
        dev = torch.full((rows, 4), float("nan"), dtype=torch.float32, device="cuda:0")
        assert g.submap_near_device(*first, dev) == rows   # not waited for
        host = g.near_keyframes(*second)
        torch.cuda.synchronize()
        assert recorded(K, second, host), (first, second)
        assert recorded(K, first, dev.cpu().numpy()), (first, second)


def test_device_near_cloud_errors_and_empty_store(pcm):
    g = pcm.LoamRegistration(0)
    out = np.zeros((4, 4), np.float32)
    assert g.submap_near_device(0, 0, -1, 0.2, out) == 0   # no key frame: nothing to assemble, as pcm_loam_submap_near
    kf = near_keyframes(2)
    g = filled(pcm, kf)
    for args in ((-1, 0, -1, 0.2), (2, 0, -1, 0.2), (0, -1, -1, 0.2), (0, 0, 2, 0.2), (0, 0, -1, -0.1), (0, 0, -1, float("nan"))):
        with pytest.raises(pcm.capi.PcmError) as e:
            g.submap_near_device(*args, out)
        assert e.value.code == -1
    import ctypes
    ndt = pcm.PclNdtRegistration(0)
    n = ctypes.c_size_t(0)
    assert ndt._L.pcm_loam_submap_near_dev(ndt.handle, 0, 0, -1, 0.2, out.ctypes.data, 4, 0, ctypes.byref(n)) == -1   # not a LOAM context


# ---- verification ---------------------------------------------------------------------------------------------------------------
def loop_keyframes():
    """K = 5 key frames 0.5 m apart along a short track through a small synth_loam scene.  Key frame 4 is the loop key: its stored
    pose is off by a known 0.3 m / 2 degrees (the drift the verification measures).  With the 0.2 m leaf the current cloud
    (key frame 4) has about 400 points and the previous one (key frames 0..2) about 1200."""
    if "loop" in _CACHE:
        return _CACHE["loop"]
    scene = synth.make_scene(5, 4.0, n_boxes=10, n_cyls=3)
    rng = np.random.default_rng(11)
    segs = synth_loam._segments(scene)
    pool_c = synth_loam._sample_edges(segs, 6000, rng, 0.01)
    pool_s = synth_loam._sample_planes(scene, 24000, rng, 0.01)
    cx, cy = 0.5 * scene.lx - 1.0, 0.5 * scene.ly
    true = np.array([[rng.normal(0, 0.01), rng.normal(0, 0.01), 0.05 * k, cx + 0.5 * k, cy + 0.1 * k, 1.5] for k in range(5)], np.float32)
    corner, surf = [], []
    for k in range(5):
        out = []
        for pool, n in ((pool_c, 140), (pool_s, 330)):
            d = np.linalg.norm(pool[:, :2] - true[k, 3:5].astype(np.float64)[None], axis=1)
            idx = np.nonzero(d < 7.0)[0]
            idx = idx[rng.permutation(idx.size)[:n]]
            b = synth_loam._to_body(pool[idx], true[k])
            b[:, 3] = rng.integers(0, 256, b.shape[0]).astype(np.float32)
            out.append(b)
        corner.append(out[0]); surf.append(out[1])
    stored = true.copy()
    stored[4, 2] += np.float32(math.radians(2.0))
    stored[4, 3] += np.float32(0.3 * math.cos(0.7)); stored[4, 4] += np.float32(0.3 * math.sin(0.7))
    times = 100.0 + 40.0 * np.arange(5)
    _CACHE["loop_true"] = true
    _CACHE["loop"] = synth_keyframes.KeyFrames(stored, times.astype(np.float64), corner, surf, float(times[-1] + 0.1))
    return _CACHE["loop"]


def composition(pcm, g, kf, key_cur, key_pre, **params):
    """today's path through the host, on the same context state"""
    p = dict(R.DEFAULTS, **params)
    cur = g.near_keyframes(key_cur, 0, p["wrt_key"], p["near_leaf"])
    prev = g.near_keyframes(key_pre, p["history_search_num"], p["wrt_key"], p["near_leaf"])

    def ndt():
        n = pcm.PclNdtRegistration(0, voxel_resolution=p["ndt_resolution"], num_neighbors=p["ndt_num_neighbors"], translation_eps=p["ndt_epsilon"])
        n.set_input_target(prev)
        n.set_input_source(cur)
        r = n.align()
        return r.converged, r.iterations, r.T, n.get_fitness_score()

    return R.perform_loop_closure(len(cur), len(prev), ndt, kf.poses[key_cur], kf.poses[key_pre], p)


def assert_same(got, ref):
    assert got.status == R.STATUS_NAMES[ref["status"]]
    assert (got.num_cur_points, got.num_prev_points) == (ref["num_cur_points"], ref["num_prev_points"])
    assert (got.iterations, got.converged) == (ref["iterations"], ref["converged"])
    assert got.fitness == ref["fitness"] and got.noise_variance == ref["noise_variance"]
    assert np.array_equal(bits(got.correction), bits(ref["correction"]))
    for k in ("pose_from", "pose_to", "between", "between6"):
        d = np.abs(getattr(got, k) - ref[k]).max()
        print(k, "worst |difference| =", d)
        assert np.array_equal(getattr(got, k), ref[k]), k   # CPU tolerance: 10 x 0.0


def accepted_case(pcm):
    if "accepted" not in _CACHE:
        kf = loop_keyframes()
        g = filled(pcm, kf)
        got = g.loop_verify(4, 1, history_search_num=1)
        _CACHE["accepted"] = (kf, g, got, composition(pcm, g, kf, 4, 1, history_search_num=1))
    return _CACHE["accepted"]


def test_verify_accepted_equals_composition(pcm):
    kf, g, got, ref = accepted_case(pcm)
    print("clouds:", got.num_cur_points, got.num_prev_points, "iterations:", got.iterations, "fitness:", got.fitness)
    assert 300 <= got.num_cur_points <= 520 and 1000 <= got.num_prev_points <= 1500
    assert got.accepted and got.converged and got.iterations >= 1
    assert_same(got, ref)
    # the correction works against the known drift: poseFrom is nearer to key frame 4's true pose than the stored pose, which is
    # 2 degrees / 0.3 m off.  How near is NDT's business (it stops at a step below its epsilon of 0.01); nearer it must be, and
    # the swapped composition tWrong * correction would move the position elsewhere.
    true = _CACHE["loop_true"][4].astype(np.float64)
    yaw_err, pos_err = abs(got.pose_from[2] - true[2]), float(np.linalg.norm(got.pose_from[3:6] - true[3:6]))
    print("residual yaw error [deg]:", math.degrees(yaw_err), "of 2; residual position error [m]:", pos_err, "of 0.3")
    assert yaw_err < math.radians(2.0) and pos_err < 0.3
    assert got.noise_variance == float(np.float32(got.fitness)) and (got.key_cur, got.key_pre) == (4, 1)
    # with respect to one key frame (the option, not the reference's SC path): still the composition
    got_w = g.loop_verify(4, 1, history_search_num=1, fitness_threshold=0.3, wrt_key=4)
    assert_same(got_w, composition(pcm, g, kf, 4, 1, history_search_num=1, fitness_threshold=0.3, wrt_key=4))
    # a second verification on the same verifier context gives the same bits
    again = g.loop_verify(4, 1, history_search_num=1, fitness_threshold=0.3)
    assert_same(again, ref)


def test_verify_rejected_fitness(pcm):
    kf, g, acc, _ = accepted_case(pcm)
    assert acc.fitness > 0.0
    thr = 0.5 * acc.fitness   # below the measured fitness of the accepted case
    got = g.loop_verify(4, 1, history_search_num=1, fitness_threshold=thr)
    assert got.status == "rejected_fitness" and not got.accepted and got.converged
    assert_same(got, composition(pcm, g, kf, 4, 1, history_search_num=1, fitness_threshold=thr))
    assert np.array_equal(bits(got.correction), bits(acc.correction)) and got.fitness == acc.fitness
    assert not got.between.any() and not got.between6.any()   # no factor for a rejected pair


def test_verify_rejected_size(pcm):
    """299 current points, and 999 previous points, against the reference's gates of 300 and 1000 (no leaf: a cloud's size is the
    sum of its key frames' points); 300 and 1000 pass the gates"""
    kf = loop_keyframes()

    def store(n_cur, n_prev):
        g = pcm.LoamRegistration(0)
        prev_pts = np.concatenate([kf.corner[1], kf.surf[1], kf.corner[2], kf.surf[2], kf.corner[0], kf.surf[0]])[:n_prev]
        cur_pts = np.concatenate([kf.corner[4], kf.surf[4]])[:n_cur]
        assert len(prev_pts) == n_prev and len(cur_pts) == n_cur
        g.add_keyframe(kf.poses[1], 1.0, prev_pts[:100], prev_pts[100:])
        g.add_keyframe(kf.poses[4], 2.0, cur_pts[:50], cur_pts[50:])
        return g

    for n_cur, n_prev, rejected in ((299, 1000, True), (300, 999, True), (300, 1000, False)):
        g = store(n_cur, n_prev)
        got = g.loop_verify(1, 0, history_search_num=0, near_leaf=0.0, fitness_threshold=1e9)
        assert (got.num_cur_points, got.num_prev_points) == (n_cur, n_prev)
        assert (got.status == "rejected_size") == rejected
        if rejected:
            assert not g.loop_verifier_exists   # NDT did not run: the verifier was never created
            assert got.iterations == 0 and np.array_equal(got.correction, np.eye(4, dtype=np.float32))
        else:
            assert g.loop_verifier_exists and got.iterations >= 1
        poses = np.stack([kf.poses[1], kf.poses[4]])
        two = synth_keyframes.KeyFrames(poses, None, None, None, 0.0)
        assert_same(got, composition(pcm, g, two, 1, 0, history_search_num=0, near_leaf=0.0, fitness_threshold=1e9))


def snapshot(g, K):
    s = {"kf": [g.get_keyframe(k) for k in range(K)], "sc": g.sc_count, "n": g.num_keyframes}
    s["info"] = g.submap_info()
    return s


def same_snapshot(a, b):
    ok = a["sc"] == b["sc"] and a["n"] == b["n"]
    for (c0, s0), (c1, s1) in zip(a["kf"], b["kf"]):
        ok = ok and np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(s0), bits(s1))
    for k in a["info"]:
        ok = ok and np.array_equal(a["info"][k].view(np.uint32), b["info"][k].view(np.uint32))
    return ok


def test_verify_leaves_the_context_untouched(pcm):
    kf = loop_keyframes()
    frame_c, frame_s = kf.corner[3], kf.surf[3]

    def run(verify):
        g = filled(pcm, kf)
        g.sc_add(keyframe=0)
        g.update_submap(kf.time_cur, search_radius=50.0)
        g.set_input_source(frame_c, frame_s)
        before = snapshot(g, 5)
        if verify:
            assert g.loop_verify(4, 1, history_search_num=1, fitness_threshold=0.3).accepted
            assert g.loop_closure(kf.time_cur, radius=10.0, time_diff_s=30.0, history_search_num=1).status == "no_loop"
            assert same_snapshot(before, snapshot(g, 5))
        r1 = g.scan2map(kf.poses[3])                       # align on the target and source set before the verification
        r = g.update_submap(kf.time_cur, search_radius=50.0)
        assert not r.rebuilt                               # the submap still knows its target
        g.set_keyframe_poses(kf.poses[:1], 0)              # forces the next update to rebuild
        g.update_submap(kf.time_cur + 1.0, search_radius=49.0)
        r2 = g.scan2map(kf.poses[3])
        return r1, r2, snapshot(g, 5)

    a1, a2, sa = run(False)
    b1, b2, sb = run(True)
    for a, b in ((a1, b1), (a2, b2)):
        assert np.array_equal(bits(a.x), bits(b.x)) and (a.iterations, a.converged, a.num_corner, a.num_surf) == (b.iterations, b.converged, b.num_corner, b.num_surf)
    assert same_snapshot(sa, sb)


def test_loop_closure(pcm):
    kf = loop_keyframes()
    g = filled(pcm, kf)
    # key frames 40 s apart but fewer than 11: detectLoopClosureDistance needs loopKeyCur - id > 10 -> no candidate, no verifier
    assert g.detect_loop_distance(kf.time_cur) is None
    got = g.loop_closure(kf.time_cur, history_search_num=1)
    assert got.status == "no_loop" and (got.key_cur, got.key_pre) == (-1, -1) and not g.loop_verifier_exists
    # thirteen key frames: the track's first three, nine far away, then the loop key.  Key frames 0 and 1 lie more than 10 key
    # frames back; 1 is the nearer one
    g = pcm.LoamRegistration(0)
    order = [0, 1, 2] + [3] * 9 + [4]
    poses = kf.poses[order].copy()
    poses[3:12, 3] += 100.0
    for i, k in enumerate(order):
        g.add_keyframe(poses[i], 100.0 + 40.0 * i, kf.corner[k], kf.surf[k])
    t_cur = 100.0 + 40.0 * 12 + 0.1
    pair = g.detect_loop_distance(t_cur)
    assert pair == (12, 1)
    got = g.loop_closure(t_cur, history_search_num=1, fitness_threshold=0.3)
    assert (got.key_cur, got.key_pre) == pair and g.loop_verifier_exists
    want = g.loop_verify(pair[0], pair[1], history_search_num=1, fitness_threshold=0.3)
    assert got.status == want.status == "accepted"
    for k in ("num_cur_points", "num_prev_points", "iterations", "converged", "fitness", "noise_variance"):
        assert getattr(got, k) == getattr(want, k)
    for k in ("correction", "pose_from", "pose_to", "between", "between6"):
        assert np.array_equal(getattr(got, k), getattr(want, k))


def test_errors_leave_the_state_unchanged(pcm):
    import ctypes
    kf = loop_keyframes()
    empty = pcm.LoamRegistration(0)
    with pytest.raises(pcm.capi.PcmError) as e:
        empty.loop_verify(0, 0)
    assert e.value.code == -1 and empty.num_keyframes == 0 and not empty.loop_verifier_exists
    g = filled(pcm, kf)
    g.update_submap(kf.time_cur, search_radius=50.0)
    before = snapshot(g, 5)
    for args, params in (((5, 1), {}), ((4, -1), {}), ((-1, 1), {}), ((4, 5), {}), ((4, 1), {"wrt_key": 5}), ((4, 1), {"history_search_num": -1}),
                         ((4, 1), {"near_leaf": -1.0}), ((4, 1), {"ndt_num_neighbors": 5}), ((4, 1), {"ndt_epsilon": 0.0}), ((4, 1), {"ndt_resolution": 0.0})):
        with pytest.raises(pcm.capi.PcmError) as e:
            g.loop_verify(*args, **params)
        assert e.value.code == -1, (args, params)
    assert same_snapshot(before, snapshot(g, 5)) and not g.loop_verifier_exists
    assert not g.update_submap(kf.time_cur, search_radius=50.0).rebuilt
    # a context of another model
    ndt = pcm.PclNdtRegistration(0)
    r = pcm.capi.PcmLoamLoopResult()
    assert ndt._L.pcm_loam_loop_verify(ndt.handle, None, 0, 0, ctypes.byref(r)) == -1
    assert ndt._L.pcm_loam_loop_closure(ndt.handle, None, 10.0, 30.0, 0.0, ctypes.byref(r)) == -1
    assert ndt._L.pcm_loam_loop_verifier_exists(ndt.handle) == -1
