"""GPU checks of performSCLoopClosure on the device (pcm_loam_sc_loop_verify, pcm_loam_sc_loop_closure): a verification equals
the composition it replaces on the same context state -- near_keyframes(..., wrt_key=0) x 2 -> a fresh icp.IterativeClosestPoint
with the settings of mapOptmization.cpp:769-772 -> align -> get_fitness_score -> the numpy restatement of :817-834
(tests/icp_ref.py) -- with the correction and the fitness as equalities; every rejection status; and nothing of the LOAM context
(key frames, Scan Context store, target, source, the NDT verifier) is touched.  Six key frames of about 470 features; the gates
are lowered through the params.

Tolerance of `between`: the header (loam_loop.h) and the restatement take the same double sin / cos of the same six numbers and
differ in the order of three-term sums of products of entries <= 3 (a few ulp of 3): 1e-12, as tests/test_icp.py; `pose_from`
is an equality."""
import ctypes
import importlib
import math

import numpy as np
import pytest

import icp_ref as R

pytestmark = pytest.mark.gpu

synth = importlib.import_module("pointcloud-slam_amd.synth")
synth_keyframes = importlib.import_module("pointcloud-slam_amd.synth_keyframes")
synth_loam = importlib.import_module("pointcloud-slam_amd.synth_loam")
_CACHE = {}
K_FRAMES, CUR, PRE = 6, 5, 1
PARAMS = dict(history_search_num=1, min_cur_points=100, min_prev_points=300)


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def keyframes():
    """Six key frames 0.5 m apart along a short track through a small synth_loam scene; the stored pose of the last one is off by
    0.3 m / 2 degrees, the drift the verification measures."""
    if "kf" in _CACHE:
        return _CACHE["kf"]
    scene = synth.make_scene(5, 4.0, n_boxes=10, n_cyls=3)
    rng = np.random.default_rng(12)
    pool_c = synth_loam._sample_edges(synth_loam._segments(scene), 6000, rng, 0.01)
    pool_s = synth_loam._sample_planes(scene, 24000, rng, 0.01)
    cx, cy = 0.5 * scene.lx - 1.0, 0.5 * scene.ly
    true = np.array([[rng.normal(0, 0.01), rng.normal(0, 0.01), 0.05 * k, cx + 0.5 * k, cy + 0.1 * k, 1.5] for k in range(K_FRAMES)], np.float32)
    corner, surf = [], []
    for k in range(K_FRAMES):
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
    stored[CUR, 2] += np.float32(math.radians(2.0))
    stored[CUR, 3] += np.float32(0.3 * math.cos(0.7)); stored[CUR, 4] += np.float32(0.3 * math.sin(0.7))
    times = 100.0 + 40.0 * np.arange(K_FRAMES)
    _CACHE["kf"] = synth_keyframes.KeyFrames(stored, times.astype(np.float64), corner, surf, float(times[-1] + 0.1))
    return _CACHE["kf"]


def filled(pcm, kf):
    g = pcm.LoamRegistration(0)
    for k in range(len(kf.times)):
        assert g.add_keyframe(kf.poses[k], kf.times[k], kf.corner[k], kf.surf[k]) == k
    return g


def composition(g, key_cur, key_pre, history_search_num=1, near_leaf=0.2, max_corr=150.0, **_):
    """today's path through the host, on the same context state"""
    from pointcloud_slam_amd import icp
    cur = g.near_keyframes(key_cur, 0, 0, near_leaf)
    prev = g.near_keyframes(key_pre, history_search_num, 0, near_leaf)
    v = icp.IterativeClosestPoint(0, voxel_resolution=1.0, max_iterations=100, max_correspondence_distance=max_corr, transformation_epsilon=1e-6,
                                  euclidean_fitness_epsilon=1e-6)
    v.set_input_target(prev)
    v.set_input_source(cur)
    r = v.align()
    return cur, prev, r, v.get_fitness_score(), v.get_fitness_score(T=np.eye(4))


def accepted(pcm):
    from pointcloud_slam_amd import loam
    if "acc" not in _CACHE:
        g = filled(pcm, keyframes())
        got = loam.loam_sc_loop_verify(g, CUR, PRE, **PARAMS)
        _CACHE["acc"] = (g, got, composition(g, CUR, PRE))
    return _CACHE["acc"]


def test_accepted_equals_composition(pcm):
    from pointcloud_slam_amd import capi, loam
    g, got, (cur, prev, r, fitness, fitness_identity) = accepted(pcm)
    print("clouds:", got.num_cur_points, got.num_prev_points, "iterations:", got.icp_iterations, "stop:", got.icp_stop_reason, "fitness:", got.fitness)
    assert (got.num_cur_points, got.num_prev_points) == (len(cur), len(prev)) and 300 <= len(cur) <= 520 and 1000 <= len(prev) <= 1500
    assert got.accepted and got.icp_converged and got.icp_iterations == r.iterations >= 1 and (got.key_cur, got.key_pre) == (CUR, PRE)
    assert np.array_equal(bits(got.correction), bits(r.T)) and got.fitness == fitness
    assert got.icp_stop_reason in (capi.PCM_ICP_STOP_ITERATIONS, capi.PCM_ICP_STOP_TRANSFORM, capi.PCM_ICP_STOP_ABS_MSE, capi.PCM_ICP_STOP_REL_MSE)
    pf, B, b6 = R.sc_between(got.correction)
    assert np.array_equal(got.pose_from, pf) and not got.pose_to.any()
    for name, a, b in (("between", got.between, B), ("between6", got.between6, b6)):
        d = np.abs(a - b).max()
        print(name, "worst |difference| =", d)
        assert d <= 1e-12
    assert (got.noise_variance, got.cauchy_k, got.yaw_diff_rad) == (0.5, 1.0, 0.0)
    # with every pair kept (150 m) an ICP step never raises the mean squared nearest-neighbour distance (Besl & McKay 1992,
    # the convergence theorem), so the clouds end nearer each other than they started; how near is the operator's business on
    # two differently sampled clouds of 423 and 1201 points
    print("fitness at the identity:", fitness_identity, "after:", got.fitness)
    assert got.fitness < fitness_identity and got.fitness < 0.3
    # a second verification on the same verifier gives the same bits
    again = loam.loam_sc_loop_verify(g, CUR, PRE, **PARAMS)
    assert np.array_equal(bits(again.correction), bits(got.correction)) and again.fitness == got.fitness and np.array_equal(again.between, got.between)
    assert loam.loam_sc_loop_verifier_exists(g) and not g.loop_verifier_exists   # the NDT verifier was never created


def test_rejections(pcm):
    from pointcloud_slam_amd import capi, loam
    g, acc, _ = accepted(pcm)
    # size: one below each gate, then exactly at the gates
    nc, npv = acc.num_cur_points, acc.num_prev_points
    for gates, rejected in (((nc + 1, npv), True), ((nc, npv + 1), True), ((nc, npv), False)):
        got = loam.loam_sc_loop_verify(g, CUR, PRE, history_search_num=1, min_cur_points=gates[0], min_prev_points=gates[1])
        assert (got.status == "rejected_size") == rejected and (got.num_cur_points, got.num_prev_points) == (nc, npv)
        if rejected:
            assert got.icp_iterations == 0 and got.icp_stop_reason == capi.PCM_ICP_STOP_NONE and np.array_equal(got.correction, np.eye(4, dtype=np.float32))
    fresh = filled(pcm, keyframes())
    assert loam.loam_sc_loop_verify(fresh, CUR, PRE, history_search_num=1, min_cur_points=10 ** 6).status == "rejected_size"
    assert not loam.loam_sc_loop_verifier_exists(fresh)   # ICP did not run: the verifier was never created
    # not converged: no pair within a millimetre -> fewer than 3 correspondences
    got = loam.loam_sc_loop_verify(g, CUR, PRE, icp_max_correspondence_distance=1e-3, **PARAMS)
    assert got.status == "rejected_not_converged" and not got.icp_converged and got.icp_stop_reason == capi.PCM_ICP_STOP_NO_CORRESPONDENCES
    assert np.array_equal(got.correction, np.eye(4, dtype=np.float32)) and not got.between.any()
    # fitness: a threshold below the measured fitness of the accepted case
    got = loam.loam_sc_loop_verify(g, CUR, PRE, fitness_threshold=0.5 * acc.fitness, **PARAMS)
    assert got.status == "rejected_fitness" and got.icp_converged and got.fitness == acc.fitness
    assert np.array_equal(bits(got.correction), bits(acc.correction)) and not got.between.any() and not got.between6.any()


def snapshot(g):
    s = {"kf": [g.get_keyframe(k) for k in range(K_FRAMES)], "sc": g.sc_count, "n": g.num_keyframes, "info": g.submap_info()}
    s["desc"] = [g.sc_get(i) for i in range(g.sc_count)]
    return s


def same_snapshot(a, b):
    ok = a["sc"] == b["sc"] and a["n"] == b["n"]
    for (c0, s0), (c1, s1) in zip(a["kf"], b["kf"]):
        ok = ok and np.array_equal(bits(c0), bits(c1)) and np.array_equal(bits(s0), bits(s1))
    for k in a["info"]:
        ok = ok and np.array_equal(a["info"][k].view(np.uint32), b["info"][k].view(np.uint32))
    for x, y in zip(a["desc"], b["desc"]):
        ok = ok and all(np.array_equal(u, v) for u, v in zip(x, y))
    return ok


def test_context_and_ndt_verifier_are_untouched(pcm):
    from pointcloud_slam_amd import loam
    kf = keyframes()

    def run(verify):
        g = filled(pcm, kf)
        g.sc_add(keyframe=0)
        g.update_submap(kf.time_cur, search_radius=50.0)
        g.set_input_source(kf.corner[3], kf.surf[3])
        ndt0 = g.loop_verify(CUR, PRE, history_search_num=1)   # creates the NDT verifier
        before = snapshot(g)
        if verify:
            assert loam.loam_sc_loop_verify(g, CUR, PRE, **PARAMS).accepted
            assert loam.loam_sc_loop_closure(g, **PARAMS).status == "no_loop"   # one descriptor: no search set, no loop
            assert same_snapshot(before, snapshot(g))
        ndt1 = g.loop_verify(CUR, PRE, history_search_num=1)
        assert np.array_equal(bits(ndt0.correction), bits(ndt1.correction)) and ndt0.fitness == ndt1.fitness and ndt0.iterations == ndt1.iterations
        r1 = g.scan2map(kf.poses[3])                       # align on the target and source set before the verification
        assert not g.update_submap(kf.time_cur, search_radius=50.0).rebuilt   # the submap still knows its target
        return r1, snapshot(g)

    a, sa = run(False)
    b, sb = run(True)
    assert np.array_equal(bits(a.x), bits(b.x)) and (a.iterations, a.converged, a.num_corner, a.num_surf) == (b.iterations, b.converged, b.num_corner, b.num_surf)
    assert same_snapshot(sa, sb)


def test_closure_without_a_loop(pcm):
    from pointcloud_slam_amd import loam
    empty = pcm.LoamRegistration(0)
    got = loam.loam_sc_loop_closure(empty)
    assert got.status == "no_loop" and (got.key_cur, got.key_pre) == (-1, -1)   # :737 no key pose: nothing to do
    g = filled(pcm, keyframes())
    assert loam.loam_sc_loop_closure(g, **PARAMS).status == "no_loop"           # no descriptor
    for k in range(K_FRAMES):
        g.sc_add(keyframe=k)
    got = loam.loam_sc_loop_closure(g, **PARAMS)   # six descriptors, all inside num_exclude_recent: detectLoopClosureID finds nothing
    assert g.sc_detect().loop_id == -1
    assert got.status == "no_loop" and (got.key_cur, got.key_pre) == (-1, -1) and not loam.loam_sc_loop_verifier_exists(g)
    assert got.icp_iterations == 0 and np.array_equal(got.correction, np.eye(4, dtype=np.float32))


def test_errors_leave_the_state_unchanged(pcm):
    from pointcloud_slam_amd import capi, loam
    empty = pcm.LoamRegistration(0)
    with pytest.raises(capi.PcmError) as e:
        loam.loam_sc_loop_verify(empty, 0, 0)
    assert e.value.code == -1 and not loam.loam_sc_loop_verifier_exists(empty)
    kf = keyframes()
    g = filled(pcm, kf)
    g.update_submap(kf.time_cur, search_radius=50.0)
    before = snapshot(g)
    for args, params in (((K_FRAMES, 1), {}), ((CUR, -1), {}), ((-1, 1), {}), ((CUR, K_FRAMES), {}), ((CUR, PRE), {"history_search_num": -1}),
                         ((CUR, PRE), {"near_leaf": -1.0}), ((CUR, PRE), {"icp_max_iterations": 0}), ((CUR, PRE), {"icp_max_correspondence_distance": 0.0}),
                         ((CUR, PRE), {"icp_transformation_epsilon": float("nan")}), ((CUR, PRE), {"icp_voxel_resolution": 0.0}),
                         ((CUR, PRE), {"fitness_threshold": float("nan")}), ((CUR, PRE), {"min_cur_points": -1})):
        with pytest.raises(capi.PcmError) as e:
            loam.loam_sc_loop_verify(g, *args, **params)
        assert e.value.code == -1, (args, params)
    with pytest.raises(capi.PcmError) as e:
        loam.loam_sc_loop_closure(g, icp_max_iterations=0)
    assert e.value.code == -1
    with pytest.raises(KeyError):
        loam.loam_sc_loop_verify(g, CUR, PRE, no_such_field=1)
    assert same_snapshot(before, snapshot(g)) and not loam.loam_sc_loop_verifier_exists(g) and not g.loop_verifier_exists
    assert not g.update_submap(kf.time_cur, search_radius=50.0).rebuilt
    other = pcm.PclNdtRegistration(0)   # a context of another model
    r = capi.PcmLoamScLoopResult()
    assert other._L.pcm_loam_sc_loop_verify(other.handle, None, 0, 0, ctypes.byref(r)) == -1
    assert other._L.pcm_loam_sc_loop_closure(other.handle, None, ctypes.byref(r)) == -1
    assert other._L.pcm_loam_sc_loop_verifier_exists(other.handle) == -1
