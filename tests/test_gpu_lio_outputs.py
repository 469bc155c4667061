"""GPU checks of the jueying_lio frame outputs and the saved map (pcm_lio_frame_world .. pcm_lio_map_export)
against the numpy float64 restatement of tests/lio_outputs_ref.py.  The device and the restatement do the same IEEE double operations
in the same order and cast once to float, so every cloud is compared bit for bit (uint32 patterns).  The inputs of the restatement
are the frame's records as the single operators give them on a second context (the frame entry points equal those bit for bit:
tests/test_gpu_lio_frame.py, tests/test_gpu_lidar_handlers.py).  ``-m gpu``."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_handlers_cases as K  # noqa: E402
import lidar_handlers_ref as LR  # noqa: E402
import lio_outputs_case as case  # noqa: E402
import lio_outputs_ref as ref  # noqa: E402

pytestmark = pytest.mark.gpu
NO_INPUT, INVALID = -2, -1


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


def _poses(st):
    """11 IMU poses over the 0.1 s of a frame that end at the state `st`: a sensor moving at 1.6 m/s and turning at 0.05 rad/s."""
    from scipy.spatial.transform import Rotation
    vel, gyr = np.array([1.5, -0.5, 0.1]), np.array([0.01, -0.02, 0.05])
    R_end = Rotation.from_quat(st["rot"])
    poses = np.zeros((11, 22))
    for k in range(11):
        dt = 0.01 * (k - 10)
        poses[k, 0] = 0.01 * k; poses[k, 4:7] = gyr; poses[k, 7:10] = vel; poses[k, 10:13] = st["pos"] + vel * dt
        poses[k, 13:22] = (R_end * Rotation.from_rotvec(gyr * dt)).as_matrix().ravel()
    return poses


def _trim(b, msg, kept):
    """The shortest prefix of the message of which the driver-message filter keeps `kept` points."""
    full = b.livox_filter(msg, 6, case.POINT_FILTER_NUM, case.BLIND)
    assert len(full) >= kept
    lo, hi = kept, len(msg)
    while lo < hi:
        mid = (lo + hi) // 2
        if len(b.livox_filter(msg[:mid], 6, case.POINT_FILTER_NUM, case.BLIND)) >= kept:
            hi = mid
        else:
            lo = mid + 1
    return msg[:lo]


@pytest.fixture(scope="module")
def world(pcm):
    """The room, an operator-by-operator context, and three Livox frames: 257, 1 025 and 40 kept points (the last one down-samples to
    fewer than 64); the second is motion-compensated."""
    scene, submap, T, Tw = case.room()
    b = pcm.P2PlaneRegistration(0, **case.KW)
    st = case.state_of(Tw)
    frames = []
    for kept, seed, poses in ((257, 11, None), (1025, 12, _poses(st)), (40, 13, None)):
        msg = _trim(b, case.message(scene, T, 3000, seed), kept)
        flt = b.livox_filter(msg, 6, case.POINT_FILTER_NUM, case.BLIND)
        if poses is not None:
            b.undistort(flt, 9, poses, *case.args(st))
        ds = b.voxel_downsample(flt, case.LEAF)
        assert len(flt) == kept and len(ds) % 64 != 0 and len(ds) % 256 != 0
        frames.append(dict(msg=msg, poses=poses, dense=flt, down=ds))
    assert len(frames[2]["down"]) < 64
    return dict(scene=scene, submap=submap, T=T, Tw=Tw, b=b, state=st, frames=frames)


def _begin(g, f, st, leaf=case.LEAF):
    return g.lio_frame_begin(f["msg"], f["poses"], *case.args(st), num_scans=6, point_filter_num=case.POINT_FILTER_NUM, blind=case.BLIND, leaf_size=leaf)


@pytest.mark.parametrize("sort_source", [0, 1])
def test_world_and_body_clouds_bit_for_bit(pcm, world, sort_source):
    import torch
    st = world["state"]
    g = pcm.P2PlaneRegistration(0, sort_source=sort_source, **case.KW)
    g.set_input_target(world["submap"])
    for f in world["frames"]:
        assert _begin(g, f, st) == len(f["down"])
        if sort_source and len(f["down"]) >= 5:
            g.obs_model(*case.args(st), False, True)        # the scan is re-ordered inside; the outputs keep the caller's order
        want = dict(dense=ref.frame_world(st, f["dense"]), down=ref.frame_world(st, f["down"]), body=ref.frame_body(st, f["dense"]))
        assert np.all(want["dense"][:, :3] < 0)
        for key, call in (("dense", lambda out=None: g.lio_frame_world(*case.args(st), dense=True, out=out)),
                          ("down", lambda out=None: g.lio_frame_world(*case.args(st), dense=False, out=out)),
                          ("body", lambda out=None: g.lio_frame_body(*case.args(st), out=out))):
            host = call()
            assert same(host, want[key]), key
            d = torch.full((len(host) + 3, 4), 7.0, device="cuda")
            assert call(d) == len(host)
            back = d.cpu().numpy()
            assert same(back[:len(host)], want[key]) and np.all(back[len(host):] == 7.0), key
    assert np.array_equal(g.get_source(), np.ascontiguousarray(world["frames"][2]["down"][:, :3]))    # the frame calls are untouched


def test_cloud_entry_frame(pcm, world):
    """A PointCloud2 frame (RoboSense, 1 025 points) through pcm_lio_frame_begin_cloud: time-sorted, compensated, down-sampled."""
    st, b = world["state"], world["b"]
    rec, d = K.sized_case(LR.RSLIDAR, 1025, 16, False)
    desc = K.to_api(d)
    g = pcm.P2PlaneRegistration(0, **case.KW)
    poses = K.poses()
    n = g.lio_frame_begin_cloud(rec, desc, poses, *case.args(st), leaf_size=case.LEAF)
    flt, _ = b.lidar_filter(rec, desc)
    srt = LR.stable_time_sort(flt)
    b.undistort(srt, 9, poses, *case.args(st))
    ds = b.voxel_downsample(srt, case.LEAF)
    assert n == len(ds) and len(srt) % 64 != 0
    assert same(g.lio_frame_world(*case.args(st), dense=True), ref.frame_world(st, srt))
    assert same(g.lio_frame_world(*case.args(st), dense=False), ref.frame_world(st, ds))
    assert same(g.lio_frame_body(*case.args(st)), ref.frame_body(st, srt))


@pytest.fixture(scope="module")
def effect(world, pcm):
    sc = case.effect_scene()
    b = world["b"]
    flt = b.livox_filter(sc.msg, 6, case.POINT_FILTER_NUM, case.BLIND)
    ds = b.voxel_downsample(flt, case.LEAF)
    return sc, dict(msg=sc.msg, poses=None, dense=flt, down=ds)


@pytest.mark.parametrize("ref_semantics", [False, True])
def test_effect_cloud(pcm, effect, ref_semantics):
    """Count = n_eff of the last ObsModel call (pcm_obs_model, then pcm_lio_update) and records = the restatement fed the flags the
    library reports (pcm_get_lio_members; pcm_get_planes + the float row test), with sort_source off and on."""
    import lio_iekf_ref as iekf
    sc, f = effect
    st, n = sc.state, len(f["down"])
    xyz = f["down"][:, :3]
    out_state = case.state_of(sc.T_world)                         # the clouds may be published with any state
    expected = {}
    for sort_source in (0, 1):
        g = pcm.P2PlaneRegistration(0, sort_source=sort_source, flags=4 if ref_semantics else 0, **case.KW)
        g.set_input_target(sc.submap)
        with pytest.raises(pcm.PcmError) as e:
            g.lio_frame_effect(*case.args(out_state))
        assert e.value.code == NO_INPUT
        assert _begin(g, f, st) == n
        with pytest.raises(pcm.PcmError) as e:                    # a frame, but no ObsModel call yet
            g.lio_frame_effect(*case.args(out_state))
        assert e.value.code == NO_INPUT
        # -- pcm_obs_model
        n_eff = g.obs_model(*case.args(st), False, True)[2]
        got = g.lio_frame_effect(*case.args(out_state))
        assert len(got) == n_eff and 0 < n_eff < n
        if ref_semantics:
            flags = g.get_lio_members(n)[1]
        elif sort_source == 0:
            planes = g.get_planes(n)
            flags = ref.default_selected(st, xyz, planes)
            assert np.isnan(planes[:, 0]).any() and (~np.isnan(planes[:, 0]) & ~flags).any()      # both halves of the flag at work
        else:
            flags = expected["obs_flags"]                           # the planes lie in the re-ordered order: the unsorted run's flags
        assert flags.sum() == n_eff
        assert same(got, ref.frame_effect(out_state, f["down"], flags))
        if sort_source == 0:
            expected["obs_flags"] = flags
        else:
            assert np.array_equal(flags, expected["obs_flags"])
        # -- pcm_lio_update: the flags at the state of its last executed call
        x0 = iekf.make_state(pos=st["pos"], rot=st["rot"], off_R=st["off_R"], off_T=st["off_T"], grav=(0.0, 0.0, -iekf.LENGTH))
        r = g.lio_update(x0, np.diag(iekf.INIT_P_DIAG))
        last = g.lio_update_trace(r.iterations - 1)
        xs = r.x
        upd_state = dict(rot=xs["rot"], pos=xs["pos"], off_R=xs["off_R"], off_T=xs["off_T"])
        import torch
        d = torch.zeros((n, 4), device="cuda")
        k = g.lio_frame_effect(*case.args(upd_state), out=d)
        assert k == r.n_eff_last == last["n_eff"] and k > 0
        if ref_semantics:
            flags = g.get_lio_members(n)[1]
        elif sort_source == 0:
            flags = ref.default_selected(last["x"], xyz, g.get_planes(n))
        else:
            flags = expected["upd_flags"]
        assert flags.sum() == k
        assert same(d.cpu().numpy()[:k], ref.frame_effect(upd_state, f["down"], flags))
        if sort_source == 0:
            expected["upd_flags"] = flags
        # too small a buffer: the count, nothing written
        small = np.full((k - 1, 4), 5.0, np.float32)
        with pytest.raises(pcm.PcmError) as e:
            g.lio_frame_effect(*case.args(upd_state), out=small)
        assert e.value.code == INVALID and "has %d" % k in str(e.value) and np.all(small == 5.0)


def test_saved_map_log(pcm, world):
    st = world["state"]
    g = pcm.P2PlaneRegistration(0, **case.KW)
    assert g.lio_map_info()["points"] == 0 and len(g.lio_map_export()) == 0
    m = ref.SavedMap()
    order = [0, 1, 2, 1, 0, 1, 1]
    fired = []
    for k, i in enumerate(order):
        f = world["frames"][i]
        dense = k % 2 == 0
        _begin(g, f, st)
        info = g.lio_map_append(*case.args(st), dense=dense, pcd_save_interval=-1)
        m.append(ref.frame_world(st, f["dense"] if dense else f["down"]), -1)
        assert info["points"] == len(m.cloud()) and info["frames_appended"] == k + 1 and not info["chunk_ready"] and info["capacity"] >= info["points"]
        fired.append(info["chunk_ready"])
    want = m.cloud()
    info = g.lio_map_info()
    assert info["growths"] >= 2 and info["scan_wait_num"] == len(order) and info["pcd_index"] == 0      # interval <= 0: never a chunk
    assert same(g.lio_map_get(), want) and same(g.lio_map_export(), want)
    n0 = len(m.frames[0])
    assert same(g.lio_map_get(0, 1), want[:1]) and same(g.lio_map_get(len(want) - 1, 1), want[-1:]) and len(g.lio_map_get(len(want), 0)) == 0
    assert same(g.lio_map_get(n0 - 3, 9), want[n0 - 3:n0 + 6])                                      # across a frame boundary
    with pytest.raises(pcm.PcmError) as e:
        g.lio_map_get(len(want) - 1, 2)
    assert e.value.code == INVALID
    import torch
    d = torch.zeros((len(want), 4), device="cuda")
    assert g.lio_map_get(5, 100, out=d) == 100 and same(d.cpu().numpy()[:100], want[5:105])
    # export: z window, leaf, both
    z = np.sort(want[:, 2].astype(np.float64))
    z_min, z_max = float(z[len(z) // 4]), float(z[3 * len(z) // 4])
    win = g.lio_map_export(0.0, z_min, z_max)
    assert same(win, ref.export(want, 0.0, z_min, z_max)) and 0 < len(win) < len(want)
    cells, _ = g.voxel_downsample_large(want, 0.4)
    assert same(g.lio_map_export(0.4), cells) and 0 < len(cells) < len(want)
    assert same(g.lio_map_export(0.4, z_min, z_max), ref.pass_through_z(cells, z_min, z_max))
    assert g.lio_map_export(0.4, z_min, z_max, out=d) == len(ref.pass_through_z(cells, z_min, z_max))
    small = np.full((len(want) - 1, 4), 5.0, np.float32)
    with pytest.raises(pcm.PcmError) as e:
        g.lio_map_export(out=small)
    assert e.value.code == INVALID and np.all(small == 5.0)
    # chunks: interval 2 fires on the 2nd and 4th append, with a clear between
    g.lio_map_clear()
    assert g.lio_map_info()["points"] == 0 and g.lio_map_info()["scan_wait_num"] == 0 and g.lio_map_info()["capacity"] == info["capacity"]
    m = ref.SavedMap()
    seen = []
    for k in range(4):
        f = world["frames"][k % 3]
        _begin(g, f, st)
        i2 = g.lio_map_append(*case.args(st), dense=False, pcd_save_interval=2)
        ready, index = m.append(ref.frame_world(st, f["down"]), 2)
        assert i2["chunk_ready"] == ready and i2["pcd_index"] == index
        seen.append((i2["chunk_ready"], i2["pcd_index"]))
        if ready:
            assert same(g.lio_map_get(), m.cloud())
            g.lio_map_clear(); m.clear()
    assert seen == [(False, 0), (True, 1), (False, 1), (True, 2)]


def test_refusals(pcm, world):
    st, f = world["state"], world["frames"][0]
    g = pcm.P2PlaneRegistration(0, **case.KW)
    calls = (lambda: g.lio_frame_world(*case.args(st)), lambda: g.lio_frame_world(*case.args(st), dense=True), lambda: g.lio_frame_body(*case.args(st)),
             lambda: g.lio_frame_effect(*case.args(st)), lambda: g.lio_map_append(*case.args(st)))

    def refused(who):
        for c in calls:
            with pytest.raises(pcm.PcmError) as e:
                c()
            assert e.value.code == NO_INPUT and (who is None or who in str(e.value)), str(e.value)

    refused(None)                                                   # before any frame
    _begin(g, f, st)
    assert len(g.lio_frame_world(*case.args(st))) == len(f["down"])
    g.set_input_source(f["down"])
    refused("pcm_set_source")
    _begin(g, f, st)
    g.voxel_downsample(f["dense"], 0.5)
    refused("pcm_voxel_downsample")
    _begin(g, f, st)
    g.livox_filter(f["msg"], 6, 1, 0.1)
    refused("pcm_livox_filter")
    _begin(g, f, st)
    n = len(f["dense"])
    small = np.full((n - 1, 4), 5.0, np.float32)
    with pytest.raises(pcm.PcmError) as e:
        g.lio_frame_world(*case.args(st), dense=True, out=small)
    assert e.value.code == INVALID and "has %d" % n in str(e.value) and np.all(small == 5.0)
    import ctypes as C
    cnt = C.c_size_t()
    assert g._L.pcm_lio_frame_world(g._h, None, 1, None, 0, 0, C.byref(cnt)) == INVALID            # null state
    assert g._L.pcm_lio_frame_body(g._h, None, None, 0, 0, C.byref(cnt)) == INVALID
    assert g._L.pcm_lio_frame_effect(g._h, None, None, 0, 0, C.byref(cnt)) == INVALID
    assert g._L.pcm_lio_map_append(g._h, None, 0, -1, None) == INVALID
    assert g.lio_map_info()["points"] == 0


def test_odometry_with_the_saved_map_changes_nothing_else(pcm, synth):
    """LioOdometry over 3 init frames, the first scan and 3 frames with pcd_save_en on and off: the same stages, poses bit for bit
    and the same map; the saved map holds the three registered frames and interval 2 gives one chunk."""
    import lio_iekf_ref as iekf
    import lio_predict_case as pc
    scene = synth.scene_for_points(4321, 20000, 8.0)
    T = np.eye(4); T[:3, 3] = synth.sensor_pose(scene, 12)[:3, 3]
    rng = np.random.default_rng(31)
    frames, t = [], 50.0
    for f in range(7):
        n = 8 if f < 3 else 20
        imu = pc.samples(rng, n, t0=t)
        imu[:, 1:4] = np.array([0.0, 0.0, 9.81]) + 0.01 * rng.normal(size=(n, 3))
        imu[:, 4:7] = 0.002 * rng.normal(size=(n, 3))
        sc, ex = synth.livox_scan(scene, T, 2000, 900 + f, point_filter_num=1)
        frames.append((synth.custom_msg(sc, ex), imu, t + 0.001, imu[-1, 0] + 0.001))
        t = imu[-1, 0]
    runs = []
    for save in (False, True):
        g = pcm.P2PlaneRegistration(0, **case.KW)
        od = pcm.LioOdometry(g, x=iekf.make_state(), filter_size_map=0.5, pcd_save_en=save, dense_pub_en=True, pcd_save_interval=2,
                             num_scans=6, point_filter_num=1, blind=0.1, leaf_size=0.5)
        stages, states, worlds = [], [], []
        for msg, imu, tb, te in frames:
            stages.append(od.process(msg, imu, tb, te))
            states.append(iekf.state_to_vec(od.x).copy())
            if save and stages[-1] == "updated":
                worlds.append(g.lio_frame_world(*od._pose_args(), dense=True))
        runs.append(dict(stages=stages, states=np.array(states), P=od.P.copy(), target=g.get_target(), od=od, worlds=worlds))
    a, b = runs
    assert a["stages"] == b["stages"] == ["init"] * 3 + ["first_scan"] + ["updated"] * 3
    assert np.array_equal(a["states"].view(np.uint64), b["states"].view(np.uint64)) and np.array_equal(a["P"].view(np.uint64), b["P"].view(np.uint64))
    assert same(a["target"], b["target"])
    assert a["od"].finish() is None and a["od"].chunks == []
    od, w = b["od"], b["worlds"]
    assert [i for i, _ in od.chunks] == [1] and same(od.chunks[0][1], np.concatenate(w[:2]))
    assert same(od.finish(), w[2])
