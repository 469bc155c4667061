"""GPU checks of pcm_lidar_filter and pcm_lio_frame_begin_cloud against the per-point restatement of the reference's handlers
(tests/lidar_handlers_ref.py).

What is compared: the kept set, its order, x y z, intensity and the zero fields byte for byte; the curvature bit for bit where the
points carry times.  On the yaw path the device's double atan2 may differ from libm's in the last bit, which can move a
curvature by one float ulp and no more: every no-time case first asserts, on the restatement's own values, that compared yaws
differ by more than 1e-6 degree (or come from bit-identical x, y) and that |b - time_last| is 0 or more than 1e-6 ms, so no
comparison can fall the other way and a difference of about 360 / 3.61 anywhere is a failure.  Curvatures that differ by one ulp
may be at most 0.1 % of the kept points; the share is taken over all kept points of a test (a sweep over sizes counts its points
together: most of its clouds keep fewer than the 1000 points at which one point is 0.1 %), and each test prints it.  First run
on an MI355X: 0 of 31 885 kept points of the two no-time sweeps and 0 of 129 510 of the two 70 400-point no-time clouds differed."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_handlers_cases as K  # noqa: E402
import lidar_handlers_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

F = np.float32
ULP_SHARE = 0.001
CASES = [(t, True) for t in K.TYPES] + [(R.VELODYNE, False), (R.RSLIDAR, False)]


def dev(a):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).cuda()
    torch.cuda.synchronize()          # the context works on a stream of its own
    return t


def filled(nbytes):
    """A device buffer of 0xAB bytes, complete before the context's stream writes into it."""
    import torch
    t = torch.full((nbytes,), 0xAB, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    return t


@pytest.fixture(scope="module")
def ctx(pcm):
    return pcm.OccupancyMap2D(0)      # a context of any model


def compare(got, want: R.Result, exact):
    """Everything but the curvature byte for byte; the curvature bit for bit (exact) or within one ulp.  -> points that differ."""
    assert got.shape == want.out.shape, (got.shape, want.out.shape)
    g, w = got.view(np.uint32), want.out.view(np.uint32)
    cols = [c for c in range(12) if c != 9]
    assert np.array_equal(g[:, cols], w[:, cols])
    d = np.abs(g[:, 9].astype(np.int64) - w[:, 9].astype(np.int64))      # finite curvatures of one sign: the ulp distance
    assert np.all(np.isfinite(want.out[:, 9]))
    assert d.max(initial=0) <= (0 if exact else 1), (int(d.max()), int(np.argmax(d)), got[np.argmax(d), 9], want.out[np.argmax(d), 9])
    return int(np.count_nonzero(d))


@pytest.mark.parametrize("t,given", CASES)
def test_sizes_and_ring_counts(pcm, ctx, t, given):
    differ = kept = 0
    for rings in K.RING_COUNTS:
        for n in K.SIZES:
            rec, d = K.sized_case(t, n, rings, given)
            want = R.handler(rec, d)
            if not given:
                K.assert_margins(want)
            got, g = ctx.lidar_filter(rec, K.to_api(d))
            assert g == want.given == (given or n == 0), (rings, n)
            differ += compare(got, want, given)
            kept += len(want.kept)
    print("type %d given %d: %d of %d kept points differ by one ulp" % (t, given, differ, kept))
    assert kept > 3000 and differ <= ULP_SHARE * kept


@pytest.fixture(scope="module")
def big():
    out = {}
    for t, given in ((R.VELODYNE, False), (R.RSLIDAR, False), (R.RSLIDAR, True)):
        rec, d = K.big_case(t, given)
        want = R.handler(rec, d)
        if not given:
            K.assert_margins(want)
            assert want.wraps > 1000
        out[(t, given)] = (rec, d, want)
    return out


@pytest.mark.parametrize("t,given", [(R.VELODYNE, False), (R.RSLIDAR, False), (R.RSLIDAR, True)])
def test_big_cloud_host_device_and_run_to_run(pcm, ctx, big, t, given):
    """70400 points: 275 scan workgroups, so the workgroup tops take two rounds, and every ring's run crosses 17 workgroups."""
    rec, d, want = big[(t, given)]
    a = K.to_api(d)
    got, g = ctx.lidar_filter(rec, a)                                  # host in, host out
    assert g == given
    differ = compare(got, want, given)
    print("type %d given %d: %d of %d kept points differ by one ulp" % (t, given, differ, len(want.kept)))
    assert differ <= ULP_SHARE * len(want.kept)
    d_rec = dev(rec)
    buf = filled((len(rec) + 2) * 48)
    m, g = ctx.lidar_filter(d_rec, a, out=buf[:len(rec) * 48])         # device in, device out
    assert m == len(got) and g == given
    b = buf.cpu().numpy()
    assert np.array_equal(b[:m * 48].view(F).reshape(m, 12).view(np.uint32), got.view(np.uint32)) and np.all(b[len(rec) * 48:] == 0xAB)
    again, _ = ctx.lidar_filter(d_rec, a)                              # device in, host out; a second run
    assert np.array_equal(again.view(np.uint32), got.view(np.uint32))
    m2, _ = ctx.lidar_filter(rec, a, out=buf[:len(rec) * 48])          # host in, device out
    assert m2 == m and np.array_equal(buf.cpu().numpy()[:m * 48], b[:m * 48])


def test_errors_leave_the_context_usable(pcm, ctx):
    rec, d = K.sized_case(R.RSLIDAR, 1025, 16, False)
    want = R.handler(rec, d)
    K.assert_margins(want)
    good = K.to_api(d)
    bad_ring = K.to_api(R.Desc(**{**d.__dict__, "num_scans": 8}))
    for cloud in (rec, dev(rec)):
        with pytest.raises(pcm.PcmError) as e:
            ctx.lidar_filter(cloud, bad_ring)
        assert e.value.code == -1 and "1025" in str(e.value) and "ring" in str(e.value)
        got, _ = ctx.lidar_filter(cloud, good)
        compare(got, want, False)
    for k, v in (("num_scans", 257), ("point_filter_num", 0), ("time_offset_bytes", 28), ("ring_offset_bytes", 31), ("time_offset_bytes", 22)):
        with pytest.raises(pcm.PcmError) as e:
            ctx.lidar_filter(rec, pcm.lidar_desc("rslidar", **{k: v}))
        assert e.value.code == -1, k
    with pytest.raises(pcm.PcmError):
        pcm.Registration(0).lio_frame_begin_cloud(rec, bad_ring)
    # an output buffer that is too small: the count is reported, nothing is written past the capacity
    buf = filled(len(want.kept) * 48)
    cap = len(want.kept) - 7
    with pytest.raises(pcm.PcmError) as e:
        ctx.lidar_filter(rec, good, out=buf[:cap * 48])
    assert e.value.code == -1 and np.all(buf.cpu().numpy()[cap * 48:] == 0xAB)
    got, _ = ctx.lidar_filter(rec, good)
    compare(got, want, False)


def _scene_cloud(synth, scene, T, n, seed, given):
    """A RoboSense cloud over real geometry: the scene's points, dealt to 16 rings."""
    sc, _ = synth.livox_scan(scene, T, n, seed)
    idx = np.arange(n)
    return K.pack_case(R.RSLIDAR, np.ascontiguousarray(sc[:, :3], F), idx % 16, idx // 16, given, seed)


@pytest.mark.parametrize("with_poses", [False, True])
@pytest.mark.parametrize("leaf", [0.0, 0.5])
def test_frame_entry_equals_the_single_operators(pcm, synth, with_poses, leaf):
    from scipy.spatial.transform import Rotation
    scene = synth.scene_for_points(1234, 100000, 8.0)
    submap = synth.sample_submap(scene, 100000, 4321)
    T = synth.sensor_pose(scene, 77)
    a = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)   # frame entry
    b = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)   # operator by operator
    c = pcm.P2PlaneRegistration(0, voxel_resolution=0.5, num_neighbors=27)   # never sees a PointCloud2 cloud
    for r in (a, b, c):
        r.set_input_target(submap)
    sc, ex = synth.livox_scan(scene, T, 20000, 5)
    msg = synth.custom_msg(sc, ex)
    n_c = c.lio_frame_begin(msg, None, leaf_size=0.5)
    livox_src = c.get_source()
    assert a.lio_frame_begin(msg, None, leaf_size=0.5) == n_c and np.array_equal(a.get_source(), livox_src)   # before

    rot = Rotation.from_matrix(T[:3, :3]).as_quat(); pos = T[:3, 3].copy()
    off_R, off_T = [0.0, 0.0, 0.0, 1.0], [0.02, -0.01, 0.03]
    poses = K.poses() if with_poses else None
    end = dict(rot_xyzw=rot, pos=pos, off_R_xyzw=off_R, off_T=off_T)
    for given, on_device in ((False, False), (True, True)):
        rec, d = _scene_cloud(synth, scene, T, 20000, 9, given)
        desc = K.to_api(d)
        n_a = a.lio_frame_begin_cloud(dev(rec) if on_device else rec, desc, poses, leaf_size=leaf, **end)
        flt, g = b.lidar_filter(rec, desc)
        assert g == given
        srt = R.stable_time_sort(flt)
        assert np.any(np.diff(flt[:, 9]) < 0)                       # the sort has work to do
        if with_poses:
            b.undistort(srt, 9, poses, rot, pos, off_R, off_T)
        ds = b.voxel_downsample(srt, leaf) if leaf > 0 else srt
        assert n_a == len(ds) and n_a > 1000
        assert np.array_equal(a.get_source().view(np.uint32), np.ascontiguousarray(ds[:, :3]).view(np.uint32))
        b.set_input_source(ds)
        for rematch in (True, False):
            ra = a.obs_model(rot, pos, off_R, off_T, False, rematch)
            rb = b.obs_model(rot, pos, off_R, off_T, False, rematch)
            assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and ra[2] == rb[2]
            assert with_poses or ra[2] > 0                           # the uncompensated scan lies in the map

    assert a.lio_frame_begin(msg, None, leaf_size=0.5) == n_c and np.array_equal(a.get_source(), livox_src)   # after
