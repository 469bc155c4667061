"""CPU checks of the PointCloud2 handler arithmetic (pointcloud-slam_amd/csrc/lidar_handlers.h, compiled with g++ through
tests/lidar_handlers_hooks.cpp) against the per-point Python restatement of the reference's handlers
(tests/lidar_handlers_ref.py), bit for bit -- both sides use libm's atan2 --: the four handlers with and without point times, the
serial chain against its composition form in three groupings, ties, a NaN in mid-ring, both blind-test edges, the candidate
stride, the dropped first point of a ring, given_offset_time, the descriptor rules, the struct layouts and the sort key.  No GPU."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lidar_handlers_cases as K  # noqa: E402
import lidar_handlers_ref as R  # noqa: E402

F = np.float32


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    from pointcloud_slam_amd import capi
    so = str(tmp_path_factory.mktemp("lidar_hooks") / "lidar_handlers_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "lidar_handlers_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.lh_hook_filter.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(capi.PcmLidarDesc), C.c_void_p, C.c_size_t, C.POINTER(C.c_size_t), C.POINTER(C.c_int),
                                 C.POINTER(C.c_uint), C.c_char_p, C.c_size_t]
    L.lh_hook_defaults.argtypes = [C.c_int, C.POINTER(capi.PcmLidarDesc)]
    L.lh_hook_defaults.restype = None
    L.lh_hook_time_key.argtypes = [C.c_float]
    L.lh_hook_time_key.restype = C.c_uint
    L.lh_hook_yaw.argtypes = [C.c_float, C.c_float]
    L.lh_hook_yaw.restype = C.c_double
    L.lh_hook_b.argtypes = [C.c_double, C.c_double]
    L.lh_hook_b.restype = C.c_float
    L.lh_hook_chain.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_int, C.c_void_p]
    L.lh_hook_chain.restype = None
    L.lh_hook_layout.argtypes = [C.c_void_p]
    return L


def api_desc(H, d: R.Desc):
    """The binding's struct of a restatement descriptor, filled without the HIP library."""
    from pointcloud_slam_amd import capi, registration as reg
    a = capi.PcmLidarDesc()
    H.lh_hook_defaults(d.type, C.byref(a))
    a.time_kind, a.ring_kind = reg.LIDAR_TIME_KIND[d.time_kind], reg.LIDAR_RING_KIND[d.ring_kind]
    for k in ("num_scans", "point_filter_num", "time_scale", "stride_bytes", "xyz_offset_bytes", "intensity_offset_bytes", "time_offset_bytes", "ring_offset_bytes", "blind"):
        setattr(a, k, getattr(d, k))
    return a


def hook(H, rec, d, capacity=None):
    """(rc, (m, 12) float32 records, given, bad rings, why) of the header's serial loop."""
    n = rec.shape[0]
    cap = n if capacity is None else capacity
    out = np.full((max(cap, 1), 12), np.nan, F)
    m, given, bad = C.c_size_t(), C.c_int(), C.c_uint()
    why = C.create_string_buffer(256)
    a = api_desc(H, d)
    rec = np.ascontiguousarray(rec)
    rc = H.lh_hook_filter(rec.ctypes.data, n, C.byref(a), out.ctypes.data, cap, C.byref(m), C.byref(given), C.byref(bad), why, 256)
    return rc, out[:min(m.value, cap)], bool(given.value), bad.value, why.value.decode()


def both(H, rec, d):
    want = R.handler(rec, d)
    rc, out, given, bad, why = hook(H, rec, d)
    assert rc == 0 and bad == 0, why
    assert given == want.given
    assert out.shape == want.out.shape and np.array_equal(out.view(np.uint32), want.out.view(np.uint32))
    return want


def test_layout_and_defaults(H):
    from pointcloud_slam_amd import capi
    o = (C.c_long * 16)()
    H.lh_hook_layout(o)
    S = capi.PcmLidarDesc
    assert list(o) == [C.sizeof(S), S.type.offset, S.time_kind.offset, S.ring_kind.offset, S.num_scans.offset, S.point_filter_num.offset, S.time_scale.offset,
                       S.stride_bytes.offset, S.xyz_offset_bytes.offset, S.intensity_offset_bytes.offset, S.time_offset_bytes.offset, S.ring_offset_bytes.offset,
                       S.blind.offset, S.reserved.offset, capi.PCM_ABI_VERSION, capi.PCM_LIDAR_MAX_SCANS]
    assert capi.PCM_ABI_VERSION == 3
    assert (capi.PCM_LIDAR_VELODYNE, capi.PCM_LIDAR_OUSTER, capi.PCM_LIDAR_RSLIDAR, capi.PCM_LIDAR_LIVOX_STD) == (R.VELODYNE, R.OUSTER, R.RSLIDAR, R.LIVOX_STD)
    for name in ("pcm_lidar_default_desc", "pcm_lidar_filter", "pcm_lio_frame_begin_cloud"):
        assert name in capi.SYMBOLS
    # the reference's PCL structs (EIGEN_ALIGN16) and config files
    want = {R.VELODYNE: (32, 16, 20, "f32", 24, "u16", 16, 1, 0.5, 1e3), R.RSLIDAR: (32, 16, 24, "f64", 20, "u16", 16, 1, 0.5, 1000.0),
            R.LIVOX_STD: (32, 16, 24, "f64", None, None, 6, 2, 0.1, 1000.0), R.OUSTER: (48, 16, 20, "u32", 26, "u8", 64, 3, 4.0, 1e-3)}
    from pointcloud_slam_amd import registration as reg
    for t, (stride, ioff, toff, tk, roff, rk, scans, pfn, blind, ts) in want.items():
        a = capi.PcmLidarDesc()
        H.lh_hook_defaults(t, C.byref(a))
        d = R.default_desc(t)
        assert (a.stride_bytes, a.xyz_offset_bytes, a.intensity_offset_bytes, a.time_offset_bytes, a.time_kind) == (stride, 0, ioff, toff, reg.LIDAR_TIME_KIND[tk])
        assert (a.num_scans, a.point_filter_num, a.blind, a.time_scale) == (scans, pfn, blind, F(ts))
        if roff is not None:
            assert (a.ring_offset_bytes, a.ring_kind) == (roff, reg.LIDAR_RING_KIND[rk])
        assert (d.stride_bytes, d.intensity_offset_bytes, d.time_offset_bytes, d.time_kind, d.num_scans, d.point_filter_num, d.blind) == (stride, ioff, toff, tk, scans, pfn, blind)
        assert all(v == 0 for v in a.reserved)


# Ouster and Livox clouds always carry times
HANDLER_CASES = [(t, True) for t in K.TYPES] + [(R.VELODYNE, False), (R.RSLIDAR, False)]


@pytest.mark.parametrize("t,given", HANDLER_CASES)
@pytest.mark.parametrize("pfn", [1, 2, 3])
def test_handlers_bit_for_bit(H, t, given, pfn):
    rec, d = K.sized_case(t, 1500, 16, given, point_filter_num=pfn)
    want = both(H, rec, d)
    assert want.given == given and 0 < len(want.kept) < 1500
    assert np.all(want.kept % pfn == 0)                      # the candidate stride is on the original index
    if not given:
        K.assert_margins(want)
        assert want.wraps > 0                                 # more than one revolution: the + 360 / 3.61 branch is taken ...
        wrapped = want.out[:, 9] > 360.0 / 3.61
        assert wrapped.any() and wrapped[np.flatnonzero(wrapped)[0]:].sum() > 16   # ... and persists
    if given and t == R.RSLIDAR:
        assert (want.out[:, 9] < 0).any()                    # stamps below the first point's: negative curvatures


@pytest.mark.parametrize("t", K.TYPES)
@pytest.mark.parametrize("n", [0, 1, 2, 65])
@pytest.mark.parametrize("rings", [1, 128])
def test_small_sizes(H, t, n, rings):
    for given in ([True, False] if t in (R.VELODYNE, R.RSLIDAR) else [True]):
        rec, d = K.sized_case(t, n, rings, given)
        both(H, rec, d)
    if n == 0:
        rc, out, given, bad, _ = hook(H, np.zeros((0, R.default_desc(t).stride_bytes), np.uint8), R.default_desc(t))
        assert (rc, len(out), given) == (0, 0, True)          # pinned: the reference reads points[-1]


def ring_chain(n_rev=2.6, n=400, seed=5):
    """b and first flags of one ring spun over n_rev revolutions, from the restatement's own yaw arithmetic."""
    rng = np.random.default_rng(seed)
    az = 77.0 - np.sort(rng.uniform(0.0, 360.0 * n_rev, n))
    x, y = np.cos(np.deg2rad(az)).astype(F), np.sin(np.deg2rad(az)).astype(F)
    yaw = [math.atan2(float(b), float(a)) * 57.2957 for a, b in zip(x, y)]
    b = [F(0)] + [F((yaw[0] - w) / 3.61) if w <= yaw[0] else F((yaw[0] - w + 360.0) / 3.61) for w in yaw[1:]]
    return np.array(b, F), np.array([1] + [0] * (n - 1), np.int32), x, y, yaw


def test_chain_equals_composition_in_every_grouping(H):
    b, first, x, y, yaw = ring_chain()
    # two rings back to back (a constant function cuts the chain), ties and a NaN in mid-ring
    b2 = np.concatenate([b, b[::-1][:150]]).astype(F)
    f2 = np.concatenate([first, [1], np.zeros(149, np.int32)]).astype(np.int32)
    b2[40] = b2[39]                      # b == time_last: no wrap, the test is a strict <
    b2[200] = np.nan
    serial = R.chain_serial(b2, f2)
    assert np.nanmax(serial) > 360.0 / 3.61 and serial[41] < 360.0 / 3.61
    assert serial[40] == serial[39]
    assert math.isnan(serial[200]) and serial[201] == b2[201]        # a NaN time_last compares false: the next point does not wrap
    for ref_fn, grouping in ((R.chain_left_fold, 1), (R.chain_tree, 2), (R.chain_blocks3, 3)):
        got = ref_fn(b2, f2)
        assert np.array_equal(got.view(np.uint32), serial.view(np.uint32)), grouping
    for grouping in (0, 1, 2, 3):
        out = np.zeros(len(b2), F)
        H.lh_hook_chain(b2.ctypes.data, f2.ctypes.data, len(b2), grouping, out.ctypes.data)
        assert np.array_equal(out.view(np.uint32), serial.view(np.uint32)), grouping
    # the header's yaw and b against the restatement's, bit for bit
    for k in range(1, len(x)):
        assert H.lh_hook_yaw(x[k], y[k]) == yaw[k]
        assert F(H.lh_hook_b(yaw[k], yaw[0])).tobytes() == b[k].tobytes()


def hand_cloud(t, pts, rings, times=None, **over):
    pts = np.asarray(pts, F).reshape(-1, 3)
    n = len(pts)
    d = R.default_desc(t)
    for k, v in over.items():
        setattr(d, k, v)
    return R.pack(d, pts, np.arange(n, dtype=F) + 1, np.zeros(n) if times is None else times, np.asarray(rings)), d


@pytest.mark.parametrize("t", [R.VELODYNE, R.RSLIDAR])
def test_yaw_ties_first_point_and_nan(H, t):
    a = [3.0, 4.0, 0.5]
    pts = [a, [2.0, 5.0, 0.1], a, [1.0, 6.0, 0.2], [1.0, 6.0, 0.2], [np.nan, 1.0, 1.0], [0.5, 6.0, 0.3], [6.0, -1.0, 0.3], [3.1, 3.9, 0.2]]
    #      first ring0   first ring1     tie w/ fp   later      b == time_last   NaN           after NaN        other ring       ring 0, wraps
    rings = [0, 1, 0, 0, 0, 0, 0, 1, 0]
    rec, d = hand_cloud(t, pts, rings, num_scans=2)
    want = both(H, rec, d)
    K.assert_margins(want)
    assert not want.given
    assert list(want.kept) == [2, 3, 4, 6, 7, 8]             # ring firsts 0 and 1 dropped although i % 1 == 0; the NaN point fails the blind test
    c = want.out[:, 9]
    assert c[0] == 0.0                                        # yaw == yaw_fp from identical (x, y): b = 0, not 360 / 3.61
    assert c[1] == c[2] and c[1] > 0                          # b == time_last: no wrap
    assert 0 < c[3] < c[2]                                    # below the time before the NaN, but compared against the NaN: not wrapped
    assert c[5] > 360.0 / 3.61                                # behind the first point's yaw again, below time_last: wrapped
    # the first point of a ring leaves whatever the candidate stride says
    rec, d = hand_cloud(t, [a, [2.0, 5.0, 0.1], [1.0, 6.0, 0.2], [0.5, 6.0, 0.3]], [0, 0, 0, 0], point_filter_num=2)
    assert list(both(H, rec, d).kept) == [2]


@pytest.mark.parametrize("t", K.TYPES)
def test_blind_edge(H, t):
    # r^2 = 9 + 16 + 0 exactly: equal to blind^2 at blind = 5
    times = [1.0, 2.0, 3.0] if t != R.OUSTER else [1000, 2000, 3000]
    rec, d = hand_cloud(t, [[3.0, 4.0, 0.0], [3.0, 4.0, 0.5], [3.0, 3.9, 0.0]], [0, 0, 0], times=times, blind=5.0, point_filter_num=1)
    want = both(H, rec, d)
    assert want.given
    assert list(want.kept) == ([0, 1] if t in (R.OUSTER, R.LIVOX_STD) else [1])


@pytest.mark.parametrize("t", [R.VELODYNE, R.RSLIDAR])
def test_given_offset_time_flips_at_zero(H, t):
    pts = [[3.0, 4.0, 0.5], [2.0, 5.0, 0.1], [1.0, 6.0, 0.2]]
    tiny = 1e-30 if t == R.VELODYNE else 5e-324
    for last, given in ((tiny, True), (0.0, False), (-1.0, False)):
        rec, d = hand_cloud(t, pts, [0, 0, 0], times=[7.0, 8.0, last])
        want = both(H, rec, d)
        assert want.given == given
        assert len(want.kept) == (3 if given else 2)


def test_bad_arguments(H):
    rec, d = K.sized_case(R.RSLIDAR, 200, 16, False)
    d.num_scans = 8                                            # rings reach 15
    with pytest.raises(R.BadArgument) as e:
        R.handler(rec, d)
    assert "200" in str(e.value)
    rc, _, _, bad, _ = hook(H, rec, d)
    assert rc == -1 and bad == int(str(e.value).split()[0])
    d.num_scans = 16
    for k, v in (("num_scans", 257), ("point_filter_num", 0), ("stride_bytes", 28), ("time_offset_bytes", 26), ("stride_bytes", 30), ("ring_offset_bytes", 31)):
        bad_d = R.Desc(**{**d.__dict__, k: v})
        with pytest.raises(R.BadArgument):
            R.check_desc(bad_d)
        rc, _, _, _, why = hook(H, rec[:, :max(bad_d.stride_bytes, 1)] if k == "stride_bytes" else rec, bad_d)
        assert rc == -1 and why, k
    # with times the ring is not read: a ring past num_scans is no error
    rec, d = K.sized_case(R.RSLIDAR, 200, 16, True)
    d.num_scans = 8
    both(H, rec, d)


def test_capacity_and_other_kinds(H):
    rec, d = K.sized_case(R.VELODYNE, 300, 16, False)
    want = R.handler(rec, d)
    rc, out, _, _, _ = hook(H, rec, d, capacity=10)
    assert rc == 0 and np.array_equal(out.view(np.uint32), want.out[:10].view(np.uint32))
    # a Velodyne cloud with double times and uint8 rings in a 40-byte record whose x starts at byte 4
    xyz, ring, col = K.spin_points(3, 16, 40)
    d = R.Desc(R.VELODYNE, "f64", "u8", 16, 2, 1e3, 40, 4, 20, 24, 33, 0.5)
    for tm in (col * 5.5e-5 + 1e-6, np.zeros(len(col))):
        both(H, R.pack(d, xyz, np.ones(len(xyz)), tm, ring, fill=0xEE), d)


def test_time_key_orders_like_a_stable_sort(H):
    rng = np.random.default_rng(11)
    v = np.concatenate([rng.uniform(-50, 150, 300), [0.0, -0.0, 0.0, -0.0, 1e-45, -1e-45, -3.0, -3.0, 99.75, 99.75, np.inf, -np.inf]]).astype(F)
    v = v[rng.permutation(len(v))]
    keys = [H.lh_hook_time_key(x) for x in v]
    assert keys == [R.time_key(x) for x in v]
    by_key = sorted(range(len(v)), key=lambda i: keys[i])
    by_value = sorted(range(len(v)), key=lambda i: float(v[i]))
    assert by_key == by_value                                 # -0.0 and 0.0 stay in input order, negatives below, no NaN in range
    rec = np.zeros((len(v), 12), F)
    rec[:, 9] = v
    rec[:, 0] = np.arange(len(v))
    assert list(R.stable_time_sort(rec)[:, 0].astype(int)) == by_value
