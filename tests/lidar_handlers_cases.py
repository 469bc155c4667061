"""Seeded clouds for the PointCloud2 handler tests (tests/test_lidar_handlers.py, tests/test_gpu_lidar_handlers.py): spinning
scans emitted column by column as the drivers do, packed in the reference's PCL struct layouts, with the edge points of every
rule.  Azimuth columns are at least 0.01 degree apart and ranges are drawn per point, so the yaw comparisons of a case have wide
margins except where a test builds a tie from bit-identical (x, y) on purpose; every no-time case asserts its margins on the
restatement's values (assert_margins) before anything is compared."""
import math

import numpy as np

import lidar_handlers_ref as R

F = np.float32
YAW_MARGIN_DEG = 1e-6
B_MARGIN_MS = 1e-6
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1025, 4099]
RING_COUNTS = [1, 16, 128]
TYPES = [R.VELODYNE, R.OUSTER, R.RSLIDAR, R.LIVOX_STD]


def spin_points(seed, rings, cols, sweep_deg=400.0, start_deg=100.0, empty_ring=None, single_ring=None):
    """(xyz, ring, column) of a clockwise spin over sweep_deg degrees (more than one revolution by default, so offset times wrap),
    emitted column by column with the rings of a column in a fixed shuffled order.  Ranges 1..40 m with a few points inside the
    blind radius.  empty_ring: a ring without points; single_ring: a ring with one point."""
    rng = np.random.default_rng(seed)
    order = rng.permutation(rings)
    col = np.repeat(np.arange(cols), rings)
    ring = np.tile(order, cols)
    az = np.deg2rad(start_deg - (col + rng.uniform(0.1, 0.4, col.size)) * (sweep_deg / max(cols, 1)))
    el = np.deg2rad(-15.0 + 30.0 * ring / max(rings - 1, 1))
    r = rng.uniform(1.0, 40.0, col.size)
    near = rng.random(col.size) < 0.08
    r[near] = rng.uniform(0.02, 0.45, int(near.sum()))
    xyz = np.stack([r * np.cos(el) * np.cos(az), r * np.cos(el) * np.sin(az), r * np.sin(el)], 1).astype(F)
    keep = np.ones(col.size, bool)
    if empty_ring is not None:
        keep &= ring != empty_ring
    if single_ring is not None:
        idx = np.flatnonzero(ring == single_ring)
        keep[idx[1:]] = False
    return xyz[keep], ring[keep], col[keep]


def pack_case(t, xyz, ring, col, given, seed=0, **desc_over):
    """Records of the type's struct.  given: the drivers' times (RoboSense stamps are absolute and dip below the first point's, so
    curvatures go negative); else every time is 0."""
    d = R.default_desc(t)
    d.num_scans = max(d.num_scans, int(ring.max()) + 1 if len(ring) else 1)
    if d.num_scans > 255 and d.ring_kind == "u8":
        d.ring_kind = "u16"
    for k, v in desc_over.items():
        setattr(d, k, v)
    n = len(xyz)
    rng = np.random.default_rng(seed + 1000)
    inten = rng.uniform(0, 255, n).astype(F)
    if not given:
        tm = np.zeros(n)
    elif t == R.VELODYNE:
        tm = (col * 5.5e-5 + 1e-6).astype(np.float32)                 # seconds
    elif t == R.OUSTER:
        tm = (col * 55000 + 17).astype(np.uint32)                     # nanoseconds
    else:
        tm = 1.6e9 + 0.002 + col * 5.5e-5 - (np.arange(n) % 7 == 3) * 0.0031   # absolute seconds
    return R.pack(d, xyz, inten, tm, ring if d.type in (R.VELODYNE, R.RSLIDAR) else None, fill=0xCD), d


def sized_case(t, n, rings, given, seed=None, **desc_over):
    """n points of a `rings`-ring spin; with more than 2 rings one ring is empty and one has a single point."""
    seed = (t * 131 + n * 7 + rings) if seed is None else seed
    cols = math.ceil(n / max(rings - 2, 1)) + 2
    kw = dict(empty_ring=rings - 2, single_ring=1) if rings > 2 else {}
    xyz, ring, col = spin_points(seed, rings, cols, **kw)
    assert len(xyz) >= n
    return pack_case(t, xyz[:n], ring[:n], col[:n], given, seed, **desc_over)


def big_case(t, given):
    """16 x 4400 = 70400 points: 275 scan workgroups (two rounds of workgroup tops), every ring's run crosses 17 of them."""
    xyz, ring, col = spin_points(99, 16, 4400, sweep_deg=520.0)
    return pack_case(t, xyz, ring, col, given, 99)


def assert_margins(res: R.Result):
    assert R.yaw_margin(res) > YAW_MARGIN_DEG, R.yaw_margin(res)
    assert R.b_margin(res) > B_MARGIN_MS, R.b_margin(res)


def to_api(d: R.Desc):
    """The binding's descriptor of a restatement descriptor."""
    import pointcloud_slam_amd as pcm
    return pcm.lidar_desc(d.type, time_kind=d.time_kind, ring_kind=d.ring_kind, num_scans=d.num_scans, point_filter_num=d.point_filter_num,
                          time_scale=d.time_scale, stride_bytes=d.stride_bytes, xyz_offset_bytes=d.xyz_offset_bytes,
                          intensity_offset_bytes=d.intensity_offset_bytes, time_offset_bytes=d.time_offset_bytes, ring_offset_bytes=d.ring_offset_bytes,
                          blind=d.blind)


def poses(k=12, span_s=0.12):
    """(k, 22) Pose6D rows over the frame: a gentle turn and drift (offset_time, acc, gyr, vel, pos, rot row-major)."""
    P = np.zeros((k, 22))
    for j in range(k):
        tt = span_s * j / (k - 1)
        a = 0.3 * tt
        P[j, 0] = tt
        P[j, 1:4] = [0.1, -0.05, 0.02]
        P[j, 4:7] = [0.01, 0.02, 0.3]
        P[j, 7:10] = [1.0, 0.2, 0.0]
        P[j, 10:13] = [1.0 * tt, 0.2 * tt, 0.0]
        P[j, 13:22] = [math.cos(a), -math.sin(a), 0, math.sin(a), math.cos(a), 0, 0, 0, 1]
    return P
