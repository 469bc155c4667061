"""CPU checks of the scan-fusion arithmetic (pointcloud-slam_amd/csrc/scan_fuse.h, compiled with g++ through
tests/scan_fuse_hooks.cpp) against the numpy restatement of the reference's nodes (tests/scan_fuse_ref.py), byte for byte: every
kind of segment and every branch of it, hand-made points on the edges of each rule, the three output layouts, the counters, the
argument rules and the struct layouts of the binding.  No GPU."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_fuse_cases as K  # noqa: E402
import scan_fuse_ref as R  # noqa: E402

F = np.float32
IDENT = np.eye(4).reshape(16)


@pytest.fixture(scope="module")
def H(tmp_path_factory):
    from pointcloud_slam_amd import capi
    so = str(tmp_path_factory.mktemp("scan_hooks") / "scan_fuse_hooks.so")
    subprocess.run(["g++", "-O2", "-std=c++17", "-ffp-contract=off", "-Wall", "-Werror", "-fPIC", "-shared", "-I", os.path.join(ROOT, "pointcloud-slam_amd", "csrc"),
                    os.path.join(ROOT, "tests", "scan_fuse_hooks.cpp"), "-o", so], check=True)
    L = C.CDLL(so)
    L.scan_hook_fuse.argtypes = [C.POINTER(capi.PcmScanSegment), C.c_int, C.POINTER(capi.PcmScanFuseParams), C.c_void_p, C.c_size_t,
                                 C.POINTER(capi.PcmScanFuseResult), C.c_char_p, C.c_size_t]
    L.scan_hook_defaults.argtypes = [C.POINTER(capi.PcmScanFuseParams)]
    L.scan_hook_defaults.restype = None
    L.scan_hook_pitch.argtypes = [C.c_float, C.c_float, C.c_float, C.c_double]
    L.scan_hook_pitch.restype = C.c_double
    L.scan_hook_layout.argtypes = [C.c_void_p]
    return L


def hook_fuse(H, api_segs, pdict, capacity=None, n_segs=None):
    """(rc, records, counts, why) of the header's host composition."""
    from pointcloud_slam_amd import capi, registration as reg
    arr, keep = reg.scan_segments(api_segs)
    p, keep_p = reg.scan_fuse_params(H.scan_hook_defaults, pdict)
    total = sum(arr[k].n for k in range(len(api_segs)))
    cap = total if capacity is None else capacity
    out = np.full((max(cap, 1), 32), 0xAB, np.uint8)
    r = capi.PcmScanFuseResult()
    why = C.create_string_buffer(256)
    rc = H.scan_hook_fuse(arr, len(api_segs) if n_segs is None else n_segs, C.byref(p), out.ctypes.data, cap, C.byref(r), why, 256)
    return rc, out, reg.scan_result(r, min(len(api_segs), 8)), why.value.decode()


def run_both(H, segs, P):
    want = R.fuse(segs, P)
    rc, out, counts, why = hook_fuse(H, [K.to_api(s) for s in segs], K.params_dict(P))
    assert rc == 0, why
    K.check_counts(counts, want)
    assert np.array_equal(out[:want.n_out], want.out)
    return want


def depth_rec(points):
    p = np.asarray(points, F).reshape(-1, 3)
    rec = np.zeros((p.shape[0], 32), np.uint8)
    rec.view(F).reshape(-1, 8)[:, :3] = p
    return rec


def at_pitch(p, r=1.0, az=0.3):
    el = p / 28.6478897565
    return [r * math.cos(el) * math.cos(az), r * math.cos(el) * math.sin(az), r * math.sin(el)]


def test_layout_defaults_and_symbols(H):
    from pointcloud_slam_amd import capi
    o = (C.c_long * 16)()
    H.scan_hook_layout(o)
    S, P, Rs = capi.PcmScanSegment, capi.PcmScanFuseParams, capi.PcmScanFuseResult
    assert list(o) == [C.sizeof(S), S.points.offset, S.timestamp_offset_bytes.offset, S.ring_table.offset, S.dt_nsec.offset, S.T.offset,
                       C.sizeof(P), P.pitch_ring_table.offset, P.depth_intensity.offset, P.output_layout.offset, P.reserved.offset,
                       C.sizeof(Rs), C.sizeof(capi.PcmScanSegmentCounts), Rs.n_out.offset, Rs.status.offset, capi.PCM_ABI_VERSION]
    p = P()
    H.scan_hook_defaults(C.byref(p))
    D = R.Params()
    assert (p.depth_filter, p.pitch_scale, p.pitch_min, p.pitch_max, p.pitch_offset) == (D.depth_filter, D.pitch_scale, D.pitch_min, D.pitch_max, D.pitch_offset)
    assert (p.ring_below, p.ring_otherwise, p.depth_intensity, p.output_layout) == (47, 51, 100.0, capi.PCM_SCAN_OUT_XYZIRT)
    assert not p.pitch_ring_table and p.pitch_ring_table_len == 0      # the library embeds no table
    for name in ("pcm_scan_default_fuse_params", "pcm_scan_fuse", "pcm_scan_fused"):
        assert name in capi.SYMBOLS


@pytest.mark.parametrize("layout", [R.OUT_XYZIRT, R.OUT_XYZIR, R.OUT_XYZI])
def test_layout_case_matches_the_restatement(H, layout):
    segs = K.layout_case(0)
    P = K.default_params(layout)
    want = run_both(H, segs, P)
    assert R.boundary_margin(want.pitch, P) >= K.PITCH_MARGIN
    # the case is what it claims to be
    assert want.n_in == [640, 640, 255, 0, 256, 70, 1025] and want.n_kept[5] == 0 and want.n_nan[5] == 70
    assert all(want.n_nan[k] > 0 for k in (0, 1, 2, 4, 6)) and all(want.n_depth_filtered[k] > 0 for k in (2, 4, 6))
    assert want.n_pitch_index_clamped >= 6
    rec = want.out.view(F).reshape(-1, 8)
    assert np.all(rec[:, 3] == 1.0) and not want.out[:, 22:24].any() and not want.out[:, 28:].any()
    if layout != R.OUT_XYZIRT:
        assert not want.out[:, 24:28].any()
    if layout == R.OUT_XYZI:
        assert not want.out[:, 20:].any()
    else:
        rings = want.out.view(np.uint16).reshape(-1, 16)[want.out_offset[2]:, 10]
        table = set(int(v) for v in P.pitch_table)
        assert {47, 51} <= set(int(v) for v in rings) and len(set(int(v) for v in rings) & table) > 10


def test_depth_points_on_every_edge(H):
    pts = [[np.nan, 1, 1], [1, np.nan, 1], [1, 1, np.nan],      # a NaN in each coordinate
           [0.2, 0.1, 1.5],                                      # z == depth_filter exactly: kept
           [0.2, 0.1, np.nextafter(F(1.5), F(2))],               # one ulp beyond: dropped
           [0.0, 0.0, 0.0],                                      # dist = 0 -> NaN pitch -> ring 51
           at_pitch(-40.5), at_pitch(-39.6), at_pitch(0.0), at_pitch(11.2),
           at_pitch(11.7), at_pitch(11.9),                       # index 52: clamped and counted
           at_pitch(12.4), at_pitch(44.0),
           [0.0, 0.0, 0.7], [0.0, 0.0, -0.7]]                    # straight up / down
    P = K.default_params()
    P.depth_filter = 1.5
    seg = R.Depth(depth_rec(pts), IDENT, 3, -250000000)          # dt_nsec negative
    want = run_both(H, [seg], P)
    assert (want.n_nan, want.n_depth_filtered, want.n_kept, want.n_pitch_index_clamped) == ([3], [1], [12], 2)
    assert R.boundary_margin(want.pitch, P) > 0.05
    ring = want.out.view(np.uint16).reshape(-1, 16)[:, 10]
    t = P.pitch_table
    assert list(ring[:10]) == [51, 51, 47, t[0], t[40], t[51], 51, 51, 51, 51]      # the first: pitch 40 of (0.2, 0.1, 1.5)
    assert np.all(want.out.view(F).reshape(-1, 8)[:, 6] == F(3 * 1.0 + -250000000 / 1000000000.0))
    assert np.all(want.out.view(F).reshape(-1, 8)[:, 4] == 100.0)
    # filter off
    P.depth_filter = -1.0
    want = run_both(H, [R.Depth(depth_rec([[0.1, 0.1, 1e6], [0.1, 0.2, 3.0]]), IDENT)], P)
    assert want.n_kept == [2] and want.n_depth_filtered == [0]
    # a rotated, translated camera: the doubles of the transform, rounded once
    T = K.synth_fusion.camera_T(1)
    rng = np.random.default_rng(5)
    P = K.default_params()
    run_both(H, [R.Depth(depth_rec(rng.uniform(-1.5, 1.7, (4000, 3))), T, -2, 5)], P)


def test_depth_infinite_coordinate_passes(H):
    """+Inf is no NaN: the point is kept.  Compared away from the coordinates that become NaN (Inf * 0 in the transform): the sign
    of a generated NaN is the processor's, not the algorithm's."""
    P = K.default_params()
    P.depth_filter = -1.0
    seg = R.Depth(depth_rec([[np.inf, 0.3, 0.5], [0.3, 0.2, 0.5]]), IDENT)
    want = R.fuse([seg], P)
    rc, out, counts, why = hook_fuse(H, [K.to_api(seg)], K.params_dict(P))
    assert rc == 0 and counts["n_kept"] == [2] and want.n_kept == [2]
    got, ref = out[:2].view(F).reshape(2, 8), want.out.view(F).reshape(2, 8)
    assert np.isinf(got[0, 0]) and np.isnan(got[0, 1]) and np.isnan(ref[0, 1])
    assert np.array_equal(out[:2, 12:], want.out[:, 12:]) and np.array_equal(out[1], want.out[1])
    assert want.out.view(np.uint16).reshape(2, 16)[0, 10] == 51       # NaN pitch


@pytest.mark.parametrize("pack", ["rs_f32", "rs_u8", "hesai"])
def test_lidar_xyzirt_records(H, pack):
    S = K.synth_fusion
    pts, row, _, _ = S.lidar_cloud(3, 16, 24)
    pts[0] = np.nan                                              # the first record is dropped but supplies timestamp[0]
    rec, lay = getattr(S, "pack_" + pack)(pts, S.ring_table(16)[row], 1)
    if lay["itype"] == "u8":
        rec[5, 16] = 255
    seg = R.LidarXYZIRT(rec, **lay)
    want = run_both(H, [seg], K.default_params())
    ts = R.field(rec, lay["toff"], np.float64)
    keep = ~np.isnan(pts).any(axis=1)
    assert np.array_equal(want.out.view(F).reshape(-1, 8)[:, 6], (ts[keep] - ts[0]).astype(F)) and want.n_nan[0] >= 1
    assert np.isinf(want.out.view(F).reshape(-1, 8)[:, 0]).sum() == 1          # Inf passes
    if lay["itype"] == "u8" and keep[5]:
        assert 255.0 in want.out.view(F).reshape(-1, 8)[:, 4]
    # odd stride (not a multiple of 16) and an unaligned view of the same records
    rec2 = np.zeros((rec.shape[0], rec.shape[1] + 4), np.uint8)
    rec2[:, :rec.shape[1]] = rec
    seg2 = R.LidarXYZIRT(rec2, **lay)
    assert np.array_equal(run_both(H, [seg2], K.default_params()).out, want.out)


@pytest.mark.parametrize("rows,width", [(16, 24), (128, 3)])
def test_lidar_xyzi_ring_from_position(H, rows, width):
    S = K.synth_fusion
    pts, row, _, _ = S.lidar_cloud(4, rows, width)
    table = S.ring_table(rows) + (65536 if rows == 16 else 0)     # an int beyond uint16 wraps as the assignment to `ring` does
    seg = R.LidarXYZI(S.pack_xyzi(pts, 2), width, rows, table)
    P = K.default_params(R.OUT_XYZIR)
    want = run_both(H, [seg], P)
    keep = ~np.isnan(pts).any(axis=1)
    assert np.array_equal(want.out.view(np.uint16).reshape(-1, 16)[:, 10], S.ring_table(rows)[row[keep]].astype(np.uint16))
    assert not want.out[:, 24:28].any()


def test_argument_errors(H):
    from pointcloud_slam_amd import registration as reg
    S = K.synth_fusion
    P = K.params_dict(K.default_params())
    pts, row, _, _ = S.lidar_cloud(4, 16, 8)
    rec = S.pack_xyzi(pts, 0)
    ok = reg.lidar_xyzi_segment(rec, 8, 16, S.identity_table(16))
    assert hook_fuse(H, [ok], P)[0] == 0
    rc, _, _, why = hook_fuse(H, [reg.lidar_xyzi_segment(rec[:64], 2, 32, S.identity_table(32))], P)      # height 32
    assert rc == -1 and "neither 16 nor 128" in why
    rc, _, _, why = hook_fuse(H, [reg.lidar_xyzi_segment(rec, 8, 16, S.identity_table(15))], P)           # a table too short
    assert rc == -1 and "too short" in why
    assert hook_fuse(H, [reg.lidar_xyzi_segment(rec[:120], 8, 16, S.identity_table(15))], P)[0] == 0      # ... but long enough for 15 rows
    rc, _, _, why = hook_fuse(H, [reg.lidar_xyzi_segment(rec, 1, 128, S.identity_table(127))], P)
    assert rc == -1 and "too short" in why
    arr9 = [ok] * 9                                                                                          # 9 segments
    from pointcloud_slam_amd import capi
    arr = (capi.PcmScanSegment * 9)()
    a1, keep = reg.scan_segments([ok])
    for k in range(9):
        C.memmove(C.byref(arr[k]), C.byref(a1[0]), C.sizeof(capi.PcmScanSegment))
    p, kp = reg.scan_fuse_params(H.scan_hook_defaults, P)
    r = capi.PcmScanFuseResult()
    why = C.create_string_buffer(256)
    assert H.scan_hook_fuse(arr, 9, C.byref(p), None, 0, C.byref(r), why, 256) == -1 and b"at most 8" in why.value and len(arr9) == 9
    assert H.scan_hook_fuse(arr, 8, C.byref(p), None, 0, C.byref(r), why, 256) == -1 and b"too small" in why.value      # 8 pass the rules
    # capacity too small: the counts are set, nothing is written past the capacity
    want = R.fuse([R.LidarXYZI(rec, 8, 16, S.identity_table(16))], K.default_params())
    rc, out, counts, why = hook_fuse(H, [ok], P, capacity=want.n_out - 1)
    assert rc == -1 and "too small" in why
    K.check_counts(counts, want)
    assert np.array_equal(out[:want.n_out - 1], want.out[:-1])
    # depth segments need the caller's table
    d = reg.depth_segment(np.zeros((4, 32), np.uint8), IDENT)
    noP = dict(P, pitch_ring_table=None)
    rc, _, _, why = hook_fuse(H, [d], noP)
    assert rc == -1 and "pitch ring table" in why
    assert hook_fuse(H, [ok], noP)[0] == 0
    bad = reg.lidar_xyzirt_segment(np.zeros((4, 32), np.uint8), 32, 16, 20, 28)                              # timestamp leaves the record
    assert hook_fuse(H, [bad], P)[0] == -1


def test_pitch_sqrt_is_the_float_overload(H):
    """dist = (double)sqrtf(float sum).  The header's asin is libm's, the restatement's numpy's: each is within 4 ulp of asin, a
    value of at most pi / 2, so the pitches (at most 45) agree to 8 ulp of 45 = 5.7e-14; sqrt in double of the same float sum
    moves dist by up to 2^-25 of itself and the pitch by 1e-7 and more."""
    rng = np.random.default_rng(0)
    o = rng.uniform(-2, 2, (2000, 3)).astype(F)
    got = np.array([H.scan_hook_pitch(float(a), float(b), float(c), 28.6478897565) for a, b, c in o])
    want = R.pitch_of(o[:, 0], o[:, 1], o[:, 2], 28.6478897565)
    assert np.isfinite(got).all() and np.abs(got - want).max() <= 1e-13
    s = (o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1]) + o[:, 2] * o[:, 2]
    other = np.arcsin(o[:, 2].astype(np.float64) / np.sqrt(s.astype(np.float64))) * 28.6478897565
    assert np.abs(other - got).max() > 1e-8
