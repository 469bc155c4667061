"""GPU checks of pcm_scan_fuse / pcm_scan_fused against the numpy restatement of the reference's nodes (tests/scan_fuse_ref.py):
output bytes and every counter equal, for host, device and mixed inputs, the output in the context's buffer, a caller's device
buffer and a host buffer, and the three layouts; run-to-run identity; and LoamRegistration.frame_begin_fused against frame_begin
fed the restatement's fused cloud from the host.

The device's double asin may differ from numpy's in the last bits.  That can change a ring only where pitch + 40 sits on a half or
pitch sits on -40 / 12; the generator keeps every camera point 1e-5 away from those values and each test asserts 1e-6 on the
restatement's own pitches before it compares, so no point is left out of the comparison."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import scan_fuse_cases as K  # noqa: E402
import scan_fuse_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


PLACE = {"host": lambda k: None, "device": lambda k: dev, "mixed": lambda k: dev if k % 2 else None}


@pytest.fixture(scope="module")
def ctx(pcm):
    return pcm.OccupancyMap2D(0)      # a context of any model


@pytest.fixture(scope="module")
def case():
    segs = K.layout_case(0)
    want = {lay: R.fuse(segs, K.default_params(lay)) for lay in (R.OUT_XYZIRT, R.OUT_XYZIR, R.OUT_XYZI)}
    assert R.boundary_margin(want[R.OUT_XYZIRT].pitch, K.default_params()) >= K.PITCH_MARGIN
    return segs, want


def fused_bytes(reg, n):
    """The records pcm_scan_fused points at, copied to the host."""
    ptr, m = reg.fused_scan()
    assert m == n
    if n == 0:
        return np.zeros((0, 32), np.uint8)
    return _tensor_from_ptr(ptr, n * 32).cpu().numpy().reshape(n, 32).copy()


def _tensor_from_ptr(ptr, nbytes):
    """A uint8 tensor over device memory the context owns (no copy)."""
    import torch

    class _Holder:
        __cuda_array_interface__ = {"shape": (nbytes,), "typestr": "|u1", "data": (ptr, False), "version": 2}
    return torch.as_tensor(_Holder(), device="cuda")


@pytest.mark.parametrize("place", ["host", "device", "mixed"])
@pytest.mark.parametrize("where", ["context", "device_buffer", "host_buffer"])
def test_layout_case_bytes_and_counters(pcm, ctx, case, place, where):
    import torch
    segs, wants = case
    want = wants[R.OUT_XYZIRT]
    P = K.params_dict(K.default_params())
    api = [K.to_api(s, PLACE[place](k)) for k, s in enumerate(segs)]
    if where == "context":
        ret, counts = ctx.fuse_scans(api, P)
        assert ret is None
        got = fused_bytes(ctx, want.n_out)
    elif where == "device_buffer":
        buf = torch.full(((want.n_out + 3) * 32,), 0xAB, dtype=torch.uint8, device="cuda")
        ret, counts = ctx.fuse_scans(api, P, out=buf)
        b = buf.cpu().numpy().reshape(-1, 32)
        got = b[:want.n_out]
        assert np.all(b[want.n_out:] == 0xAB)                     # nothing written past n_out
    else:
        got, counts = ctx.fuse_scans(api, P, out="host")
    K.check_counts(counts, want)
    assert got.shape == want.out.shape and np.array_equal(got, want.out)


@pytest.mark.parametrize("layout", [R.OUT_XYZIR, R.OUT_XYZI])
def test_other_layouts(ctx, case, layout):
    segs, wants = case
    got, counts = ctx.fuse_scans([K.to_api(s) for s in segs], K.params_dict(K.default_params(layout)), out="host")
    K.check_counts(counts, wants[layout])
    assert np.array_equal(got, wants[layout].out)


def test_run_to_run_identity_and_nothing_kept(ctx, case):
    segs, wants = case
    api = [K.to_api(s, dev) for s in segs]
    P = K.params_dict(K.default_params())
    a, _ = ctx.fuse_scans(api, P, out="host")
    b, _ = ctx.fuse_scans(api, P, out="host")
    assert np.array_equal(a, b) and np.array_equal(a, wants[R.OUT_XYZIRT].out)
    none = K.nothing_kept_case()
    want = R.fuse(none, K.default_params())
    assert want.n_out == 0
    for out in (None, "host"):
        ret, counts = ctx.fuse_scans([K.to_api(s) for s in none], P, out=out)
        K.check_counts(counts, want)
    assert ctx.fused_scan() == (0, 0)


def test_capacity_too_small_and_converters(pcm, ctx, case):
    import torch
    segs, wants = case
    want = wants[R.OUT_XYZIRT]
    P = K.params_dict(K.default_params())
    buf = torch.full(((want.n_out - 5) * 32 + 64,), 0xAB, dtype=torch.uint8, device="cuda")
    with pytest.raises(pcm.PcmError) as e:
        ctx.fuse_scans([K.to_api(s) for s in segs], P, out=buf[:(want.n_out - 5) * 32])
    assert e.value.code == -1
    K.check_counts(e.value.counts, want)
    b = buf.cpu().numpy()
    assert np.array_equal(b[:(want.n_out - 5) * 32].reshape(-1, 32), want.out[:-5]) and np.all(b[(want.n_out - 5) * 32:] == 0xAB)
    # the converters are the one-segment case
    S = K.synth_fusion
    pts, row, _, _ = S.lidar_cloud(7, 16, 24)
    rec, lay = S.pack_rs_f32(pts, S.ring_table(16)[row], 1)
    got, _ = pcm.rs_to_velodyne(ctx, rec, "XYZIRT")
    assert np.array_equal(got, R.fuse([R.LidarXYZIRT(rec, **lay)], K.default_params()).out)
    rec, lay = S.pack_hesai(pts, S.ring_table(16)[row], 1)
    got, _ = pcm.hesai_to_velodyne(ctx, rec, "XYZIR")
    assert np.array_equal(got, R.fuse([R.LidarXYZIRT(rec, **lay)], K.default_params(R.OUT_XYZIR)).out)
    xyzi = S.pack_xyzi(pts, 2)
    got, _ = pcm.rs_to_velodyne(ctx, xyzi, organised=(24, 16, S.ring_table(16)))
    assert np.array_equal(got, R.fuse([R.LidarXYZI(xyzi, 24, 16, S.ring_table(16))], K.default_params(R.OUT_XYZIR)).out)


def test_frame_begin_fused_leaves_the_same_features(pcm):
    """16 x 1800 LiDAR + one small camera: the front end on the context's fused buffer against the front end fed the
    restatement's fused cloud from the host; every debug array bit for bit."""
    S = K.synth_fusion
    pts, row, _, _ = S.lidar_cloud(2, 16, 1800, nan_frac=0.05)
    pts[np.isinf(pts).any(axis=1)] = np.nan          # the front end's range image takes finite points
    rec, lay = S.pack_rs_u8(pts, S.identity_table(16)[row], 3)
    T = S.camera_T(0)
    segs = [R.LidarXYZIRT(rec, **lay), R.Depth(S.depth_cloud(9, T, 700, branches=False), T, 0, 5000000)]
    P = K.default_params()
    P.pitch_table = np.arange(52, dtype=np.int32) % 16   # camera rings inside the 16 scan lines
    P.ring_below, P.ring_otherwise = 0, 15
    want = R.fuse(segs, P)
    assert R.boundary_margin(want.pitch, P) >= K.PITCH_MARGIN
    fp = dict(n_scan=16, horizon_scan=1800)
    a, b = pcm.LoamRegistration(0), pcm.LoamRegistration(0)
    ra, counts = a.frame_begin_fused([K.to_api(s) for s in segs], K.params_dict(P), **fp)
    K.check_counts(counts, want)
    rb = b.set_input_scan(want.out, stride=32, intensity_offset=16, ring_offset=20, **fp)
    assert ra == rb and ra["num_corner"] > 0 and ra["num_surf"] > 0
    ia, ib = a.feature_info(), b.feature_info()
    assert set(ia) == set(ib)
    for k in ia:
        assert ia[k].shape == ib[k].shape and np.array_equal(ia[k].view(np.uint8), ib[k].view(np.uint8)), k
