"""GPU checks of cachePointCloud on the device (pcm_loam_cloud_prepare / pcm_loam_frame_begin_cloud[_batch])
against the per-point restatement of tests/loam_cloud_ref.py: the prepared records byte for byte, padding included, and the raw
cloud through the front end against the restatement's records through pcm_loam_frame_begin_deskew, every array an equality."""
import ctypes as C

import numpy as np
import pytest

import loam_cloud_ref as R
import loam_deskew_ref as D

pytestmark = pytest.mark.gpu

from pointcloud_slam_amd import capi, loam as LM   # noqa: E402

ERR_INVALID_ARGUMENT, ERR_UNSUPPORTED = -1, -4   # include/pcm_amd.h
INFO = ("start", "end", "col_ind", "range", "cloud", "curvature", "neighbor_picked", "label", "corner_scan", "surf_scan")
CLOUD_INFO = ("n_in", "n_out", "n_nonfinite", "ring_synthesised", "time_synthesised", "time_available")
RS = (R.RSLIDAR_16, R.RSLIDAR_RUBY, R.RSLIDAR_32)
TSC = 1000.0
_REF = {}


def _all_but(n, keep):
    return tuple(i for i in range(n) if i not in keep)


# name -> (height, width, point_step, keywords of R.make_case)
CASES = {
    "16x12_nan_first_lastrow_lastcol": (16, 12, 32, dict(nan_at=(0, 15 * 12 + 3, 2 * 12 + 11))),
    "128x5_no_time_synth_time": (128, 5, 26, dict(has_time=False, synth_time=True, nan_at=(0, 77))),
    "32x7_no_fields_synth_both": (32, 7, 26, dict(has_ring=False, has_time=False, synth_time=True)),
    "32x7_no_fields_synth_off": (32, 7, 32, dict(has_ring=False, has_time=False, synth_ring=False, nan_at=(3,))),
    "2x2_synth_both": (2, 2, 32, dict(synth_time=True)),
    "height_1": (1, 9, 26, dict(synth_time=True, nan_at=(4,))),
    "width_1": (9, 1, 32, dict(synth_time=True, nan_at=(8,))),
    "empty_height": (0, 5, 32, dict()),
    "empty_width": (5, 0, 26, dict()),
    "all_nan": (4, 8, 26, dict(nan_at=tuple(range(32)))),
    "dense_with_nans": (16, 12, 26, dict(is_dense=True, synth_time=True, nan_at=(0, 50, 191))),
    "fields_present_synth_off": (16, 12, 26, dict(synth_ring=False, nan_at=(1,))),
    "fields_present_synth_time_over": (16, 12, 32, dict(synth_time=True)),
    # 3 * 64 + 1 finite records among NaNs, records 100 .. 292: wave boundaries at 128 and 192 and the workgroup boundary at 256
    # fall inside the kept run
    "193_finite_among_nans": (16, 64, 26, dict(has_time=False, synth_time=True, nan_at=_all_but(1024, range(100, 293)))),
}


def ref(name, lidar_type, kind):
    key = (name, lidar_type, kind)
    if key not in _REF:
        h, w, step, kw = CASES[name]
        raw, d = R.make_case(h, w, step, kind, lidar_type, seed=len(name) + 7 * lidar_type, **kw)
        want, info = R.cache_point_cloud(raw, d)
        want.setflags(write=False)
        raw.setflags(write=False)
        _REF[key] = (raw, d, want, info)
    return _REF[key]


def new_reg(pcm):
    return pcm.LoamRegistration(0)


def device(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def pick(info):
    return {k: info[k] for k in CLOUD_INFO}


@pytest.mark.parametrize("kind", [R.MAPPING, R.LOCALIZATION], ids=["mapping", "localization"])
@pytest.mark.parametrize("lidar_type", RS, ids=["rslidar_16", "rslidar_ruby", "rslidar_32"])
def test_prepare_equals_restatement_byte_for_byte(pcm, lidar_type, kind):
    import torch
    g = new_reg(pcm)
    size = R.RECORD[kind][0]
    for name in CASES:
        raw, d, want, winfo = ref(name, lidar_type, kind)
        cd = R.capi_desc(capi, d)
        got, info = LM.loam_cloud_prepare(g, raw, cd, out="host")                      # host bytes in, host records out
        print(name, "host n_out", info["n_out"], "of", info["n_in"])
        assert pick(info) == winfo and info["status"] == 0, name
        assert got.shape == want.shape and got.tobytes() == want.tobytes(), name
        out = torch.full((max(1, d.height * d.width), size), 0xA5, dtype=torch.uint8, device="cuda:0")
        _, info = LM.loam_cloud_prepare(g, device(raw), cd, out=out)                   # device bytes in, device records out
        assert pick(info) == winfo, name
        got = out.cpu().numpy()
        assert got[:winfo["n_out"]].tobytes() == want.tobytes(), name
        assert (got[winfo["n_out"]:] == 0xA5).all(), name
        _, info = LM.loam_cloud_prepare(g, raw, cd)                                    # into the context
        ptr, n, stride = C.c_void_p(), C.c_size_t(), C.c_size_t()
        assert g._L.pcm_loam_cloud_cached(g.handle, C.byref(ptr), C.byref(n), C.byref(stride)) == 0
        assert (n.value, stride.value, bool(ptr.value)) == (winfo["n_out"], size, winfo["n_out"] > 0), name


def test_two_runs_give_the_same_bytes_and_counts_are_what_the_case_says(pcm):
    g = new_reg(pcm)
    raw, d, want, winfo = ref("193_finite_among_nans", R.RSLIDAR_RUBY, R.MAPPING)
    assert winfo["n_out"] == 193 and winfo["n_nonfinite"] == 1024 - 193
    a, _ = LM.loam_cloud_prepare(g, raw, R.capi_desc(capi, d), out="host")
    b, _ = LM.loam_cloud_prepare(g, raw, R.capi_desc(capi, d), out="host")
    assert a.tobytes() == b.tobytes() == want.tobytes()
    raw, d, want, winfo = ref("dense_with_nans", R.RSLIDAR_16, R.LOCALIZATION)
    assert winfo["n_out"] == 192 and winfo["n_nonfinite"] == 0                         # is_dense: nothing dropped, NaN or not
    raw, d, want, winfo = ref("all_nan", R.RSLIDAR_32, R.MAPPING)
    assert winfo["n_out"] == 0


@pytest.mark.parametrize("kind", [R.MAPPING, R.LOCALIZATION], ids=["mapping", "localization"])
def test_capacity_too_small(pcm, kind):
    import torch
    g = new_reg(pcm)
    raw, d, want, winfo = ref("16x12_nan_first_lastrow_lastcol", R.RSLIDAR_16, kind)
    cd = R.capi_desc(capi, d)
    size, cap, guard = R.RECORD[kind][0], 100, 8
    assert winfo["n_out"] == 189
    r = capi.PcmLoamCloudResult()
    out = torch.full((cap + guard, size), 0xA5, dtype=torch.uint8, device="cuda:0")
    rc = g._L.pcm_loam_cloud_prepare(g.handle, raw.ctypes.data, C.byref(cd), capi.MEM_HOST, out.data_ptr(), cap, capi.MEM_DEVICE, C.byref(r))
    assert rc == ERR_INVALID_ARGUMENT and "too small" in g._L.pcm_last_error(g.handle).decode()
    assert (r.n_in, r.n_out, r.n_nonfinite) == (192, 189, 3)
    got = out.cpu().numpy()
    assert got[:cap].tobytes() == want[:cap].tobytes() and (got[cap:] == 0xA5).all()
    host = np.full((cap + guard, size), 0xA5, np.uint8)
    r = capi.PcmLoamCloudResult()
    rc = g._L.pcm_loam_cloud_prepare(g.handle, raw.ctypes.data, C.byref(cd), capi.MEM_HOST, host.ctypes.data, cap, capi.MEM_HOST, C.byref(r))
    assert rc == ERR_INVALID_ARGUMENT and (r.n_in, r.n_out) == (192, 189) and (host[cap:] == 0xA5).all()
    with pytest.raises(pcm.PcmError) as e:
        LM.loam_cloud_prepare(g, raw, cd, out=np.zeros((cap, size), np.uint8))
    assert e.value.code == ERR_INVALID_ARGUMENT


def test_velodyne(pcm):
    g = new_reg(pcm)
    for kind in (R.MAPPING, R.LOCALIZATION):
        raw, d = R.make_case(6, 40, 26, kind, R.VELODYNE, seed=3, synth_ring=False, is_dense=True, nan_at=(7,))
        want, winfo = R.cache_point_cloud(raw, d)
        got, info = LM.loam_cloud_prepare(g, raw, R.capi_desc(capi, d), out="host")
        assert pick(info) == winfo and got.tobytes() == want.tobytes() and info["time_available"] == 1 and info["n_out"] == 240
        raw, d = R.make_case(6, 40, 32, kind, R.VELODYNE, seed=4, synth_ring=False, is_dense=True, has_time=False)
        want, winfo = R.cache_point_cloud(raw, d)
        got, info = LM.loam_cloud_prepare(g, device(raw), R.capi_desc(capi, d), out="host")
        assert pick(info) == winfo and got.tobytes() == want.tobytes() and info["time_available"] == 0
        for kw, text in ((dict(is_dense=False), "not in dense format"), (dict(is_dense=True, has_ring=False), "ring channel not available")):
            raw, d = R.make_case(6, 40, 32, kind, R.VELODYNE, seed=5, synth_ring=False, **kw)
            with pytest.raises(ValueError):
                R.cache_point_cloud(raw, d)
            with pytest.raises(pcm.PcmError, match=text) as e:
                LM.loam_cloud_prepare(g, raw, R.capi_desc(capi, d), out="host")
            assert e.value.code == ERR_INVALID_ARGUMENT


def test_misuse_is_refused_with_a_readable_error(pcm):
    g = new_reg(pcm)
    raw, d, _, _ = ref("2x2_synth_both", R.RSLIDAR_16, R.MAPPING)

    def refused(text, code=ERR_INVALID_ARGUMENT, reg=g, data=raw, **kw):
        cd = R.capi_desc(capi, d)
        for k, v in kw.items():
            setattr(cd, k, v)
        with pytest.raises(pcm.PcmError, match=text) as e:
            LM.loam_cloud_prepare(reg, data, cd, out="host")
        assert e.value.code == code
        with pytest.raises(pcm.PcmError, match=text) as e:
            LM.loam_frame_begin_cloud(reg, data, cd, horizon_scan=256)
        assert e.value.code == code

    refused("past point_step", time_offset_bytes=28)
    refused("past point_step", ring_offset_bytes=31)
    refused("misaligned", xyz_offset_bytes=2)
    refused("misaligned", ring_offset_bytes=27)
    refused("lidar_type", lidar_type=9)
    refused("record_kind", record_kind=5)
    refused("intensity_kind", intensity_kind=capi.PCM_LOAM_INTENSITY_FLOAT)
    refused("PCM_MODEL_LOAM", code=ERR_UNSUPPORTED, reg=pcm.P2PlaneRegistration(0))
    cd = R.capi_desc(capi, d)
    r = capi.PcmLoamCloudResult()
    odd = np.zeros(4 * 32 + 2, np.uint8)[2:]                                           # a 2-byte aligned base
    assert odd.ctypes.data % 4 == 2
    assert g._L.pcm_loam_cloud_prepare(g.handle, odd.ctypes.data, C.byref(cd), capi.MEM_HOST, None, 0, 0, C.byref(r)) == ERR_INVALID_ARGUMENT
    assert "4-byte aligned" in g._L.pcm_last_error(g.handle).decode()
    cda = R.capi_desc(capi, d)
    cdb = R.capi_desc(capi, ref("2x2_synth_both", R.RSLIDAR_16, R.LOCALIZATION)[1])
    with pytest.raises(pcm.PcmError, match="one record_kind"):
        LM.loam_frame_begin_cloud_batch([g, new_reg(pcm)], [raw, ref("2x2_synth_both", R.RSLIDAR_16, R.LOCALIZATION)[0]], [cda, cdb], horizon_scan=256)


# ---- end to end ------------------------------------------------------------------------------------------------------------------
FP = dict(n_scan=16, horizon_scan=256)
GYRO, VEL = (0.4, 0.3, 2.0), (4.0, 1.0, 0.2)     # roll / pitch / yaw rates [rad/s], velocity [m/s]


def motion(tsc):
    imu, odom = D.sampled_tables(tsc, 200.0, 0.1, GYRO, VEL, 0.005)
    dk = D.build_tables(tsc, imu, odom)
    assert dk["imu_available"] and dk["odom_deskew"]
    return dk


def e2e_cloud(seed, lidar_type=R.RSLIDAR_16, height=16, width=256, nan_head=1, kind=R.MAPPING, step=32):
    """An organised cloud without a time field, 5 % NaN records, the first ``nan_head`` records among them."""
    rng = np.random.default_rng(1000 + seed)
    n = height * width
    nan_at = tuple(range(nan_head)) + tuple(int(i) for i in rng.choice(np.arange(nan_head, n), n // 20 - nan_head, replace=False))
    return R.make_case(height, width, step, kind, lidar_type, seed=seed, has_time=False, synth_time=True, nan_at=nan_at, scene="room")


def same_info(ia, ib):
    for k in INFO:
        assert ia[k].dtype == ib[k].dtype and ia[k].shape == ib[k].shape and ia[k].tobytes() == ib[k].tobytes(), k


@pytest.mark.parametrize("memory", ["host", "device"])
def test_frame_begin_cloud_equals_frame_begin_deskew_on_the_restatement(pcm, memory):
    a, b = new_reg(pcm), new_reg(pcm)
    for frame, seed in enumerate((11, 12)):                                            # two frames: the cross-frame state is carried
        raw, d = e2e_cloud(seed)
        rec, winfo = R.cache_point_cloud(raw, d)
        assert winfo["n_nonfinite"] == 16 * 256 // 20 and winfo["time_available"] == 1
        dk = motion(TSC + 0.1 * frame)
        ra, ca = LM.loam_frame_begin_cloud(a, device(raw) if memory == "device" else raw, R.capi_desc(capi, d), dk, **FP)
        rb = LM.loam_frame_begin_deskew(b, rec, dk, **FP)
        print("frame", frame, ra)
        assert pick(ca) == winfo and ra == rb and ra["num_extracted"] > 1000 and ra["num_corner"] > 0 and ra["num_surf"] > 0
        same_info(a.feature_info(), b.feature_info())
        assert (a.n_corner, a.n_surf) == (b.n_corner, b.n_surf)


def test_t0_is_the_first_finite_record(pcm):
    """Records 0 .. 39 are NaN, so t_0 is record 40's synthesised time (2.2 ms); with the raw record 0's time (0) instead, a
    yaw rate of 2 rad/s moves a point at 20 m by 9 cm: cloud_deskewed must differ from that wrong answer."""
    a, b, wrong = new_reg(pcm), new_reg(pcm), new_reg(pcm)
    raw, d = e2e_cloud(13, nan_head=40)
    rec, winfo = R.cache_point_cloud(raw, d)
    t = rec[:, 24:32].copy().view("<f8").reshape(-1)
    assert t[0] == R.time_of(R.RSLIDAR_16, 0, 40) > 2e-3
    dk = motion(TSC)
    ra, ca = LM.loam_frame_begin_cloud(a, raw, R.capi_desc(capi, d), dk, **FP)
    rb = LM.loam_frame_begin_deskew(b, rec, dk, **FP)
    assert ra == rb and pick(ca) == winfo
    ia = a.feature_info()
    same_info(ia, b.feature_info())
    rec0 = rec.copy()
    rec0[0, 24:32] = np.frombuffer(np.float64(R.time_of(R.RSLIDAR_16, 0, 0)).tobytes(), np.uint8)   # the raw record 0's time as t_0
    LM.loam_frame_begin_deskew(wrong, rec0, dk, **FP)
    iw = wrong.feature_info()
    assert iw["cloud"].shape != ia["cloud"].shape or (iw["cloud"] != ia["cloud"]).any()
    # and without a deskew descriptor, or without a time, the frame is the plain front end's
    c, e = new_reg(pcm), new_reg(pcm)
    rc_, _ = LM.loam_frame_begin_cloud(c, raw, R.capi_desc(capi, d), None, **FP)
    assert rc_ == e.set_input_scan(rec, **FP)
    same_info(c.feature_info(), e.feature_info())
    raw2, d2 = R.make_case(16, 256, 32, R.MAPPING, R.RSLIDAR_16, seed=13, has_time=False, synth_time=False, nan_at=(0,))
    rec2, winfo2 = R.cache_point_cloud(raw2, d2)
    rf, cf = LM.loam_frame_begin_cloud(c, raw2, R.capi_desc(capi, d2), dk, **FP)       # time_available == 0: the descriptor is ignored
    assert cf["time_available"] == 0 == winfo2["time_available"] and rf == e.set_input_scan(rec2, **FP)
    same_info(c.feature_info(), e.feature_info())


def test_batch_of_three_equals_three_single_calls(pcm):
    clouds = [e2e_cloud(21), R.make_case(32, 100, 26, R.MAPPING, R.RSLIDAR_RUBY, seed=22, has_time=False, synth_time=True, is_dense=True, nan_at=(5,)),
              R.make_case(0, 0, 32, R.MAPPING, R.RSLIDAR_32, seed=23)]
    dks = [motion(TSC), None, motion(TSC)]
    batch = [new_reg(pcm) for _ in clouds]
    single = [new_reg(pcm) for _ in clouds]
    for frame in range(2):
        res, cres = LM.loam_frame_begin_cloud_batch(batch, [c[0] for c in clouds], [R.capi_desc(capi, c[1]) for c in clouds], dks, **FP)
        for i, (raw, d) in enumerate(clouds):
            r1, c1 = LM.loam_frame_begin_cloud(single[i], raw, R.capi_desc(capi, d), dks[i], **FP)
            assert res[i] == r1 and cres[i] == c1, i
            assert pick(c1) == R.cache_point_cloud(raw, d)[1], i
            same_info(batch[i].feature_info(), single[i].feature_info())
        assert res[0]["num_extracted"] > 1000 and res[2]["num_extracted"] == 0 and cres[2]["n_in"] == 0
