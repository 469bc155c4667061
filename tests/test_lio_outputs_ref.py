"""CPU checks of the jueying_lio frame outputs and saved map: the numpy restatement (tests/lio_outputs_ref.py)
against an independent rotation-matrix formulation, its chunk counter against a literal transcription of
jueying_lio/src/laser_mapping.cc:776-791, the host bookkeeping header (csrc/lio_outputs.h) under AddressSanitizer and UBSan in a
stand-alone program, the presence of the C ABI and Python surfaces, and -- with the oracle -- that the scene of the GPU effect-cloud
test has rejected planes and points that fail the 81 pd2^2 test.  No GPU."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
from scipy.spatial.transform import Rotation

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lio_outputs_ref as ref  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "pointcloud-slam_amd", "csrc")
NAMES = ["pcm_lio_frame_world", "pcm_lio_frame_body", "pcm_lio_frame_effect", "pcm_lio_map_append", "pcm_lio_map_info_get", "pcm_lio_map_get",
         "pcm_lio_map_clear", "pcm_lio_map_export"]


def _state(seed):
    rng = np.random.default_rng(seed)
    return dict(rot=Rotation.from_rotvec(rng.uniform(-2, 2, 3)).as_quat(), pos=rng.uniform(-300, -100, 3),
                off_R=Rotation.from_rotvec(rng.uniform(-0.3, 0.3, 3)).as_quat(), off_T=rng.uniform(-0.2, 0.2, 3))


def _records(n, seed):
    rng = np.random.default_rng(seed)
    rec = np.zeros((n, 12), np.float32)
    rec[:, :3] = rng.uniform(-60, 60, (n, 3))
    rec[:, 8] = np.arange(n) * 0.25 + 1.0
    rec[:, 9] = rng.uniform(0, 0.1, n)
    return rec


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_restatement_equals_the_rotation_matrix_formulation(seed):
    """Term-by-term _transformVector against R p + t with R from scipy, in float64: 1e-12 relative to the largest coordinate."""
    st, rec = _state(seed), _records(1000, seed)
    p = rec[:, :3].astype(np.float64)
    R, oR = Rotation.from_quat(st["rot"]).as_matrix(), Rotation.from_quat(st["off_R"]).as_matrix()
    imu = p @ oR.T + st["off_T"]
    world = imu @ R.T + st["pos"]
    for got, want in ((ref.lidar_to_imu_d(st, rec[:, :3]), imu), (ref.body_to_world_d(st, rec[:, :3]), world)):
        assert np.max(np.abs(got - want)) <= 1e-12 * np.max(np.abs(want))
    w, b = ref.frame_world(st, rec), ref.frame_body(st, rec)
    assert w.dtype == np.float32 and np.max(np.abs(w[:, :3].astype(np.float64) - world)) <= 2.0 ** -24 * np.max(np.abs(world)) * 1.01   # one rounding to float
    assert np.array_equal(w[:, 3], rec[:, 8]) and np.array_equal(b[:, 3], rec[:, 8])       # intensity is copied
    sel = np.arange(len(rec)) % 3 == 1
    e = ref.frame_effect(st, rec, sel)
    assert len(e) == sel.sum() and np.array_equal(e[:, :3], w[sel, :3]) and np.array_equal(e[:, 3], np.abs(e[:, 2]))
    assert np.all(w[:, :3] < 0)                                                             # the negative octant


def _transcription(sizes, interval):
    """laser_mapping.cc:776-791 as written: -> per frame (chunk index written or 0, scan_wait_num after, cloud size after)."""
    pcl_wait_save, scan_wait_num, pcd_index, out = 0, 0, 0, []
    for n in sizes:
        pcl_wait_save += n
        scan_wait_num += 1
        wrote = 0
        if pcl_wait_save > 0 and interval > 0 and scan_wait_num >= interval:
            pcd_index += 1
            wrote = pcd_index
            pcl_wait_save = 0
            scan_wait_num = 0
        out.append((wrote, scan_wait_num, pcl_wait_save))
    return out


@pytest.mark.parametrize("interval", [-1, 1, 2, 3])
def test_chunk_counter_equals_the_transcription(interval):
    sizes = [257, 1025, 40, 513, 64, 3, 700]
    want = _transcription(sizes, interval)
    m = ref.SavedMap()
    for f, n in enumerate(sizes):
        ready, index = m.append(np.full((n, 4), f, np.float32), interval)
        assert ready == (want[f][0] != 0)
        if ready:
            assert index == want[f][0] and len(m.cloud()) == sum(sizes[f + 1 - interval:f + 1])
            m.clear()
        assert (m.scan_wait_num, len(m.cloud())) == want[f][1:]
    if interval <= 0:
        assert all(w[0] == 0 for w in want) and len(m.cloud()) == sum(sizes)               # :781: never a chunk


def test_export_restatement():
    cloud = np.array([[0, 0, -1, 1], [0, 0, 0.5, 2], [np.nan, 0, 0.5, 3], [0, np.inf, 0.5, 4], [0, 0, 2, 5], [0, 0, 2.5, 6]], np.float32)
    assert np.array_equal(ref.export(cloud).view(np.uint32), cloud.view(np.uint32))         # leaf 0, z_min > z_max: as it is
    assert ref.export(cloud, 0.0, 0.5, 2.0)[:, 3].tolist() == [2.0, 5.0]                     # limits inclusive, non-finite rows dropped
    assert ref.export(cloud, 0.1, -10, 10, voxel_grid=lambda c, leaf: c[::2])[:, 3].tolist() == [1.0, 5.0]


def test_host_bookkeeping_under_sanitizers(tmp_path):
    """csrc/lio_outputs.h through tests/lio_outputs_hooks.cpp: a stand-alone program built with -fsanitize=address,undefined."""
    hdr = os.path.join(CSRC, "lio_outputs.h")
    assert "#include <hip" not in open(hdr).read() and '#include "' not in open(hdr).read()
    exe = str(tmp_path / "lio_outputs_hooks")
    subprocess.run(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tests", "lio_outputs_hooks.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout + r.stderr


def test_surfaces_are_present():
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(CSRC, "exports.map")).read(), flags=re.S)
    header = open(os.path.join(ROOT, "include", "pcm_amd.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s;" % name, text), name + " is not in exports.map"
        assert re.search(r"\bint %s\(pcm_ctx \*ctx" % name, header), name + " is not declared in pcm_amd.h"
    assert "PCM_ABI_VERSION 3" in header and "typedef struct pcm_lio_map_info" in header
    import pointcloud_slam_amd as pcm
    assert set(NAMES) <= set(pcm.capi.SYMBOLS)
    for m in ("lio_frame_world", "lio_frame_body", "lio_frame_effect", "lio_map_append", "lio_map_info", "lio_map_get", "lio_map_clear", "lio_map_export"):
        assert callable(getattr(pcm.Registration, m, None)), m
    assert callable(getattr(pcm.LioOdometry, "finish", None))
    import inspect
    assert {"pcd_save_en", "dense_pub_en", "pcd_save_interval"} <= set(inspect.signature(pcm.LioOdometry.__init__).parameters)
    assert C_sizeof_info(pcm) == 48
    lib = os.path.join(ROOT, "pointcloud-slam_amd", "libpcm_amd.so")
    if os.path.exists(lib):
        syms = subprocess.run(["nm", "-D", "--defined-only", lib], capture_output=True, text=True, check=True).stdout
        for name in NAMES:
            assert re.search(r" T %s$" % name, syms, flags=re.M), name + " is not exported"


def C_sizeof_info(pcm):
    import ctypes
    return ctypes.sizeof(pcm.capi.PcmLioMapInfo)


def test_effect_scene_has_rejected_planes_and_failed_residual_tests():
    """The scene of the GPU effect-cloud test (tests/lio_outputs_case.py), on the oracle: after a matching ObsModel call some points
    have no accepted plane, and some with a plane fail |p_body| > 81 pd2^2, so the two halves of the flag are both exercised."""
    import lio_outputs_case as case
    from oracle import Oracle
    from oracle import loader
    sc = case.effect_scene()
    flt = loader.livox_filter(sc.msg, 6, case.POINT_FILTER_NUM, case.BLIND)
    ds = loader.voxel_downsample(flt, case.LEAF)
    st = sc.state
    o = Oracle("P2PLANE", "GN", **case.KW)
    o.set_input_target(sc.submap); o.set_input_source(ds)
    n_eff = o.obs_model(st["rot"], st["pos"], st["off_R"], st["off_T"], False, True)[2]
    planes, have_plane = o.get_planes(len(ds))          # after ObsModel the oracle's flag is the plane's validity only
    assert (~have_plane).sum() > 0, "no rejected plane"
    assert 0 < n_eff < have_plane.sum(), "no point fails the 81 pd2^2 test"
    planes = planes.copy(); planes[~have_plane, 0] = np.nan
    assert ref.default_selected(st, ds[:, :3], planes).sum() == n_eff    # the float restatement of the row test agrees with the oracle
