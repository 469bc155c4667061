"""CPU tests of the Python binding's shared parts (no GPU): the public surface equals the committed dump, the parameter filler
keeps every call site's rules, and the buffer helper accepts and refuses what each call site states."""
import ctypes as C
import importlib.util
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _flatten(d, path=""):
    if isinstance(d, dict):
        for k, v in d.items():
            yield from _flatten(v, path + "/" + k)
    else:
        yield path, d


def test_public_surface_is_the_committed_dump(pcm):
    """tools/dump_public_surface.py of this tree against tests/public_surface.json, dumped before the binding was split by subsystem:
    names, kinds, signatures, docstring digests and constants of the package, of ``registration`` and of every public class."""
    spec = importlib.util.spec_from_file_location("dump_public_surface", os.path.join(ROOT, "tools", "dump_public_surface.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    got = dict(_flatten(json.loads(json.dumps(tool.surface()))))
    want = dict(_flatten(json.load(open(os.path.join(ROOT, "tests", "public_surface.json")))))
    assert len(want) > 300
    assert sorted(set(got) ^ set(want)) == []
    assert {k: (want[k], got[k]) for k in want if got[k] != want[k]} == {}


# ---- the parameter filler ------------------------------------------------------------------------------------------------------
def _param_sites(pcm):
    """(struct, default function, hook, exception, a field, a value for it) of every call site of fill_params with a params struct."""
    from pointcloud_slam_amd import capi, loam, occ
    return [(capi.PcmLoamParams, "pcm_loam_default_params", None, KeyError, "iter_num", 7),
            (capi.PcmLoamFeatureParams, "pcm_loam_default_feature_params", loam._feature_key, KeyError, "n_scan", 32),
            (capi.PcmLoamSubmapParams, "pcm_loam_default_submap_params", None, KeyError, "surf_leaf", 0.75),
            (capi.PcmLoamScParams, "pcm_loam_default_sc_params", None, KeyError, "num_ring", 11),
            (capi.PcmLoamLoopParams, "pcm_loam_default_loop_params", None, KeyError, "history_search_num", 3),
            (capi.PcmOccParams, "pcm_occ_default_params", occ._occ_key, TypeError, "resolution", 0.25),
            (capi.PcmLoamDynmapParams, "pcm_loam_default_dynmap_params", None, KeyError, "margin", 9),
            (capi.PcmLoamGlobalParams, "pcm_loam_default_global_params", None, KeyError, "leaf", 0.5),
            (capi.PcmLoamTilesParams, "pcm_loam_default_tiles_params", None, KeyError, "tile_size", 12.5)]


def _fill(pcm, site, **kw):
    from pointcloud_slam_amd import _binding, occ
    cls, default, hook, exc = site[:4]
    unknown = occ._occ_unknown if exc is TypeError else KeyError
    return _binding.fill_params(cls, getattr(pcm.load_library(), default), kw, hook, unknown)


def test_fill_params_at_every_call_site(pcm):
    L = pcm.load_library()
    for site in _param_sites(pcm):
        cls, default, hook, exc, field, value = site
        ref = cls()
        C.memset(C.byref(ref), 0xA5, C.sizeof(ref))
        getattr(L, default)(C.byref(ref))
        assert bytes(_fill(pcm, site)) == bytes(ref), cls.__name__
        p = _fill(pcm, site, **{field: value})
        assert getattr(p, field) == value, cls.__name__
        setattr(ref, field, value)
        assert bytes(p) == bytes(ref), cls.__name__
        with pytest.raises(exc):
            _fill(pcm, site, no_such_field=1)
        for name, _ in cls._fields_:
            if name.startswith("reserved"):
                with pytest.raises(exc):
                    _fill(pcm, site, **{name: 0})


def test_fill_params_hooks(pcm):
    from pointcloud_slam_amd import capi, registration as reg
    sites = {s[0]: s for s in _param_sites(pcm)}
    feat = sites[capi.PcmLoamFeatureParams]
    base = _fill(pcm, feat).flags
    assert _fill(pcm, feat, force_serial_sort=True).flags == base | capi.PCM_LOAM_FEATURES_FORCE_SERIAL_SORT
    assert _fill(pcm, feat, force_serial_sort=False).flags == base & ~capi.PCM_LOAM_FEATURES_FORCE_SERIAL_SORT
    occ = sites[capi.PcmOccParams]
    p = _fill(pcm, occ, use_nan=True, fill_with_white=0, max_z=3)
    assert (p.use_nan, p.fill_with_white, p.max_z) == (1, 0, 3.0) and _fill(pcm, occ, use_nan=7.5).use_nan == 1
    with pytest.raises(TypeError, match="unknown occupancy parameter 'flags'"):
        _fill(pcm, occ, flags=1)
    # the tenth struct, through its own entry point: the table is kept alive and the layout goes by name
    L = pcm.load_library()
    ref = capi.PcmScanFuseParams()
    L.pcm_scan_default_fuse_params(C.byref(ref))
    assert bytes(reg.scan_fuse_params(L.pcm_scan_default_fuse_params, None)[0]) == bytes(ref)
    p, keep = reg.scan_fuse_params(L.pcm_scan_default_fuse_params, {"pitch_ring_table": [3, 1, 2], "layout": "XYZIR", "ring_below": 5})
    assert (p.pitch_ring_table, p.pitch_ring_table_len) == (keep[0].ctypes.data, 3) and keep[0].dtype == np.int32 and list(keep[0]) == [3, 1, 2]
    assert (p.output_layout, p.ring_below) == (capi.PCM_SCAN_OUT_XYZIR, 5)
    for bad in ("no_such_field", "reserved"):
        with pytest.raises(KeyError):
            reg.scan_fuse_params(L.pcm_scan_default_fuse_params, {bad: 1})
    # lidar_desc and lio_imu_state go through the same filler
    d = reg.lidar_desc("velodyne", time_kind="f64", ring_kind=capi.PCM_LIDAR_RING_UINT8, num_scans=16)
    assert (d.type, d.time_kind, d.ring_kind, d.num_scans) == (capi.PCM_LIDAR_VELODYNE, capi.PCM_LIDAR_TIME_DOUBLE, capi.PCM_LIDAR_RING_UINT8, 16)
    s = reg.lio_imu_state(mean_acc=(1, 2, 3), last_imu=(0.5, 1, 2, 3, 4, 5, 6), need_init=0)
    assert (list(s.mean_acc), s.last_imu.t, list(s.last_imu.gyr), s.need_init) == ([1.0, 2.0, 3.0], 0.5, [4.0, 5.0, 6.0], 0)
    for make in (lambda k: reg.lidar_desc("ouster", **{k: 1}), lambda k: reg.lio_imu_state(**{k: 1})):
        for bad in ("no_such_field", "reserved"):
            with pytest.raises(KeyError):
                make(bad)


# ---- the buffer helper ---------------------------------------------------------------------------------------------------------
HOST = 0   # capi.MEM_HOST
RULES = {   # call-site rule -> (keywords, an accepted float32 shape, a shape with a wrong column count)
    "points (set_input_*, target_insert, sc_add)": (dict(cols=(3, None), convert=True), (5, 3), (5, 2)),
    "cloud out (export_map, keyframe_global_map, get_tile, submap_near_device)": (dict(cols=(4, 4), write=True), (5, 4), (5, 5)),
    "records (voxel_downsample_large points)": (dict(cols=(3, 16), convert=True), (5, 16), (5, 17)),
    "records out (voxel_downsample_large out)": (dict(cols=(3, 16), write=True), (5, 3), (5, 2)),
    "flat 16-byte records (LIO outputs)": (dict(record=16, write=True), (42,), None),
}


@pytest.mark.parametrize("rule", sorted(RULES))
def test_buffer_arg_rules(pcm, rule):
    import torch
    from pointcloud_slam_amd._binding import buffer_arg
    kw, shape, wrong = RULES[rule]
    convert, write = kw.get("convert", False), kw.get("write", False)
    a = np.arange(np.prod(shape), dtype=np.float32).reshape(shape)
    rows, row_bytes = (shape[0], 4 * shape[1]) if "cols" in kw else (a.size // 4, 16)
    ptr, n, stride, mem, keep = buffer_arg(a, **kw)
    assert (ptr, n, stride, mem) == (a.ctypes.data, rows, row_bytes, HOST) and keep is a
    strided = np.zeros((shape[0], 2 * shape[-1]) if len(shape) == 2 else (2 * shape[0],), np.float32)[..., ::2]
    refused = [np.float32(1.0)] if "cols" in kw else []
    if wrong is not None:
        refused.append(np.zeros(wrong, np.float32))
    if convert:   # host data is converted: another dtype, a strided view, a list and a host torch tensor all arrive as float32 rows
        for b in (a.astype(np.float64), np.asfortranarray(a), a.tolist(), torch.from_numpy(a.copy())):
            ptr, n, stride, mem, keep = buffer_arg(b, **kw)
            assert (ptr, n, stride, mem) == (keep.ctypes.data, rows, row_bytes, HOST)
            assert keep.dtype == np.float32 and keep.flags.c_contiguous and (keep == a).all()
        t = torch.from_numpy(a)
        assert buffer_arg(t, **kw)[0] == t.data_ptr()   # read in place, not copied
    else:         # the library writes (or reads in place): only a ready float32 array will do
        refused += [a.astype(np.float64), a.astype(np.int32), strided, a.tolist(), torch.from_numpy(a.copy())]
    if write:
        ro = a.copy()
        ro.setflags(write=False)
        refused.append(ro)
    for b in refused:
        with pytest.raises(ValueError):
            buffer_arg(b, **kw)


def test_buffer_arg_byte_records(pcm):
    """Scans and handler input: records of a stride of any element type; a size that is no whole number of records is refused."""
    from pointcloud_slam_amd._binding import buffer_arg
    rec = np.zeros((7, 48), np.uint8)
    assert buffer_arg(rec, record=48, f32=False, convert=True)[:4] == (rec.ctypes.data, 7, 48, HOST)
    structured = np.zeros(5, np.dtype([("t", "u4"), ("xyz", "f4", 3), ("tag", "u1", 4)]))
    assert buffer_arg(structured, record=20, f32=False, convert=True)[:4] == (structured.ctypes.data, 5, 20, HOST)
    with pytest.raises(ValueError):
        buffer_arg(rec, record=32 * 5, f32=False, convert=True)
    out = np.zeros((4, 32), np.uint8)
    assert buffer_arg(out, record=32, f32=False, write=True)[:4] == (out.ctypes.data, 4, 32, HOST)
    out.setflags(write=False)
    for bad in (out, np.zeros((4, 64), np.uint8)[:, ::2], [[0] * 32]):
        with pytest.raises(ValueError):
            buffer_arg(bad, record=32, f32=False, write=True)


def test_stored_result_accessor(pcm):
    from pointcloud_slam_amd._binding import Context
    c = Context.__new__(Context)
    with pytest.raises(pcm.PcmError, match="submap_info before update_submap") as e:
        c._stored("_submap", "submap_info before update_submap")
    assert e.value.code == -2
    c._submap = 5
    assert c._stored("_submap", "submap_info before update_submap") == 5
