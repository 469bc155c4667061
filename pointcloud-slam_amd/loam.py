"""jueying_slam's LOAM on one HIP device (a PCM_MODEL_LOAM ``pcm_ctx``), grouped as DESIGN.md groups it: scan-to-map, the
front end (section 10), key frames and submap (11), Scan Context and loop (12, 19), localisation tiles and crop (14, 31),
global map and export (20).  ``LoamRegistration`` at the end names the groups."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from ._binding import Context, buffer_arg, default_config, fill_params
from .occ import _OccMixin
from .scan import FUSED_INTENSITY, FUSED_RING, FUSED_STRIDE, _ScanMixin, _VoxelLargeMixin


def _pose6(pose6):
    return np.ascontiguousarray(pose6, dtype=np.float32).reshape(6)


def _xyzi(a):
    a = np.asarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("expected an (N,>=3) float32 array")
    b = np.zeros((a.shape[0], 4), np.float32)
    b[:, :min(4, a.shape[1])] = a[:, :4]
    return b


# ---- LOAM scan-to-map (jueying_slam mapOptmization.cpp:1560-1586) -------------------------------------------------------------
@dataclasses.dataclass
class LoamResult:
    x: np.ndarray             # (6,) float32 transformTobeMapped: roll, pitch, yaw, x, y, z
    iterations: int
    converged: bool
    degenerate: bool
    status: int               # PCM_OK or PCM_ERR_TOO_FEW_FEATURES (pose left as given)
    eigenvalues: np.ndarray   # (6,) of A^T A at iteration 0, descending
    num_corner: int
    num_surf: int
    corner_fitness: float
    surf_fitness: float
    maps_built: bool


def _loam_result(r: capi.PcmLoamResult) -> LoamResult:
    return LoamResult(np.array(r.x[:], np.float32), r.iterations, bool(r.converged), bool(r.degenerate), r.status,
                      np.array(r.eigenvalues[:]), r.num_corner, r.num_surf, r.corner_fitness, r.surf_fitness, bool(r.maps_built))


def _feature_pair(corner, surf):
    """Both clouds as (N,4) float32 host arrays (one stride for the two)."""
    out = []
    for a in (corner, surf):
        a = np.asarray(a, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("expected (N,>=3) float32 arrays")
        b = np.zeros((a.shape[0], 4), np.float32)
        b[:, :3] = a[:, :3]
        out.append(b)
    return out


class _ScanToMap:
    def set_input_target(self, corner, surf, tag: int = 0):
        c, s = _feature_pair(corner, surf)
        self._check(self._L.pcm_loam_set_target(self._h, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], 16, capi.MEM_HOST, tag))

    def set_input_source(self, corner, surf, tag: int = 0):
        c, s = _feature_pair(corner, surf)
        self._check(self._L.pcm_loam_set_source(self._h, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], 16, capi.MEM_HOST, tag))
        self.n_corner, self.n_surf = c.shape[0], s.shape[0]

    def scan2map(self, x6, **params) -> LoamResult:
        p = fill_params(capi.PcmLoamParams, self._L.pcm_loam_default_params, {**self.params, **params})
        x = _pose6(x6)
        r = capi.PcmLoamResult()
        self._check(self._L.pcm_loam_align(self._h, C.byref(p), x.ctypes.data, C.byref(r)), (capi.PCM_OK, capi.PCM_ERR_TOO_FEW_FEATURES))
        return _loam_result(r)

    def coefficients(self, x6):
        """Parity hook at a fixed pose: (corner (Nc,4), surf (Ns,4)) coefficients (coeff.xyz, intensity; NaN = not selected),
        A^T A (6,6), A^T b (6,), counts (selected corner, selected surf, corner / surf features with sqDis[0] <= 1)."""
        x = _pose6(x6)
        co = np.zeros((self.n_corner, 4), np.float32)
        su = np.zeros((self.n_surf, 4), np.float32)
        AtA = np.zeros((6, 6))
        AtB = np.zeros(6)
        cnt = np.zeros(4, np.int32)
        self._check(self._L.pcm_loam_coefficients(self._h, x.ctypes.data, co.ctypes.data, su.ctypes.data, AtA.ctypes.data, AtB.ctypes.data, cnt.ctypes.data))
        return co, su, AtA, AtB, cnt

    def neighbours(self, x6):
        """Parity hook: the 5 nearest map indices with d^2 <= 1 (ascending (d^2, index), -1 pads) of every corner / surf feature."""
        x = _pose6(x6)
        cn = np.zeros((self.n_corner, 5), np.int32)
        sn = np.zeros((self.n_surf, 5), np.int32)
        self._check(self._L.pcm_loam_neighbours(self._h, x.ctypes.data, cn.ctypes.data, sn.ctypes.data))
        return cn, sn


def loam_align_batch(regs, x6s, **params):
    """scan2MapOptimization of independent LoamRegistration objects in lock-step launches (pcm_loam_align_batch)."""
    L = capi.load_library()
    n = len(regs)
    p = fill_params(capi.PcmLoamParams, L.pcm_loam_default_params, {**regs[0].params, **params})
    x = np.ascontiguousarray(x6s, dtype=np.float32).reshape(n, 6)
    arr = (C.c_void_p * n)(*[r.handle for r in regs])
    out = (capi.PcmLoamResult * n)()
    rc = L.pcm_loam_align_batch(arr, n, C.byref(p), x.ctypes.data, out)
    if rc not in (capi.PCM_OK, capi.PCM_ERR_TOO_FEW_FEATURES):
        raise capi.PcmError(rc, (L.pcm_last_error(regs[0].handle) or b"").decode())
    return [_loam_result(out[i]) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------
# LOAM front end: imageProjection + featureExtraction + downsampleCurrentScan on the device
# ---------------------------------------------------------------------------------------------------------------------------
XYZIRT_STRIDE, XYZIRT_INTENSITY, XYZIRT_RING = 48, 16, 32   # PointXYZIRT (imageProjection.cpp:7-19)


def pack_xyzirt(xyz, intensity=None, ring=None, timestamp=None) -> np.ndarray:
    """48-byte PointXYZIRT records as an (N, 48) uint8 array: x y z floats at 0, uint8 intensity at 16, double timestamp at 24
    (never read), uint16 ring at 32."""
    xyz = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    n = xyz.shape[0]
    rec = np.zeros((n, XYZIRT_STRIDE), np.uint8)
    rec[:, 0:12] = np.ascontiguousarray(xyz).view(np.uint8).reshape(n, 12)
    if intensity is not None:
        rec[:, XYZIRT_INTENSITY] = np.asarray(intensity).astype(np.uint8).reshape(n)
    if timestamp is not None:
        rec[:, 24:32] = np.ascontiguousarray(np.asarray(timestamp, np.float64).reshape(n)).view(np.uint8).reshape(n, 8)
    if ring is not None:
        rec[:, XYZIRT_RING:XYZIRT_RING + 2] = np.ascontiguousarray(np.asarray(ring).astype(np.uint16).reshape(n)).view(np.uint8).reshape(n, 2)
    return rec


def _feature_key(p, k, v):
    if k != "force_serial_sort":
        return False
    p.flags = (p.flags | capi.PCM_LOAM_FEATURES_FORCE_SERIAL_SORT) if v else (p.flags & ~capi.PCM_LOAM_FEATURES_FORCE_SERIAL_SORT)
    return True


def _feature_args(L, feature_params: dict):
    """The keywords of a front-end call split into the record layout (stride, intensity offset, ring offset) and pcm_loam_feature_params."""
    fp = dict(feature_params)
    layout = (fp.pop("stride", XYZIRT_STRIDE), fp.pop("intensity_offset", XYZIRT_INTENSITY), fp.pop("ring_offset", XYZIRT_RING))
    return layout, fill_params(capi.PcmLoamFeatureParams, L.pcm_loam_default_feature_params, fp, _feature_key)


def _features_result(r: capi.PcmLoamFeaturesResult) -> dict:
    return {k: getattr(r, k) for k, _ in r._fields_ if k != "reserved"}


class _FrontEnd:
    def set_input_scan(self, cloud, **feature_params) -> dict:
        """featureExtraction + downsampleCurrentScan of one ring-tagged scan into this context's LOAM source, on the device
        (pcm_loam_frame_begin).  Then ``scan2map`` as after ``set_input_source``."""
        (stride, ioff, roff), p = _feature_args(self._L, feature_params)
        ptr, n, _, mem, keep = buffer_arg(cloud, record=stride, f32=False, convert=True, what="scan:")
        r = capi.PcmLoamFeaturesResult()
        self._check(self._L.pcm_loam_frame_begin(self._h, ptr, n, stride, ioff, roff, mem, C.byref(p), C.byref(r)))
        del keep
        self.n_corner, self.n_surf = r.num_corner, r.num_surf
        return _features_result(r)

    def frame_begin_fused(self, segments, fuse_params=None, **feature_params):
        """fuse_scans into the context's device buffer, then pcm_loam_frame_begin on it where it lies -> (features result, counts)."""
        _, counts = self.fuse_scans(segments, fuse_params, out=None)
        ptr, n = self.fused_scan()
        _, p = _feature_args(self._L, feature_params)   # the layout is the fused records', whatever the keywords say
        r = capi.PcmLoamFeaturesResult()
        self._check(self._L.pcm_loam_frame_begin(self._h, ptr, n, FUSED_STRIDE, FUSED_INTENSITY, FUSED_RING, capi.MEM_DEVICE, C.byref(p), C.byref(r)))
        self.n_corner, self.n_surf = r.num_corner, r.num_surf
        return _features_result(r), counts

    def feature_info(self) -> dict:
        """Parity hook: the last frame's intermediate arrays (pcm_loam_feature_info)."""
        cnt = np.zeros(4, np.int32)
        self._check(self._L.pcm_loam_feature_info(self._h, cnt.ctypes.data, *([None] * 10)))
        n, nc, ns, nsc = (int(v) for v in cnt)
        out = {"start": np.zeros(nsc, np.int32), "end": np.zeros(nsc, np.int32), "col_ind": np.zeros(n, np.int32), "range": np.zeros(n, np.float32),
               "cloud": np.zeros((n, 4), np.float32), "curvature": np.zeros(n, np.float32), "neighbor_picked": np.zeros(n, np.int32),
               "label": np.zeros(n, np.int32), "corner_scan": np.zeros((nc, 4), np.float32), "surf_scan": np.zeros((ns, 4), np.float32)}
        self._check(self._L.pcm_loam_feature_info(self._h, cnt.ctypes.data, *(out[k].ctypes.data for k in
                                                  ("start", "end", "col_ind", "range", "cloud", "curvature", "neighbor_picked", "label", "corner_scan", "surf_scan"))))
        return out


def loam_extract_features(reg: LoamRegistration, cloud, **feature_params):
    """One scan to (corner (Nc,4), surf (Ns,4), info): laserCloudCornerLastDS / laserCloudSurfLastDS as (x, y, z, intensity) on
    the host (pcm_loam_extract_features; the context's LOAM source is left as it is, its cross-frame state advances)."""
    (stride, ioff, roff), p = _feature_args(reg._L, feature_params)
    ptr, n, _, mem, keep = buffer_arg(cloud, record=stride, f32=False, convert=True, what="scan:")
    r = capi.PcmLoamFeaturesResult()
    cap = max(1, n)
    corner = np.zeros((cap, 4), np.float32)
    surf = np.zeros((cap, 4), np.float32)
    reg._check(reg._L.pcm_loam_extract_features(reg.handle, ptr, n, stride, ioff, roff, mem, C.byref(p), corner.ctypes.data, cap,
                                                surf.ctypes.data, cap, C.byref(r)))
    del keep
    info = _features_result(r)
    return corner[:r.num_corner].copy(), surf[:r.num_surf].copy(), info


def loam_frame_begin_batch(regs, clouds, **feature_params):
    """pcm_loam_frame_begin of n scans into n LoamRegistration contexts in one set of launches; returns n result dicts."""
    L = capi.load_library()
    (stride, ioff, roff), p = _feature_args(L, feature_params)
    n = len(regs)
    if len(clouds) != n:
        raise ValueError("one scan per context")
    args = [buffer_arg(c, record=stride, f32=False, convert=True, what="scan:") for c in clouds]
    mems = {a[3] for a in args}
    if len(mems) != 1:
        raise ValueError("all scans of a batch must be host arrays or all device tensors")
    hs = (C.c_void_p * n)(*[r.handle for r in regs])
    ptrs = (C.c_void_p * n)(*[a[0] for a in args])
    ns = (C.c_size_t * n)(*[a[1] for a in args])
    out = (capi.PcmLoamFeaturesResult * n)()
    regs[0]._check(L.pcm_loam_frame_begin_batch(hs, n, ptrs, ns, stride, ioff, roff, mems.pop(), C.byref(p), out))
    res = [_features_result(out[i]) for i in range(n)]
    for reg, r in zip(regs, res):
        reg.n_corner, reg.n_surf = r["num_corner"], r["num_surf"]
    return res


# ---- IMU / odometry deskew in front of the features -----------------------------------------------------
def loam_deskew_tables(time_scan_cur, imu, odom=None, time_scan_next=float("inf")):
    """deskewInfo (pcm_loam_deskew_tables): ``imu`` (N,4) rows of (stamp, gyro x y z) after imuConverter, ``odom`` (M,4) rows of
    (stamp, x, y, z), both front first.  ``time_scan_next`` = inf is new_localization.cpp's form (no upper gate, no break).
    Returns None while waiting for IMU data, else a dict: the descriptor fields ``time_scan_cur``, ``imu`` (n_imu,4) rows of
    (time, rot x y z), ``odom`` (n_odom,4) rows of (time, increment x y z), ``imu_available``, and the builder's ``imu_skipped``,
    ``odom_skipped``, ``odom_available``, ``odom_deskew``, ``start_odom_index``.  It is what the *_deskew calls take."""
    L = capi.load_library()
    im = np.ascontiguousarray(imu, dtype=np.float64).reshape(-1, 4)
    od = np.ascontiguousarray(odom if odom is not None else np.zeros((0, 4)), dtype=np.float64).reshape(-1, 4)
    inp = capi.PcmLoamDeskewInput(time_scan_cur=time_scan_cur, time_scan_next=time_scan_next, imu=im.ctypes.data, odom=od.ctypes.data,
                                  n_imu=im.shape[0], n_odom=od.shape[0])
    ci, co = max(1, min(im.shape[0], 1024)), max(1, min(od.shape[0], 1024))
    it, ot = np.zeros((4, ci)), np.zeros((4, co))
    r = capi.PcmLoamDeskewResult()
    rc = L.pcm_loam_deskew_tables(C.byref(inp), it.ctypes.data, ci, ot.ctypes.data, co, None, C.byref(r))
    if rc != capi.PCM_OK:
        raise capi.PcmError(rc, "pcm_loam_deskew_tables: more than 1024 table entries" if rc == capi.PCM_ERR_UNSUPPORTED else "pcm_loam_deskew_tables")
    if r.status == capi.PCM_LOAM_DESKEW_WAITING:
        return None
    out = {k: getattr(r, k) for k, _ in r._fields_ if k not in ("reserved", "status", "n_imu", "n_odom")}
    out.update(time_scan_cur=float(time_scan_cur), imu=it[:, :r.n_imu].T.copy(), odom=ot[:, :r.n_odom].T.copy())
    return out


def _deskew_arg(deskew):
    """``deskew`` (None, or a dict with time_scan_cur, imu (n,4), optional odom (m,4), imu_available, optional time_offset and
    time_kind) as a pcm_loam_deskew -> (struct or None, keep-alive)."""
    if deskew is None:
        return None, None
    im = np.ascontiguousarray(np.asarray(deskew["imu"], dtype=np.float64).reshape(-1, 4).T)
    odom = deskew.get("odom")
    od = np.ascontiguousarray(np.asarray(odom if odom is not None else np.zeros((0, 4)), dtype=np.float64).reshape(-1, 4).T)
    d = capi.PcmLoamDeskew(time_scan_cur=deskew["time_scan_cur"], n_imu=im.shape[1], n_odom=od.shape[1],
                           imu_available=int(deskew.get("imu_available", 1)), time_kind=deskew.get("time_kind", capi.PCM_LOAM_TIME_DOUBLE),
                           time_offset_bytes=deskew.get("time_offset", 24))
    if im.shape[1]:
        d.imu_time, d.imu_rot_x, d.imu_rot_y, d.imu_rot_z = (im[k].ctypes.data for k in range(4))
    if od.shape[1]:
        d.odom_time, d.odom_incre_x, d.odom_incre_y, d.odom_incre_z = (od[k].ctypes.data for k in range(4))
    return d, (im, od)


def loam_extract_features_deskew(reg: LoamRegistration, cloud, deskew=None, **feature_params):
    """loam_extract_features with deskewPoint in front (pcm_loam_extract_features_deskew); ``deskew``: loam_deskew_tables' dict."""
    (stride, ioff, roff), p = _feature_args(reg._L, feature_params)
    ptr, n, _, mem, keep = buffer_arg(cloud, record=stride, f32=False, convert=True, what="scan:")
    d, keep_d = _deskew_arg(deskew)
    r = capi.PcmLoamFeaturesResult()
    cap = max(1, n)
    corner = np.zeros((cap, 4), np.float32)
    surf = np.zeros((cap, 4), np.float32)
    reg._check(reg._L.pcm_loam_extract_features_deskew(reg.handle, ptr, n, stride, ioff, roff, mem, C.byref(p), corner.ctypes.data, cap,
                                                       surf.ctypes.data, cap, C.byref(r), C.byref(d) if d is not None else None))
    del keep, keep_d
    return corner[:r.num_corner].copy(), surf[:r.num_surf].copy(), _features_result(r)


def loam_frame_begin_deskew(reg: LoamRegistration, cloud, deskew=None, **feature_params) -> dict:
    """LoamRegistration.set_input_scan with deskewPoint in front (pcm_loam_frame_begin_deskew)."""
    (stride, ioff, roff), p = _feature_args(reg._L, feature_params)
    ptr, n, _, mem, keep = buffer_arg(cloud, record=stride, f32=False, convert=True, what="scan:")
    d, keep_d = _deskew_arg(deskew)
    r = capi.PcmLoamFeaturesResult()
    reg._check(reg._L.pcm_loam_frame_begin_deskew(reg.handle, ptr, n, stride, ioff, roff, mem, C.byref(p), C.byref(r), C.byref(d) if d is not None else None))
    del keep, keep_d
    reg.n_corner, reg.n_surf = r.num_corner, r.num_surf
    return _features_result(r)


def loam_frame_begin_batch_deskew(regs, clouds, deskews, **feature_params):
    """loam_frame_begin_batch with one ``deskew`` (or None) per frame (pcm_loam_frame_begin_batch_deskew)."""
    L = capi.load_library()
    (stride, ioff, roff), p = _feature_args(L, feature_params)
    n = len(regs)
    if len(clouds) != n or len(deskews) != n:
        raise ValueError("one scan and one deskew (or None) per context")
    args = [buffer_arg(c, record=stride, f32=False, convert=True, what="scan:") for c in clouds]
    mems = {a[3] for a in args}
    if len(mems) != 1:
        raise ValueError("all scans of a batch must be host arrays or all device tensors")
    ds = [_deskew_arg(d) for d in deskews]
    hs = (C.c_void_p * n)(*[r.handle for r in regs])
    ptrs = (C.c_void_p * n)(*[a[0] for a in args])
    ns = (C.c_size_t * n)(*[a[1] for a in args])
    dp = (C.POINTER(capi.PcmLoamDeskew) * n)(*[C.pointer(d) if d is not None else C.POINTER(capi.PcmLoamDeskew)() for d, _ in ds])
    out = (capi.PcmLoamFeaturesResult * n)()
    regs[0]._check(L.pcm_loam_frame_begin_batch_deskew(hs, n, ptrs, ns, stride, ioff, roff, mems.pop(), C.byref(p), out, dp))
    res = [_features_result(out[i]) for i in range(n)]
    for reg, r in zip(regs, res):
        reg.n_corner, reg.n_surf = r["num_corner"], r["num_surf"]
    return res


# ---- cachePointCloud: the driver's organised cloud to the front end's records ---------------------------
LOAM_LIDAR_TYPE = {"velodyne": capi.PCM_LOAM_LIDAR_VELODYNE, "rslidar_ruby": capi.PCM_LOAM_LIDAR_RSLIDAR_RUBY,
                   "rslidar_16": capi.PCM_LOAM_LIDAR_RSLIDAR_16, "rslidar_32": capi.PCM_LOAM_LIDAR_RSLIDAR_32}
LOAM_CLOUD_KIND = {"mapping": capi.PCM_LOAM_CLOUD_MAPPING, "localization": capi.PCM_LOAM_CLOUD_LOCALIZATION}
LOAM_CLOUD_STRIDE = {capi.PCM_LOAM_CLOUD_MAPPING: 48, capi.PCM_LOAM_CLOUD_LOCALIZATION: 32}


def _cloud_desc_key(p, k, v):
    if k in ("ring_offset_bytes", "time_offset_bytes") and v is None:   # the message has no such field
        setattr(p, k, capi.PCM_LOAM_FIELD_ABSENT)
        return True
    return False


def loam_cloud_desc(lidar_type, record_kind="mapping", **overrides) -> capi.PcmLoamCloudDesc:
    """pcm_loam_cloud_default_desc of a lidar type ("velodyne" | "rslidar_ruby" | "rslidar_16" | "rslidar_32", or the
    reference's elidar_type number) and a record kind ("mapping" | "localization"), with any field of pcm_loam_cloud_desc
    overridden (height, width, point_step, the offsets -- ``ring_offset_bytes`` / ``time_offset_bytes`` None: the message has
    no such field --, is_dense, synth_ring, synth_time)."""
    t = LOAM_LIDAR_TYPE.get(lidar_type, lidar_type) if isinstance(lidar_type, str) else int(lidar_type)
    k = LOAM_CLOUD_KIND.get(record_kind, record_kind) if isinstance(record_kind, str) else int(record_kind)
    default = capi.load_library().pcm_loam_cloud_default_desc
    return fill_params(capi.PcmLoamCloudDesc, lambda d: default(t, k, d), overrides, _cloud_desc_key)


def _cloud_result(r: capi.PcmLoamCloudResult) -> dict:
    return {k: getattr(r, k) for k, _ in r._fields_ if k != "reserved"}


def _cloud_arg(data, desc):
    """The raw bytes of ``desc.height x desc.width`` records of ``desc.point_step`` bytes -> (pointer, memory, keep-alive)."""
    ptr, n, _, mem, keep = buffer_arg(data, record=max(1, desc.point_step), f32=False, convert=True, what="cloud:")
    if n != desc.height * desc.width:
        raise ValueError("cloud: %d records of %d bytes, the descriptor says %d x %d" % (n, desc.point_step, desc.height, desc.width))
    return (ptr if n else None), mem, keep


def loam_cloud_prepare(reg: LoamRegistration, data, desc, out=None):
    """cachePointCloud on the device (pcm_loam_cloud_prepare): ``data`` the organised cloud's raw bytes (host array or device
    tensor), ``desc`` from loam_cloud_desc.  out None: the records stay in the context's device buffer -> (None, result); out
    "host": -> ((n_out, 48 | 32) uint8 array, result); out a device tensor or a host array of capacity x (48 | 32) bytes:
    filled -> (out, result).  A capacity below n_out raises PcmError; nothing past the capacity is written."""
    stride = LOAM_CLOUD_STRIDE.get(desc.record_kind, 48)   # an unknown kind is the library's to refuse
    ptr, mem, keep = _cloud_arg(data, desc)
    r = capi.PcmLoamCloudResult()
    optr, cap, omem, ret, keep_o = None, 0, capi.MEM_HOST, None, None
    if isinstance(out, str) and out == "host":
        ret = np.zeros((max(desc.height * desc.width, 1), stride), np.uint8)
        optr, cap = ret.ctypes.data, ret.shape[0]
    elif out is not None:
        optr, cap, _, omem, keep_o = buffer_arg(out, record=stride, f32=False, write=True, what="out:")
        ret = out
    reg._check(reg._L.pcm_loam_cloud_prepare(reg.handle, ptr, C.byref(desc), mem, optr, cap, omem, C.byref(r)))
    del keep, keep_o
    if isinstance(out, str):
        ret = ret[:r.n_out].copy()
    return ret, _cloud_result(r)


def loam_frame_begin_cloud(reg: LoamRegistration, data, desc, deskew=None, **feature_params):
    """The raw organised cloud through cachePointCloud and the front end into the context's LOAM source
    (pcm_loam_frame_begin_cloud) -> (features result, cloud result).  ``deskew``: loam_deskew_tables' dict or None; its time
    field is the prepared record's, and it is ignored when the cloud has no time (``time_available`` 0).  The record layout
    keywords of the other front-end calls do not apply."""
    _, p = _feature_args(reg._L, feature_params)
    ptr, mem, keep = _cloud_arg(data, desc)
    d, keep_d = _deskew_arg(deskew)
    r, cr = capi.PcmLoamFeaturesResult(), capi.PcmLoamCloudResult()
    reg._check(reg._L.pcm_loam_frame_begin_cloud(reg.handle, ptr, C.byref(desc), mem, C.byref(p), C.byref(r), C.byref(d) if d is not None else None, C.byref(cr)))
    del keep, keep_d
    reg.n_corner, reg.n_surf = r.num_corner, r.num_surf
    return _features_result(r), _cloud_result(cr)


def loam_frame_begin_cloud_batch(regs, datas, descs, deskews=None, **feature_params):
    """loam_frame_begin_cloud of n clouds into n LoamRegistration contexts in one round of launches
    (pcm_loam_frame_begin_cloud_batch) -> (n features results, n cloud results).  One record kind per batch."""
    L = capi.load_library()
    _, p = _feature_args(L, feature_params)
    n = len(regs)
    deskews = [None] * n if deskews is None else deskews
    if len(datas) != n or len(descs) != n or len(deskews) != n:
        raise ValueError("one cloud, one descriptor and one deskew (or None) per context")
    args = [_cloud_arg(a, d) for a, d in zip(datas, descs)]
    mems = {a[1] for a in args}
    if len(mems) != 1:
        raise ValueError("all clouds of a batch must be host arrays or all device tensors")
    ds = [_deskew_arg(d) for d in deskews]
    hs = (C.c_void_p * n)(*[r.handle for r in regs])
    ptrs = (C.c_void_p * n)(*[a[0] for a in args])
    da = (capi.PcmLoamCloudDesc * n)()
    for i, d in enumerate(descs):
        C.memmove(C.byref(da[i]), C.byref(d), C.sizeof(capi.PcmLoamCloudDesc))
    dp = (C.POINTER(capi.PcmLoamDeskew) * n)(*[C.pointer(d) if d is not None else C.POINTER(capi.PcmLoamDeskew)() for d, _ in ds])
    out, cout = (capi.PcmLoamFeaturesResult * n)(), (capi.PcmLoamCloudResult * n)()
    regs[0]._check(L.pcm_loam_frame_begin_cloud_batch(hs, n, ptrs, da, mems.pop(), C.byref(p), out, dp, cout))
    res = [_features_result(out[i]) for i in range(n)]
    for reg, r in zip(regs, res):
        reg.n_corner, reg.n_surf = r["num_corner"], r["num_surf"]
    return res, [_cloud_result(cout[i]) for i in range(n)]


# ---------------------------------------------------------------------------------------------------------------------------
# LOAM key-frame store and surrounding-key-frame submap on the device
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoamSubmapResult:
    num_keyframes: int
    num_near: int
    num_pose_leaves: int
    num_selected: int
    num_skipped: int
    num_corner_in: int
    num_surf_in: int
    num_corner_map: int
    num_surf_map: int
    rebuilt: bool
    status: int


class _KeyFrames:
    def add_keyframe(self, pose6, time, corner=None, surf=None) -> int:
        """saveKeyFramesAndFactor: a key frame with pose6 (roll, pitch, yaw, x, y, z), its time and its (N,4) x y z intensity clouds in
        the body frame.  Without clouds the context's current LOAM source is copied on the device.  Returns the key frame's index."""
        x = _pose6(pose6)
        if (corner is None) != (surf is None):
            raise ValueError("pass both clouds or neither")
        if corner is None:
            self._check(self._L.pcm_loam_keyframe_add(self._h, x.ctypes.data, float(time), None, 0, None, 0, 16, capi.MEM_HOST))
        else:
            c, s = _xyzi(corner), _xyzi(surf)
            self._check(self._L.pcm_loam_keyframe_add(self._h, x.ctypes.data, float(time), c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], 16, capi.MEM_HOST))
        return self.num_keyframes - 1

    def set_keyframe_poses(self, poses, first: int = 0):
        """correctPoses: new (n,6) poses for key frames first .. first + n - 1."""
        x = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 6)
        self._check(self._L.pcm_loam_keyframe_set_poses(self._h, int(first), x.shape[0], x.ctypes.data))

    @property
    def num_keyframes(self) -> int:
        n = self._L.pcm_loam_keyframe_count(self._h)
        if n < 0:
            self._check(n)
        return n

    def clear_keyframes(self):
        self._check(self._L.pcm_loam_keyframe_clear(self._h))

    def get_keyframe(self, key: int):
        """(corner (Nc,4), surf (Ns,4)) of one stored key frame: body frame, x y z intensity."""
        get, h, other = self._L.pcm_loam_keyframe_get, self._h, C.c_size_t(0)
        return (self._counted(lambda p, cap, mem, n: get(h, int(key), p, cap, None, 0, C.byref(n), C.byref(other))),
                self._counted(lambda p, cap, mem, n: get(h, int(key), None, 0, p, cap, C.byref(other), C.byref(n))))

    def update_submap(self, time_cur, **params) -> LoamSubmapResult:
        """extractSurroundingKeyFrames at timeLaserInfoCur = time_cur: the down-sampled corner / surf submap of the surrounding key
        frames becomes this context's target (pcm_loam_submap_update)."""
        p = fill_params(capi.PcmLoamSubmapParams, self._L.pcm_loam_default_submap_params, params)
        r = capi.PcmLoamSubmapResult()
        self._check(self._L.pcm_loam_submap_update(self._h, C.byref(p), float(time_cur), C.byref(r)))
        self._submap = r
        return LoamSubmapResult(r.num_keyframes, r.num_near, r.num_pose_leaves, r.num_selected, r.num_skipped, r.num_corner_in, r.num_surf_in,
                                r.num_corner_map, r.num_surf_map, bool(r.rebuilt), r.status)

    def near_keyframes(self, key: int, search_num: int, wrt_key: int = -1, leaf: float = 0.2) -> np.ndarray:
        """loopFindNearKeyframes (wrt_key < 0) / loopFindNearKeyframesWithRespectTo: (M,4) x y z intensity on the host."""
        n = C.c_size_t(0)
        total = 0
        K = self.num_keyframes
        for k in range(max(0, key - search_num), min(K, key + search_num + 1)):
            a, b = C.c_size_t(0), C.c_size_t(0)
            self._check(self._L.pcm_loam_keyframe_get(self._h, k, None, 0, None, 0, C.byref(a), C.byref(b)))
            total += a.value + b.value
        out = np.zeros((max(1, total), 4), np.float32)
        self._check(self._L.pcm_loam_submap_near(self._h, int(key), int(search_num), int(wrt_key), float(leaf), out.ctypes.data, out.shape[0], C.byref(n)))
        return out[:n.value].copy()

    def submap_near_device(self, key: int, search_num: int, wrt_key: int = -1, leaf: float = 0.2, out=None):
        """pcm_loam_submap_near_dev: the cloud of ``near_keyframes``, bit for bit, as (x, y, z, intensity) rows of ``out`` -- a
        contiguous (cap, 4) float32 device tensor (written on the context's stream; with leaf == 0 the call does not wait) or a
        (cap, 4) float32 host array.  Returns the number of rows written."""
        n = C.c_size_t(0)
        ptr, cap, _, mem, _ = buffer_arg(out, (4, 4), write=True)
        rc = self._L.pcm_loam_submap_near_dev(self._h, int(key), int(search_num), int(wrt_key), float(leaf), ptr, cap, mem, C.byref(n))
        self._near_count = n.value
        self._check(rc)
        return n.value

    def submap_info(self) -> dict:
        """Parity hook: the last update's selection and its clouds before and after the VoxelGrids (pcm_loam_submap_info)."""
        r = self._stored("_submap", "submap_info before update_submap")
        out = {"keys": np.zeros(r.num_selected, np.int32), "corner_in": np.zeros((r.num_corner_in, 4), np.float32),
               "surf_in": np.zeros((r.num_surf_in, 4), np.float32), "corner_map": np.zeros((r.num_corner_map, 4), np.float32),
               "surf_map": np.zeros((r.num_surf_map, 4), np.float32)}
        self._check(self._L.pcm_loam_submap_info(self._h, *(out[k].ctypes.data for k in ("keys", "corner_in", "surf_in", "corner_map", "surf_map"))))
        return out

    def occ_insert_keyframes(self, first: int = 0, n: int = None):
        """Key frames first .. first + n - 1 (default: all from `first`) into the context's occupancy map, read in place."""
        if n is None:
            n = self.num_keyframes - first
        self._check(self._L.pcm_occ_insert_keyframes(self._h, int(first), int(n)))


# ---------------------------------------------------------------------------------------------------------------------------
# Scan Context descriptors and loop detection; loop verification on the device (pcm_loam_loop_*, section 19)
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoamLoopResult:
    """pcm_loam_sc_detect: detectLoopClosureID's pair (loop_id, yaw_diff_rad) and what led to it; ``candidates`` = one
    (index, ring-key d2, distance, shift) per evaluated candidate (the first 64), in candidate order."""
    loop_id: int
    yaw_diff_rad: float
    min_dist: float
    nn_idx: int
    nn_align: int
    num_descriptors: int
    tree_size: int
    tree_rebuilt: bool
    num_evaluated: int
    candidates: list
    status: int


LOOP_STATUS = {capi.PCM_LOAM_LOOP_ACCEPTED: "accepted", capi.PCM_LOAM_LOOP_REJECTED_SIZE: "rejected_size",
               capi.PCM_LOAM_LOOP_REJECTED_NOT_CONVERGED: "rejected_not_converged", capi.PCM_LOAM_LOOP_REJECTED_FITNESS: "rejected_fitness",
               capi.PCM_LOAM_LOOP_NONE: "no_loop"}


@dataclasses.dataclass
class LoamLoopFactor:
    """pcm_loam_loop_verify / pcm_loam_loop_closure: performLoopClosure's outcome for one pair.  ``status`` is one of LOOP_STATUS's
    names; the factor (``between`` 4x4 float64 = poseFrom.between(poseTo), ``between6`` roll pitch yaw x y z, ``noise_variance``)
    is meaningful when ``accepted``."""
    status: str
    key_cur: int
    key_pre: int
    num_cur_points: int
    num_prev_points: int
    iterations: int
    converged: bool
    fitness: float
    noise_variance: float
    correction: np.ndarray
    pose_from: np.ndarray
    pose_to: np.ndarray
    between: np.ndarray
    between6: np.ndarray

    @property
    def accepted(self) -> bool:
        return self.status == "accepted"


def _loop_factor(r: capi.PcmLoamLoopResult) -> LoamLoopFactor:
    return LoamLoopFactor(LOOP_STATUS[r.status], r.key_cur, r.key_pre, r.num_cur_points, r.num_prev_points, r.ndt_iterations, bool(r.ndt_converged),
                          r.fitness, float(np.float32(r.noise_variance)), np.array(r.correction, np.float32).reshape(4, 4), np.array(r.pose_from),
                          np.array(r.pose_to), np.array(r.between).reshape(4, 4), np.array(r.between6))


class _LoopDetection:
    def sc_add(self, points=None, keyframe=None, near=None, **params) -> int:
        """makeAndSaveScancontextAndKeys of one cloud: ``points`` (an (N,>=3) float32 host array or a contiguous (N,C) float32 device
        tensor; VoxelGrid of ``leaf`` first), or the stored surf cloud of key frame ``keyframe``.  Returns the descriptor's index."""
        if sum(a is not None for a in (points, keyframe, near)) != 1:
            raise ValueError("pass exactly one of points, keyframe, near")
        p = fill_params(capi.PcmLoamScParams, self._L.pcm_loam_default_sc_params, params)
        r = capi.PcmLoamScAddResult()
        if near is not None:
            self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_KEYFRAME_NEAR, int(near), None, 0, 16, capi.MEM_HOST, C.byref(r)))
        elif keyframe is not None:
            self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_KEYFRAME_SURF, int(keyframe), None, 0, 16, capi.MEM_HOST, C.byref(r)))
        else:
            ptr, n, stride, mem, keep = buffer_arg(points, (3, None), convert=True)
            self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_POINTS, -1, ptr, n, stride, mem, C.byref(r)))
        self._sc_last_add = r
        return r.index

    def sc_add_near(self, key: int, search_num: int, wrt_key: int = -1, leaf: float = 0.2, **params) -> int:
        """MULTI_SCAN_FEAT: the descriptor of the near-key-frame cloud ``near_keyframes(key, search_num, wrt_key, leaf)``, built on the
        device and read in place (pcm_loam_sc_add_near); equals ``sc_add(points=that cloud, leaf=0.0)``.  Returns its index."""
        p = fill_params(capi.PcmLoamScParams, self._L.pcm_loam_default_sc_params, params)
        r = capi.PcmLoamScAddResult()
        self._check(self._L.pcm_loam_sc_add_near(self._h, C.byref(p), int(key), int(search_num), int(wrt_key), float(leaf), C.byref(r)))
        self._sc_last_add = r
        return r.index

    def sc_put(self, desc):
        """A ready (num_ring, num_sector) descriptor (e.g. of a saved map); its keys are derived on the device."""
        d = np.asarray(desc, dtype=np.float64)
        if d.ndim != 2:
            raise ValueError("expected a (num_ring, num_sector) array")
        col = np.ascontiguousarray(d.T)   # column-major, ring fastest
        self._check(self._L.pcm_loam_sc_put(self._h, col.ctypes.data, d.shape[0], d.shape[1]))

    @property
    def sc_count(self) -> int:
        n = self._L.pcm_loam_sc_count(self._h)
        if n < 0:
            self._check(n)
        return n

    def sc_get(self, i: int):
        """(descriptor (num_ring, num_sector) float64, ring key (num_ring,) float32, sector key (num_sector,) float64)."""
        R, S = C.c_int(0), C.c_int(0)
        self._check(self._L.pcm_loam_sc_shape(self._h, C.byref(R), C.byref(S)))
        col = np.zeros((max(1, S.value), max(1, R.value)))
        rk = np.zeros(max(1, R.value), np.float32)
        sk = np.zeros(max(1, S.value))
        self._check(self._L.pcm_loam_sc_get(self._h, int(i), col.ctypes.data, rk.ctypes.data, sk.ctypes.data))
        return np.ascontiguousarray(col.T), rk, sk

    def sc_clear(self):
        self._check(self._L.pcm_loam_sc_clear(self._h))

    def sc_detect(self, **params) -> LoamLoopResult:
        """detectLoopClosureID of the last descriptor (pcm_loam_sc_detect); num_candidates=0 compares against the whole search set."""
        p = fill_params(capi.PcmLoamScParams, self._L.pcm_loam_default_sc_params, params)
        r = capi.PcmLoamScResult()
        self._check(self._L.pcm_loam_sc_detect(self._h, C.byref(p), C.byref(r)))
        m = min(64, r.num_evaluated)
        cands = [(r.cand_index[t], float(np.float32(r.cand_d2[t])), r.cand_dist[t], r.cand_shift[t]) for t in range(m)]
        return LoamLoopResult(r.loop_id, r.yaw_diff_rad, r.min_dist, r.nn_idx, r.nn_align, r.num_descriptors, r.tree_size, bool(r.tree_rebuilt),
                              r.num_evaluated, cands, r.status)

    def sc_distance(self, i: int, j: int, **params):
        """distanceBtnScanContext(descriptor i, descriptor j) -> (distance, shift)."""
        p = fill_params(capi.PcmLoamScParams, self._L.pcm_loam_default_sc_params, params)
        d, s = C.c_double(0.0), C.c_int32(0)
        self._check(self._L.pcm_loam_sc_distance(self._h, C.byref(p), int(i), int(j), C.byref(d), C.byref(s)))
        return d.value, s.value

    def detect_loop_distance(self, time_cur, radius: float = 10.0, time_diff_s: float = 30.0):
        """detectLoopClosureDistance on the stored key poses: (key_cur, key_pre) or None."""
        a, b = C.c_int32(-1), C.c_int32(-1)
        rc = self._L.pcm_loam_loop_detect_distance(self._h, float(radius), float(time_diff_s), float(time_cur), C.byref(a), C.byref(b))
        if rc < 0:
            self._check(rc)
        return (a.value, b.value) if rc == 1 else None

    def loop_verify(self, key_cur: int, key_pre: int, **params) -> LoamLoopFactor:
        """performLoopClosure :645-731 for the pair (pcm_loam_loop_verify): near clouds, size gates, pclomp NDT, fitness, loop factor."""
        p = fill_params(capi.PcmLoamLoopParams, self._L.pcm_loam_default_loop_params, params)
        r = capi.PcmLoamLoopResult()
        self._check(self._L.pcm_loam_loop_verify(self._h, C.byref(p), int(key_cur), int(key_pre), C.byref(r)))
        return _loop_factor(r)

    def loop_closure(self, time_cur, radius: float = 10.0, time_diff_s: float = 30.0, **params) -> LoamLoopFactor:
        """detectLoopClosureDistance + verification in one call (pcm_loam_loop_closure); status "no_loop" without a candidate.  The
        loopIndexContainer bookkeeping stays with the caller."""
        p = fill_params(capi.PcmLoamLoopParams, self._L.pcm_loam_default_loop_params, params)
        r = capi.PcmLoamLoopResult()
        self._check(self._L.pcm_loam_loop_closure(self._h, C.byref(p), float(radius), float(time_diff_s), float(time_cur), C.byref(r)))
        return _loop_factor(r)

    @property
    def loop_verifier_exists(self) -> bool:
        n = self._L.pcm_loam_loop_verifier_exists(self._h)
        if n < 0:
            self._check(n)
        return bool(n)


@dataclasses.dataclass
class LoamScLoopFactor:
    """pcm_loam_sc_loop_verify / pcm_loam_sc_loop_closure: performSCLoopClosure's outcome for one pair.  ``status`` is one of
    LOOP_STATUS's names; the factor (``between`` = poseFrom.between(identity), ``noise_variance`` 0.5 under a Cauchy kernel of
    ``cauchy_k``) is meaningful when ``accepted``."""
    status: str
    key_cur: int
    key_pre: int
    num_cur_points: int
    num_prev_points: int
    icp_iterations: int
    icp_converged: bool
    icp_stop_reason: int
    yaw_diff_rad: float
    fitness: float
    noise_variance: float
    cauchy_k: float
    correction: np.ndarray
    pose_from: np.ndarray
    pose_to: np.ndarray
    between: np.ndarray
    between6: np.ndarray

    @property
    def accepted(self) -> bool:
        return self.status == "accepted"


def _sc_loop_factor(r: capi.PcmLoamScLoopResult) -> LoamScLoopFactor:
    return LoamScLoopFactor(LOOP_STATUS[r.status], r.key_cur, r.key_pre, r.num_cur_points, r.num_prev_points, r.icp_iterations, bool(r.icp_converged),
                            r.icp_stop_reason, float(np.float32(r.yaw_diff_rad)), r.fitness, float(np.float32(r.noise_variance)), r.cauchy_k,
                            np.array(r.correction, np.float32).reshape(4, 4), np.array(r.pose_from), np.array(r.pose_to),
                            np.array(r.between).reshape(4, 4), np.array(r.between6))


def loam_sc_loop_verify(reg, key_cur: int, key_pre: int, **params) -> LoamScLoopFactor:
    """performSCLoopClosure :750-834 for the pair (pcm_loam_sc_loop_verify): both near clouds under key frame 0, size gates,
    point-to-point ICP from the identity, fitness, loop factor."""
    p = fill_params(capi.PcmLoamScLoopParams, reg._L.pcm_loam_default_sc_loop_params, params)
    r = capi.PcmLoamScLoopResult()
    reg._check(reg._L.pcm_loam_sc_loop_verify(reg._h, C.byref(p), int(key_cur), int(key_pre), C.byref(r)))
    return _sc_loop_factor(r)


def loam_sc_loop_closure(reg, **params) -> LoamScLoopFactor:
    """Scan Context detection of the last key frame + verification in one call (pcm_loam_sc_loop_closure); status "no_loop"
    without a candidate.  The loopIndexContainer bookkeeping stays with the caller."""
    p = fill_params(capi.PcmLoamScLoopParams, reg._L.pcm_loam_default_sc_loop_params, params)
    r = capi.PcmLoamScLoopResult()
    reg._check(reg._L.pcm_loam_sc_loop_closure(reg._h, C.byref(p), C.byref(r)))
    return _sc_loop_factor(r)


def loam_sc_loop_verifier_exists(reg) -> bool:
    n = reg._L.pcm_loam_sc_loop_verifier_exists(reg._h)
    if n < 0:
        reg._check(n)
    return bool(n)


# ---------------------------------------------------------------------------------------------------------------------------
# LOAM localisation map: area tiles and the per-frame crop on the device; the key-frame map cut into
# tiles (section 31)
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoamMapLoadResult:
    num_corner_tiles: int
    num_surf_tiles: int
    num_corner_selected: int
    num_surf_selected: int
    num_corner_points: int
    num_surf_points: int
    generation: int
    changed: bool


@dataclasses.dataclass
class LoamMapCropResult:
    num_corner_in: int
    num_surf_in: int
    num_corner: int
    num_surf: int
    num_nonfinite: int
    rebuilt: bool
    x_lo: np.float32
    x_hi: np.float32
    y_lo: np.float32
    y_hi: np.float32
    status: int


@dataclasses.dataclass
class LoamTilesResult:
    num_corner_tiles: int
    num_surf_tiles: int
    corner_points_in: int
    surf_points_in: int
    corner_points_out: int
    surf_points_out: int
    num_nonfinite: int


_TILE_LIST = {0: 0, 1: 1, "corner": 0, "surf": 1}


def _crop_result(r: capi.PcmLoamDynmapCropResult) -> LoamMapCropResult:
    return LoamMapCropResult(r.num_corner_in, r.num_surf_in, r.num_corner, r.num_surf, r.num_nonfinite, bool(r.rebuilt), np.float32(r.x_lo),
                             np.float32(r.x_hi), np.float32(r.y_lo), np.float32(r.y_hi), r.status)


def loam_share_tiles(reg, other):
    """``reg`` reads the tile store ``other`` holds from now on (pcm_loam_tile_share): the tiles exist once on the device however many
    LoamRegistration objects hold them.  ``reg``'s selection starts over: ``load_map`` before its next ``crop_map``.  While a store is
    shared, ``add_tile`` and ``build_tiles`` on any holder raise PcmError (UNSUPPORTED); ``clear_tiles`` detaches that object alone."""
    reg._check(reg._L.pcm_loam_tile_share(reg.handle, other.handle))
    reg._dm_load = reg._dm_crop = None
    reg._tile_size = getattr(other, "_tile_size", None)


def loam_tile_share_count(reg) -> int:
    """LoamRegistration objects holding ``reg``'s tile store (1 = not shared) (pcm_loam_tile_share_count)."""
    n = reg._L.pcm_loam_tile_share_count(reg.handle)
    if n < 0:
        reg._check(n)
    return n


def loam_crop_map_batch(regs, poses6, **params):
    """crop_map of several LoamRegistration objects in one round of launches (pcm_loam_dynmap_crop_batch): object i is cropped at
    poses6[i]; its target and its LoamMapCropResult are those of a single ``crop_map``, bit for bit.  The objects may share one tile
    store (``loam_share_tiles``) or hold their own.  An object that cannot be cropped carries its code in ``status`` while the others
    complete; PcmError when the call as a whole fails."""
    L = capi.load_library()
    n = len(regs)
    p = fill_params(capi.PcmLoamDynmapParams, L.pcm_loam_default_dynmap_params, params)
    x = np.ascontiguousarray(poses6, dtype=np.float32).reshape(n, 6)
    arr = (C.c_void_p * n)(*[r.handle for r in regs])
    out = (capi.PcmLoamDynmapCropResult * n)()
    rc = L.pcm_loam_dynmap_crop_batch(arr, n, C.byref(p), x.ctypes.data, out)
    if rc != capi.PCM_OK and all(out[i].status == capi.PCM_OK for i in range(n)):
        raise capi.PcmError(rc, (L.pcm_last_error(regs[0].handle) or b"").decode())
    for i, reg in enumerate(regs):
        if out[i].status == capi.PCM_OK:
            reg._dm_crop = capi.PcmLoamDynmapCropResult.from_buffer_copy(out[i])
    return [_crop_result(out[i]) for i in range(n)]


def write_arealist(path, areas):
    """dynamic_map.h:90-106: one line per area, ``path,x_min,y_min,z_min,x_max,y_max,z_max``, the numbers as std::to_string writes
    doubles (``%f``: 6 decimals).  areas: (path, (6 numbers)) pairs."""
    with open(path, "w") as f:
        for name, box in areas:
            f.write(",".join([str(name)] + ["%f" % float(v) for v in box]) + "\n")


def read_arealist(path):
    """dynamic_map.h:37-88: lines split at commas, column 0 the PCD path, columns 1..6 through std::stod.  Returns a list of
    (path, float64 array of 6) pairs in file order."""
    areas = []
    with open(path) as f:
        for line in f.read().split("\n"):
            if line == "":
                continue
            cols = line.split(",")
            areas.append((cols[0], np.array([float(c) for c in cols[1:7]], np.float64)))
    return areas


class _LocalisationTiles:
    def add_tile(self, which, box, points) -> int:
        """One area tile of the corner (0, "corner") or surf (1, "surf") list: box = (x_min, y_min, z_min, x_max, y_max, z_max) as in the
        CSV area list, points an (N,>=3) array of x y z [intensity] in the map frame (N may be 0).  Returns the tile's index."""
        b = np.ascontiguousarray(box, dtype=np.float64).reshape(6)
        a = np.asarray(points, np.float32)
        pts = _xyzi(a.reshape(0, 4) if a.size == 0 else a)
        idx = self._L.pcm_loam_tile_add(self._h, _TILE_LIST[which], b.ctypes.data, pts.ctypes.data, pts.shape[0], 16, capi.MEM_HOST)
        if idx < 0:
            self._check(idx)
        self._tile_size = None   # the list now holds a tile that build_tiles did not name
        return idx

    def num_tiles(self, which) -> int:
        n = self._L.pcm_loam_tile_count(self._h, _TILE_LIST[which])
        if n < 0:
            self._check(n)
        return n

    def clear_tiles(self):
        self._check(self._L.pcm_loam_tile_clear(self._h))
        self._dm_load = self._dm_crop = None
        self._tile_size = None

    def _build_tiles(self, first, n, params, ms=None):
        if n is None:
            n = self.num_keyframes - first
        p = fill_params(capi.PcmLoamTilesParams, self._L.pcm_loam_default_tiles_params, params)
        r = capi.PcmLoamTilesResult()
        if ms is None:
            self._check(self._L.pcm_loam_tiles_build(self._h, C.byref(p), int(first), int(n), C.byref(r)))
        else:
            self._check(self._L.pcm_loam_tiles_build_ms(self._h, C.byref(p), int(first), int(n), C.byref(r), ms.ctypes.data))
        self._dm_load = self._dm_crop = None
        self._tile_size = float(p.tile_size)
        return r

    def build_tiles(self, first: int = 0, n: int = None, **params) -> LoamTilesResult:
        """pcm_loam_tiles_build: replaces both tile lists with the tiles of key frames first .. first + n - 1 (default: all from
        ``first``) under their current poses (tile_size, leaf_corner, leaf_surf); the map does not leave the device.  ``load_map`` /
        ``crop_map`` then run on them as on tiles from ``add_tile``."""
        r = self._build_tiles(first, n, params)
        return LoamTilesResult(r.num_corner_tiles, r.num_surf_tiles, int(r.corner_points_in), int(r.surf_points_in), int(r.corner_points_out),
                               int(r.surf_points_out), int(r.num_nonfinite))

    def build_tiles_ms(self, first: int = 0, n: int = None, **params) -> dict:
        """Measurement hook (pcm_loam_tiles_build_ms): build_tiles with device events at its stage boundaries.  Returns the stage
        times in ms: {"corner": {stage: ms}, "surf": {stage: ms}, "gather": ms, "arena_copy": ms}; ``workspace_host`` is host time."""
        S = capi.PCM_LOAM_TILES_STAGES
        ms = np.zeros(2 * S + 2, np.float32)
        self._build_tiles(first, n, params, ms)
        out = {name: {k: float(v) for k, v in zip(capi.TILES_STAGE_NAMES, ms[m * S:(m + 1) * S])} for m, name in enumerate(("corner", "surf"))}
        out["gather"], out["arena_copy"] = float(ms[2 * S]), float(ms[2 * S + 1])
        return out

    def tile_info(self, which, i: int) -> dict:
        """Tile ``i`` of a list, from ``add_tile`` or ``build_tiles``: box (x_min, y_min, z_min, x_max, y_max, z_max) float64, ixy (the
        index pair; (0, 0) for a tile added by hand) and its number of points (pcm_loam_tile_info)."""
        box = np.zeros(6, np.float64)
        ixy = np.zeros(2, np.int32)
        n = C.c_size_t(0)
        self._check(self._L.pcm_loam_tile_info(self._h, _TILE_LIST[which], int(i), box.ctypes.data, ixy.ctypes.data, C.byref(n)))
        return {"box": box, "ixy": (int(ixy[0]), int(ixy[1])), "n": int(n.value)}

    def get_tile(self, which, i: int, out=None):
        """The (n, 4) x y z intensity points of tile ``i`` (pcm_loam_tile_get).  Without ``out``: a host array.  With a contiguous
        (cap, 4) float32 device tensor or host array: written there, returns n."""
        return self._counted(lambda p, cap, mem, n: self._L.pcm_loam_tile_get(self._h, _TILE_LIST[which], int(i), p, cap, mem, C.byref(n)), out, cols=(4, 4))

    def tiles_arealist(self, which, prefix: str = ""):
        """The rows ``write_arealist`` takes for the tiles ``build_tiles`` left in a list: (path, box) with path
        ``f"{prefix}{tile_size:g}_{ix}_{iy}.pcd"``.  There is no PCD writer here: the caller writes ``get_tile(which, i)`` to each path."""
        ts = getattr(self, "_tile_size", None)
        if ts is None:
            raise capi.PcmError(-2, "tiles_arealist needs the lists as build_tiles left them (no build yet, or add_tile / clear_tiles since)")
        rows = []
        for i in range(self.num_tiles(which)):
            t = self.tile_info(which, i)
            rows.append(("%s%g_%d_%d.pcd" % (prefix, ts, t["ixy"][0], t["ixy"][1]), t["box"]))
        return rows

    def need_map_load(self, pose6, **params) -> bool:
        """dynamic_load_map_run's trigger: has the pose moved farther than area_size from the last load_map (pcm_loam_dynmap_need_load)."""
        p = fill_params(capi.PcmLoamDynmapParams, self._L.pcm_loam_default_dynmap_params, params)
        x = _pose6(pose6)
        rc = self._L.pcm_loam_dynmap_need_load(self._h, C.byref(p), x.ctypes.data)
        if rc < 0:
            self._check(rc)
        return bool(rc)

    def load_map(self, pose6, **params) -> LoamMapLoadResult:
        """create_pcd for both lists: selects the tiles around pose6 (margin) and records the pose; no points move (pcm_loam_dynmap_load)."""
        p = fill_params(capi.PcmLoamDynmapParams, self._L.pcm_loam_default_dynmap_params, params)
        x = _pose6(pose6)
        r = capi.PcmLoamDynmapLoadResult()
        self._check(self._L.pcm_loam_dynmap_load(self._h, C.byref(p), x.ctypes.data, C.byref(r)))
        self._dm_load = r
        return LoamMapLoadResult(r.num_corner_tiles, r.num_surf_tiles, r.num_corner_selected, r.num_surf_selected, r.num_corner_points,
                                 r.num_surf_points, r.generation, bool(r.changed))

    def crop_map(self, pose6, **params) -> LoamMapCropResult:
        """dynamic_load_map(pose6): the selected tiles through the frame's window become this context's target (pcm_loam_dynmap_crop)."""
        p = fill_params(capi.PcmLoamDynmapParams, self._L.pcm_loam_default_dynmap_params, params)
        x = _pose6(pose6)
        r = capi.PcmLoamDynmapCropResult()
        self._check(self._L.pcm_loam_dynmap_crop(self._h, C.byref(p), x.ctypes.data, C.byref(r)))
        self._dm_crop = r
        return _crop_result(r)

    def dynmap_info(self) -> dict:
        """Parity hook: the selected tile indices of both lists and, after crop_map, the two cropped clouds (pcm_loam_dynmap_info)."""
        ld, cr = self._stored("_dm_load", "dynmap_info before load_map"), getattr(self, "_dm_crop", None)
        out = {"corner_tiles": np.zeros(ld.num_corner_selected, np.int32), "surf_tiles": np.zeros(ld.num_surf_selected, np.int32)}
        ptrs = [out["corner_tiles"].ctypes.data, out["surf_tiles"].ctypes.data, None, None]
        if cr is not None:
            out["corner"] = np.zeros((cr.num_corner, 4), np.float32)
            out["surf"] = np.zeros((cr.num_surf, 4), np.float32)
            ptrs[2:] = [out["corner"].ctypes.data, out["surf"].ctypes.data]
        self._check(self._L.pcm_loam_dynmap_info(self._h, *ptrs))
        return out

    def global_map(self, out=None):
        """globalMap = cropped corner ++ cropped surf as (M,4) x y z intensity.  Without ``out``: a host array.  With a contiguous (cap,4)
        float32 CUDA tensor: written there without leaving the device, returns the number of points M (the NDT branch then passes
        ``out[:M]`` to ``PclNdtRegistration.set_input_target``)."""
        n = C.c_size_t(0)
        if out is not None:
            ptr, cap, _, mem, _ = buffer_arg(out, (4, 4), write=True)
            if mem != capi.MEM_DEVICE:
                raise ValueError("expected a contiguous (cap,4) float32 CUDA tensor")
            self._check(self._L.pcm_loam_dynmap_global(self._h, ptr, cap, C.byref(n), mem))
            return n.value
        cr = self._stored("_dm_crop", "global_map before crop_map")
        a = np.zeros((cr.num_corner + cr.num_surf, 4), np.float32)
        self._check(self._L.pcm_loam_dynmap_global(self._h, a.ctypes.data, a.shape[0], C.byref(n), capi.MEM_HOST))
        return a[:n.value]


# ---------------------------------------------------------------------------------------------------------------------------
# LOAM global map and saved map from the key frames on the device
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoamGlobalMapResult:
    num_near: int
    num_pose_leaves: int
    num_skipped: int
    num_used: int
    points_in: int
    points_out: int


_EXPORT_WHICH = {0: 0, 1: 1, 2: 2, "corner": 0, "surf": 1, "both": 2}


class _GlobalMap:
    def keyframe_global_keys(self, **params) -> np.ndarray:
        """publishGlobalMap's selection (pcm_loam_global_keys): the key frame of every used pose leaf, in list order.  ``leaf`` plays
        no part in it."""
        p = fill_params(capi.PcmLoamGlobalParams, self._L.pcm_loam_default_global_params, params)
        keys = np.zeros(max(1, self.num_keyframes), np.int32)
        n = C.c_size_t(0)
        self._check(self._L.pcm_loam_global_keys(self._h, C.byref(p), keys.ctypes.data, keys.size, C.byref(n)))
        return keys[:n.value].copy()

    def keyframe_global_map(self, out=None, **params):
        """publishGlobalMap (pcm_loam_global_map; search_radius, keypose_density, leaf).  Without ``out``: the (n, 4) x y z intensity
        cells on the host.  With a contiguous (cap, 4) float32 device tensor or host array: written there, returns the number of
        rows.  ``keyframe_global_result`` holds the counts of the last call."""
        p = fill_params(capi.PcmLoamGlobalParams, self._L.pcm_loam_default_global_params, params)
        q = capi.PcmLoamGlobalParams(p.search_radius, p.keypose_density, 0.0)   # without a leaf and a buffer: the host-only query of points_in
        r = capi.PcmLoamGlobalResult()
        self._global_result = r

        def call(ptr, cap, mem, n):
            rc = self._L.pcm_loam_global_map(self._h, C.byref(q if ptr is None else p), ptr, cap, mem, C.byref(r))
            n.value = int(r.points_in if ptr is None else r.points_out)
            return rc

        return self._counted(call, out, cols=(4, 4))

    @property
    def keyframe_global_result(self) -> LoamGlobalMapResult:
        r = self._stored("_global_result", "keyframe_global_result before keyframe_global_map")
        return LoamGlobalMapResult(r.num_near, r.num_pose_leaves, r.num_skipped, r.num_used, int(r.points_in), int(r.points_out))

    def export_map(self, which="both", first: int = 0, n: int = None, out=None):
        """The saved map (pcm_loam_map_export) of key frames first .. first + n - 1 (default: all from ``first``): "corner" = their
        corner clouds under their poses, "surf" = their surf clouds, "both" = all corner clouds, then all surf clouds (jueying.pcd when
        the range is the whole store); no VoxelGrid.  Without ``out``: an (N, 4) host array.  With a (cap, 4) float32 device tensor or
        host array: written there (a device tensor without a wait), returns N."""
        if n is None:
            n = self.num_keyframes - first
        w = _EXPORT_WHICH[which]
        return self._counted(lambda p, cap, mem, cnt: self._L.pcm_loam_map_export(self._h, w, int(first), int(n), p, cap, mem, C.byref(cnt)), out,
                             cols=(4, 4), store="_export_count")


class LoamRegistration(Context, _ScanToMap, _FrontEnd, _KeyFrames, _LoopDetection, _LocalisationTiles, _GlobalMap, _OccMixin, _ScanMixin,
                       _VoxelLargeMixin):
    """jueying_slam's LOAM edge / plane scan-to-map optimisation on one HIP device (a PCM_MODEL_LOAM ``pcm_ctx``).

    ``set_input_target(corner_map, surf_map)`` = laserCloudCornerFromMapDS / laserCloudSurfFromMapDS,
    ``set_input_source(corner, surf)`` = laserCloudCornerLastDS / laserCloudSurfLastDS (body frame),
    ``scan2map(x6)`` = scan2MapOptimization from transformTobeMapped = x6 (roll, pitch, yaw, x, y, z)."""

    def __init__(self, device: int = 0, **params):
        super().__init__(device, default_config("LOAM"))
        self.params = dict(params)
        fill_params(capi.PcmLoamParams, self._L.pcm_loam_default_params, self.params)   # unknown names fail here
        self.n_corner = self.n_surf = 0
