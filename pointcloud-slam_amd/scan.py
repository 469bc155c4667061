"""Scan pre-processing every context offers: scan fusion and the ring converters (fusion_lidar_camera / rs_to_velodyne /
hesai_to_velodyne), the PointCloud2 handlers of jueying_lio's PointCloudPreprocess (section 16) and
pcl::VoxelGridLarge (section 22)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from ._binding import buffer_arg, fill_params

FUSED_STRIDE, FUSED_INTENSITY, FUSED_RING, FUSED_TIME = 32, 16, 20, 24   # the output records (VelodynePointXYZIRT)
_SCAN_LAYOUT = {"XYZI": capi.PCM_SCAN_OUT_XYZI, "XYZIR": capi.PCM_SCAN_OUT_XYZIR, "XYZIRT": capi.PCM_SCAN_OUT_XYZIRT, 0: 0, 1: 1, 2: 2}
_SCAN_ITYPE = {"f32": capi.PCM_SCAN_INTENSITY_FLOAT, "u8": capi.PCM_SCAN_INTENSITY_UINT8}
_SCAN_RULE = {"height": capi.PCM_SCAN_RING_BY_HEIGHT, "div_width": capi.PCM_SCAN_RING_DIV_WIDTH, "mod_height": capi.PCM_SCAN_RING_MOD_HEIGHT}


@dataclasses.dataclass
class ScanSegment:
    """One input of fuse_scans.  points: a host array or a device tensor of n x stride bytes."""
    kind: int
    points: object
    stride: int
    intensity_offset: int = 16
    ring_offset: int = 0
    timestamp_offset: int = 0
    intensity_type: str = "f32"
    ring_rule: str = "height"
    width: int = 0
    height: int = 0
    ring_table: object = None
    T: object = None
    dt_sec: int = 0
    dt_nsec: int = 0


def lidar_xyzirt_segment(points, stride=32, intensity_offset=16, ring_offset=20, timestamp_offset=24, intensity_type="f32") -> ScanSegment:
    """Vendor XYZIRT records (default layout: rs_to_velodyne.cpp's RsPointXYZIRT)."""
    return ScanSegment(capi.PCM_SCAN_LIDAR_XYZIRT, points, stride, intensity_offset, ring_offset, timestamp_offset, intensity_type)


def lidar_xyzi_segment(points, width, height, ring_table, stride=32, intensity_offset=16, intensity_type="f32", ring_rule="height") -> ScanSegment:
    """An organised pcl::PointXYZI cloud; ring_table is the node's own row -> ring array."""
    return ScanSegment(capi.PCM_SCAN_LIDAR_XYZI, points, stride, intensity_offset, intensity_type=intensity_type, ring_rule=ring_rule, width=width,
                       height=height, ring_table=ring_table)


def depth_segment(points, T, dt_sec=0, dt_nsec=0, stride=32) -> ScanSegment:
    """A depth-camera cloud (pcl::PointXYZRGB records); T: the node's camera_T entry, 16 doubles."""
    return ScanSegment(capi.PCM_SCAN_DEPTH, points, stride, T=T, dt_sec=dt_sec, dt_nsec=dt_nsec)


def scan_segments(segments):
    """(ctypes array of pcm_scan_segment, objects to keep alive while it is in use)."""
    arr = (capi.PcmScanSegment * max(len(segments), 1))()
    keep = []
    for k, s in enumerate(segments):
        ptr, n, _, mem, ka = buffer_arg(s.points, record=s.stride, f32=False, convert=True, what="scan:")
        keep.append(ka)
        g = arr[k]
        g.kind, g.memory, g.points, g.n, g.stride_bytes = s.kind, mem, ptr if n else None, n, s.stride
        g.intensity_offset_bytes, g.ring_offset_bytes, g.timestamp_offset_bytes = s.intensity_offset, s.ring_offset, s.timestamp_offset
        g.intensity_type, g.ring_rule, g.width, g.height = _SCAN_ITYPE[s.intensity_type], _SCAN_RULE[s.ring_rule], int(s.width), int(s.height)
        if s.ring_table is not None:
            t = np.ascontiguousarray(s.ring_table, np.int32)
            keep.append(t)
            g.ring_table, g.ring_table_len = t.ctypes.data, t.size
        g.dt_sec, g.dt_nsec = int(s.dt_sec), int(s.dt_nsec)
        if s.T is not None:
            g.T[:] = [float(v) for v in np.asarray(s.T, np.float64).reshape(16)]
    return arr, keep


def scan_fuse_params(defaults, params: dict):
    """pcm_scan_fuse_params from the defaults `defaults(p)` fills and keyword overrides (pitch_ring_table: an int array; layout)."""
    keep = []

    def key(p, k, v):
        if k == "pitch_ring_table":
            if v is not None:
                t = np.ascontiguousarray(v, np.int32)
                keep.append(t)
                p.pitch_ring_table, p.pitch_ring_table_len = t.ctypes.data, t.size
        elif k in ("layout", "output_layout"):
            p.output_layout = _SCAN_LAYOUT[v]
        else:
            return False
        return True

    return fill_params(capi.PcmScanFuseParams, defaults, params or {}, key), keep


def scan_result(r: capi.PcmScanFuseResult, n_segs: int) -> dict:
    d = {k: [getattr(r.seg[s], k) for s in range(n_segs)] for k in ("n_in", "n_nan", "n_depth_filtered", "n_kept", "out_offset")}
    d.update(n_out=r.n_out, n_pitch_index_clamped=r.n_pitch_index_clamped, status=r.status)
    return d


# ---- PointCloud2 handlers of jueying_lio's PointCloudPreprocess (pcm_lidar_filter) -----------------------------
LIDAR_TYPE = {"velodyne": capi.PCM_LIDAR_VELODYNE, "ouster": capi.PCM_LIDAR_OUSTER, "rslidar": capi.PCM_LIDAR_RSLIDAR, "livox": capi.PCM_LIDAR_LIVOX_STD}
LIDAR_TIME_KIND = {"f32": capi.PCM_LIDAR_TIME_FLOAT, "f64": capi.PCM_LIDAR_TIME_DOUBLE, "u32": capi.PCM_LIDAR_TIME_UINT32}
LIDAR_RING_KIND = {"u8": capi.PCM_LIDAR_RING_UINT8, "u16": capi.PCM_LIDAR_RING_UINT16}
NORMAL_STRIDE = 48   # pcl::PointXYZINormal


def _lidar_desc_key(d, k, v):
    table = {"time_kind": LIDAR_TIME_KIND, "ring_kind": LIDAR_RING_KIND}.get(k)
    if table is None or not isinstance(v, str):
        return False
    setattr(d, k, table[v])
    return True


def lidar_desc(type, **overrides) -> capi.PcmLidarDesc:
    """The reference's PCL struct layout and config values of a LiDAR type ("velodyne" | "ouster" | "rslidar" | "livox", or the
    reference's LidarType number), with any field of pcm_lidar_desc overridden (time_kind / ring_kind also by name: "f32" "f64" "u32",
    "u8" "u16")."""
    kind = LIDAR_TYPE.get(type, type) if isinstance(type, str) else int(type)
    default = capi.load_library().pcm_lidar_default_desc
    return fill_params(capi.PcmLidarDesc, lambda d: default(kind, d), overrides, _lidar_desc_key)


class _ScanMixin:
    """pcm_scan_* and pcm_lidar_filter of the context ``self._h``."""

    def fuse_scans(self, segments, params=None, out=None):
        """pcm_scan_fuse.  out None: the records stay on the device in the context's buffer -> (None, counts); out "host": -> ((n_out, 32)
        uint8 array, counts); out a device tensor or a host array of capacity x 32 bytes: filled -> (out, counts)."""
        arr, keep = scan_segments(segments)
        p, keep_p = scan_fuse_params(self._L.pcm_scan_default_fuse_params, params)
        r = capi.PcmScanFuseResult()
        ptr, cap, mem, ret = None, 0, capi.MEM_HOST, None
        if isinstance(out, str) and out == "host":
            ret = np.zeros((max(sum(a.n for a in arr[:len(segments)]), 1), FUSED_STRIDE), np.uint8)
            ptr, cap = ret.ctypes.data, ret.shape[0]
        elif out is not None:
            ptr, cap, _, mem, ret = buffer_arg(out, record=FUSED_STRIDE, f32=False, write=True, what="out:")
        rc = self._L.pcm_scan_fuse(self._h, arr, len(segments), C.byref(p), ptr, cap, mem, C.byref(r))
        counts = scan_result(r, len(segments))
        del keep, keep_p
        if rc != capi.PCM_OK:
            e = capi.PcmError(rc, (self._L.pcm_last_error(self._h) or b"").decode())
            e.counts = counts
            raise e
        if isinstance(out, str):
            ret = ret[:r.n_out]
        return ret, counts

    def fused_scan(self):
        """(device pointer, n) of the records the last fuse_scans(out=None) left in the context."""
        ptr, n = C.c_void_p(), C.c_size_t()
        self._check(self._L.pcm_scan_fused(self._h, C.byref(ptr), C.byref(n)))
        return ptr.value or 0, n.value

    def lidar_filter(self, points, desc, out=None):
        """The handler of desc.type on n records of desc.stride_bytes (a host array or a device tensor): -> ((m, 12) float32
        pcl::PointXYZINormal records in input order, given_offset_time).  out: a device tensor of at least n x 48 bytes to fill instead
        (-> (m, given_offset_time))."""
        ptr, n, _, mem, keep = buffer_arg(points, record=desc.stride_bytes, f32=False, convert=True, what="points:")
        m, given = C.c_size_t(), C.c_int()
        if out is None:
            ret = np.zeros((max(n, 1), 12), np.float32)
            rc = self._L.pcm_lidar_filter(self._h, ptr, n, mem, C.byref(desc), ret.ctypes.data, n, capi.MEM_HOST, C.byref(m), C.byref(given))
        else:
            optr, cap, _, omem, _ = buffer_arg(out, record=NORMAL_STRIDE, f32=False, write=True, what="out:")
            rc = self._L.pcm_lidar_filter(self._h, ptr, n, mem, C.byref(desc), optr, cap, omem, C.byref(m), C.byref(given))
        del keep
        self._check(rc)
        return (ret[:m.value].copy() if out is None else m.value), bool(given.value)


def rs_to_velodyne(reg, points, output_type="XYZIRT", organised=None, **layout):
    """rs_to_velodyne.cpp: rsHandler_XYZIRT (vendor XYZIRT records; `layout`: lidar_xyzirt_segment's offsets) or, with
    organised = (width, height, ring_table), rsHandler_XYZI.  -> ((n, 32) uint8 records, counts)."""
    if organised is not None:
        w, h, table = organised
        seg = lidar_xyzi_segment(points, w, h, table, **layout)
        output_type = "XYZIR" if output_type == "XYZIRT" else output_type   # rsHandler_XYZI publishes VelodynePointXYZIR
    else:
        seg = lidar_xyzirt_segment(points, **layout)
    return reg.fuse_scans([seg], {"layout": output_type}, out="host")


def hesai_to_velodyne(reg, points, output_type="XYZIRT", organised=None, **layout):
    """hesai_to_velodyne.cpp: the same loops over HesaiPointXYZIRT (48 bytes: uint8 intensity @16, double timestamp @24, uint16 ring @32)."""
    if organised is None:
        layout = {**dict(stride=48, intensity_offset=16, ring_offset=32, timestamp_offset=24, intensity_type="u8"), **layout}
    return rs_to_velodyne(reg, points, output_type, organised, **layout)


def fuse_lidar_cameras(reg, lidar: ScanSegment, cameras, out=None, **params):
    """fusion_lidar_camera.cpp's callback: the LiDAR segment, then one depth segment per (points, T, dt_sec, dt_nsec) of `cameras`."""
    return reg.fuse_scans([lidar] + [depth_segment(*c) for c in cameras], params, out=out)


# ---- pcl::VoxelGridLarge on the device ---------------------------------------------------------------------------
@dataclasses.dataclass
class VoxelLargeResult:
    cells: int
    finite_points: int
    pieces: int
    depth: int
    levels: int
    host_waits: int
    workspace_bytes: int


def _voxel_large(r: capi.PcmVoxelLargeResult) -> VoxelLargeResult:
    return VoxelLargeResult(int(r.cells), int(r.finite_points), int(r.pieces), int(r.depth), int(r.levels), int(r.host_waits), int(r.workspace_bytes))


class _VoxelLargeMixin:
    """pcm_voxel_downsample_large of the context ``self._h``."""

    def voxel_downsample_large(self, points, leaf_size, out=None, rows=None):
        """pcl::VoxelGridLarge (pcm_voxel_downsample_large): the VoxelGrid of ``voxel_downsample`` for clouds whose leaf index
        overflows -- the cloud is cut along its longest axis until every piece fits, the pieces' cells follow one another in
        depth-first order.  points: (N, 3..16) float32 host array or device tensor (``rows``: only its first rows).  Without ``out``
        a host cloud returns (cells, VoxelLargeResult); with ``out`` (same memory and record width as the points) the cells are
        written there and (count, VoxelLargeResult) returns.  On an error ``voxel_large_result`` still holds the counts."""
        ptr, n, stride, mem, points = buffer_arg(points, (3, 16), convert=True, what="points:")
        if rows is not None:
            if not 0 <= int(rows) <= n:
                raise ValueError("rows exceeds the cloud")
            n = int(rows)
        r = capi.PcmVoxelLargeResult()
        self._voxel_large_result = r
        if out is not None:
            optr, cap, ostride, omem, _ = buffer_arg(out, (3, 16), write=True, what="out:")
            if ostride != stride or omem != mem:
                raise ValueError("out must have the record width and the memory of the points")
            self._check(self._L.pcm_voxel_downsample_large(self._h, ptr, n, stride, mem, float(leaf_size), optr, cap, C.byref(r)))
            return int(r.cells), _voxel_large(r)
        if mem != capi.MEM_HOST:
            raise ValueError("a device cloud needs a device tensor for the cells (out=)")
        a = np.zeros((n, points.shape[1]), np.float32)
        self._check(self._L.pcm_voxel_downsample_large(self._h, ptr, n, stride, mem, float(leaf_size), a.ctypes.data, a.shape[0], C.byref(r)))
        return a[:int(r.cells)].copy(), _voxel_large(r)

    @property
    def voxel_large_result(self) -> VoxelLargeResult:
        return _voxel_large(self._stored("_voxel_large_result", "voxel_large_result before voxel_downsample_large"))
