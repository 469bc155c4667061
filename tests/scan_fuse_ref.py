"""numpy restatement of jueying_slam's scan producers in front of imageProjection, written from the reference's lines and
independent of pointcloud-slam_amd/csrc/scan_fuse.h:

  src/tool/integrate_points/src/fusion_lidar_camera.cpp   handle_pc_msg (:112-133), the XYZI branch of callback (:296-318),
                                                          convert_depth (:188-261), fusion_data (:136-155: a plain append)
  src/tool/rs_to_velodyne/src/rs_to_velodyne.cpp          rsHandler_XYZI (:81-105), handle_pc_msg + add_ring + add_time (:107-145)
  src/tool/hesai_to_velodyne/src/hesai_to_velodyne.cpp    the same loops over HesaiPointXYZIRT

float32 / float64 casts sit exactly where the C++ has them; `sqrt` of the float sum is the float overload (C++ <math.h>), asin is
np.arcsin in double, round is C's round (half away from zero).  Where the reference reads past its 52-entry pitch table
(int(round(pitch + 40)) == 52 for 11.5 <= pitch < 12) the point gets the "otherwise" ring and is counted.  Output records are 32
bytes: x y z 1.0f, float intensity @16, uint16 ring @20, float time @24, every other byte zero."""
import dataclasses

import numpy as np

F, D = np.float32, np.float64
OUT_XYZI, OUT_XYZIR, OUT_XYZIRT = 0, 1, 2


@dataclasses.dataclass
class Params:
    depth_filter: float = 1.8              # config/fusion_param.yaml
    pitch_scale: float = 28.6478897565     # :233
    pitch_min: float = -40.0               # :236
    pitch_max: float = 12.0
    pitch_offset: float = 40.0             # :237
    pitch_table: object = None             # the node's RING_MAP_16 (the caller's)
    ring_below: int = 47                   # :245
    ring_otherwise: int = 51               # :253
    depth_intensity: float = 100.0         # :229
    layout: int = OUT_XYZIRT


@dataclasses.dataclass
class LidarXYZIRT:
    rec: np.ndarray            # (n, stride) uint8 vendor records, x y z floats first
    ioff: int
    roff: int
    toff: int
    itype: str = "f32"         # "f32" (the converters' RsPointXYZIRT) or "u8" (the fusion node's, Hesai's)


@dataclasses.dataclass
class LidarXYZI:
    rec: np.ndarray            # (n, stride) uint8, pcl::PointXYZI: intensity float @16
    width: int
    height: int
    table: object
    ioff: int = 16
    itype: str = "f32"


@dataclasses.dataclass
class Depth:
    rec: np.ndarray            # (n, stride) uint8, pcl::PointXYZRGB: x y z floats first
    T: object                  # camera_T[camera], 16 doubles
    dt_sec: int = 0
    dt_nsec: int = 0


def field(rec, off, dtype):
    n = rec.shape[0]
    size = np.dtype(dtype).itemsize
    return np.ascontiguousarray(rec[:, off:off + size]).view(dtype).reshape(n)


def c_round(v):
    """round() of <math.h>: to nearest, halves away from zero."""
    v = np.asarray(v, D)
    t = np.trunc(v)
    return t + np.where(np.abs(v - t) >= 0.5, np.sign(v), 0.0)


def u16(table):
    return (np.asarray(table, np.int64) & 0xFFFF).astype(np.uint16)


def xyz_of(rec):
    return field(rec, 0, F), field(rec, 4, F), field(rec, 8, F)


def intensity_of(rec, off, itype):
    return field(rec, off, F) if itype == "f32" else field(rec, off, np.uint8).astype(F)


def pitch_of(ox, oy, oz, scale):
    """:232-233 on the float members of new_point."""
    s = (ox * ox + oy * oy) + oz * oz                 # float32 products and sums
    dist = np.sqrt(s).astype(D)                       # sqrt(float) -> float, widened by `double dist =`
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.arcsin(oz.astype(D) / dist) * D(scale)


def convert_depth(seg, P):
    """(x, y, z, intensity, ring, time) of the kept points, the two drop counts, the clamp count and the pitches."""
    x, y, z = xyz_of(seg.rec)
    nan = np.isnan(x) | np.isnan(y) | np.isnan(z)
    with np.errstate(invalid="ignore"):
        far = ~nan & ((z.astype(D) > D(P.depth_filter)) & (D(P.depth_filter) >= 0))          # :218
    keep = ~nan & ~far
    X, Y, Z = x[keep].astype(D), y[keep].astype(D), z[keep].astype(D)                          # :221
    T = np.asarray(seg.T, D).reshape(16)
    with np.errstate(invalid="ignore", over="ignore"):                                         # an Inf coordinate: Inf * 0
        ox = (X * T[0] + Y * T[4] + Z * T[8] + T[12]).astype(F)                                # :226-228
        oy = (X * T[1] + Y * T[5] + Z * T[9] + T[13]).astype(F)
        oz = (X * T[2] + Y * T[6] + Z * T[10] + T[14]).astype(F)
    pitch = pitch_of(ox, oy, oz, P.pitch_scale)
    table = u16(P.pitch_table)
    ring = np.full(pitch.shape, P.ring_otherwise, np.int64)                                    # :252-253 (NaN lands here)
    with np.errstate(invalid="ignore"):
        mid = (pitch >= P.pitch_min) & (pitch < P.pitch_max)                                   # :236
        low = ~mid & (pitch < P.pitch_min)                                                     # :244
    idx = c_round(pitch[mid] + D(P.pitch_offset)).astype(np.int64)                             # :237
    inside = (idx >= 0) & (idx < table.size)
    r_mid = np.full(idx.shape, P.ring_otherwise, np.int64)
    r_mid[inside] = table[idx[inside]]
    ring[mid] = r_mid
    ring[low] = P.ring_below
    time = F(seg.dt_sec * 1.0 + seg.dt_nsec / 1000000000.0)                                    # :258
    n = ox.shape[0]
    return (ox, oy, oz, np.full(n, P.depth_intensity, F), ring.astype(np.uint16), np.full(n, time, F),
            int(nan.sum()), int(far.sum()), int((~inside).sum()), pitch)


def convert_xyzirt(seg):
    x, y, z = xyz_of(seg.rec)
    nan = np.isnan(x) | np.isnan(y) | np.isnan(z)
    keep = ~nan
    ts = field(seg.rec, seg.toff, D)
    time = (ts[keep] - ts[0]).astype(F) if ts.size else np.zeros(0, F)                         # :130 / add_time
    return (x[keep], y[keep], z[keep], intensity_of(seg.rec, seg.ioff, seg.itype)[keep], field(seg.rec, seg.roff, np.uint16)[keep], time,
            int(nan.sum()))


def convert_xyzi(seg):
    x, y, z = xyz_of(seg.rec)
    nan = np.isnan(x) | np.isnan(y) | np.isnan(z)
    keep = ~nan
    ids = np.arange(x.shape[0], dtype=np.int64)
    if seg.height == 16:
        k = ids // seg.width                                                                   # :311-312
    elif seg.height == 128:
        k = ids % seg.height                                                                   # :313-314
    else:
        raise ValueError("the reference leaves `ring` unset for height %d" % seg.height)
    ring = u16(seg.table)[k[keep]]
    n = int(keep.sum())
    return x[keep], y[keep], z[keep], intensity_of(seg.rec, seg.ioff, seg.itype)[keep], ring, np.zeros(n, F), int(nan.sum())


def records(x, y, z, intensity, ring, time, layout):
    n = x.shape[0]
    out = np.zeros((n, 32), np.uint8)
    f = out.view(F).reshape(n, 8)
    f[:, 0], f[:, 1], f[:, 2], f[:, 3], f[:, 4] = x, y, z, F(1.0), intensity
    if layout != OUT_XYZI:
        out.view(np.uint16).reshape(n, 16)[:, 10] = ring
    if layout == OUT_XYZIRT:
        f[:, 6] = time
    return out


@dataclasses.dataclass
class Fused:
    out: np.ndarray            # (n_out, 32) uint8
    n_in: list
    n_nan: list
    n_depth_filtered: list
    n_kept: list
    out_offset: list
    n_out: int
    n_pitch_index_clamped: int
    pitch: np.ndarray          # the pitch of every kept camera point, in output order


def fuse(segments, P=None) -> Fused:
    P = P or Params()
    parts, n_in, n_nan, n_far, n_kept, offs, pitches = [], [], [], [], [], [], []
    clamped, at = 0, 0
    for seg in segments:
        far = 0
        if isinstance(seg, Depth):
            x, y, z, i, r, t, nan, far, cl, pitch = convert_depth(seg, P)
            clamped += cl
            pitches.append(pitch)
        elif isinstance(seg, LidarXYZIRT):
            x, y, z, i, r, t, nan = convert_xyzirt(seg)
        else:
            x, y, z, i, r, t, nan = convert_xyzi(seg)
        parts.append(records(x, y, z, i, r, t, P.layout))
        n_in.append(seg.rec.shape[0]); n_nan.append(nan); n_far.append(far); n_kept.append(x.shape[0]); offs.append(at)
        at += x.shape[0]
    out = np.concatenate(parts) if parts else np.zeros((0, 32), np.uint8)
    return Fused(out, n_in, n_nan, n_far, n_kept, offs, at, clamped, np.concatenate(pitches) if pitches else np.zeros(0, D))


def boundary_margin(pitch, P) -> float:
    """Smallest distance of a finite pitch to a value where a last-bit difference of asin could change the ring: pitch_min,
    pitch_max, and the halves k + 0.5 of pitch + pitch_offset inside [pitch_min, pitch_max)."""
    p = np.asarray(pitch, D)
    p = p[np.isfinite(p)]
    if p.size == 0:
        return float("inf")
    m = min(float(np.abs(p - P.pitch_min).min()), float(np.abs(p - P.pitch_max).min()))
    mid = p[(p >= P.pitch_min) & (p < P.pitch_max)] + P.pitch_offset
    if mid.size:
        m = min(m, float(np.abs(mid - np.floor(mid) - 0.5).min()))
    return m
