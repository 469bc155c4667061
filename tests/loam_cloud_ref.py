"""A literal per-point restatement of jueying_slam's cachePointCloud in both nodes (src/imageProjection.cpp:258-479 with the
48-byte PointXYZIRT of :7-19; src/new_localization.cpp:1560-1731 with the 32-byte PointXYZIRT of :26-38) and of
myremoveNaNFromPointCloud (src/imageProjection.cpp:211-256), written from the reference lines and independent of
csrc/loam_cloud.h.  Python's float is the C++ double and every operator below is one IEEE operation in the order of the C++
expression; numpy.float32 stands where the reference has a float.  Slow on purpose: loops over (h, w) as the reference does."""
import math

import numpy as np

VELODYNE, RSLIDAR_RUBY, RSLIDAR_16, RSLIDAR_32 = 0, 1, 2, 3   # include/utility.h:116-121
MAPPING, LOCALIZATION = 0, 1
F32 = np.float32

# the two node structs: (size, intensity dtype, intensity offset, ring offset, time dtype, time offset)
RECORD = {MAPPING: (48, "<u1", 16, 32, "<f8", 24), LOCALIZATION: (32, "<f4", 16, 20, "<f4", 24)}


def ring_of(lidar_type, h):
    """laserCloudIn->at(w,h).ring = ... (:328, :369, :444): an int expression assigned to uint16_t."""
    if lidar_type == RSLIDAR_16:
        r = h if h < 8 else 15 - (h - 8)
    else:
        r = h
    return r & 0xFFFF


def time_of(lidar_type, h, w):
    """The double expression assigned to the time field (:349, :386, :461)."""
    if lidar_type == RSLIDAR_16:
        return h * 2.8 * 1e-6 + w * 55.5 * 1e-6
    if lidar_type == RSLIDAR_RUBY:
        k = 64 if (h + 1) % 64 == 0 else (h + 1) % 64
        q = F32(k - 1) / F32(4.0)                       # (... - 1) / 4.f: int -> float, float division
        return 3.236 * float(q) * 1e-6 + w * 55.552 * 1e-6
    s = F32(h // 16)                                    # float(h/16): int division, then float
    return (w * 55.52 + h % 16 * 2.88 + 1.44 * float(s)) * 1e-6


class Desc:
    """The message as the node sees it: where the fields lie (None: the message has none) and the two flags of this call."""

    def __init__(self, height, width, point_step, x, intensity, ring, time, is_dense, lidar_type, kind, synth_ring, synth_time):
        self.height, self.width, self.point_step = height, width, point_step
        self.x, self.intensity, self.ring, self.time = x, intensity, ring, time
        self.is_dense, self.lidar_type, self.kind, self.synth_ring, self.synth_time = is_dense, lidar_type, kind, synth_ring, synth_time


def cache_point_cloud(raw, d):
    """raw: height * width * point_step message bytes.  Returns (records (n_out, 48 | 32) uint8, info) or raises ValueError
    where the node shuts down."""
    size, idt, ioff, roff, tdt, toff = RECORD[d.kind]
    raw = np.frombuffer(bytes(raw), np.uint8)
    n = d.height * d.width
    assert raw.size == n * d.point_step
    # pcl::fromROSMsg into the node's struct: fields of the same name and type are copied, the rest keep the value of a fresh
    # point (x y z 1, everything else 0)
    cloud = np.zeros((n, size), np.uint8)
    for i in range(n):
        rec = raw[i * d.point_step:(i + 1) * d.point_step]
        cloud[i, 0:12] = rec[d.x:d.x + 12]
        cloud[i, 12:16] = np.frombuffer(F32(1.0).tobytes(), np.uint8)
        isz = np.dtype(idt).itemsize
        cloud[i, ioff:ioff + isz] = rec[d.intensity:d.intensity + isz]
        if d.ring is not None:
            cloud[i, roff:roff + 2] = rec[d.ring:d.ring + 2]
        if d.time is not None:
            tsz = np.dtype(tdt).itemsize
            cloud[i, toff:toff + tsz] = rec[d.time:d.time + tsz]
    info = {"n_in": n, "n_out": n, "n_nonfinite": 0, "ring_synthesised": 0, "time_synthesised": 0, "time_available": int(d.time is not None)}
    if d.lidar_type == VELODYNE:
        if not d.is_dense:
            raise ValueError("Point cloud is not in dense format, please remove NaN points first!")       # :280-285
        if d.ring is None:
            raise ValueError("Point cloud ring channel not available, please configure your point cloud data!")   # :299-303
        return cloud, info
    if d.lidar_type not in (RSLIDAR_RUBY, RSLIDAR_16, RSLIDAR_32):
        raise ValueError("Undefined lidar type")                                                          # :475-478
    # height == 0 or width == 0: the library's definition is the empty cloud (the reference's unsigned height-1 wraps there);
    # Python's signed ranges below are empty
    if d.synth_ring:
        info["ring_synthesised"] = 1
        for h in range(0, d.height - 1):                                                                  # :326-327
            for w in range(0, d.width - 1):
                i = h * d.width + w                                                                       # at(w, h)
                cloud[i, roff:roff + 2] = np.frombuffer(np.uint16(ring_of(d.lidar_type, h)).tobytes(), np.uint8)
    if d.synth_time:
        info["time_synthesised"] = 1
        info["time_available"] = 1
        for h in range(0, d.height - 1):                                                                  # :347-348
            for w in range(0, d.width - 1):
                i = h * d.width + w
                t = time_of(d.lidar_type, h, w)
                cloud[i, toff:toff + np.dtype(tdt).itemsize] = np.frombuffer(np.array(t, np.float64).astype(tdt).tobytes(), np.uint8)
    if not d.is_dense:                                                                                    # :356-361
        out = []
        for i in range(n):                                                                                # :234-243
            x, y, z = np.frombuffer(cloud[i, 0:12].tobytes(), "<f4")
            if not math.isfinite(x) or not math.isfinite(y) or not math.isfinite(z):
                continue
            out.append(cloud[i])
        info["n_out"] = len(out)
        info["n_nonfinite"] = n - len(out)
        cloud = np.array(out, np.uint8).reshape(len(out), size)
    return cloud, info


def make_raw(height, width, point_step, x, intensity, ring, time, kind, seed, nan_at=(), intensity_scale=255.0, scene="noise"):
    """A seeded organised cloud as message bytes: finite points on a rough cylinder, every padding byte random (so a copied
    padding byte shows), the message's ring = (h * 7 + 3) & 0xffff and time = a random value where it has the fields;
    ``nan_at``: record indices whose x, y or z (cycling) is NaN / inf.  scene "room": the walls of a 20 m x 12 m room with a
    pillar at 4 m every 64 columns and a millimetre of noise, so the front end finds edges and planes in it."""
    size, idt, _, _, tdt, _ = RECORD[kind]
    rng = np.random.default_rng(seed)
    n = height * width
    raw = rng.integers(0, 256, (n, point_step), dtype=np.uint8)
    if n == 0:
        return raw
    hh, ww = np.divmod(np.arange(n), max(width, 1))
    az = 2.0 * np.pi * ww / max(width, 1) + rng.uniform(-1e-3, 1e-3, n)
    rr = rng.uniform(3.0, 40.0, n)
    if scene == "room":
        rr = np.minimum(10.0 / np.maximum(np.abs(np.sin(az)), 1e-9), 6.0 / np.maximum(np.abs(np.cos(az)), 1e-9))
        rr = np.where((ww % 64 >= 20) & (ww % 64 < 27), 4.0, rr) + rng.uniform(-1e-3, 1e-3, n)
    el = np.deg2rad(-15.0 + 30.0 * hh / max(height - 1, 1))
    if scene == "room":   # rr is the horizontal distance
        xyz = np.stack([rr * np.sin(az), rr * np.cos(az), rr * np.tan(el)], axis=1).astype("<f4")
    else:
        xyz = np.stack([rr * np.cos(el) * np.sin(az), rr * np.cos(el) * np.cos(az), rr * np.sin(el)], axis=1).astype("<f4")
    bad = [np.nan, np.inf, -np.inf]
    for k, i in enumerate(nan_at):
        xyz[i, k % 3] = bad[k % 3]
    raw[:, x:x + 12] = xyz.view(np.uint8).reshape(n, 12)
    inten = rng.uniform(0.0, intensity_scale, n)
    raw[:, intensity:intensity + np.dtype(idt).itemsize] = inten.astype(idt).view(np.uint8).reshape(n, -1)
    if ring is not None:
        raw[:, ring:ring + 2] = ((hh * 7 + 3) & 0xFFFF).astype("<u2").view(np.uint8).reshape(n, 2)
    if time is not None:
        raw[:, time:time + np.dtype(tdt).itemsize] = rng.uniform(0.0, 0.1, n).astype(tdt).view(np.uint8).reshape(n, -1)
    return raw


def capi_desc(capi, d):
    """``d`` as the library's descriptor, field by field (not through the library's defaults)."""
    c = capi.PcmLoamCloudDesc()
    c.height, c.width, c.point_step = d.height, d.width, d.point_step
    c.xyz_offset_bytes, c.intensity_offset_bytes = d.x, d.intensity
    c.ring_offset_bytes = capi.PCM_LOAM_FIELD_ABSENT if d.ring is None else d.ring
    c.time_offset_bytes = capi.PCM_LOAM_FIELD_ABSENT if d.time is None else d.time
    c.intensity_kind = capi.PCM_LOAM_INTENSITY_UINT8 if d.kind == MAPPING else capi.PCM_LOAM_INTENSITY_FLOAT
    c.ring_kind = capi.PCM_LOAM_RING_UINT16
    c.time_kind = capi.PCM_LOAM_TIME_DOUBLE if d.kind == MAPPING else capi.PCM_LOAM_TIME_FLOAT
    c.is_dense, c.lidar_type, c.record_kind = int(d.is_dense), d.lidar_type, d.kind
    c.synth_ring, c.synth_time = int(d.synth_ring), int(d.synth_time)
    return c


# message layouts of the tests: (point_step, x, intensity, ring, time) per record kind.  32: padded, every field 4-aligned; 26:
# unpacked records follow each other without padding (odd records begin at a 2-byte boundary) and the localisation ring sits at
# an odd multiple of 2
LAYOUTS = {(32, MAPPING): (32, 0, 12, 28, 16), (32, LOCALIZATION): (32, 0, 12, 24, 16),
           (26, MAPPING): (26, 0, 12, 24, 16), (26, LOCALIZATION): (26, 0, 12, 22, 16)}


def make_case(height, width, step, kind, lidar_type, seed, has_ring=True, has_time=True, synth_ring=True, synth_time=False, is_dense=False, nan_at=(), scene="noise"):
    """(raw message bytes (n, point_step) uint8, Desc) of one test cloud."""
    ps, x, io, ro, to = LAYOUTS[(step, kind)]
    ro, to = (ro if has_ring else None), (to if has_time else None)
    raw = make_raw(height, width, ps, x, io, ro, to, kind, seed, nan_at, scene=scene)
    return raw, Desc(height, width, ps, x, io, ro, to, is_dense, lidar_type, kind, synth_ring, synth_time)
