"""numpy restatement of the LOAM deskew: jueying_slam's deskewInfo (the gate, imuDeskewInfo, odomDeskewInfo;
imageProjection.cpp:483-642, new_localization.cpp:1733-1886), findRotation / findPosition as written (the linear scan) and the live
deskewPoint (new_localization.cpp:1948-1977), inside projectPointCloud as imageProjection.cpp:760-782 calls it.  float32 / float64
exactly as the C++ types say; sin / cos are libm's double functions rounded to float, as tests/loam_ref.py takes them.  With
``dtype=F64`` the same formulas run in double throughout (what the physical-sanity test compares the float form with).  It shares no
code with csrc/loam_deskew.h; the rest of the front end is tests/loam_features_ref.py's."""
from __future__ import annotations

import math

import numpy as np

import loam_features_ref as R

F32, F64 = np.float32, np.float64
MAX_ENTRIES = 1024
WAITING = "waiting"
_plain_project = R.project   # `extract` below puts `project` in its place while it runs


class TooMany(Exception):
    """more table entries than the library holds (the reference's arrays overflow beyond imuFrequency)"""


# ---- deskewInfo ----------------------------------------------------------------------------------------------------------------
def build_tables(time_scan_cur, imu, odom=None, time_scan_next=math.inf):
    """imu: rows (stamp, gyro x y z); odom: rows (stamp, x y z); front first.  WAITING, or a dict with the tables as (n,4) rows of
    (time, x, y, z) and the flags.  Plain Python floats: IEEE doubles, one operation per operator."""
    imu = [tuple(float(v) for v in row) for row in np.asarray(imu, F64).reshape(-1, 4)]
    odom = [tuple(float(v) for v in row) for row in np.asarray(odom if odom is not None else np.zeros((0, 4)), F64).reshape(-1, 4)]
    open_end = time_scan_next == math.inf
    if not imu or imu[0][0] > time_scan_cur or (not open_end and imu[-1][0] < time_scan_next):
        return WAITING
    out = dict(time_scan_cur=float(time_scan_cur), imu_skipped=0, odom_skipped=0, imu_available=0, odom_available=0, odom_deskew=0, start_odom_index=-1)
    # imuDeskewInfo
    q = list(imu)
    while q and q[0][0] < time_scan_cur - 0.01:
        q.pop(0)
        out["imu_skipped"] += 1
    tab = []
    for (t, gx, gy, gz) in q:
        if t > time_scan_next + 0.01:
            break
        if len(tab) >= MAX_ENTRIES:
            raise TooMany("imu")
        if not tab:
            tab.append((t, 0.0, 0.0, 0.0))
            continue
        pt, px, py, pz = tab[-1]
        dt = t - pt
        tab.append((t, px + gx * dt, py + gy * dt, pz + gz * dt))
    out["imu"] = np.array(tab, F64).reshape(-1, 4)
    out["imu_available"] = 1 if len(tab) - 1 > 0 else 0
    # odomDeskewInfo
    q = list(odom)
    while q and q[0][0] < time_scan_cur - 0.01:
        q.pop(0)
        out["odom_skipped"] += 1
    tab = []
    if q and not (q[0][0] > time_scan_cur):
        for i, row in enumerate(q):
            out["start_odom_index"] = out["odom_skipped"] + i
            if row[0] < time_scan_cur:
                continue
            break
        out["odom_available"] = 1
        x0 = y0 = z0 = 0.0
        for (t, x, y, z) in q:
            if t > time_scan_next + 0.01:
                break
            if len(tab) >= MAX_ENTRIES:
                raise TooMany("odom")
            if not tab:
                x0, y0, z0 = x, y, z
                tab.append((t, 0.0, 0.0, 0.0))
                continue
            tab.append((t, x - x0, y - y0, z - z0))
        out["odom_deskew"] = 1 if len(tab) - 1 > 0 else 0
    out["odom"] = np.array(tab, F64).reshape(-1, 4)
    return out


# ---- findRotation / findPosition -----------------------------------------------------------------------------------------------
def front_linear(time, t):
    """The first j < cur with t < time[j], else cur (cur = n - 1), for every t."""
    cur = time.shape[0] - 1
    if cur == 0:
        return np.zeros(t.shape[0], np.int64)
    lt = t[:, None] < time[None, :cur]
    return np.where(lt.any(axis=1), lt.argmax(axis=1), cur)


def front_pmax(time, t):
    """The same index by binary search over the prefix maximum of the times (scalar t)."""
    pm, m = [], -math.inf
    for v in time.tolist():
        if v > m:
            m = v
        pm.append(m)
    lo, hi = 0, len(pm) - 1
    while lo < hi:
        mid = (lo + hi) >> 1
        if t < pm[mid]:
            hi = mid
        else:
            lo = mid + 1
    return lo


def find(table, t, dtype=F32):
    """table: (n,4) rows of (time, x, y, z) in arrival order, t: (m,) float64 -> (m,3) of dtype.  No table: zeros."""
    t = np.asarray(t, F64).reshape(-1)
    table = np.asarray(table, F64).reshape(-1, 4)
    if table.shape[0] == 0:
        return np.zeros((t.shape[0], 3), dtype)
    time, val = table[:, 0], table[:, 1:]
    front = front_linear(time, t)
    back = np.maximum(front - 1, 0)
    tf, tb = time[front], time[back]
    direct = (t > tf) | (front == 0)
    with np.errstate(all="ignore"):
        ratio_front = (t - tb) / (tf - tb)
        ratio_back = (tf - t) / (tf - tb)
        blend = val[front] * ratio_front[:, None] + val[back] * ratio_back[:, None]
    return np.where(direct[:, None], val[front], blend).astype(dtype)


# ---- the transform ---------------------------------------------------------------------------------------------------------------
def _trig(fn, a, dtype):
    return np.array([fn(v) for v in a.astype(F64).tolist()], F64).astype(dtype)


def pose(rot, pos, dtype=F32):
    """pcl::getTransformation(pos, rot) for (m,3) arrays -> (m,3,4); the expression order of tests/loam_ref.py's pose_matrix."""
    rot, pos = np.asarray(rot, dtype).reshape(-1, 3), np.asarray(pos, dtype).reshape(-1, 3)
    A, B = _trig(math.cos, rot[:, 2], dtype), _trig(math.sin, rot[:, 2], dtype)
    Cc, D = _trig(math.cos, rot[:, 1], dtype), _trig(math.sin, rot[:, 1], dtype)
    E, Fv = _trig(math.cos, rot[:, 0], dtype), _trig(math.sin, rot[:, 0], dtype)
    DE, DF = D * E, D * Fv
    T = np.empty((rot.shape[0], 3, 4), dtype)
    T[:, 0, 0] = A * Cc; T[:, 0, 1] = A * DF - B * E; T[:, 0, 2] = B * Fv + A * DE
    T[:, 1, 0] = B * Cc; T[:, 1, 1] = A * E + B * DF; T[:, 1, 2] = B * DE - A * Fv
    T[:, 2, 0] = -D; T[:, 2, 1] = Cc * Fv; T[:, 2, 2] = Cc * E
    T[:, :, 3] = pos
    return T


def affine_inverse(T, dtype=F32):
    """Affine3f::inverse(): Matrix3f::inverse() by cofactors (column 0 first, det = (c00 m00 + c10 m10) + c20 m20, one reciprocal),
    translation = -(inverse * t) summed left to right.  T: (3,4)."""
    m = np.asarray(T, dtype)[:, :3]
    cof = np.empty((3, 3), dtype)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            cof[i, j] = dtype(m[i1, j1] * m[i2, j2]) - dtype(m[i1, j2] * m[i2, j1])
    det = dtype(dtype(cof[0, 0] * m[0, 0]) + dtype(cof[1, 0] * m[1, 0])) + dtype(cof[2, 0] * m[2, 0])
    with np.errstate(all="ignore"):
        invdet = dtype(1) / dtype(det)
    out = np.empty((3, 4), dtype)
    for r in range(3):
        for c in range(3):
            out[r, c] = cof[c, r] * invdet
        t = T[:, 3]
        out[r, 3] = -dtype(dtype(dtype(out[r, 0] * t[0]) + dtype(out[r, 1] * t[1])) + dtype(out[r, 2] * t[2]))
    return out


def transform_points(start_inv, final, pts, dtype=F32):
    """transBt = transStartInverse * transFinal per point ((m,3,4)), then a x + b y + c z + d per row, left to right."""
    S = np.asarray(start_inv, dtype)
    pts = np.asarray(pts, dtype)
    B = np.empty_like(final)
    for r in range(3):
        a, b, c = S[r, 0], S[r, 1], S[r, 2]
        for k in range(3):
            B[:, r, k] = (a * final[:, 0, k] + b * final[:, 1, k]) + c * final[:, 2, k]
        B[:, r, 3] = ((a * final[:, 0, 3] + b * final[:, 1, 3]) + c * final[:, 2, 3]) + S[r, 3]
    x, y, z = pts[:, 0], pts[:, 1], pts[:, 2]
    return np.stack([((B[:, r, 0] * x + B[:, r, 1] * y) + B[:, r, 2] * z) + B[:, r, 3] for r in range(3)], axis=1)


def deskew_points(dk, pts, t, t_first, dtype=F32):
    """deskewPoint of pts (m,3) at the point times t (m,), with transStartInverse from the point time t_first."""
    imu, odom = dk["imu"], dk.get("odom")
    odom = np.zeros((0, 4)) if odom is None else odom
    s = pose(find(imu, [t_first], dtype), find(odom, [t_first], dtype), dtype)[0]
    final = pose(find(imu, t, dtype), find(odom, t, dtype), dtype)
    return transform_points(affine_inverse(s, dtype), final, pts, dtype)


# ---- projectPointCloud with the live deskewPoint -----------------------------------------------------------------------------
def stamps(rec):
    """PointXYZIRT's double timestamp (offset 24 of the 48-byte record)."""
    rec = np.ascontiguousarray(rec).reshape(-1, 48)
    return rec[:, 24:32].copy().view(F64).reshape(-1)


def project(rec, p, dk, first=None):
    """R.project's tuple with the owners' points and ranges replaced by the deskewed ones (imageProjection.cpp:777-782).  The
    column, the raw range test and the ownership stay the raw point's; point time = time_scan_cur + (t_i - t_0), t_0 record 0's.
    first: the record whose time starts the transform (default: the smallest record index that passes the tests)."""
    cells, own, col, rng, xyz, inten = _plain_project(rec, p)
    if dk is None or not dk.get("imu_available", 1) or own.shape[0] == 0:
        return cells, own, col, rng, xyz, inten
    ts = stamps(rec)
    t = dk["time_scan_cur"] + (ts - ts[0])
    first = int(own.min()) if first is None else first
    q = deskew_points(dk, xyz[own], t[own], t[first])
    xyz, rng = xyz.copy(), rng.copy()
    xyz[own] = q
    x, y, z = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(all="ignore"):
        rng[own] = np.sqrt((x * x + y * y) + z * z).astype(F32)
    return cells, own, col, rng, xyz, inten


def extract(st, rec, sorter, params=None, dk=None, first=None):
    """R.extract with `project` above in the place of its projection: everything behind the projection is the old restatement."""
    R.project = lambda rec_, p_: project(rec_, p_, dk, first)
    try:
        return R.extract(st, rec, sorter, params)
    finally:
        R.project = _plain_project


# ---- motion for the tests: constant rates sampled into tables --------------------------------------------------------------------
def sampled_tables(time_scan_cur, rate_hz, duration, gyro, vel, lead=0.005):
    """IMU and odometry queues of a body turning at `gyro` rad/s and moving at `vel` m/s, sampled at rate_hz from `lead` seconds
    before time_scan_cur for `duration` seconds -> (imu rows, odom rows)."""
    n = int(round(duration * rate_hz)) + 1
    t = time_scan_cur - lead + np.arange(n) / rate_hz
    imu = np.concatenate([t[:, None], np.broadcast_to(np.asarray(gyro, F64), (n, 3))], axis=1)
    odom = np.concatenate([t[:, None], (t - t[0])[:, None] * np.asarray(vel, F64)[None, :]], axis=1)
    return imu, odom
