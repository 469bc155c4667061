"""numpy float64 restatement of the last block of LaserMapping::Run (jueying_lio/src/laser_mapping.cc:361-385) and Finish (:887-900):
the two PointBodyToWorld overloads (:855-875), PointBodyLidarToIMU (:877-885), the saved map with its chunk counter (:776-791) and
the export through pcd2map's filters (src/tool/pcd2map/src/pcd2map.cpp:60-72).

Every rotation is Eigen's Quaternion::_transformVector spelled out term by term -- uv = 2 (q.vec x v); r = v + w uv + q.vec x uv, each
component (v + w uv) + c -- in IEEE double, one operation at a time, so a device kernel that does the same operations in the same
order gives the same bits.  Quaternions are (x, y, z, w)."""
import numpy as np


def qrot(q, v):
    """q * v for (n, 3) float64 rows v: Eigen _transformVector operation order."""
    q = np.asarray(q, np.float64)
    v = np.asarray(v, np.float64)
    x, y, z, w = q[0], q[1], q[2], q[3]
    v0, v1, v2 = v[:, 0], v[:, 1], v[:, 2]
    uv0 = y * v2 - z * v1
    uv1 = z * v0 - x * v2
    uv2 = x * v1 - y * v0
    uv0 = uv0 + uv0
    uv1 = uv1 + uv1
    uv2 = uv2 + uv2
    c0 = y * uv2 - z * uv1
    c1 = z * uv0 - x * uv2
    c2 = x * uv1 - y * uv0
    return np.stack([(v0 + w * uv0) + c0, (v1 + w * uv1) + c1, (v2 + w * uv2) + c2], axis=1)


def lidar_to_imu_d(state, xyz):
    """offset_R_L_I * p + offset_T_L_I in double (:879)."""
    t = np.asarray(state["off_T"], np.float64)
    r = qrot(state["off_R"], np.asarray(xyz, np.float32).astype(np.float64))
    return np.stack([r[:, 0] + t[0], r[:, 1] + t[1], r[:, 2] + t[2]], axis=1)


def body_to_world_d(state, xyz):
    """rot * (offset_R_L_I * p + offset_T_L_I) + pos in double (:857-858)."""
    p = np.asarray(state["pos"], np.float64)
    r = qrot(state["rot"], lidar_to_imu_d(state, xyz))
    return np.stack([r[:, 0] + p[0], r[:, 1] + p[1], r[:, 2] + p[2]], axis=1)


def _records(xyz_d, intensity):
    out = np.empty((len(xyz_d), 4), np.float32)
    out[:, :3] = xyz_d.astype(np.float32)         # po->x = p_global(0)
    out[:, 3] = intensity
    return out


def frame_world(state, records):
    """PointBodyToWorld(const PointType*, ...) over (n, 12) PointXYZINormal rows (intensity = column 8) -> (n, 4) float32."""
    records = np.asarray(records, np.float32)
    return _records(body_to_world_d(state, records[:, :3]), records[:, 8])


def frame_body(state, records):
    """PointBodyLidarToIMU over (n, 12) rows -> (n, 4) float32."""
    records = np.asarray(records, np.float32)
    return _records(lidar_to_imu_d(state, records[:, :3]), records[:, 8])


def frame_effect(state, records, selected):
    """PointBodyToWorld(const V3F&, ...) over corr_pts_ = the rows of the down-sampled scan with `selected`, in scan order (:645-653):
    intensity = std::abs(po->z) of the float just written."""
    records = np.asarray(records, np.float32)[np.asarray(selected, bool)]
    out = _records(body_to_world_d(state, records[:, :3]), 0.0)
    out[:, 3] = np.abs(out[:, 2])
    return out


class SavedMap:
    """pcl_wait_save_, scan_wait_num and pcd_index_ with the library's division of work: append() reports the chunk, the caller
    fetches the cloud and calls clear()."""

    def __init__(self):
        self.frames = []
        self.scan_wait_num = 0
        self.pcd_index = 0
        self.frames_appended = 0

    def cloud(self):
        return np.concatenate(self.frames) if self.frames else np.zeros((0, 4), np.float32)

    def append(self, world, pcd_save_interval):
        self.frames.append(np.asarray(world, np.float32))
        self.frames_appended += 1
        self.scan_wait_num += 1
        ready = len(self.cloud()) > 0 and pcd_save_interval > 0 and self.scan_wait_num >= pcd_save_interval
        if ready:
            self.pcd_index += 1
        return ready, self.pcd_index

    def clear(self):
        self.frames = []
        self.scan_wait_num = 0


def pass_through_z(cloud, z_min, z_max):
    """pcl::PassThrough on z, setFilterLimitsNegative(false): finite x, y, z and z_min <= z <= z_max, in order."""
    cloud = np.asarray(cloud, np.float32)
    z = cloud[:, 2].astype(np.float64)
    keep = np.isfinite(cloud[:, :3]).all(axis=1) & (z >= z_min) & (z <= z_max)
    return cloud[keep]


def export(cloud, leaf_size=0.0, z_min=1.0, z_max=0.0, voxel_grid=None):
    """Finish + pcd2map: voxel_grid(cloud, leaf) when leaf_size > 0 (the caller's VoxelGrid), then the z window when z_min <= z_max."""
    out = np.asarray(cloud, np.float32)
    if leaf_size > 0:
        out = voxel_grid(out, leaf_size)
    if z_min <= z_max:
        out = pass_through_z(out, z_min, z_max)
    return out


def lio_pose_f(state):
    """(q_wl, t_wl) of ObsModel as floats (:602-603): (rot * off_R).cast<float>(), (rot * off_T + pos).cast<float>()."""
    a = np.asarray(state["rot"], np.float64)
    b = np.asarray(state["off_R"], np.float64)
    q = np.array([a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1],
                  a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2],
                  a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0],
                  a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2]])
    t = qrot(a, np.asarray(state["off_T"], np.float64)[None, :])[0] + np.asarray(state["pos"], np.float64)
    return q.astype(np.float32), t.astype(np.float32)


def default_selected(state, xyz, planes):
    """The default semantics' row test in float, as the search kernel evaluates it: a plane is stored (x not NaN) and
    |p_body| > 81 pd2^2 with pd2 = n . p_world + d at the float pose of `state` (:627-631)."""
    F = np.float32
    q, t = lio_pose_f(state)
    p = np.asarray(xyz, F)
    px, py, pz = p[:, 0], p[:, 1], p[:, 2]
    x, y, z, w = q
    uv0 = y * pz - z * py; uv1 = z * px - x * pz; uv2 = x * py - y * px
    uv0 = uv0 + uv0; uv1 = uv1 + uv1; uv2 = uv2 + uv2
    c0 = y * uv2 - z * uv1; c1 = z * uv0 - x * uv2; c2 = x * uv1 - y * uv0
    w0 = (px + w * uv0 + c0) + t[0]; w1 = (py + w * uv1 + c1) + t[1]; w2 = (pz + w * uv2 + c2) + t[2]
    pl = np.asarray(planes, F)
    with np.errstate(invalid="ignore"):
        pd2 = pl[:, 0] * w0 + pl[:, 1] * w1 + pl[:, 2] * w2 + pl[:, 3]
        norm = np.sqrt(px * px + py * py + pz * pz)
        return ~np.isnan(pl[:, 0]) & (norm > F(81.0) * pd2 * pd2)
