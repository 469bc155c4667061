"""jueying_lio on a P2PLANE context: the measurement model and the frame calls, the iterated Kalman update, ImuProcess::Process
(pcm_lio_imu_init, pcm_lio_propagate), the frame outputs and the saved map (section 25), and
LaserMapping::Run composed from them (``LioOdometry``)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from ._binding import buffer_arg, fill_params

IMU_STATE_VECTORS = ("mean_acc", "mean_gyr", "cov_acc", "cov_gyr", "cov_bias_gyr", "cov_bias_acc", "cov_acc_scale", "cov_gyr_scale", "lidar_T_wrt_imu",
                     "lidar_R_wrt_imu", "angvel_last", "acc_s_last")
IMU_STATE_SCALARS = ("last_lidar_end_time", "init_iter_num", "first_frame", "need_init")
LIO_STATE_FIELDS = (("pos", 3), ("rot", 4), ("off_R", 4), ("off_T", 3), ("vel", 3), ("bg", 3), ("ba", 3), ("grav", 3))


@dataclasses.dataclass
class LioUpdateResult:
    """Result of Registration.lio_update: the updated state (dict as given) and covariance, and the loop's counters."""
    x: dict
    P: np.ndarray
    iterations: int       # ObsModel calls made (<= max_iter + 1)
    rematches: int        # of those, with converge = true
    valid_calls: int      # calls with n_eff >= 1
    t: int                # the loop's converge counter at exit
    n_eff_last: int
    sum_h2_last: float
    status: int


def _imu_state_key(s, k, v):
    if k in IMU_STATE_VECTORS:
        getattr(s, k)[:] = [float(t) for t in v]
    elif k == "last_imu":
        v = [float(t) for t in v]
        s.last_imu.t = v[0]; s.last_imu.acc[:] = v[1:4]; s.last_imu.gyr[:] = v[4:7]
    else:
        return False   # a scalar is set as it is; anything else is no member
    return True


def lio_imu_state(**overrides) -> capi.PcmLioImuState:
    """The members of ImuProcess with the constructor's values (pcm_lio_default_imu_state), any of them overridden: the vectors by a
    sequence, last_imu by the 7 numbers t, acc, gyr, the scalars by a number."""
    return fill_params(capi.PcmLioImuState, capi.load_library().pcm_lio_default_imu_state, overrides, _imu_state_key)


def _lio_state(rot_xyzw, pos, off_R_xyzw, off_T) -> capi.PcmLioState:
    st = capi.PcmLioState()
    st.rot[:] = list(map(float, rot_xyzw)); st.pos[:] = list(map(float, pos)); st.off_R[:] = list(map(float, off_R_xyzw)); st.off_T[:] = list(map(float, off_T))
    return st


def _filter_state(x) -> capi.PcmLioFilterState:
    st = capi.PcmLioFilterState()
    if isinstance(x, dict):
        for k, _ in LIO_STATE_FIELDS:
            getattr(st, k)[:] = [float(v) for v in x[k]]
    else:
        v = np.ascontiguousarray(x, np.float64).reshape(26)
        C.memmove(C.byref(st), v.ctypes.data, 26 * 8)
    return st


def _filter_dict(st) -> dict:
    return {k: np.array(getattr(st, k)[:]) for k, _ in LIO_STATE_FIELDS}


def _imu_rows(imu) -> np.ndarray:
    a = np.ascontiguousarray(imu, np.float64)
    if a.ndim != 2 or a.shape[1] != 7:
        raise ValueError("expected (n, 7) IMU rows: t, acc, gyr")
    return a


def _pose_rows(poses):
    """(pointer, count, keep-alive) of (K,22) Pose6D rows; None = none."""
    if poses is None:
        return None, 0, None
    pa = np.ascontiguousarray(poses, dtype=np.float64)
    assert pa.ndim == 2 and pa.shape[1] == 22
    return pa.ctypes.data, pa.shape[0], pa


def _map_info_dict(info) -> dict:
    return dict(points=int(info.points), capacity=int(info.capacity), frames_appended=int(info.frames_appended), growths=int(info.growths),
                scan_wait_num=int(info.scan_wait_num), pcd_index=int(info.pcd_index), chunk_ready=bool(info.chunk_ready))


class _LioMixin:
    """The jueying_lio calls of the context ``self._h``."""

    LIO_STATE_FIELDS = LIO_STATE_FIELDS

    # -- the measurement model and the map ------------------------------------------------------------------------------------------
    def obs_model(self, rot_xyzw, pos, off_R_xyzw, off_T, extrinsic_est_en=False, converge=True):
        """jueying_lio's ObsModel + the IEKF reduction (pcm_obs_model):
        returns (HTH 12x12, HTh 12, n_eff, sum_h2, valid)."""
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        out = capi.PcmObsResult()
        self._check(self._L.pcm_obs_model(self._h, C.byref(st), int(extrinsic_est_en), int(converge), C.byref(out)))
        return np.array(out.HTH[:]).reshape(12, 12), np.array(out.HTh[:]), out.n_eff, out.sum_h2, bool(out.valid)

    def get_lio_members(self, n: int):
        """(residuals_, point_selected_surf_) as the last obs_model left them (reference-semantics mode only)."""
        res = np.zeros(n, np.float32); sel = np.zeros(n, np.uint8)
        self._check(self._L.pcm_get_lio_members(self._h, res.ctypes.data, sel.ctypes.data, n))
        return res, sel.astype(bool)

    def map_incremental(self, rot_xyzw, pos, off_R_xyzw, off_T, filter_size_map: float, ekf_inited: bool = True) -> int:
        """LaserMapping::MapIncremental with the add-filter; returns the number of points inserted."""
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        n = C.c_size_t()
        self._check(self._L.pcm_map_incremental(self._h, C.byref(st), C.c_float(filter_size_map), int(ekf_inited), C.byref(n)))
        return n.value

    def lio_search_path(self) -> tuple:
        """(lists, tile): matching ObsModel launches (obs_model with rematch, the matching rounds of lio_update) served by the lists
        kernel and by the tile kernel since the context was made or reset_stats (pcm_lio_search_path)."""
        n = np.zeros(2, np.uint64)
        self._check(self._L.pcm_lio_search_path(self._h, n.ctypes.data))
        return int(n[0]), int(n[1])

    # -- pre-processing ---------------------------------------------------------------------------------------------------------------
    def undistort(self, points, time_index, poses, rot_xyzw, pos, off_R_xyzw, off_T):
        """Motion compensation of a scan into its frame-end pose, in place (ImuProcess::UndistortPcl's backward propagation,
        jueying_lio/include/imu_processing.hpp:245-285).  points: (N,F) float32 (x,y,z first, time [ms] in column time_index,
        sorted by time); poses: (K,22) float64 rows = Pose6D (offset_time, acc, gyr, vel, pos, rot row-major)."""
        assert points.dtype == np.float32 and points.flags["C_CONTIGUOUS"] and points.ndim == 2
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.ndim == 2 and poses.shape[1] == 22
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        self._check(self._L.pcm_undistort(self._h, points.ctypes.data, points.shape[0], points.strides[0], 4 * int(time_index), capi.MEM_HOST,
                                          poses.ctypes.data, poses.shape[0], C.byref(st)))
        return points

    def livox_filter(self, msg_points, num_scans: int = 6, point_filter_num: int = 1, blind: float = 0.01) -> np.ndarray:
        """PointCloudPreprocess::AviaHandler (pointcloud_preprocess.cc:44-88): livox CustomPoint records (20-byte structured array:
        offset_time u4, x y z f4, reflectivity tag line u1, pad) -> (m, 12) float32 pcl::PointXYZINormal records in input order."""
        a = np.ascontiguousarray(msg_points)
        assert a.dtype.itemsize == 20
        out = np.zeros((max(len(a), 1), 12), np.float32)
        m = C.c_size_t()
        self._check(self._L.pcm_livox_filter(self._h, a.ctypes.data, len(a), capi.MEM_HOST, int(num_scans), int(point_filter_num), float(blind), out.ctypes.data, len(out), C.byref(m)))
        return out[:m.value].copy()

    # -- one frame ----------------------------------------------------------------------------------------------------------------------
    def lio_frame_begin(self, msg_points, poses=None, rot_xyzw=(0, 0, 0, 1.0), pos=(0, 0, 0), off_R_xyzw=(0, 0, 0, 1.0), off_T=(0, 0, 0),
                        num_scans: int = 6, point_filter_num: int = 2, blind: float = 0.1, leaf_size: float = 0.5) -> int:
        """Front end of one LaserMapping::Run frame on the device (pcm_lio_frame_begin): raw livox CustomPoint records (20-byte
        structured array; host array or a CUDA uint8 tensor) -> driver-message filter -> motion compensation (poses: (K,22) Pose6D rows,
        None = none) -> voxel-grid down-sampling -> source of this object.  Returns the number of scan points."""
        mem, ptr, n = capi.MEM_HOST, None, 0
        if hasattr(msg_points, "data_ptr"):
            assert msg_points.is_cuda and msg_points.element_size() * msg_points.numel() % 20 == 0
            mem, ptr, n = capi.MEM_DEVICE, msg_points.data_ptr(), msg_points.element_size() * msg_points.numel() // 20
            self._keep_frame = msg_points
        else:
            a = np.ascontiguousarray(msg_points)
            assert a.dtype.itemsize == 20
            ptr, n = a.ctypes.data, len(a)
            self._keep_frame = a
        prm = capi.PcmLioFrameParams(int(num_scans), int(point_filter_num), float(blind), float(leaf_size), 0)
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        pp, npose, keep = _pose_rows(poses)
        m = C.c_size_t()
        self._check(self._L.pcm_lio_frame_begin(self._h, C.c_void_p(ptr), C.c_size_t(n), mem, C.byref(prm), C.c_void_p(pp), int(npose), C.byref(st), C.byref(m)))
        return m.value

    def lio_frame_begin_cloud(self, points, desc, poses=None, rot_xyzw=(0, 0, 0, 1.0), pos=(0, 0, 0), off_R_xyzw=(0, 0, 0, 1.0), off_T=(0, 0, 0),
                              leaf_size: float = 0.5) -> int:
        """lio_frame_begin for a sensor_msgs::PointCloud2 cloud (pcm_lio_frame_begin_cloud): the records of msg.data (a host array or a
        device tensor) -> handler of desc.type -> stable sort by time -> motion compensation (poses: (K,22) Pose6D rows, None = none) ->
        voxel-grid down-sampling -> source of this object.  Returns the number of scan points."""
        ptr, n, _, mem, keep = buffer_arg(points, record=desc.stride_bytes, f32=False, convert=True, what="points:")
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        pp, npose, keep_p = _pose_rows(poses)
        m = C.c_size_t()
        rc = self._L.pcm_lio_frame_begin_cloud(self._h, ptr, n, mem, C.byref(desc), C.c_float(leaf_size), C.c_void_p(pp), int(npose), C.byref(st), C.byref(m))
        del keep
        self._check(rc)
        return m.value

    def lio_frame_end(self, rot_xyzw, pos, off_R_xyzw, off_T, filter_size_map: float, ekf_inited: bool = True) -> int:
        """Back end of the frame (pcm_lio_frame_end = MapIncremental with the updated state); returns the points inserted."""
        return self.map_incremental(rot_xyzw, pos, off_R_xyzw, off_T, filter_size_map, ekf_inited)

    # -- the filter -----------------------------------------------------------------------------------------------------------------------
    def lio_update(self, x, P, R: float = None, max_iter: int = None, extrinsic_est_en: bool = False, limit=None) -> "LioUpdateResult":
        """jueying_lio's iterated Kalman update (esekf::update_iterated_dyn_share_modified) on the device: pcm_lio_update.
        x: the propagated state_ikfom as a dict of pos(3) rot(4: x,y,z,w) off_R(4) off_T(3) vel(3) bg(3) ba(3) grav(3), or the 26 numbers
        in that order; P: 23 x 23 covariance.  One call per frame between lio_frame_begin and lio_frame_end; the inputs are not changed.
        Parameters default to the reference's (R 0.001, max_iter 4, limit 0.001 each)."""
        st = _filter_state(x)
        Pm = np.array(P, np.float64).reshape(23, 23).copy()
        prm = capi.PcmLioUpdateParams()
        self._L.pcm_lio_default_update_params(C.byref(prm))
        if R is not None:
            prm.R = float(R)
        if max_iter is not None:
            prm.max_iter = int(max_iter)
        prm.extrinsic_est_en = int(bool(extrinsic_est_en))
        if limit is not None:
            prm.limit[:] = [float(v) for v in np.broadcast_to(np.asarray(limit, np.float64), (23,))]
        res = capi.PcmLioUpdateResult()
        self._check(self._L.pcm_lio_update(self._h, C.byref(prm), C.byref(st), Pm.ctypes.data, C.byref(res)))
        return LioUpdateResult(x=_filter_dict(st), P=Pm, iterations=res.iterations, rematches=res.rematches, valid_calls=res.valid_calls, t=res.t,
                               n_eff_last=res.n_eff_last, sum_h2_last=res.sum_h2_last, status=res.status)

    def lio_update_trace(self, call: int):
        """ObsModel call `call` of the last lio_update: dict(x, converge, n_eff, HTH (12x12), HTh (12), dx_ (23))."""
        st = capi.PcmLioFilterState()
        cv, ne = C.c_int32(), C.c_int32()
        sums = np.zeros(90); dx = np.zeros(23)
        self._check(self._L.pcm_lio_update_trace(self._h, int(call), C.byref(st), C.byref(cv), C.byref(ne), sums.ctypes.data, dx.ctypes.data))
        HTH = np.zeros((12, 12))
        iu = np.triu_indices(12)
        HTH[iu] = sums[:78]
        HTH = HTH + np.triu(HTH, 1).T
        return dict(x=_filter_dict(st), converge=bool(cv.value), n_eff=ne.value, HTH=HTH, HTh=sums[78:90].copy(), dx_=dx)

    def lio_imu_init(self, imu_state: capi.PcmLioImuState, imu, x, P):
        """One init frame of ImuProcess::Process (pcm_lio_imu_init; host arithmetic): imu_state is advanced in place, -> (x, P) with grav,
        bg, the extrinsics and the initial covariance set.  imu: (n, 7) rows t, acc, gyr; x as for lio_update."""
        a = _imu_rows(imu)
        st = _filter_state(x)
        Pm = np.array(P, np.float64).reshape(23, 23).copy()
        rc = self._L.pcm_lio_imu_init(C.byref(imu_state), a.ctypes.data, a.shape[0], C.byref(st), Pm.ctypes.data)
        if rc != capi.PCM_OK:
            raise capi.PcmError(rc, "pcm_lio_imu_init: no sample, a sample that is not finite, or an IMU state that is already initialised")
        return _filter_dict(st), Pm

    def lio_propagate(self, imu_state: capi.PcmLioImuState, imu, t_beg: float, t_end: float, x, P, capacity: int = None):
        """The forward propagation of one frame on the device (pcm_lio_propagate): esekf::predict per IMU sample and the closing one.
        imu_state is advanced in place; -> (x, P, poses) with the propagated state and covariance for lio_update and the (k, 22) Pose6D
        rows for lio_frame_begin / lio_frame_begin_cloud / undistort.  The inputs x and P are not changed."""
        a = _imu_rows(imu)
        st = _filter_state(x)
        Pm = np.array(P, np.float64).reshape(23, 23).copy()
        cap = a.shape[0] + 1 if capacity is None else int(capacity)
        poses = np.zeros((max(cap, 1), 22))
        k = C.c_int32()
        self._check(self._L.pcm_lio_propagate(self._h, C.byref(imu_state), a.ctypes.data, a.shape[0], float(t_beg), float(t_end), C.byref(st), Pm.ctypes.data,
                                              poses.ctypes.data, cap, C.byref(k)))
        return _filter_dict(st), Pm, poses[:k.value].copy()

    # -- the frame outputs and the saved map (pcm_lio_frame_world .. pcm_lio_map_export) -----------------------------------------------
    def lio_frame_world(self, rot_xyzw, pos, off_R_xyzw, off_T, dense: bool = False, out=None):
        """PublishFrameWorld's cloud of the current frame (pcm_lio_frame_world; laser_mapping.cc:747-762): (x, y, z, intensity) rows in the
        world frame; dense = every undistorted point, else the down-sampled scan in the order of get_source()."""
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        return self._counted(lambda p, cap, mem, n: self._L.pcm_lio_frame_world(self._h, C.byref(st), int(bool(dense)), p, cap, mem, C.byref(n)), out)

    def lio_frame_body(self, rot_xyzw, pos, off_R_xyzw, off_T, out=None):
        """PublishFrameBody's cloud (pcm_lio_frame_body; :794-808): the undistorted scan in the IMU body frame."""
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        return self._counted(lambda p, cap, mem, n: self._L.pcm_lio_frame_body(self._h, C.byref(st), p, cap, mem, C.byref(n)), out)

    def lio_frame_effect(self, rot_xyzw, pos, off_R_xyzw, off_T, out=None):
        """PublishFrameEffectWorld's cloud (pcm_lio_frame_effect; :810-823): the points that gave a row to the last ObsModel call, in scan
        order, in the world frame, intensity = |z|."""
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        return self._counted(lambda p, cap, mem, n: self._L.pcm_lio_frame_effect(self._h, C.byref(st), p, cap, mem, C.byref(n)), out)

    def lio_map_append(self, rot_xyzw, pos, off_R_xyzw, off_T, dense: bool = False, pcd_save_interval: int = -1) -> dict:
        """`*pcl_wait_save_ += *laserCloudWorld` on the device (pcm_lio_map_append; :776-791) -> lio_map_info(); chunk_ready / pcd_index say
        when the reference would write jueying_<pcd_index>.pcd and clear the cloud (fetch the log, then lio_map_clear)."""
        st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
        info = capi.PcmLioMapInfo()
        self._check(self._L.pcm_lio_map_append(self._h, C.byref(st), int(bool(dense)), int(pcd_save_interval), C.byref(info)))
        return _map_info_dict(info)

    def lio_map_info(self) -> dict:
        info = capi.PcmLioMapInfo()
        self._check(self._L.pcm_lio_map_info_get(self._h, C.byref(info)))
        return _map_info_dict(info)

    def lio_map_get(self, first: int = 0, count: int = None, out=None):
        """Records [first, first + count) of the saved-map log (count None: to its end) as (count, 4) float32 rows, or into `out`."""
        if count is None:
            count = max(self.lio_map_info()["points"] - int(first), 0)
        if out is not None:
            ptr, cap, _, mem, _ = buffer_arg(out, record=16, write=True)
            if cap < count:
                raise ValueError("lio_map_get: the buffer holds %d records, the slice has %d" % (cap, count))
            self._check(self._L.pcm_lio_map_get(self._h, int(first), int(count), C.c_void_p(ptr), mem))
            return int(count)
        res = np.zeros((int(count), 4), np.float32)
        self._check(self._L.pcm_lio_map_get(self._h, int(first), int(count), C.c_void_p(res.ctypes.data), capi.MEM_HOST))
        return res

    def lio_map_clear(self):
        """pcl_wait_save_->clear(); scan_wait_num = 0 (pcm_lio_map_clear)."""
        self._check(self._L.pcm_lio_map_clear(self._h))

    def lio_map_export(self, leaf_size: float = 0.0, z_min: float = 1.0, z_max: float = 0.0, out=None):
        """LaserMapping::Finish's cloud, optionally through pcd2map's filters (pcm_lio_map_export): VoxelGrid of leaf_size (> 0), then
        the records with z_min <= z <= z_max (applied when z_min <= z_max).  Defaults: the log as it is."""
        return self._counted(lambda p, cap, mem, n: self._L.pcm_lio_map_export(self._h, C.c_float(leaf_size), float(z_min), float(z_max), p, cap, mem,
                                                                               C.byref(n)), out)


class LioOdometry:
    """LaserMapping::Run (laser_mapping.cc:301-356) over one Registration (P2PLANE): ImuProcess::Process, the first-scan branch, the
    down-sampled frame, the iterated Kalman update and the map update, every step one of the object's existing calls.
    `propagate(imu_state, imu, t_beg, t_end, x, P) -> (x, P, poses)` defaults to the object's lio_propagate (tests hand in a host
    restatement of the same step)."""
    INIT_TIME = 0.1          # options.h:11
    MIN_POINTS = 5           # laser_mapping.cc:331

    def __init__(self, reg: Registration, imu_state: capi.PcmLioImuState = None, x=None, P=None, filter_size_map: float = 0.5, propagate=None,
                 update_params: dict = None, pcd_save_en: bool = False, dense_pub_en: bool = False, pcd_save_interval: int = -1, **frame_params):
        self.reg = reg
        # the offline branch of Run's last block (laser_mapping.cc:362-365): PublishFrameWorld into the saved map
        self.pcd_save_en = bool(pcd_save_en)
        self.dense_pub_en = bool(dense_pub_en)
        self.pcd_save_interval = int(pcd_save_interval)
        self.chunks = []         # (pcd_index, (n, 4) records) of every jueying_<k>.pcd the reference would have written
        self.imu_state = imu_state if imu_state is not None else lio_imu_state()
        self.x = _filter_dict(_filter_state(x)) if x is not None else _filter_dict(_filter_state([0, 0, 0, 0, 0, 0, 1, 0, 0, 0, 1] + [0] * 12 + [9.809, 0, 0]))
        self.P = np.eye(23) if P is None else np.array(P, np.float64).reshape(23, 23).copy()
        self.filter_size_map = float(filter_size_map)
        self.frame_params = dict(frame_params)
        self.update_params = dict(update_params or {})
        self.propagate = propagate if propagate is not None else reg.lio_propagate
        self.first_scan = True
        self.first_lidar_time = 0.0
        self.ekf_inited = False
        self.last_update = None

    def _pose_args(self):
        return self.x["rot"], self.x["pos"], self.x["off_R"], self.x["off_T"]

    def _frame_begin(self, msg_points, poses, kw) -> int:
        try:
            return self.reg.lio_frame_begin(msg_points, poses, *self._pose_args(), **kw)
        except capi.PcmError as e:
            if e.code != -2:                                   # PCM_ERR_NO_INPUT: "No point, skip this scan!"
                raise
            return 0

    def process(self, msg_points, imu, t_beg: float, t_end: float) -> str:
        """One synchronised package (measures_): the frame's driver message, its IMU samples, lidar_bag_time_ and lidar_end_time_.
        -> what became of it: "no_imu" | "init" | "no_points" | "first_scan" | "too_few_points" | "updated"."""
        if len(imu) == 0:
            return "no_imu"                                    # Process returns on an empty queue; scan_undistort_ stays empty
        if self.imu_state.need_init:
            self.x, self.P = self.reg.lio_imu_init(self.imu_state, imu, self.x, self.P)
            return "init"
        self.x, self.P, poses = self.propagate(self.imu_state, imu, t_beg, t_end, self.x, self.P)
        if self.first_scan:                                    # ivox_->AddPoints(scan_undistort_->points)
            kw = dict(self.frame_params); kw["leaf_size"] = 0.0
            if self._frame_begin(msg_points, poses, kw) == 0:
                return "no_points"
            self.reg.target_insert(self.reg.get_source())
            self.first_lidar_time = float(t_beg)
            self.first_scan = False
            return "first_scan"
        self.ekf_inited = (float(t_beg) - self.first_lidar_time) >= self.INIT_TIME
        n = self._frame_begin(msg_points, poses, self.frame_params)
        if n == 0:
            return "no_points"
        if n < self.MIN_POINTS:
            return "too_few_points"
        self.last_update = self.reg.lio_update(self.x, self.P, **self.update_params)
        self.x, self.P = self.last_update.x, self.last_update.P
        self.reg.lio_frame_end(*self._pose_args(), self.filter_size_map, self.ekf_inited)
        if self.pcd_save_en:                                   # PublishFrameWorld  :363-365, 776-791
            info = self.reg.lio_map_append(*self._pose_args(), dense=self.dense_pub_en, pcd_save_interval=self.pcd_save_interval)
            if info["chunk_ready"]:
                self.chunks.append((info["pcd_index"], self.reg.lio_map_get()))
                self.reg.lio_map_clear()
        return "updated"

    def finish(self, leaf_size: float = 0.0, z_min: float = 1.0, z_max: float = 0.0):
        """LaserMapping::Finish (:887-900): the cloud of jueying.pcd as (n, 4) float32 rows, or None where the reference writes no
        file (pcd_save_en off, or an empty cloud); leaf_size / z_min / z_max: pcd2map's filters on top (lio_map_export)."""
        if not self.pcd_save_en or self.reg.lio_map_info()["points"] == 0:
            return None
        return self.reg.lio_map_export(leaf_size, z_min, z_max)
