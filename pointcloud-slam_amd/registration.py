"""Host-side mirror of the reference's registration operator surface.

Same names, argument meaning and call order as the reference's pybind module
``pygicp`` (/root/reference/src/pointcloud_match/fast_gicp/src/python/main.cpp:135-215:
``set_input_target/source``, ``align``, ``swap_source_and_target``,
``get_final_transformation``, ``get_final_hessian`` ...) and the
``pcl::Registration`` setters it wraps, so the parity tests read like the
reference's gtest (src/test/gicp_test.cpp:147-201).  All compute goes through
the C ABI of include/pcm_amd.h; nothing here touches oracle/.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi


@dataclasses.dataclass
class RegistrationResult:
    T: np.ndarray            # (4,4) float32 final_transformation_
    T64: np.ndarray          # (4,4) float64 pose before the float cast
    H: np.ndarray            # (6,6) final_hessian_
    cost: float
    iterations: int
    converged: bool
    num_linearize: int
    num_compute_error: int
    num_inliers: int
    status: int


def _result(r: capi.PcmResult) -> RegistrationResult:
    return RegistrationResult(np.array(r.T[:], np.float32).reshape(4, 4), np.array(r.T64[:]).reshape(4, 4),
                              np.array(r.H[:]).reshape(6, 6), r.cost, r.iterations, bool(r.converged),
                              r.num_linearize, r.num_compute_error, r.num_inliers, r.status)


def _points(a):
    """Accept (N,>=3) float32 host arrays or torch CUDA tensors; returns (ptr, n, stride, memory, keepalive)."""
    if hasattr(a, "data_ptr") and hasattr(a, "is_cuda"):
        if a.dtype.__str__() != "torch.float32" or a.dim() != 2 or a.shape[1] < 3 or not a.is_contiguous():
            raise ValueError("expected a contiguous (N,>=3) float32 tensor")
        mem = capi.MEM_DEVICE if a.is_cuda else capi.MEM_HOST
        return a.data_ptr(), a.shape[0], a.shape[1] * 4, mem, a
    arr = np.ascontiguousarray(a, dtype=np.float32)
    if arr.ndim != 2 or arr.shape[1] < 3:
        raise ValueError("expected an (N,>=3) float32 array")
    return arr.ctypes.data, arr.shape[0], arr.shape[1] * 4, capi.MEM_HOST, arr


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


class Registration:
    """One registration object bound to a HIP device (= one ``pcm_ctx``)."""

    model = "P2PLANE"
    defaults = {}

    def __init__(self, device: int = 0, model: str = None, **params):
        self._L = capi.load_library()
        cfg = capi.PcmConfig()
        self._L.pcm_default_config(C.byref(cfg))
        if model is not None:
            self.model = model
        cfg.model = capi.MODEL[self.model]
        for k, v in self.defaults.items():
            setattr(cfg, k, v)
        self._cfg = cfg
        self._h = self._L.pcm_create(device, C.byref(cfg))
        if not self._h:
            raise capi.PcmError(-3, "pcm_create failed")
        self._keep = {}
        self._last = None
        self._set(**params)

    # -- plumbing ---------------------------------------------------------
    def _check(self, rc, allow=(capi.PCM_OK,)):
        if rc not in allow:
            raise capi.PcmError(rc, (self._L.pcm_last_error(self._h) or b"").decode())

    def _set(self, **kw):
        for k, v in kw.items():
            if k == "optimizer" and isinstance(v, str):
                v = capi.OPTIMIZER[v]
            if k == "regularization" and isinstance(v, str):
                v = capi.REGULARIZATION[v]
            if not hasattr(self._cfg, k):
                raise KeyError(k)
            setattr(self._cfg, k, v)
        rc = self._L.pcm_set_config(self._h, C.byref(self._cfg))
        if rc != capi.PCM_OK:   # refused (e.g. it would rebuild a shared target): the view follows the object, which is unchanged
            self._L.pcm_get_config(self._h, C.byref(self._cfg))
        self._check(rc)

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.pcm_destroy(h)

    @property
    def handle(self):
        return self._h

    @property
    def config(self):
        """The object's pcm_config (read-only view; change it through the setters)."""
        return self._cfg

    # -- pcl::Registration / LsqRegistration setters ------------------------
    def set_max_iterations(self, n): self._set(max_iterations=int(n))            # setMaximumIterations
    def set_transformation_epsilon(self, e): self._set(translation_eps=float(e))   # setTransformationEpsilon
    def set_rotation_epsilon(self, e): self._set(rotation_eps=float(e))            # lsq_registration_impl.hpp:27-29
    def set_initial_lambda_factor(self, f): self._set(lm_init_lambda_factor=float(f))  # :32-34
    def set_optimizer(self, name): self._set(optimizer=name)                       # lsq_optimizer_type_
    def set_resolution(self, r): self._set(voxel_resolution=float(r))              # fast_vgicp_impl.hpp:28-30
    def set_num_neighbors(self, n): self._set(num_neighbors=int(n))                # setNeighborSearchMethod / ivox_nearby_type

    def set_neighbor_search_method(self, method: str, radius: float = -1.0):
        """pygicp's set_neighbor_search_method (src/python/main.cpp:195-212): DIRECT1 / DIRECT7 / DIRECT27, or DIRECT_RADIUS with the radius in
        voxels for the CUDA-core models."""
        if method == "DIRECT_RADIUS":
            self._set(neighbor_search_radius=float(radius))
        else:
            self._set(neighbor_search_radius=0.0, num_neighbors={"DIRECT1": 1, "DIRECT7": 7, "DIRECT27": 27}[method])

    def set_max_correspondence_distance(self, d): self._set(max_corr_dist=float(d))   # corr_dist_threshold_ (GICP family); the point-to-plane search radius is set_max_range
    def set_max_range(self, r): self._set(max_range=float(r))                        # IVox max_range (ivox3d.h:80)
    def set_num_threads(self, n): pass                                              # setNumThreads: no meaning on the GPU
    def set_stream(self, hip_stream: int): self._check(self._L.pcm_set_stream(self._h, hip_stream))
    def set_profiling(self, flags: int): self._check(self._L.pcm_set_profiling(self._h, int(flags)))

    # -- inputs -------------------------------------------------------------
    def set_input_target(self, cloud, tag: int = 0):
        ptr, n, stride, mem, keep = _points(cloud)
        self._check(self._L.pcm_set_target(self._h, ptr, n, stride, mem, tag))

    def set_input_source(self, cloud, tag: int = 0):
        ptr, n, stride, mem, keep = _points(cloud)
        self._check(self._L.pcm_set_source(self._h, ptr, n, stride, mem, tag))

    def swap_source_and_target(self): self._check(self._L.pcm_swap_source_and_target(self._h))
    def clear_source(self): self._check(self._L.pcm_clear_source(self._h))
    def clear_target(self): self._check(self._L.pcm_clear_target(self._h))

    def share_target(self, other: "Registration"):
        """Register against the target ``other`` holds from now on (pcm_share_target): the cloud, its voxel map and everything the
        model derives from them exist once on the device, however many objects hold them -- what the reference's objects get from
        one PointCloud::ConstPtr.  Both objects are of one model on one device and agree in the settings that decide how a target
        is built (the error names the first that differs).  While more than one object holds the target nothing may change it
        (target_insert, map_incremental, lio_frame_end, set_covariances(target=True), swap_source_and_target and such setters raise);
        set_input_target / clear_target / deleting an object detach that object only."""
        self._check(self._L.pcm_share_target(self._h, other._h))

    @property
    def target_share_count(self) -> int:
        """Objects holding this object's target (1 = not shared)."""
        n = self._L.pcm_target_share_count(self._h)
        if n < 0:
            self._check(n)
        return n

    # -- compute ------------------------------------------------------------
    def align(self, initial_guess=None) -> RegistrationResult:
        g = np.eye(4, dtype=np.float32) if initial_guess is None else np.ascontiguousarray(initial_guess, dtype=np.float32)
        res = capi.PcmResult()
        self._check(self._L.pcm_align(self._h, g.ctypes.data, C.byref(res)), allow=(capi.PCM_OK, capi.PCM_ERR_NOT_CONVERGED))
        self._last = _result(res)
        return self._last

    def evaluate_cost(self, T):
        """LsqRegistration::evaluateCost -> (cost, H, b, num_inliers)  (lsq_registration_impl.hpp:46-49)."""
        T = np.ascontiguousarray(T, dtype=np.float64)
        H = np.zeros((6, 6)); b = np.zeros(6)
        cost = C.c_double(); inl = C.c_int32()
        self._check(self._L.pcm_linearize(self._h, T.ctypes.data, H.ctypes.data, b.ctypes.data, C.byref(cost), C.byref(inl)))
        return cost.value, H, b, inl.value

    linearize = evaluate_cost

    def compute_error(self, T) -> float:
        T = np.ascontiguousarray(T, dtype=np.float64)
        cost = C.c_double()
        self._check(self._L.pcm_compute_error(self._h, T.ctypes.data, C.byref(cost)))
        return cost.value

    def obs_model(self, rot_xyzw, pos, off_R_xyzw, off_T, extrinsic_est_en=False, converge=True):
        """jueying_lio's ObsModel + the IEKF reduction (pcm_obs_model):
        returns (HTH 12x12, HTh 12, n_eff, sum_h2, valid)."""
        st = capi.PcmLioState()
        st.rot[:] = list(rot_xyzw); st.pos[:] = list(pos); st.off_R[:] = list(off_R_xyzw); st.off_T[:] = list(off_T)
        out = capi.PcmObsResult()
        self._check(self._L.pcm_obs_model(self._h, C.byref(st), int(extrinsic_est_en), int(converge), C.byref(out)))
        return np.array(out.HTH[:]).reshape(12, 12), np.array(out.HTh[:]), out.n_eff, out.sum_h2, bool(out.valid)

    def get_lio_members(self, n: int):
        """(residuals_, point_selected_surf_) as the last obs_model left them (reference-semantics mode only)."""
        res = np.zeros(n, np.float32); sel = np.zeros(n, np.uint8)
        self._check(self._L.pcm_get_lio_members(self._h, res.ctypes.data, sel.ctypes.data, n))
        return res, sel.astype(bool)

    def target_insert(self, cloud):
        """IVox::AddPoints: append points to the sliding submap (LRU beyond map_capacity voxels)."""
        ptr, n, stride, mem, keep = _points(cloud)
        self._check(self._L.pcm_target_insert(self._h, ptr, n, stride, mem))

    def map_incremental(self, rot_xyzw, pos, off_R_xyzw, off_T, filter_size_map: float, ekf_inited: bool = True) -> int:
        """LaserMapping::MapIncremental with the add-filter; returns the number of points inserted."""
        st = capi.PcmLioState()
        st.rot[:] = list(rot_xyzw); st.pos[:] = list(pos); st.off_R[:] = list(off_R_xyzw); st.off_T[:] = list(off_T)
        n = C.c_size_t()
        self._check(self._L.pcm_map_incremental(self._h, C.byref(st), C.c_float(filter_size_map), int(ekf_inited), C.byref(n)))
        return n.value

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
        st = capi.PcmLioState()
        st.rot[:] = list(map(float, rot_xyzw)); st.pos[:] = list(map(float, pos)); st.off_R[:] = list(map(float, off_R_xyzw)); st.off_T[:] = list(map(float, off_T))
        pp, npose = None, 0
        if poses is not None:
            pa = np.ascontiguousarray(poses, dtype=np.float64)
            assert pa.ndim == 2 and pa.shape[1] == 22
            pp, npose = pa.ctypes.data, pa.shape[0]
        m = C.c_size_t()
        self._check(self._L.pcm_lio_frame_begin(self._h, C.c_void_p(ptr), C.c_size_t(n), mem, C.byref(prm), C.c_void_p(pp), int(npose), C.byref(st), C.byref(m)))
        return m.value

    def lio_frame_end(self, rot_xyzw, pos, off_R_xyzw, off_T, filter_size_map: float, ekf_inited: bool = True) -> int:
        """Back end of the frame (pcm_lio_frame_end = MapIncremental with the updated state); returns the points inserted."""
        return self.map_incremental(rot_xyzw, pos, off_R_xyzw, off_T, filter_size_map, ekf_inited)

    LIO_STATE_FIELDS = (("pos", 3), ("rot", 4), ("off_R", 4), ("off_T", 3), ("vel", 3), ("bg", 3), ("ba", 3), ("grav", 3))

    def lio_update(self, x, P, R: float = None, max_iter: int = None, extrinsic_est_en: bool = False, limit=None) -> "LioUpdateResult":
        """jueying_lio's iterated Kalman update (esekf::update_iterated_dyn_share_modified) on the device: pcm_lio_update.
        x: the propagated state_ikfom as a dict of pos(3) rot(4: x,y,z,w) off_R(4) off_T(3) vel(3) bg(3) ba(3) grav(3), or the 26 numbers
        in that order; P: 23 x 23 covariance.  One call per frame between lio_frame_begin and lio_frame_end; the inputs are not changed.
        Parameters default to the reference's (R 0.001, max_iter 4, limit 0.001 each)."""
        st = capi.PcmLioFilterState()
        if isinstance(x, dict):
            for k, _ in self.LIO_STATE_FIELDS:
                getattr(st, k)[:] = [float(v) for v in x[k]]
        else:
            v = np.ascontiguousarray(x, np.float64).reshape(26)
            C.memmove(C.byref(st), v.ctypes.data, 26 * 8)
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
        xo = {k: np.array(getattr(st, k)[:]) for k, _ in self.LIO_STATE_FIELDS}
        return LioUpdateResult(x=xo, P=Pm, iterations=res.iterations, rematches=res.rematches, valid_calls=res.valid_calls, t=res.t,
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
        return dict(x={k: np.array(getattr(st, k)[:]) for k, _ in self.LIO_STATE_FIELDS}, converge=bool(cv.value), n_eff=ne.value, HTH=HTH,
                    HTh=sums[78:90].copy(), dx_=dx)

    def get_source(self) -> np.ndarray:
        n = C.c_size_t()
        self._check(self._L.pcm_get_source(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), np.float32)
        if n.value:
            self._check(self._L.pcm_get_source(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def ndt_derivatives(self, p, hessian="float"):
        """pclomp NDT: (score, gradient, Hessian) at the pose vector p = (x, y, z, roll, pitch, yaw)
        (computeDerivatives, ndt_omp_impl.hpp:168-267); hessian = "float" | None | "double" (computeHessian :498-559)."""
        p = np.ascontiguousarray(p, dtype=np.float64)
        g = np.zeros(6); H = np.zeros((6, 6)); score = C.c_double()
        mode = {"float": 0, None: 1, "double": 2}[hessian]
        self._check(self._L.pcm_ndt_derivatives(self._h, p.ctypes.data, mode, C.byref(score), g.ctypes.data, H.ctypes.data))
        return score.value, g, H

    def ndt_score(self, T) -> float:
        """pclomp NDT calculateScore of the source transformed by T (ndt_omp_impl.hpp:835-880)."""
        T = np.ascontiguousarray(T, dtype=np.float32)
        s = C.c_double()
        self._check(self._L.pcm_ndt_score(self._h, T.ctypes.data, C.byref(s)))
        return s.value

    def get_covariances(self, target: bool = False) -> np.ndarray:
        """(N,3,3) regularised covariances of the source (or target) cloud, input order
        (FastGICP::getSourceCovariances / getTargetCovariances, fast_gicp.hpp:64-70)."""
        n = C.c_size_t()
        self._check(self._L.pcm_get_covariances(self._h, int(bool(target)), None, 0, C.byref(n)))
        out = np.zeros((n.value, 3, 3), np.float64)
        if n.value:
            self._check(self._L.pcm_get_covariances(self._h, int(bool(target)), out.ctypes.data, n.value, C.byref(n)))
        return out

    def set_covariances(self, covs, target: bool = False):
        """setSourceCovariances / setTargetCovariances (fast_gicp_impl.hpp:93-100): (N,3,3) or (N,4,4) float64, input order."""
        a = np.ascontiguousarray(covs, np.float64)
        elems = a.shape[1] * a.shape[2]
        self._check(self._L.pcm_set_covariances(self._h, int(bool(target)), a.ctypes.data, a.shape[0], elems))

    def set_correspondence_randomness(self, k): self._set(k_correspondences=int(k))   # setCorrespondenceRandomness  fast_gicp_impl.hpp:61-63
    def set_regularization_method(self, m): self._set(regularization=m)               # setRegularizationMethod      :66-68

    def undistort(self, points, time_index, poses, rot_xyzw, pos, off_R_xyzw, off_T):
        """Motion compensation of a scan into its frame-end pose, in place (ImuProcess::UndistortPcl's backward propagation,
        jueying_lio/include/imu_processing.hpp:245-285).  points: (N,F) float32 (x,y,z first, time [ms] in column time_index,
        sorted by time); poses: (K,22) float64 rows = Pose6D (offset_time, acc, gyr, vel, pos, rot row-major)."""
        assert points.dtype == np.float32 and points.flags["C_CONTIGUOUS"] and points.ndim == 2
        poses = np.ascontiguousarray(poses, dtype=np.float64)
        assert poses.ndim == 2 and poses.shape[1] == 22
        st = capi.PcmLioState()
        st.rot[:] = list(map(float, rot_xyzw)); st.pos[:] = list(map(float, pos))
        st.off_R[:] = list(map(float, off_R_xyzw)); st.off_T[:] = list(map(float, off_T))
        self._check(self._L.pcm_undistort(self._h, points.ctypes.data, points.shape[0], points.strides[0], 4 * int(time_index), capi.MEM_HOST,
                                          poses.ctypes.data, poses.shape[0], C.byref(st)))
        return points

    def voxel_downsample(self, points, leaf_size) -> np.ndarray:
        """pcl::VoxelGrid down-sampling of an (N,F) float32 scan -> (M,F) centroids in leaf-index order
        (voxel_scan_.filter(), jueying_lio/src/laser_mapping.cc:323-328)."""
        points = np.ascontiguousarray(points, dtype=np.float32)
        out = np.zeros_like(points)
        m = C.c_size_t()
        self._check(self._L.pcm_voxel_downsample(self._h, points.ctypes.data, points.shape[0], points.strides[0], capi.MEM_HOST, float(leaf_size),
                                                 out.ctypes.data, out.shape[0], C.byref(m)))
        return out[:m.value].copy()

    def gicp_bfgs_set_correspondences(self, src, tgt, idx_src, idx_tgt, mahalanobis):
        """Pack the correspondence set of one outer GICP-BFGS iteration (pclomp gicp_omp_impl.hpp:199-203): src/tgt (N,F) float32
        clouds (x y z first), index pairs, mahalanobis_ as (N_src,16) float32 (column-major Matrix4f per source point)."""
        src = np.ascontiguousarray(src, np.float32); tgt = np.ascontiguousarray(tgt, np.float32)
        if src.ndim != 2 or tgt.ndim != 2 or src.shape[1] != tgt.shape[1] or src.shape[1] < 3:
            raise ValueError("src/tgt: (N,F>=3) float32 with equal record sizes")
        idx_src = np.ascontiguousarray(idx_src, np.int32); idx_tgt = np.ascontiguousarray(idx_tgt, np.int32)
        maha = np.ascontiguousarray(mahalanobis, np.float32).reshape(-1, 16)
        if len(idx_src) != len(idx_tgt) or maha.shape[0] != src.shape[0]:
            raise ValueError("one index pair per correspondence, one Mahalanobis matrix per source point")
        self._check(self._L.pcm_gicp_bfgs_set_correspondences(self._h, src.ctypes.data, src.shape[0], tgt.ctypes.data, tgt.shape[0], src.strides[0],
                                                               idx_src.ctypes.data, idx_tgt.ctypes.data, len(idx_src), maha.ctypes.data, capi.MEM_HOST))

    def gicp_bfgs_fdf(self, base_T, x, mode: int = 2):
        """(f, g) of pclomp's OptimizationFunctorWithIndices at x (gicp_omp_impl.hpp:246-365); mode 0 = operator(), 1 = df, 2 = fdf."""
        base = np.ascontiguousarray(base_T, np.float32).reshape(16); xx = np.ascontiguousarray(x, np.float64).reshape(6)
        f = C.c_double(float("nan")); g = np.full(6, np.nan)
        self._check(self._L.pcm_gicp_bfgs_fdf(self._h, base.ctypes.data, xx.ctypes.data, int(mode), C.byref(f), g.ctypes.data))
        return f.value, g

    def gicp_bfgs_update_correspondences(self, transformation, guess) -> int:
        """pclomp GICP's correspondence step on the device (gicp_omp_impl.hpp:405-472); the pairs become the functor's record set."""
        T = np.ascontiguousarray(transformation, np.float32).reshape(16); G = np.ascontiguousarray(guess, np.float32).reshape(16)
        m = C.c_size_t()
        self._check(self._L.pcm_gicp_bfgs_update_correspondences(self._h, T.ctypes.data, G.ctypes.data, C.byref(m)))
        self._bfgs_m = m.value
        return m.value

    def gicp_bfgs_get_correspondences(self):
        """(idx_src, idx_tgt, mahalanobis (m,3,3) float32) of the last device-side correspondence step."""
        m = self._bfgs_m
        isrc = np.zeros(m, np.int32); itgt = np.zeros(m, np.int32); M = np.zeros((m, 9), np.float32)
        self._check(self._L.pcm_gicp_bfgs_get_correspondences(self._h, isrc.ctypes.data, itgt.ctypes.data, M.ctypes.data, m))
        return isrc, itgt, M.reshape(-1, 3, 3)

    def livox_filter(self, msg_points, num_scans: int = 6, point_filter_num: int = 1, blind: float = 0.01) -> np.ndarray:
        """PointCloudPreprocess::AviaHandler (pointcloud_preprocess.cc:44-88): livox CustomPoint records (20-byte structured array:
        offset_time u4, x y z f4, reflectivity tag line u1, pad) -> (m, 12) float32 pcl::PointXYZINormal records in input order."""
        a = np.ascontiguousarray(msg_points)
        assert a.dtype.itemsize == 20
        out = np.zeros((max(len(a), 1), 12), np.float32)
        m = C.c_size_t()
        self._check(self._L.pcm_livox_filter(self._h, a.ctypes.data, len(a), capi.MEM_HOST, int(num_scans), int(point_filter_num), float(blind), out.ctypes.data, len(out), C.byref(m)))
        return out[:m.value].copy()

    def get_target(self) -> np.ndarray:
        """(M,3) current target points in insertion order."""
        n = C.c_size_t()
        self._check(self._L.pcm_get_target(self._h, None, 0, C.byref(n)))
        out = np.zeros((n.value, 3), np.float32)
        if n.value:
            self._check(self._L.pcm_get_target(self._h, out.ctypes.data, n.value, C.byref(n)))
        return out

    def get_neighbour_lists(self):
        """The target's per-voxel candidate lists as the device holds them (pcm_get_neighbour_lists): the list voxels' centres (L,3),
        the starts (L+1,) and the entries as xyz (E,3) and point index (E,) -- a pad entry is +inf with index 0xffffffff."""
        info = np.zeros(2, np.uint64)
        self._check(self._L.pcm_get_neighbour_lists(self._h, info.ctypes.data, None, None, None))
        nl, ne = int(info[0]), int(info[1])
        centres, starts, entries = np.zeros((nl, 4), np.float32), np.zeros(nl + 1, np.uint32), np.zeros((ne, 4), np.float32)
        self._check(self._L.pcm_get_neighbour_lists(self._h, info.ctypes.data, centres.ctypes.data, starts.ctypes.data, entries.ctypes.data))
        return centres[:, :3].copy(), starts, entries[:, :3].copy(), entries[:, 3].copy().view(np.uint32)

    following_lists = capi.PCM_FLAG_FOLLOWING_LISTS   # flags=...: candidate lists that follow a growing P2PLANE target

    def neighbour_list_info(self) -> dict:
        """The candidate lists the linearize pass reads (pcm_neighbour_list_info); all zero without lists.  For following lists:
        the pool's wasted entries, the updates since the last full build, and -- since the lists were first built -- the runs
        rewritten in place, the runs relocated and the full builds the pool's policy asked for."""
        info = np.zeros(8, np.uint64)
        self._check(self._L.pcm_neighbour_list_info(self._h, info.ctypes.data))
        names = ("lists", "live_entries", "capacity", "wasted_entries", "updates", "in_place", "relocated", "rebuilds")
        return {k: int(v) for k, v in zip(names, info)}

    def lio_search_path(self) -> tuple:
        """(lists, tile): matching ObsModel launches (obs_model with rematch, the matching rounds of lio_update) served by the lists
        kernel and by the tile kernel since the context was made or reset_stats (pcm_lio_search_path)."""
        n = np.zeros(2, np.uint64)
        self._check(self._L.pcm_lio_search_path(self._h, n.ctypes.data))
        return int(n[0]), int(n[1])

    def neighbour_list_update_ms(self) -> dict:
        """Device time of the last following-lists update timed under set_profiling(1) (pcm_neighbour_list_update_ms), by stage."""
        ms = np.zeros(5)
        self._check(self._L.pcm_neighbour_list_update_ms(self._h, ms.ctypes.data))
        return dict(zip(("dirty_lists", "classify", "rewrite", "index_merge", "total"), (float(v) for v in ms)))

    def set_neighbour_list_headroom(self, fraction: float, min_entries: int):
        """Room a full build of following lists reserves behind the runs: max(fraction * entries, min_entries) entries
        (pcm_neighbour_list_headroom; default one and a half times the entries, at least 65536)."""
        self._check(self._L.pcm_neighbour_list_headroom(self._h, C.c_float(fraction), int(min_entries)))

    def get_planes(self, n: int) -> np.ndarray:
        """(n,4) planes fitted by the last evaluate_cost (NaN row = point not selected)."""
        out = np.zeros((n, 4), np.float32)
        self._check(self._L.pcm_get_planes(self._h, out.ctypes.data, n))
        return out

    def get_fitness_score(self, max_range: float = float(np.finfo(np.float64).max), T=None) -> float:
        """pcl::Registration::getFitnessScore(max_range) (pygicp get_fitness_score, main.cpp:169-215): mean squared distance of
        the source points under the final transformation (or T) to their exact nearest target points, on the device."""
        if T is None:
            T = self._last.T
        T = np.ascontiguousarray(T, dtype=np.float32)
        s = C.c_double()
        self._check(self._L.pcm_fitness_score(self._h, T.ctypes.data, float(max_range), C.byref(s)))
        return s.value

    def get_final_transformation(self): return self._last.T
    def get_final_hessian(self): return self._last.H
    def has_converged(self): return self._last.converged

    def stats(self) -> dict:
        s = capi.PcmStats()
        self._check(self._L.pcm_get_stats(self._h, C.byref(s)))
        return {k: getattr(s, k) for k, _ in capi.PcmStats._fields_ if k != "reserved"}

    def phase_cycles(self):
        out = (C.c_uint64 * 8)()
        self._check(self._L.pcm_debug_phase_cycles(self._h, out))
        return list(out)

    def reset_stats(self): self._check(self._L.pcm_reset_stats(self._h))


class P2PlaneRegistration(Registration):
    """Point-to-plane scan-to-submap ICP with jueying_lio's matcher semantics
    (5-NN in the voxel hash -> plane fit -> n.p+d; laser_mapping.cc:592-701)
    under fast_gicp's GN/LM loop."""
    model = "P2PLANE"


class GicpRegistration(Registration):
    """Generalized ICP with FastGICP's semantics (fast_gicp/include/fast_gicp/gicp/impl/fast_gicp_impl.hpp):
    20-NN covariances regularised to planes, exact nearest-neighbour correspondences, distribution-to-
    distribution cost in double.  ``voxel_resolution`` only sizes the search grid (results do not depend on it)."""
    model = "GICP"
    defaults = {"voxel_resolution": 0.5}


class VgicpRegistration(Registration):
    """Voxelized GICP with FastVGICP's CPU semantics (impl/fast_vgicp_impl.hpp, fast_vgicp_voxel.hpp):
    additive voxel distributions at resolution 1.0, DIRECT1 neighbourhood by default (:22-25)."""
    model = "VGICP"
    defaults = {"voxel_resolution": 1.0, "num_neighbors": 1}


class PclNdtRegistration(Registration):
    """pclomp::NormalDistributionsTransform (pointcloud_match/ndt_omp/include/pclomp/ndt_omp_impl.hpp):
    Newton step with the analytic Hessian + More-Thuente line search on VoxelGridCovariance leaves;
    defaults of that class: resolution 1.0, step 0.1, outlier ratio 0.55, epsilon 0.1, 35 iterations, DIRECT7 (:48,60-63).
    ``num_neighbors``: 0 = KDTREE (radius search over the leaf centroids), 1 / 7 / 27 = DIRECT1 / DIRECT7 / DIRECT26."""
    model = "NDT_OMP"
    defaults = {"voxel_resolution": 1.0, "num_neighbors": 7, "max_iterations": 35, "translation_eps": 0.1}

    def set_step_size(self, s): self._set(ndt_step_size=float(s))                  # setStepSize       ndt_omp.h
    def set_outlier_ratio(self, r): self._set(ndt_outlier_ratio=float(r))          # setOutlierRatio   ndt_omp.h:188


class VgicpCudaRegistration(Registration):
    """FastVGICPCuda's float core (fast_gicp/src/fast_gicp/cuda/*.cu behind impl/fast_vgicp_cuda_impl.hpp): float 20-NN
    covariances and voxel distributions, D2D cost with w = sqrt(n); resolution 1.0, DIRECT1, PLANE (:24-27)."""
    model = "VGICP_CUDA"
    defaults = {"voxel_resolution": 1.0, "num_neighbors": 1}

    def set_nearest_neighbor_search_method(self, method: str):
        """setNearestNeighborSearchMethod (fast_vgicp_cuda_impl.hpp:64-66): "CPU_PARALLEL_KDTREE" / "GPU_BRUTEFORCE" (exact kNN
        covariances) or "GPU_RBF_KERNEL" (cuda/covariance_estimation_rbf.cu)."""
        self._set(covariance_method=1 if method == "GPU_RBF_KERNEL" else 0)

    def set_kernel_width(self, kernel_width: float, max_dist: float = -1.0):
        """setKernelWidth (fast_vgicp_cuda_impl.hpp:46-52): max_dist defaults to 5 x kernel_width."""
        self._set(rbf_kernel_width=float(kernel_width), rbf_max_dist=float(kernel_width * 5.0 if max_dist <= 0 else max_dist))


class NdtRegistration(Registration):
    """NDT on Gaussian voxels with the reference NDTCuda's semantics
    (fast_gicp/include/fast_gicp/ndt/ndt_cuda.hpp:21-71, src/fast_gicp/cuda/ndt_cuda.cu):
    D2D distance mode, DIRECT7 neighbourhood and resolution 1.0 by default (ndt_cuda.cu:15-22)."""
    model = "NDT_D2D"
    defaults = {"voxel_resolution": 1.0, "num_neighbors": 7}

    def set_distance_mode(self, mode: str):      # setDistanceMode(NDTDistanceMode)
        self._set(model=capi.MODEL["NDT_" + mode.upper()])


def align_batch(regs, guesses, device_out=None):
    """Align a batch of independent registration objects in lock-step launches
    (pcm_align_batch).  ``device_out``: optional device pointer (int) receiving
    the packed ``pcm_result`` records, e.g. a tensor handed to an RCCL gather."""
    L = capi.load_library()
    n = len(regs)
    g = np.ascontiguousarray(guesses, dtype=np.float32).reshape(n, 16)
    arr = (C.c_void_p * n)(*[r.handle for r in regs])
    out = (capi.PcmResult * n)()
    rc = L.pcm_align_batch(arr, n, g.ctypes.data, out, device_out)
    if rc not in (capi.PCM_OK, capi.PCM_ERR_NOT_CONVERGED):
        raise capi.PcmError(rc, (L.pcm_last_error(regs[0].handle) or b"").decode())
    res = [_result(out[i]) for i in range(n)]
    for r, x in zip(regs, res):
        r._last = x
    return res


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


def _loam_params(L, params: dict) -> capi.PcmLoamParams:
    p = capi.PcmLoamParams()
    L.pcm_loam_default_params(C.byref(p))
    for k, v in params.items():
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


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


class LoamRegistration:
    """jueying_slam's LOAM edge / plane scan-to-map optimisation on one HIP device (a PCM_MODEL_LOAM ``pcm_ctx``).

    ``set_input_target(corner_map, surf_map)`` = laserCloudCornerFromMapDS / laserCloudSurfFromMapDS,
    ``set_input_source(corner, surf)`` = laserCloudCornerLastDS / laserCloudSurfLastDS (body frame),
    ``scan2map(x6)`` = scan2MapOptimization from transformTobeMapped = x6 (roll, pitch, yaw, x, y, z)."""

    def __init__(self, device: int = 0, **params):
        self._L = capi.load_library()
        cfg = capi.PcmConfig()
        self._L.pcm_default_config(C.byref(cfg))
        cfg.model = capi.MODEL["LOAM"]
        self._h = self._L.pcm_create(device, C.byref(cfg))
        if not self._h:
            raise capi.PcmError(-3, "pcm_create failed")
        self.params = dict(params)
        _loam_params(self._L, self.params)   # unknown names fail here
        self.n_corner = self.n_surf = 0

    def _check(self, rc, allow=(capi.PCM_OK,)):
        if rc not in allow:
            raise capi.PcmError(rc, (self._L.pcm_last_error(self._h) or b"").decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.pcm_destroy(h)

    @property
    def handle(self):
        return self._h

    def set_input_target(self, corner, surf, tag: int = 0):
        c, s = _feature_pair(corner, surf)
        self._check(self._L.pcm_loam_set_target(self._h, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], 16, capi.MEM_HOST, tag))

    def set_input_source(self, corner, surf, tag: int = 0):
        c, s = _feature_pair(corner, surf)
        self._check(self._L.pcm_loam_set_source(self._h, c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], 16, capi.MEM_HOST, tag))
        self.n_corner, self.n_surf = c.shape[0], s.shape[0]

    def scan2map(self, x6, **params) -> LoamResult:
        p = _loam_params(self._L, {**self.params, **params})
        x = np.ascontiguousarray(x6, dtype=np.float32).reshape(6)
        r = capi.PcmLoamResult()
        self._check(self._L.pcm_loam_align(self._h, C.byref(p), x.ctypes.data, C.byref(r)), (capi.PCM_OK, capi.PCM_ERR_TOO_FEW_FEATURES))
        return _loam_result(r)

    def coefficients(self, x6):
        """Parity hook at a fixed pose: (corner (Nc,4), surf (Ns,4)) coefficients (coeff.xyz, intensity; NaN = not selected),
        A^T A (6,6), A^T b (6,), counts (selected corner, selected surf, corner / surf features with sqDis[0] <= 1)."""
        x = np.ascontiguousarray(x6, dtype=np.float32).reshape(6)
        co = np.zeros((self.n_corner, 4), np.float32)
        su = np.zeros((self.n_surf, 4), np.float32)
        AtA = np.zeros((6, 6))
        AtB = np.zeros(6)
        cnt = np.zeros(4, np.int32)
        self._check(self._L.pcm_loam_coefficients(self._h, x.ctypes.data, co.ctypes.data, su.ctypes.data, AtA.ctypes.data, AtB.ctypes.data, cnt.ctypes.data))
        return co, su, AtA, AtB, cnt

    def neighbours(self, x6):
        """Parity hook: the 5 nearest map indices with d^2 <= 1 (ascending (d^2, index), -1 pads) of every corner / surf feature."""
        x = np.ascontiguousarray(x6, dtype=np.float32).reshape(6)
        cn = np.zeros((self.n_corner, 5), np.int32)
        sn = np.zeros((self.n_surf, 5), np.int32)
        self._check(self._L.pcm_loam_neighbours(self._h, x.ctypes.data, cn.ctypes.data, sn.ctypes.data))
        return cn, sn


def loam_align_batch(regs, x6s, **params):
    """scan2MapOptimization of independent LoamRegistration objects in lock-step launches (pcm_loam_align_batch)."""
    L = capi.load_library()
    n = len(regs)
    p = _loam_params(L, {**regs[0].params, **params})
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


def _scan_arg(cloud, stride):
    """(pointer, n, memory, keep-alive) of ring-tagged records: a host array or a device tensor of n x stride bytes."""
    if hasattr(cloud, "data_ptr") and getattr(cloud, "is_cuda", False):
        if not cloud.is_contiguous():
            raise ValueError("device scans must be contiguous")
        nbytes = cloud.numel() * cloud.element_size()
        if nbytes % stride:
            raise ValueError("device scan size is not a multiple of the record stride")
        return cloud.data_ptr(), nbytes // stride, capi.MEM_DEVICE, cloud
    a = np.ascontiguousarray(cloud)
    if a.nbytes % stride:
        raise ValueError("scan size is not a multiple of the record stride")
    return a.ctypes.data, a.nbytes // stride, capi.MEM_HOST, a


def _feature_params(L, params: dict) -> capi.PcmLoamFeatureParams:
    p = capi.PcmLoamFeatureParams()
    L.pcm_loam_default_feature_params(C.byref(p))
    for k, v in params.items():
        if k == "force_serial_sort":
            p.flags = (p.flags | capi.PCM_LOAM_FEATURES_FORCE_SERIAL_SORT) if v else (p.flags & ~capi.PCM_LOAM_FEATURES_FORCE_SERIAL_SORT)
            continue
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


_FEATURE_LAYOUT = ("stride", "intensity_offset", "ring_offset")


def _split_layout(params: dict):
    lay = (params.pop("stride", XYZIRT_STRIDE), params.pop("intensity_offset", XYZIRT_INTENSITY), params.pop("ring_offset", XYZIRT_RING))
    return lay, params


def _features_result(r: capi.PcmLoamFeaturesResult) -> dict:
    return {k: getattr(r, k) for k, _ in r._fields_ if k != "reserved"}


def _loam_set_input_scan(self, cloud, **feature_params) -> dict:
    """featureExtraction + downsampleCurrentScan of one ring-tagged scan into this context's LOAM source, on the device
    (pcm_loam_frame_begin).  Then ``scan2map`` as after ``set_input_source``."""
    (stride, ioff, roff), fp = _split_layout(dict(feature_params))
    p = _feature_params(self._L, fp)
    ptr, n, mem, keep = _scan_arg(cloud, stride)
    r = capi.PcmLoamFeaturesResult()
    self._check(self._L.pcm_loam_frame_begin(self._h, ptr, n, stride, ioff, roff, mem, C.byref(p), C.byref(r)))
    del keep
    self.n_corner, self.n_surf = r.num_corner, r.num_surf
    return _features_result(r)


def _loam_feature_info(self) -> dict:
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


LoamRegistration.set_input_scan = _loam_set_input_scan
LoamRegistration.feature_info = _loam_feature_info


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


def _submap_params(L, params: dict) -> capi.PcmLoamSubmapParams:
    p = capi.PcmLoamSubmapParams()
    L.pcm_loam_default_submap_params(C.byref(p))
    for k, v in params.items():
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _xyzi(a):
    a = np.asarray(a, dtype=np.float32)
    if a.ndim != 2 or a.shape[1] < 3:
        raise ValueError("expected an (N,>=3) float32 array")
    b = np.zeros((a.shape[0], 4), np.float32)
    b[:, :min(4, a.shape[1])] = a[:, :4]
    return b


def _cloud_buffer(out):
    """(pointer, capacity, memory) of a contiguous (cap, 4) float32 device tensor or host array."""
    if hasattr(out, "data_ptr") and getattr(out, "is_cuda", False):
        if out.dim() != 2 or out.shape[1] != 4 or not out.is_contiguous() or out.element_size() != 4:
            raise ValueError("expected a contiguous (cap, 4) float32 device tensor")
        return out.data_ptr(), out.shape[0], capi.MEM_DEVICE
    if not isinstance(out, np.ndarray) or out.dtype != np.float32 or out.ndim != 2 or out.shape[1] != 4 or not out.flags.c_contiguous:
        raise ValueError("expected a contiguous (cap, 4) float32 array or device tensor")
    return out.ctypes.data, out.shape[0], capi.MEM_HOST


def _loam_add_keyframe(self, pose6, time, corner=None, surf=None) -> int:
    """saveKeyFramesAndFactor: a key frame with pose6 (roll, pitch, yaw, x, y, z), its time and its (N,4) x y z intensity clouds in
    the body frame.  Without clouds the context's current LOAM source is copied on the device.  Returns the key frame's index."""
    x = np.ascontiguousarray(pose6, dtype=np.float32).reshape(6)
    if (corner is None) != (surf is None):
        raise ValueError("pass both clouds or neither")
    if corner is None:
        self._check(self._L.pcm_loam_keyframe_add(self._h, x.ctypes.data, float(time), None, 0, None, 0, 16, capi.MEM_HOST))
    else:
        c, s = _xyzi(corner), _xyzi(surf)
        self._check(self._L.pcm_loam_keyframe_add(self._h, x.ctypes.data, float(time), c.ctypes.data, c.shape[0], s.ctypes.data, s.shape[0], 16, capi.MEM_HOST))
    return self.num_keyframes - 1


def _loam_set_keyframe_poses(self, poses, first: int = 0):
    """correctPoses: new (n,6) poses for key frames first .. first + n - 1."""
    x = np.ascontiguousarray(poses, dtype=np.float32).reshape(-1, 6)
    self._check(self._L.pcm_loam_keyframe_set_poses(self._h, int(first), x.shape[0], x.ctypes.data))


def _loam_num_keyframes(self) -> int:
    n = self._L.pcm_loam_keyframe_count(self._h)
    if n < 0:
        self._check(n)
    return n


def _loam_clear_keyframes(self):
    self._check(self._L.pcm_loam_keyframe_clear(self._h))


def _loam_get_keyframe(self, key: int):
    """(corner (Nc,4), surf (Ns,4)) of one stored key frame: body frame, x y z intensity."""
    nc, ns = C.c_size_t(0), C.c_size_t(0)
    self._check(self._L.pcm_loam_keyframe_get(self._h, int(key), None, 0, None, 0, C.byref(nc), C.byref(ns)))
    co = np.zeros((nc.value, 4), np.float32)
    su = np.zeros((ns.value, 4), np.float32)
    self._check(self._L.pcm_loam_keyframe_get(self._h, int(key), co.ctypes.data, nc.value, su.ctypes.data, ns.value, C.byref(nc), C.byref(ns)))
    return co, su


def _loam_update_submap(self, time_cur, **params) -> LoamSubmapResult:
    """extractSurroundingKeyFrames at timeLaserInfoCur = time_cur: the down-sampled corner / surf submap of the surrounding key
    frames becomes this context's target (pcm_loam_submap_update)."""
    p = _submap_params(self._L, params)
    r = capi.PcmLoamSubmapResult()
    self._check(self._L.pcm_loam_submap_update(self._h, C.byref(p), float(time_cur), C.byref(r)))
    self._submap = r
    return LoamSubmapResult(r.num_keyframes, r.num_near, r.num_pose_leaves, r.num_selected, r.num_skipped, r.num_corner_in, r.num_surf_in,
                            r.num_corner_map, r.num_surf_map, bool(r.rebuilt), r.status)


def _loam_near_keyframes(self, key: int, search_num: int, wrt_key: int = -1, leaf: float = 0.2) -> np.ndarray:
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


def _loam_submap_info(self) -> dict:
    """Parity hook: the last update's selection and its clouds before and after the VoxelGrids (pcm_loam_submap_info)."""
    r = getattr(self, "_submap", None)
    if r is None:
        raise capi.PcmError(-2, "submap_info before update_submap")
    out = {"keys": np.zeros(r.num_selected, np.int32), "corner_in": np.zeros((r.num_corner_in, 4), np.float32),
           "surf_in": np.zeros((r.num_surf_in, 4), np.float32), "corner_map": np.zeros((r.num_corner_map, 4), np.float32),
           "surf_map": np.zeros((r.num_surf_map, 4), np.float32)}
    self._check(self._L.pcm_loam_submap_info(self._h, *(out[k].ctypes.data for k in ("keys", "corner_in", "surf_in", "corner_map", "surf_map"))))
    return out


LoamRegistration.add_keyframe = _loam_add_keyframe
LoamRegistration.set_keyframe_poses = _loam_set_keyframe_poses
LoamRegistration.num_keyframes = property(_loam_num_keyframes)
LoamRegistration.clear_keyframes = _loam_clear_keyframes
LoamRegistration.get_keyframe = _loam_get_keyframe
LoamRegistration.update_submap = _loam_update_submap
LoamRegistration.near_keyframes = _loam_near_keyframes
LoamRegistration.submap_info = _loam_submap_info


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


def _sc_params(L, params: dict) -> capi.PcmLoamScParams:
    p = capi.PcmLoamScParams()
    L.pcm_loam_default_sc_params(C.byref(p))
    for k, v in params.items():
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _loam_sc_add(self, points=None, keyframe=None, near=None, **params) -> int:
    """makeAndSaveScancontextAndKeys of one cloud: ``points`` (an (N,>=3) float32 host array or a contiguous (N,C) float32 device
    tensor; VoxelGrid of ``leaf`` first), or the stored surf cloud of key frame ``keyframe``.  Returns the descriptor's index."""
    if sum(a is not None for a in (points, keyframe, near)) != 1:
        raise ValueError("pass exactly one of points, keyframe, near")
    p = _sc_params(self._L, params)
    r = capi.PcmLoamScAddResult()
    if near is not None:
        self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_KEYFRAME_NEAR, int(near), None, 0, 16, capi.MEM_HOST, C.byref(r)))
    elif keyframe is not None:
        self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_KEYFRAME_SURF, int(keyframe), None, 0, 16, capi.MEM_HOST, C.byref(r)))
    elif hasattr(points, "data_ptr") and getattr(points, "is_cuda", False):
        if points.dim() != 2 or points.shape[1] < 3 or not points.is_contiguous() or points.element_size() != 4:
            raise ValueError("expected a contiguous (N,>=3) float32 device tensor")
        self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_POINTS, -1, points.data_ptr(), points.shape[0], 4 * points.shape[1],
                                            capi.MEM_DEVICE, C.byref(r)))
    else:
        a = np.ascontiguousarray(points, dtype=np.float32)
        if a.ndim != 2 or a.shape[1] < 3:
            raise ValueError("expected an (N,>=3) float32 array")
        self._check(self._L.pcm_loam_sc_add(self._h, C.byref(p), capi.PCM_LOAM_SC_POINTS, -1, a.ctypes.data, a.shape[0], 4 * a.shape[1], capi.MEM_HOST, C.byref(r)))
    self._sc_last_add = r
    return r.index


def _loam_sc_add_near(self, key: int, search_num: int, wrt_key: int = -1, leaf: float = 0.2, **params) -> int:
    """MULTI_SCAN_FEAT: the descriptor of the near-key-frame cloud ``near_keyframes(key, search_num, wrt_key, leaf)``, built on the
    device and read in place (pcm_loam_sc_add_near); equals ``sc_add(points=that cloud, leaf=0.0)``.  Returns its index."""
    p = _sc_params(self._L, params)
    r = capi.PcmLoamScAddResult()
    self._check(self._L.pcm_loam_sc_add_near(self._h, C.byref(p), int(key), int(search_num), int(wrt_key), float(leaf), C.byref(r)))
    self._sc_last_add = r
    return r.index


def _loam_sc_put(self, desc):
    """A ready (num_ring, num_sector) descriptor (e.g. of a saved map); its keys are derived on the device."""
    d = np.asarray(desc, dtype=np.float64)
    if d.ndim != 2:
        raise ValueError("expected a (num_ring, num_sector) array")
    col = np.ascontiguousarray(d.T)   # column-major, ring fastest
    self._check(self._L.pcm_loam_sc_put(self._h, col.ctypes.data, d.shape[0], d.shape[1]))


def _loam_sc_count(self) -> int:
    n = self._L.pcm_loam_sc_count(self._h)
    if n < 0:
        self._check(n)
    return n


def _loam_sc_get(self, i: int):
    """(descriptor (num_ring, num_sector) float64, ring key (num_ring,) float32, sector key (num_sector,) float64)."""
    R, S = C.c_int(0), C.c_int(0)
    self._check(self._L.pcm_loam_sc_shape(self._h, C.byref(R), C.byref(S)))
    col = np.zeros((max(1, S.value), max(1, R.value)))
    rk = np.zeros(max(1, R.value), np.float32)
    sk = np.zeros(max(1, S.value))
    self._check(self._L.pcm_loam_sc_get(self._h, int(i), col.ctypes.data, rk.ctypes.data, sk.ctypes.data))
    return np.ascontiguousarray(col.T), rk, sk


def _loam_sc_clear(self):
    self._check(self._L.pcm_loam_sc_clear(self._h))


def _loam_sc_detect(self, **params) -> LoamLoopResult:
    """detectLoopClosureID of the last descriptor (pcm_loam_sc_detect); num_candidates=0 compares against the whole search set."""
    p = _sc_params(self._L, params)
    r = capi.PcmLoamScResult()
    self._check(self._L.pcm_loam_sc_detect(self._h, C.byref(p), C.byref(r)))
    m = min(64, r.num_evaluated)
    cands = [(r.cand_index[t], float(np.float32(r.cand_d2[t])), r.cand_dist[t], r.cand_shift[t]) for t in range(m)]
    return LoamLoopResult(r.loop_id, r.yaw_diff_rad, r.min_dist, r.nn_idx, r.nn_align, r.num_descriptors, r.tree_size, bool(r.tree_rebuilt),
                          r.num_evaluated, cands, r.status)


def _loam_sc_distance(self, i: int, j: int, **params):
    """distanceBtnScanContext(descriptor i, descriptor j) -> (distance, shift)."""
    p = _sc_params(self._L, params)
    d, s = C.c_double(0.0), C.c_int32(0)
    self._check(self._L.pcm_loam_sc_distance(self._h, C.byref(p), int(i), int(j), C.byref(d), C.byref(s)))
    return d.value, s.value


def _loam_detect_loop_distance(self, time_cur, radius: float = 10.0, time_diff_s: float = 30.0):
    """detectLoopClosureDistance on the stored key poses: (key_cur, key_pre) or None."""
    a, b = C.c_int32(-1), C.c_int32(-1)
    rc = self._L.pcm_loam_loop_detect_distance(self._h, float(radius), float(time_diff_s), float(time_cur), C.byref(a), C.byref(b))
    if rc < 0:
        self._check(rc)
    return (a.value, b.value) if rc == 1 else None


LoamRegistration.sc_add = _loam_sc_add
LoamRegistration.sc_put = _loam_sc_put
LoamRegistration.sc_add_near = _loam_sc_add_near
LoamRegistration.sc_get = _loam_sc_get
LoamRegistration.sc_count = property(_loam_sc_count)
LoamRegistration.sc_clear = _loam_sc_clear
LoamRegistration.sc_detect = _loam_sc_detect
LoamRegistration.sc_distance = _loam_sc_distance
LoamRegistration.detect_loop_distance = _loam_detect_loop_distance


# ---- loop verification on the device (pcm_loam_loop_*) ----
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


def _loop_params(L, params: dict) -> capi.PcmLoamLoopParams:
    p = capi.PcmLoamLoopParams()
    L.pcm_loam_default_loop_params(C.byref(p))
    for k, v in params.items():
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _loop_factor(r: capi.PcmLoamLoopResult) -> LoamLoopFactor:
    return LoamLoopFactor(LOOP_STATUS[r.status], r.key_cur, r.key_pre, r.num_cur_points, r.num_prev_points, r.ndt_iterations, bool(r.ndt_converged),
                          r.fitness, float(np.float32(r.noise_variance)), np.array(r.correction, np.float32).reshape(4, 4), np.array(r.pose_from),
                          np.array(r.pose_to), np.array(r.between).reshape(4, 4), np.array(r.between6))


def _loam_submap_near_device(self, key: int, search_num: int, wrt_key: int = -1, leaf: float = 0.2, out=None):
    """pcm_loam_submap_near_dev: the cloud of ``near_keyframes``, bit for bit, as (x, y, z, intensity) rows of ``out`` -- a
    contiguous (cap, 4) float32 device tensor (written on the context's stream; with leaf == 0 the call does not wait) or a
    (cap, 4) float32 host array.  Returns the number of rows written."""
    n = C.c_size_t(0)
    ptr, cap, mem = _cloud_buffer(out)
    rc = self._L.pcm_loam_submap_near_dev(self._h, int(key), int(search_num), int(wrt_key), float(leaf), ptr, cap, mem, C.byref(n))
    self._near_count = n.value
    self._check(rc)
    return n.value


def _loam_loop_verify(self, key_cur: int, key_pre: int, **params) -> LoamLoopFactor:
    """performLoopClosure :645-731 for the pair (pcm_loam_loop_verify): near clouds, size gates, pclomp NDT, fitness, loop factor."""
    p = _loop_params(self._L, params)
    r = capi.PcmLoamLoopResult()
    self._check(self._L.pcm_loam_loop_verify(self._h, C.byref(p), int(key_cur), int(key_pre), C.byref(r)))
    return _loop_factor(r)


def _loam_loop_closure(self, time_cur, radius: float = 10.0, time_diff_s: float = 30.0, **params) -> LoamLoopFactor:
    """detectLoopClosureDistance + verification in one call (pcm_loam_loop_closure); status "no_loop" without a candidate.  The
    loopIndexContainer bookkeeping stays with the caller."""
    p = _loop_params(self._L, params)
    r = capi.PcmLoamLoopResult()
    self._check(self._L.pcm_loam_loop_closure(self._h, C.byref(p), float(radius), float(time_diff_s), float(time_cur), C.byref(r)))
    return _loop_factor(r)


def _loam_loop_verifier_exists(self) -> bool:
    n = self._L.pcm_loam_loop_verifier_exists(self._h)
    if n < 0:
        self._check(n)
    return bool(n)


LoamRegistration.submap_near_device = _loam_submap_near_device
LoamRegistration.loop_verify = _loam_loop_verify
LoamRegistration.loop_closure = _loam_loop_closure
LoamRegistration.loop_verifier_exists = property(_loam_loop_verifier_exists)


def loam_extract_features(reg: LoamRegistration, cloud, **feature_params):
    """One scan to (corner (Nc,4), surf (Ns,4), info): laserCloudCornerLastDS / laserCloudSurfLastDS as (x, y, z, intensity) on
    the host (pcm_loam_extract_features; the context's LOAM source is left as it is, its cross-frame state advances)."""
    (stride, ioff, roff), fp = _split_layout(dict(feature_params))
    p = _feature_params(reg._L, fp)
    ptr, n, mem, keep = _scan_arg(cloud, stride)
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
    (stride, ioff, roff), fp = _split_layout(dict(feature_params))
    L = capi.load_library()
    p = _feature_params(L, fp)
    n = len(regs)
    if len(clouds) != n:
        raise ValueError("one scan per context")
    args = [_scan_arg(c, stride) for c in clouds]
    mems = {a[2] for a in args}
    if len(mems) != 1:
        raise ValueError("all scans of a batch must be host arrays or all device tensors")
    hs = (C.c_void_p * n)(*[r.handle for r in regs])
    ptrs = (C.c_void_p * n)(*[a[0] for a in args])
    ns = (C.c_size_t * n)(*[a[1] for a in args])
    out = (capi.PcmLoamFeaturesResult * n)()
    rc = L.pcm_loam_frame_begin_batch(hs, n, ptrs, ns, stride, ioff, roff, mems.pop(), C.byref(p), out)
    if rc != capi.PCM_OK:
        raise capi.PcmError(rc, (L.pcm_last_error(regs[0].handle) or b"").decode())
    res = [_features_result(out[i]) for i in range(n)]
    for reg, r in zip(regs, res):
        reg.n_corner, reg.n_surf = r["num_corner"], r["num_surf"]
    return res


# ---- 2D occupancy map (pcm_occ_*) ----
@dataclasses.dataclass
class OccupancyGrid:
    """The cropped map as nav_msgs/OccupancyGrid holds it."""
    data: np.ndarray        # (height, width) int8: -1 unknown, 0 free, 100 occupied
    resolution: float
    origin_x: float
    origin_y: float
    n_known: int

    @property
    def width(self) -> int:
        return int(self.data.shape[1])

    @property
    def height(self) -> int:
        return int(self.data.shape[0])


def _occ_params(L, params: dict) -> capi.PcmOccParams:
    p = capi.PcmOccParams()
    L.pcm_occ_default_params(C.byref(p))
    names = {f[0] for f in capi.PcmOccParams._fields_} - {"reserved"}
    for k, v in params.items():
        if k not in names:
            raise TypeError("unknown occupancy parameter %r" % k)
        setattr(p, k, int(bool(v)) if k in ("fill_with_white", "use_nan") else float(v))
    return p


class _OccMixin:
    """pcm_occ_* of the context ``self._h``."""

    def occ_reset(self, **params):
        p = _occ_params(self._L, params)
        self._check(self._L.pcm_occ_reset(self._h, C.byref(p)))

    def occ_insert_scans(self, clouds, poses):
        """Clouds (n, >= 3) float32 in the sensor frame and poses (S, 6) (roll, pitch, yaw, x, y, z) in one set of launches."""
        poses = np.ascontiguousarray(np.asarray(poses, np.float32).reshape(-1, 6))
        clouds = [np.ascontiguousarray(np.asarray(c, np.float32)[:, :3]) for c in clouds]
        if len(clouds) != poses.shape[0]:
            raise ValueError("one pose per cloud")
        ns = (C.c_size_t * max(1, len(clouds)))(*[c.shape[0] for c in clouds])
        pts = np.ascontiguousarray(np.concatenate(clouds)) if clouds else np.zeros((0, 3), np.float32)
        self._check(self._L.pcm_occ_insert_scans(self._h, pts.ctypes.data, ns, poses.ctypes.data, len(clouds), 12, capi.MEM_HOST))

    def occ_scan(self, s: int):
        """Parity hook: (ranges float32 with NaN for empty beams, angles float64) of scan s of the last insert."""
        B = self.occ_status()["beam_size"]
        r, a = np.zeros(B, np.float32), np.zeros(B, np.float64)
        self._check(self._L.pcm_occ_get_scan(self._h, int(s), r.ctypes.data, a.ctypes.data))
        return r, a

    def occ_status(self) -> dict:
        b, n, o = C.c_int32(0), C.c_uint64(0), C.c_uint64(0)
        rect = (C.c_int64 * 4)()
        self._check(self._L.pcm_occ_status(self._h, C.byref(b), C.byref(n), C.byref(o), rect))
        return {"beam_size": b.value, "n_scans": n.value, "overflow": o.value, "rect": tuple(rect)}

    def _occ_info(self):
        w, h, n = C.c_int32(0), C.c_int32(0), C.c_int64(0)
        ox, oy, res = C.c_double(0), C.c_double(0), C.c_double(0)
        self._check(self._L.pcm_occ_info(self._h, C.byref(w), C.byref(h), C.byref(ox), C.byref(oy), C.byref(res), C.byref(n)))
        return w.value, h.value, ox.value, oy.value, res.value, n.value

    def occ_map(self) -> OccupancyGrid:
        w, h, ox, oy, res, n = self._occ_info()
        g = np.zeros((h, w), np.int8)
        self._check(self._L.pcm_occ_get_map(self._h, g.ctypes.data, g.size))
        return OccupancyGrid(g, res, ox, oy, n)

    def occ_pgm(self) -> np.ndarray:
        """(height, width) uint8: the body of the P5 image, rows top-down."""
        w, h = self._occ_info()[:2]
        g = np.zeros((h, w), np.uint8)
        self._check(self._L.pcm_occ_get_pgm(self._h, g.ctypes.data, g.size))
        return g

    def occ_counts(self):
        """(n_occ, n_free) uint32 (height, width) of the cropped map."""
        w, h = self._occ_info()[:2]
        a, b = np.zeros((h, w), np.uint32), np.zeros((h, w), np.uint32)
        self._check(self._L.pcm_occ_get_counts(self._h, a.ctypes.data, b.ctypes.data, a.size))
        return a, b

    def occ_save_map(self, path_prefix: str):
        """<prefix>.pgm and <prefix>.yaml in the byte layout of the reference's saveMap; returns the two paths."""
        return save_map(path_prefix, self.occ_map())


def pgm_bytes(grid: np.ndarray) -> bytes:
    """The body of saveMap's image from an int8 grid (host code: 0..25 -> 254, >= 65 -> 0, else 205; rows top-down)."""
    g = np.asarray(grid)
    out = np.full(g.shape, 205, np.uint8)
    out[(g >= 0) & (g <= 25)] = 254
    out[g >= 65] = 0
    return out[::-1].tobytes()


def save_map(path_prefix: str, grid: OccupancyGrid):
    pgm, yaml = path_prefix + ".pgm", path_prefix + ".yaml"
    with open(pgm, "wb") as f:
        f.write(("P5\n# CREATOR: occupancy_mapping %.3f m/pix\n%d %d\n255\n" % (grid.resolution, grid.width, grid.height)).encode())
        f.write(pgm_bytes(grid.data))
    with open(yaml, "wb") as f:
        f.write(("image: %s\nresolution: %f\norigin: [%f, %f, 0.00]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n\n"
                 % (pgm, grid.resolution, grid.origin_x, grid.origin_y)).encode())
    return pgm, yaml


class OccupancyMap2D(_OccMixin):
    """jueying_slam's 2D occupancy mapping tool on one HIP device, in a context of its own.

    ``insert_scans(clouds, poses)`` = getScan + processScan per cloud, ``map()`` = getGridMap, ``save_map(prefix)`` = saveMap."""

    def __init__(self, device: int = 0, **params):
        self._L = capi.load_library()
        self._h = self._L.pcm_create(device, None)
        if not self._h:
            raise capi.PcmError(-3, "pcm_create failed")
        self.occ_reset(**params)

    def _check(self, rc, allow=(capi.PCM_OK,)):
        if rc not in allow:
            raise capi.PcmError(rc, (self._L.pcm_last_error(self._h) or b"").decode())

    def __del__(self):
        h, self._h = getattr(self, "_h", None), None
        if h:
            self._L.pcm_destroy(h)

    @property
    def handle(self):
        return self._h

    reset = _OccMixin.occ_reset
    insert_scans = _OccMixin.occ_insert_scans
    scan = _OccMixin.occ_scan
    status = _OccMixin.occ_status
    map = _OccMixin.occ_map
    pgm = _OccMixin.occ_pgm
    counts = _OccMixin.occ_counts
    save_map = _OccMixin.occ_save_map


def _loam_occ_insert_keyframes(self, first: int = 0, n: int = None):
    """Key frames first .. first + n - 1 (default: all from `first`) into the context's occupancy map, read in place."""
    if n is None:
        n = self.num_keyframes - first
    self._check(self._L.pcm_occ_insert_keyframes(self._h, int(first), int(n)))


for _name in ("occ_reset", "occ_insert_scans", "occ_scan", "occ_status", "_occ_info", "occ_map", "occ_pgm", "occ_counts", "occ_save_map"):
    setattr(LoamRegistration, _name, getattr(_OccMixin, _name))
LoamRegistration.occ_insert_keyframes = _loam_occ_insert_keyframes


# ---------------------------------------------------------------------------------------------------------------------------
# LOAM localisation map: area tiles and the per-frame crop on the device
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


def _dynmap_params(L, params: dict) -> capi.PcmLoamDynmapParams:
    p = capi.PcmLoamDynmapParams()
    L.pcm_loam_default_dynmap_params(C.byref(p))
    for k, v in params.items():
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


_TILE_LIST = {0: 0, 1: 1, "corner": 0, "surf": 1}


def _loam_add_tile(self, which, box, points) -> int:
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


def _loam_num_tiles(self, which) -> int:
    n = self._L.pcm_loam_tile_count(self._h, _TILE_LIST[which])
    if n < 0:
        self._check(n)
    return n


def _loam_clear_tiles(self):
    self._check(self._L.pcm_loam_tile_clear(self._h))
    self._dm_load = self._dm_crop = None
    self._tile_size = None


def _pose6(pose6):
    return np.ascontiguousarray(pose6, dtype=np.float32).reshape(6)


def _loam_need_map_load(self, pose6, **params) -> bool:
    """dynamic_load_map_run's trigger: has the pose moved farther than area_size from the last load_map (pcm_loam_dynmap_need_load)."""
    p = _dynmap_params(self._L, params)
    x = _pose6(pose6)
    rc = self._L.pcm_loam_dynmap_need_load(self._h, C.byref(p), x.ctypes.data)
    if rc < 0:
        self._check(rc)
    return bool(rc)


def _loam_load_map(self, pose6, **params) -> LoamMapLoadResult:
    """create_pcd for both lists: selects the tiles around pose6 (margin) and records the pose; no points move (pcm_loam_dynmap_load)."""
    p = _dynmap_params(self._L, params)
    x = _pose6(pose6)
    r = capi.PcmLoamDynmapLoadResult()
    self._check(self._L.pcm_loam_dynmap_load(self._h, C.byref(p), x.ctypes.data, C.byref(r)))
    self._dm_load = r
    return LoamMapLoadResult(r.num_corner_tiles, r.num_surf_tiles, r.num_corner_selected, r.num_surf_selected, r.num_corner_points,
                             r.num_surf_points, r.generation, bool(r.changed))


def _loam_crop_map(self, pose6, **params) -> LoamMapCropResult:
    """dynamic_load_map(pose6): the selected tiles through the frame's window become this context's target (pcm_loam_dynmap_crop)."""
    p = _dynmap_params(self._L, params)
    x = _pose6(pose6)
    r = capi.PcmLoamDynmapCropResult()
    self._check(self._L.pcm_loam_dynmap_crop(self._h, C.byref(p), x.ctypes.data, C.byref(r)))
    self._dm_crop = r
    return LoamMapCropResult(r.num_corner_in, r.num_surf_in, r.num_corner, r.num_surf, r.num_nonfinite, bool(r.rebuilt), np.float32(r.x_lo),
                             np.float32(r.x_hi), np.float32(r.y_lo), np.float32(r.y_hi), r.status)


def _loam_dynmap_info(self) -> dict:
    """Parity hook: the selected tile indices of both lists and, after crop_map, the two cropped clouds (pcm_loam_dynmap_info)."""
    ld, cr = getattr(self, "_dm_load", None), getattr(self, "_dm_crop", None)
    if ld is None:
        raise capi.PcmError(-2, "dynmap_info before load_map")
    out = {"corner_tiles": np.zeros(ld.num_corner_selected, np.int32), "surf_tiles": np.zeros(ld.num_surf_selected, np.int32)}
    ptrs = [out["corner_tiles"].ctypes.data, out["surf_tiles"].ctypes.data, None, None]
    if cr is not None:
        out["corner"] = np.zeros((cr.num_corner, 4), np.float32)
        out["surf"] = np.zeros((cr.num_surf, 4), np.float32)
        ptrs[2:] = [out["corner"].ctypes.data, out["surf"].ctypes.data]
    self._check(self._L.pcm_loam_dynmap_info(self._h, *ptrs))
    return out


def _loam_global_map(self, out=None):
    """globalMap = cropped corner ++ cropped surf as (M,4) x y z intensity.  Without ``out``: a host array.  With a contiguous (cap,4)
    float32 CUDA tensor: written there without leaving the device, returns the number of points M (the NDT branch then passes
    ``out[:M]`` to ``PclNdtRegistration.set_input_target``)."""
    n = C.c_size_t(0)
    if out is not None:
        if not (hasattr(out, "data_ptr") and getattr(out, "is_cuda", False)) or str(out.dtype) != "torch.float32" or out.dim() != 2 or out.shape[1] != 4 \
                or not out.is_contiguous():
            raise ValueError("expected a contiguous (cap,4) float32 CUDA tensor")
        self._check(self._L.pcm_loam_dynmap_global(self._h, out.data_ptr(), out.shape[0], C.byref(n), capi.MEM_DEVICE))
        return n.value
    cr = getattr(self, "_dm_crop", None)
    if cr is None:
        raise capi.PcmError(-2, "global_map before crop_map")
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


def _global_params(L, params: dict) -> capi.PcmLoamGlobalParams:
    p = capi.PcmLoamGlobalParams()
    L.pcm_loam_default_global_params(C.byref(p))
    for k, v in params.items():
        if not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _loam_keyframe_global_keys(self, **params) -> np.ndarray:
    """publishGlobalMap's selection (pcm_loam_global_keys): the key frame of every used pose leaf, in list order.  ``leaf`` plays
    no part in it."""
    p = _global_params(self._L, params)
    keys = np.zeros(max(1, self.num_keyframes), np.int32)
    n = C.c_size_t(0)
    self._check(self._L.pcm_loam_global_keys(self._h, C.byref(p), keys.ctypes.data, keys.size, C.byref(n)))
    return keys[:n.value].copy()


def _loam_keyframe_global_map(self, out=None, **params):
    """publishGlobalMap (pcm_loam_global_map; search_radius, keypose_density, leaf).  Without ``out``: the (n, 4) x y z intensity
    cells on the host.  With a contiguous (cap, 4) float32 device tensor or host array: written there, returns the number of
    rows.  ``keyframe_global_result`` holds the counts of the last call."""
    p = _global_params(self._L, params)
    r = capi.PcmLoamGlobalResult()
    self._global_result = r
    if out is not None:
        ptr, cap, mem = _cloud_buffer(out)
        rc = self._L.pcm_loam_global_map(self._h, C.byref(p), ptr, cap, mem, C.byref(r))
        self._check(rc)
        return int(r.points_out)
    q = capi.PcmLoamGlobalParams(p.search_radius, p.keypose_density, 0.0)   # without a leaf and a buffer: the host-only query of points_in
    rc = self._L.pcm_loam_global_map(self._h, C.byref(q), None, 0, capi.MEM_HOST, C.byref(r))
    if rc != capi.PCM_OK and r.points_in == 0:
        self._check(rc)
    a = np.zeros((int(r.points_in), 4), np.float32)
    self._check(self._L.pcm_loam_global_map(self._h, C.byref(p), a.ctypes.data, a.shape[0], capi.MEM_HOST, C.byref(r)))
    return a[:int(r.points_out)]


def _loam_keyframe_global_result(self) -> LoamGlobalMapResult:
    r = getattr(self, "_global_result", None)
    if r is None:
        raise capi.PcmError(-2, "keyframe_global_result before keyframe_global_map")
    return LoamGlobalMapResult(r.num_near, r.num_pose_leaves, r.num_skipped, r.num_used, int(r.points_in), int(r.points_out))


_EXPORT_WHICH = {0: 0, 1: 1, 2: 2, "corner": 0, "surf": 1, "both": 2}


def _loam_export_map(self, which="both", first: int = 0, n: int = None, out=None):
    """The saved map (pcm_loam_map_export) of key frames first .. first + n - 1 (default: all from ``first``): "corner" = their
    corner clouds under their poses, "surf" = their surf clouds, "both" = all corner clouds, then all surf clouds (jueying.pcd when
    the range is the whole store); no VoxelGrid.  Without ``out``: an (N, 4) host array.  With a (cap, 4) float32 device tensor or
    host array: written there (a device tensor without a wait), returns N."""
    if n is None:
        n = self.num_keyframes - first
    w = _EXPORT_WHICH[which]
    cnt = C.c_size_t(0)
    if out is not None:
        ptr, cap, mem = _cloud_buffer(out)
        rc = self._L.pcm_loam_map_export(self._h, w, int(first), int(n), ptr, cap, mem, C.byref(cnt))
        self._export_count = cnt.value
        self._check(rc)
        return cnt.value
    rc = self._L.pcm_loam_map_export(self._h, w, int(first), int(n), None, 0, capi.MEM_HOST, C.byref(cnt))   # the count
    if rc != capi.PCM_OK and cnt.value == 0:
        self._check(rc)
    a = np.zeros((cnt.value, 4), np.float32)
    self._check(self._L.pcm_loam_map_export(self._h, w, int(first), int(n), a.ctypes.data, a.shape[0], capi.MEM_HOST, C.byref(cnt)))
    return a


# ---------------------------------------------------------------------------------------------------------------------------
# pcl::VoxelGridLarge on the device
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class VoxelLargeResult:
    cells: int
    finite_points: int
    pieces: int
    depth: int
    levels: int
    host_waits: int
    workspace_bytes: int


def _record_buffer(a, what):
    """(pointer, rows, row bytes, memory) of a contiguous (rows, 3..16) float32 device tensor or host array."""
    if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False):
        if a.dim() != 2 or not 3 <= a.shape[1] <= 16 or not a.is_contiguous() or a.element_size() != 4:
            raise ValueError(what + ": expected a contiguous (rows, 3..16) float32 device tensor")
        return a.data_ptr(), a.shape[0], 4 * a.shape[1], capi.MEM_DEVICE
    if not isinstance(a, np.ndarray) or a.dtype != np.float32 or a.ndim != 2 or not 3 <= a.shape[1] <= 16 or not a.flags.c_contiguous:
        raise ValueError(what + ": expected a contiguous (rows, 3..16) float32 array or device tensor")
    return a.ctypes.data, a.shape[0], 4 * a.shape[1], capi.MEM_HOST


def _voxel_downsample_large(self, points, leaf_size, out=None, rows=None):
    """pcl::VoxelGridLarge (pcm_voxel_downsample_large): the VoxelGrid of ``voxel_downsample`` for clouds whose leaf index
    overflows -- the cloud is cut along its longest axis until every piece fits, the pieces' cells follow one another in
    depth-first order.  points: (N, 3..16) float32 host array or device tensor (``rows``: only its first rows).  Without ``out``
    a host cloud returns (cells, VoxelLargeResult); with ``out`` (same memory and record width as the points) the cells are
    written there and (count, VoxelLargeResult) returns.  On an error ``voxel_large_result`` still holds the counts."""
    if not (hasattr(points, "data_ptr") and getattr(points, "is_cuda", False)):
        points = np.ascontiguousarray(points, dtype=np.float32)
    ptr, n, stride, mem = _record_buffer(points, "points")
    if rows is not None:
        if not 0 <= int(rows) <= n:
            raise ValueError("rows exceeds the cloud")
        n = int(rows)
    r = capi.PcmVoxelLargeResult()
    self._voxel_large_result = r

    def result():
        return VoxelLargeResult(int(r.cells), int(r.finite_points), int(r.pieces), int(r.depth), int(r.levels), int(r.host_waits), int(r.workspace_bytes))

    if out is not None:
        optr, cap, ostride, omem = _record_buffer(out, "out")
        if ostride != stride or omem != mem:
            raise ValueError("out must have the record width and the memory of the points")
        self._check(self._L.pcm_voxel_downsample_large(self._h, ptr, n, stride, mem, float(leaf_size), optr, cap, C.byref(r)))
        return int(r.cells), result()
    if mem != capi.MEM_HOST:
        raise ValueError("a device cloud needs a device tensor for the cells (out=)")
    a = np.zeros((n, points.shape[1]), np.float32)
    self._check(self._L.pcm_voxel_downsample_large(self._h, ptr, n, stride, mem, float(leaf_size), a.ctypes.data, a.shape[0], C.byref(r)))
    return a[:int(r.cells)].copy(), result()


def _voxel_large_result(self) -> VoxelLargeResult:
    r = getattr(self, "_voxel_large_result", None)
    if r is None:
        raise capi.PcmError(-2, "voxel_large_result before voxel_downsample_large")
    return VoxelLargeResult(int(r.cells), int(r.finite_points), int(r.pieces), int(r.depth), int(r.levels), int(r.host_waits), int(r.workspace_bytes))


Registration.voxel_downsample_large = _voxel_downsample_large
Registration.voxel_large_result = property(_voxel_large_result)
LoamRegistration.voxel_downsample_large = _voxel_downsample_large
LoamRegistration.voxel_large_result = property(_voxel_large_result)

LoamRegistration.keyframe_global_keys = _loam_keyframe_global_keys
LoamRegistration.keyframe_global_map = _loam_keyframe_global_map
LoamRegistration.keyframe_global_result = property(_loam_keyframe_global_result)
LoamRegistration.export_map = _loam_export_map


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


LoamRegistration.add_tile = _loam_add_tile
LoamRegistration.num_tiles = _loam_num_tiles
LoamRegistration.clear_tiles = _loam_clear_tiles
LoamRegistration.need_map_load = _loam_need_map_load
LoamRegistration.load_map = _loam_load_map
LoamRegistration.crop_map = _loam_crop_map
LoamRegistration.dynmap_info = _loam_dynmap_info
LoamRegistration.global_map = _loam_global_map


# ---------------------------------------------------------------------------------------------------------------------------
# The key-frame map cut into localisation area tiles on the device
# ---------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass
class LoamTilesResult:
    num_corner_tiles: int
    num_surf_tiles: int
    corner_points_in: int
    surf_points_in: int
    corner_points_out: int
    surf_points_out: int
    num_nonfinite: int


def _tiles_params(L, params: dict) -> capi.PcmLoamTilesParams:
    p = capi.PcmLoamTilesParams()
    L.pcm_loam_default_tiles_params(C.byref(p))
    for k, v in params.items():
        if k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        setattr(p, k, v)
    return p


def _loam_build_tiles(self, first: int = 0, n: int = None, **params) -> LoamTilesResult:
    """pcm_loam_tiles_build: replaces both tile lists with the tiles of key frames first .. first + n - 1 (default: all from
    ``first``) under their current poses (tile_size, leaf_corner, leaf_surf); the map does not leave the device.  ``load_map`` /
    ``crop_map`` then run on them as on tiles from ``add_tile``."""
    if n is None:
        n = self.num_keyframes - first
    p = _tiles_params(self._L, params)
    r = capi.PcmLoamTilesResult()
    self._check(self._L.pcm_loam_tiles_build(self._h, C.byref(p), int(first), int(n), C.byref(r)))
    self._dm_load = self._dm_crop = None
    self._tile_size = float(p.tile_size)
    return LoamTilesResult(r.num_corner_tiles, r.num_surf_tiles, int(r.corner_points_in), int(r.surf_points_in), int(r.corner_points_out),
                           int(r.surf_points_out), int(r.num_nonfinite))


def _loam_build_tiles_ms(self, first: int = 0, n: int = None, **params) -> dict:
    """Measurement hook (pcm_loam_tiles_build_ms): build_tiles with device events at its stage boundaries.  Returns the stage
    times in ms: {"corner": {stage: ms}, "surf": {stage: ms}, "gather": ms, "arena_copy": ms}; ``workspace_host`` is host time."""
    if n is None:
        n = self.num_keyframes - first
    p = _tiles_params(self._L, params)
    r = capi.PcmLoamTilesResult()
    ms = np.zeros(2 * capi.PCM_LOAM_TILES_STAGES + 2, np.float32)
    self._check(self._L.pcm_loam_tiles_build_ms(self._h, C.byref(p), int(first), int(n), C.byref(r), ms.ctypes.data))
    self._dm_load = self._dm_crop = None
    self._tile_size = float(p.tile_size)
    S = capi.PCM_LOAM_TILES_STAGES
    out = {name: {k: float(v) for k, v in zip(capi.TILES_STAGE_NAMES, ms[m * S:(m + 1) * S])} for m, name in enumerate(("corner", "surf"))}
    out["gather"], out["arena_copy"] = float(ms[2 * S]), float(ms[2 * S + 1])
    return out


def _loam_tile_info(self, which, i: int) -> dict:
    """Tile ``i`` of a list, from ``add_tile`` or ``build_tiles``: box (x_min, y_min, z_min, x_max, y_max, z_max) float64, ixy (the
    index pair; (0, 0) for a tile added by hand) and its number of points (pcm_loam_tile_info)."""
    box = np.zeros(6, np.float64)
    ixy = np.zeros(2, np.int32)
    n = C.c_size_t(0)
    self._check(self._L.pcm_loam_tile_info(self._h, _TILE_LIST[which], int(i), box.ctypes.data, ixy.ctypes.data, C.byref(n)))
    return {"box": box, "ixy": (int(ixy[0]), int(ixy[1])), "n": int(n.value)}


def _loam_get_tile(self, which, i: int, out=None):
    """The (n, 4) x y z intensity points of tile ``i`` (pcm_loam_tile_get).  Without ``out``: a host array.  With a contiguous
    (cap, 4) float32 device tensor or host array: written there, returns n."""
    n = C.c_size_t(0)
    if out is not None:
        ptr, cap, mem = _cloud_buffer(out)
        self._check(self._L.pcm_loam_tile_get(self._h, _TILE_LIST[which], int(i), ptr, cap, mem, C.byref(n)))
        return int(n.value)
    a = np.zeros((self.tile_info(which, i)["n"], 4), np.float32)
    self._check(self._L.pcm_loam_tile_get(self._h, _TILE_LIST[which], int(i), a.ctypes.data, a.shape[0], capi.MEM_HOST, C.byref(n)))
    return a[:n.value]


def _loam_tiles_arealist(self, which, prefix: str = ""):
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


LoamRegistration.build_tiles = _loam_build_tiles
LoamRegistration.build_tiles_ms = _loam_build_tiles_ms
LoamRegistration.tile_info = _loam_tile_info
LoamRegistration.get_tile = _loam_get_tile
LoamRegistration.tiles_arealist = _loam_tiles_arealist


# ---------------------------------------------------------------------------------------------------------------------------
# Scan fusion and ring converters on the device: fusion_lidar_camera / rs_to_velodyne / hesai_to_velodyne
# ---------------------------------------------------------------------------------------------------------------------------
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
        ptr, n, mem, ka = _scan_arg(s.points, s.stride)
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
    p = capi.PcmScanFuseParams()
    defaults(C.byref(p))
    keep = []
    for k, v in (params or {}).items():
        if k == "pitch_ring_table":
            if v is not None:
                t = np.ascontiguousarray(v, np.int32)
                keep.append(t)
                p.pitch_ring_table, p.pitch_ring_table_len = t.ctypes.data, t.size
        elif k in ("layout", "output_layout"):
            p.output_layout = _SCAN_LAYOUT[v]
        elif k.startswith("reserved") or not hasattr(p, k):
            raise KeyError(k)
        else:
            setattr(p, k, v)
    return p, keep


def scan_result(r: capi.PcmScanFuseResult, n_segs: int) -> dict:
    d = {k: [getattr(r.seg[s], k) for s in range(n_segs)] for k in ("n_in", "n_nan", "n_depth_filtered", "n_kept", "out_offset")}
    d.update(n_out=r.n_out, n_pitch_index_clamped=r.n_pitch_index_clamped, status=r.status)
    return d


def _fuse_scans(self, segments, params=None, out=None):
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
        ptr, cap, mem, ret = _scan_arg(out, FUSED_STRIDE)
        if mem == capi.MEM_HOST and ret is not out:
            raise ValueError("a host output buffer must be a contiguous array")
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


def _fused_scan(self):
    """(device pointer, n) of the records the last fuse_scans(out=None) left in the context."""
    ptr, n = C.c_void_p(), C.c_size_t()
    self._check(self._L.pcm_scan_fused(self._h, C.byref(ptr), C.byref(n)))
    return ptr.value or 0, n.value


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


def _loam_frame_begin_fused(self, segments, fuse_params=None, **feature_params):
    """fuse_scans into the context's device buffer, then pcm_loam_frame_begin on it where it lies -> (features result, counts)."""
    _, counts = self.fuse_scans(segments, fuse_params, out=None)
    ptr, n = self.fused_scan()
    fp = {k: v for k, v in feature_params.items() if k not in _FEATURE_LAYOUT}
    p = _feature_params(self._L, fp)
    r = capi.PcmLoamFeaturesResult()
    self._check(self._L.pcm_loam_frame_begin(self._h, ptr, n, FUSED_STRIDE, FUSED_INTENSITY, FUSED_RING, capi.MEM_DEVICE, C.byref(p), C.byref(r)))
    self.n_corner, self.n_surf = r.num_corner, r.num_surf
    return _features_result(r), counts


for _cls in (Registration, LoamRegistration, OccupancyMap2D):
    _cls.fuse_scans = _fuse_scans
    _cls.fused_scan = _fused_scan
LoamRegistration.frame_begin_fused = _loam_frame_begin_fused


# ---- PointCloud2 handlers of jueying_lio's PointCloudPreprocess (pcm_lidar_filter) -----------------------------
LIDAR_TYPE = {"velodyne": capi.PCM_LIDAR_VELODYNE, "ouster": capi.PCM_LIDAR_OUSTER, "rslidar": capi.PCM_LIDAR_RSLIDAR, "livox": capi.PCM_LIDAR_LIVOX_STD}
LIDAR_TIME_KIND = {"f32": capi.PCM_LIDAR_TIME_FLOAT, "f64": capi.PCM_LIDAR_TIME_DOUBLE, "u32": capi.PCM_LIDAR_TIME_UINT32}
LIDAR_RING_KIND = {"u8": capi.PCM_LIDAR_RING_UINT8, "u16": capi.PCM_LIDAR_RING_UINT16}
NORMAL_STRIDE = 48   # pcl::PointXYZINormal


def lidar_desc(type, **overrides) -> capi.PcmLidarDesc:
    """The reference's PCL struct layout and config values of a LiDAR type ("velodyne" | "ouster" | "rslidar" | "livox", or the
    reference's LidarType number), with any field of pcm_lidar_desc overridden (time_kind / ring_kind also by name: "f32" "f64" "u32",
    "u8" "u16")."""
    d = capi.PcmLidarDesc()
    capi.load_library().pcm_lidar_default_desc(LIDAR_TYPE.get(type, type) if isinstance(type, str) else int(type), C.byref(d))
    for k, v in overrides.items():
        if k == "time_kind" and isinstance(v, str):
            v = LIDAR_TIME_KIND[v]
        if k == "ring_kind" and isinstance(v, str):
            v = LIDAR_RING_KIND[v]
        if k == "reserved" or not hasattr(d, k):
            raise KeyError(k)
        setattr(d, k, v)
    return d


def _lidar_filter(self, points, desc, out=None):
    """The handler of desc.type on n records of desc.stride_bytes (a host array or a device tensor): -> ((m, 12) float32
    pcl::PointXYZINormal records in input order, given_offset_time).  out: a device tensor of at least n x 48 bytes to fill instead
    (-> (m, given_offset_time))."""
    ptr, n, mem, keep = _scan_arg(points, desc.stride_bytes)
    m, given = C.c_size_t(), C.c_int()
    if out is None:
        ret = np.zeros((max(n, 1), 12), np.float32)
        rc = self._L.pcm_lidar_filter(self._h, ptr, n, mem, C.byref(desc), ret.ctypes.data, n, capi.MEM_HOST, C.byref(m), C.byref(given))
    else:
        optr, cap, omem, okeep = _scan_arg(out, NORMAL_STRIDE)
        rc = self._L.pcm_lidar_filter(self._h, ptr, n, mem, C.byref(desc), optr, cap, omem, C.byref(m), C.byref(given))
    del keep
    self._check(rc)
    return (ret[:m.value].copy() if out is None else m.value), bool(given.value)


def _lio_frame_begin_cloud(self, points, desc, poses=None, rot_xyzw=(0, 0, 0, 1.0), pos=(0, 0, 0), off_R_xyzw=(0, 0, 0, 1.0), off_T=(0, 0, 0),
                           leaf_size: float = 0.5) -> int:
    """lio_frame_begin for a sensor_msgs::PointCloud2 cloud (pcm_lio_frame_begin_cloud): the records of msg.data (a host array or a
    device tensor) -> handler of desc.type -> stable sort by time -> motion compensation (poses: (K,22) Pose6D rows, None = none) ->
    voxel-grid down-sampling -> source of this object.  Returns the number of scan points."""
    ptr, n, mem, keep = _scan_arg(points, desc.stride_bytes)
    st = capi.PcmLioState()
    st.rot[:] = list(map(float, rot_xyzw)); st.pos[:] = list(map(float, pos)); st.off_R[:] = list(map(float, off_R_xyzw)); st.off_T[:] = list(map(float, off_T))
    pp, npose = None, 0
    if poses is not None:
        pa = np.ascontiguousarray(poses, dtype=np.float64)
        assert pa.ndim == 2 and pa.shape[1] == 22
        pp, npose = pa.ctypes.data, pa.shape[0]
    m = C.c_size_t()
    rc = self._L.pcm_lio_frame_begin_cloud(self._h, ptr, n, mem, C.byref(desc), C.c_float(leaf_size), C.c_void_p(pp), int(npose), C.byref(st), C.byref(m))
    del keep
    self._check(rc)
    return m.value


for _cls in (Registration, LoamRegistration, OccupancyMap2D):
    _cls.lidar_filter = _lidar_filter
Registration.lio_frame_begin_cloud = _lio_frame_begin_cloud


# ---- ImuProcess::Process of jueying_lio: the init frames and the forward propagation (pcm_lio_imu_init, pcm_lio_propagate;
# ---- DESIGN.md section 18), and LaserMapping::Run composed from the existing frame calls ---------------------------------------------
IMU_STATE_VECTORS = ("mean_acc", "mean_gyr", "cov_acc", "cov_gyr", "cov_bias_gyr", "cov_bias_acc", "cov_acc_scale", "cov_gyr_scale", "lidar_T_wrt_imu",
                     "lidar_R_wrt_imu", "angvel_last", "acc_s_last")
IMU_STATE_SCALARS = ("last_lidar_end_time", "init_iter_num", "first_frame", "need_init")


def lio_imu_state(**overrides) -> capi.PcmLioImuState:
    """The members of ImuProcess with the constructor's values (pcm_lio_default_imu_state), any of them overridden: the vectors by a
    sequence, last_imu by the 7 numbers t, acc, gyr, the scalars by a number."""
    s = capi.PcmLioImuState()
    capi.load_library().pcm_lio_default_imu_state(C.byref(s))
    for k, v in overrides.items():
        if k in IMU_STATE_VECTORS:
            getattr(s, k)[:] = [float(t) for t in v]
        elif k == "last_imu":
            v = [float(t) for t in v]
            s.last_imu.t = v[0]; s.last_imu.acc[:] = v[1:4]; s.last_imu.gyr[:] = v[4:7]
        elif k in IMU_STATE_SCALARS:
            setattr(s, k, v)
        else:
            raise KeyError(k)
    return s


def _filter_state(x) -> capi.PcmLioFilterState:
    st = capi.PcmLioFilterState()
    if isinstance(x, dict):
        for k, _ in Registration.LIO_STATE_FIELDS:
            getattr(st, k)[:] = [float(v) for v in x[k]]
    else:
        v = np.ascontiguousarray(x, np.float64).reshape(26)
        C.memmove(C.byref(st), v.ctypes.data, 26 * 8)
    return st


def _filter_dict(st) -> dict:
    return {k: np.array(getattr(st, k)[:]) for k, _ in Registration.LIO_STATE_FIELDS}


def _imu_rows(imu) -> np.ndarray:
    a = np.ascontiguousarray(imu, np.float64)
    if a.ndim != 2 or a.shape[1] != 7:
        raise ValueError("expected (n, 7) IMU rows: t, acc, gyr")
    return a


def _lio_imu_init(self, imu_state: capi.PcmLioImuState, imu, x, P):
    """One init frame of ImuProcess::Process (pcm_lio_imu_init; host arithmetic): imu_state is advanced in place, -> (x, P) with grav,
    bg, the extrinsics and the initial covariance set.  imu: (n, 7) rows t, acc, gyr; x as for lio_update."""
    a = _imu_rows(imu)
    st = _filter_state(x)
    Pm = np.array(P, np.float64).reshape(23, 23).copy()
    rc = self._L.pcm_lio_imu_init(C.byref(imu_state), a.ctypes.data, a.shape[0], C.byref(st), Pm.ctypes.data)
    if rc != capi.PCM_OK:
        raise capi.PcmError(rc, "pcm_lio_imu_init: no sample, a sample that is not finite, or an IMU state that is already initialised")
    return _filter_dict(st), Pm


def _lio_propagate(self, imu_state: capi.PcmLioImuState, imu, t_beg: float, t_end: float, x, P, capacity: int = None):
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


Registration.lio_imu_init = _lio_imu_init
Registration.lio_propagate = _lio_propagate


# ---- the frame outputs and the saved map of jueying_lio (pcm_lio_frame_world .. pcm_lio_map_export) --------
def _lio_state(rot_xyzw, pos, off_R_xyzw, off_T) -> capi.PcmLioState:
    st = capi.PcmLioState()
    st.rot[:] = list(map(float, rot_xyzw)); st.pos[:] = list(map(float, pos)); st.off_R[:] = list(map(float, off_R_xyzw)); st.off_T[:] = list(map(float, off_T))
    return st


def _xyzi_out(out):
    """(pointer, capacity in records, memory) of a caller's buffer of 16-byte records: a float32 numpy array or CUDA tensor."""
    if hasattr(out, "data_ptr"):
        assert out.is_cuda and out.is_contiguous() and out.element_size() == 4
        return out.data_ptr(), out.numel() // 4, capi.MEM_DEVICE
    assert isinstance(out, np.ndarray) and out.dtype == np.float32 and out.flags.c_contiguous and out.flags.writeable
    return out.ctypes.data, out.size // 4, capi.MEM_HOST


def _xyzi_call(self, call, out):
    """call(ptr, capacity, memory, byref(n)) -> rc.  out None: a new (n, 4) float32 host array; else the caller's buffer is filled and
    the count returned (a buffer that is too small raises, with the needed count in the message)."""
    n = C.c_size_t()
    if out is not None:
        ptr, cap, mem = _xyzi_out(out)
        self._check(call(C.c_void_p(ptr), cap, mem, C.byref(n)))
        return n.value
    self._check(call(None, 0, capi.MEM_HOST, C.byref(n)))
    res = np.zeros((n.value, 4), np.float32)
    if n.value:
        self._check(call(C.c_void_p(res.ctypes.data), n.value, capi.MEM_HOST, C.byref(n)))
    return res


def _lio_frame_world(self, rot_xyzw, pos, off_R_xyzw, off_T, dense: bool = False, out=None):
    """PublishFrameWorld's cloud of the current frame (pcm_lio_frame_world; laser_mapping.cc:747-762): (x, y, z, intensity) rows in the
    world frame; dense = every undistorted point, else the down-sampled scan in the order of get_source()."""
    st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
    return _xyzi_call(self, lambda p, cap, mem, n: self._L.pcm_lio_frame_world(self._h, C.byref(st), int(bool(dense)), p, cap, mem, n), out)


def _lio_frame_body(self, rot_xyzw, pos, off_R_xyzw, off_T, out=None):
    """PublishFrameBody's cloud (pcm_lio_frame_body; :794-808): the undistorted scan in the IMU body frame."""
    st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
    return _xyzi_call(self, lambda p, cap, mem, n: self._L.pcm_lio_frame_body(self._h, C.byref(st), p, cap, mem, n), out)


def _lio_frame_effect(self, rot_xyzw, pos, off_R_xyzw, off_T, out=None):
    """PublishFrameEffectWorld's cloud (pcm_lio_frame_effect; :810-823): the points that gave a row to the last ObsModel call, in scan
    order, in the world frame, intensity = |z|."""
    st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
    return _xyzi_call(self, lambda p, cap, mem, n: self._L.pcm_lio_frame_effect(self._h, C.byref(st), p, cap, mem, n), out)


def _map_info_dict(info) -> dict:
    return dict(points=int(info.points), capacity=int(info.capacity), frames_appended=int(info.frames_appended), growths=int(info.growths),
                scan_wait_num=int(info.scan_wait_num), pcd_index=int(info.pcd_index), chunk_ready=bool(info.chunk_ready))


def _lio_map_append(self, rot_xyzw, pos, off_R_xyzw, off_T, dense: bool = False, pcd_save_interval: int = -1) -> dict:
    """`*pcl_wait_save_ += *laserCloudWorld` on the device (pcm_lio_map_append; :776-791) -> lio_map_info(); chunk_ready / pcd_index say
    when the reference would write jueying_<pcd_index>.pcd and clear the cloud (fetch the log, then lio_map_clear)."""
    st = _lio_state(rot_xyzw, pos, off_R_xyzw, off_T)
    info = capi.PcmLioMapInfo()
    self._check(self._L.pcm_lio_map_append(self._h, C.byref(st), int(bool(dense)), int(pcd_save_interval), C.byref(info)))
    return _map_info_dict(info)


def _lio_map_info(self) -> dict:
    info = capi.PcmLioMapInfo()
    self._check(self._L.pcm_lio_map_info_get(self._h, C.byref(info)))
    return _map_info_dict(info)


def _lio_map_get(self, first: int = 0, count: int = None, out=None):
    """Records [first, first + count) of the saved-map log (count None: to its end) as (count, 4) float32 rows, or into `out`."""
    if count is None:
        count = max(self.lio_map_info()["points"] - int(first), 0)
    if out is not None:
        ptr, cap, mem = _xyzi_out(out)
        if cap < count:
            raise ValueError("lio_map_get: the buffer holds %d records, the slice has %d" % (cap, count))
        self._check(self._L.pcm_lio_map_get(self._h, int(first), int(count), C.c_void_p(ptr), mem))
        return int(count)
    res = np.zeros((int(count), 4), np.float32)
    self._check(self._L.pcm_lio_map_get(self._h, int(first), int(count), C.c_void_p(res.ctypes.data), capi.MEM_HOST))
    return res


def _lio_map_clear(self):
    """pcl_wait_save_->clear(); scan_wait_num = 0 (pcm_lio_map_clear)."""
    self._check(self._L.pcm_lio_map_clear(self._h))


def _lio_map_export(self, leaf_size: float = 0.0, z_min: float = 1.0, z_max: float = 0.0, out=None):
    """LaserMapping::Finish's cloud, optionally through pcd2map's filters (pcm_lio_map_export): VoxelGrid of leaf_size (> 0), then
    the records with z_min <= z <= z_max (applied when z_min <= z_max).  Defaults: the log as it is."""
    return _xyzi_call(self, lambda p, cap, mem, n: self._L.pcm_lio_map_export(self._h, C.c_float(leaf_size), float(z_min), float(z_max), p, cap, mem, n), out)


Registration.lio_frame_world = _lio_frame_world
Registration.lio_frame_body = _lio_frame_body
Registration.lio_frame_effect = _lio_frame_effect
Registration.lio_map_append = _lio_map_append
Registration.lio_map_info = _lio_map_info
Registration.lio_map_get = _lio_map_get
Registration.lio_map_clear = _lio_map_clear
Registration.lio_map_export = _lio_map_export


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
