"""Host-side mirror of the reference's registration operator surface.

Same names, argument meaning and call order as the reference's pybind module
``pygicp`` (/root/reference/src/pointcloud_match/fast_gicp/src/python/main.cpp:135-215:
``set_input_target/source``, ``align``, ``swap_source_and_target``,
``get_final_transformation``, ``get_final_hessian`` ...) and the
``pcl::Registration`` setters it wraps, so the parity tests read like the
reference's gtest (src/test/gicp_test.cpp:147-201).  All compute goes through
the C ABI of include/pcm_amd.h; nothing here touches oracle/.

This module holds ``Registration``, its model subclasses and ``align_batch``, and re-exports the public names of the
subsystem modules (``lio``, ``loam``, ``occ``, ``scan``), so ``registration.X`` reaches the whole binding.
"""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import _binding, capi
from .lio import IMU_STATE_SCALARS, IMU_STATE_VECTORS, LioOdometry, LioUpdateResult, _LioMixin, lio_imu_state  # noqa: F401
from .loam import (LOOP_STATUS, XYZIRT_INTENSITY, XYZIRT_RING, XYZIRT_STRIDE, LoamGlobalMapResult, LoamLoopFactor, LoamLoopResult,  # noqa: F401
                   LoamMapCropResult, LoamMapLoadResult, LoamRegistration, LoamResult, LoamSubmapResult, LoamTilesResult, loam_align_batch,
                   loam_extract_features, loam_frame_begin_batch, pack_xyzirt, read_arealist, write_arealist)
from .occ import OccupancyGrid, OccupancyMap2D, pgm_bytes, save_map  # noqa: F401
from .scan import (FUSED_INTENSITY, FUSED_RING, FUSED_STRIDE, FUSED_TIME, LIDAR_RING_KIND, LIDAR_TIME_KIND, LIDAR_TYPE, NORMAL_STRIDE,  # noqa: F401
                   ScanSegment, VoxelLargeResult, _ScanMixin, _VoxelLargeMixin, depth_segment, fuse_lidar_cameras, hesai_to_velodyne,
                   lidar_desc, lidar_xyzi_segment, lidar_xyzirt_segment, rs_to_velodyne, scan_fuse_params, scan_result, scan_segments)


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


class Registration(_binding.Context, _LioMixin, _ScanMixin, _VoxelLargeMixin):
    """One registration object bound to a HIP device (= one ``pcm_ctx``)."""

    model = "P2PLANE"
    defaults = {}

    def __init__(self, device: int = 0, model: str = None, **params):
        if model is not None:
            self.model = model
        cfg = _binding.default_config(self.model)
        for k, v in self.defaults.items():
            setattr(cfg, k, v)
        self._cfg = cfg
        super().__init__(device, cfg)
        self._keep = {}
        self._last = None
        self._set(**params)

    # -- plumbing ---------------------------------------------------------
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

    # -- inputs: (N,>=3) float32 host data or CUDA tensors ---------------------
    def set_input_target(self, cloud, tag: int = 0):
        ptr, n, stride, mem, keep = _binding.buffer_arg(cloud, (3, None), convert=True)
        self._check(self._L.pcm_set_target(self._h, ptr, n, stride, mem, tag))

    def set_input_source(self, cloud, tag: int = 0):
        ptr, n, stride, mem, keep = _binding.buffer_arg(cloud, (3, None), convert=True)
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

    def target_insert(self, cloud):
        """IVox::AddPoints: append points to the sliding submap (LRU beyond map_capacity voxels)."""
        ptr, n, stride, mem, keep = _binding.buffer_arg(cloud, (3, None), convert=True)
        self._check(self._L.pcm_target_insert(self._h, ptr, n, stride, mem))

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

    def get_source(self) -> np.ndarray:
        return self._counted(lambda p, cap, mem, n: self._L.pcm_get_source(self._h, p, cap, C.byref(n)), shape=(3,))

    def get_target(self) -> np.ndarray:
        """(M,3) current target points in insertion order."""
        return self._counted(lambda p, cap, mem, n: self._L.pcm_get_target(self._h, p, cap, C.byref(n)), shape=(3,))

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
        return self._counted(lambda p, cap, mem, n: self._L.pcm_get_covariances(self._h, int(bool(target)), p, cap, C.byref(n)), shape=(3, 3),
                             dtype=np.float64)

    def set_covariances(self, covs, target: bool = False):
        """setSourceCovariances / setTargetCovariances (fast_gicp_impl.hpp:93-100): (N,3,3) or (N,4,4) float64, input order."""
        a = np.ascontiguousarray(covs, np.float64)
        elems = a.shape[1] * a.shape[2]
        self._check(self._L.pcm_set_covariances(self._h, int(bool(target)), a.ctypes.data, a.shape[0], elems))

    def set_correspondence_randomness(self, k): self._set(k_correspondences=int(k))   # setCorrespondenceRandomness  fast_gicp_impl.hpp:61-63
    def set_regularization_method(self, m): self._set(regularization=m)               # setRegularizationMethod      :66-68

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
