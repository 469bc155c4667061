"""Point-to-point ICP on the device (PCM_MODEL_ICP, include/pcm_amd.h): ``IterativeClosestPoint`` with
pcl::IterativeClosestPoint's setters in snake case.  All compute goes through the C ABI (``capi``)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from ._binding import Context, buffer_arg, default_config

PCM_MODEL_ICP = capi.PCM_MODEL_ICP
STOP_REASON = {capi.PCM_ICP_STOP_NONE: "none", capi.PCM_ICP_STOP_ITERATIONS: "iterations", capi.PCM_ICP_STOP_TRANSFORM: "transform",
               capi.PCM_ICP_STOP_ABS_MSE: "abs_mse", capi.PCM_ICP_STOP_REL_MSE: "rel_mse", capi.PCM_ICP_STOP_NO_CORRESPONDENCES: "no_correspondences"}


@dataclasses.dataclass
class IcpResult:
    """One align(): ``T`` float32 4x4 (getFinalTransformation), ``T64`` the double pose it was rounded from, the stop reason (one
    of STOP_REASON's names), N and the mean squared pair distance of the last iteration."""
    T: np.ndarray
    T64: np.ndarray
    iterations: int
    converged: bool
    stop_reason: str
    num_pairs: int
    mse: float


class IterativeClosestPoint(Context):
    """pcl::IterativeClosestPoint<PointXYZ, PointXYZ> on one HIP device.  Clouds are (N,>=3) float32 host arrays or contiguous
    float32 device tensors; an (N,4) device tensor given as the source is read in place and must stay alive until align() returns."""

    def __init__(self, device: int = 0, voxel_resolution: float = None, **params):
        cfg = default_config("ICP")
        if voxel_resolution is not None:
            cfg.voxel_resolution = float(voxel_resolution)
        super().__init__(device, cfg)
        self._p = capi.PcmIcpParams()
        self._L.pcm_icp_default_params(C.byref(self._p))
        self._last = None
        self._keep = [None, None]
        for k, v in params.items():
            if k.startswith("reserved") or not hasattr(self._p, k):
                raise KeyError(k)
            setattr(self._p, k, v)
        if params:
            self._push()

    def _push(self):
        self._check(self._L.pcm_icp_set_params(self._h, C.byref(self._p)))

    def _set(self, field, value):
        old = getattr(self._p, field)
        setattr(self._p, field, value)
        try:
            self._push()
        except capi.PcmError:
            setattr(self._p, field, old)
            raise

    # ---- PCL's setters ----
    def set_maximum_iterations(self, n: int):
        self._set("max_iterations", int(n))

    def set_max_correspondence_distance(self, d: float):
        self._set("max_correspondence_distance", float(d))

    def set_transformation_epsilon(self, eps: float):
        self._set("transformation_epsilon", float(eps))

    def set_transformation_rotation_epsilon(self, eps: float):
        self._set("rotation_epsilon", float(eps))

    def set_euclidean_fitness_epsilon(self, eps: float):
        self._set("euclidean_fitness_epsilon", float(eps))

    @property
    def params(self) -> dict:
        p = capi.PcmIcpParams()
        self._check(self._L.pcm_icp_get_params(self._h, C.byref(p)))
        return {k: getattr(p, k) for k, _ in p._fields_ if not k.startswith("reserved")}

    # ---- clouds ----
    def set_input_target(self, points):
        ptr, n, stride, mem, keep = buffer_arg(points, (3, None), convert=True)
        self._check(self._L.pcm_set_target(self._h, ptr, n, stride, mem, 0))
        self._keep[0] = None   # copied

    def set_input_source(self, points):
        ptr, n, stride, mem, keep = buffer_arg(points, (3, None), convert=True)
        self._check(self._L.pcm_set_source(self._h, ptr, n, stride, mem, 0))
        self._keep[1] = keep   # a 16-byte-stride device buffer is used in place

    # ---- registration ----
    def align(self, guess=None) -> IcpResult:
        g = np.eye(4, dtype=np.float32) if guess is None else np.ascontiguousarray(guess, dtype=np.float32).reshape(4, 4)
        r = capi.PcmResult()
        self._check(self._L.pcm_align(self._h, g.ctypes.data, C.byref(r)))
        info = capi.PcmIcpInfo()
        self._check(self._L.pcm_icp_last(self._h, C.byref(info)))
        self._last = IcpResult(np.array(r.T, np.float32).reshape(4, 4), np.array(r.T64).reshape(4, 4), r.iterations, bool(r.converged),
                               STOP_REASON[info.stop_reason], int(info.num_pairs), info.mse)
        return self._last

    def get_final_transformation(self) -> np.ndarray:
        return self._stored("_last", "get_final_transformation before align").T

    def has_converged(self) -> bool:
        return self._stored("_last", "has_converged before align").converged

    def get_fitness_score(self, max_range: float = float(np.finfo(np.float64).max), T=None) -> float:
        """pcl::Registration::getFitnessScore(max_range) at the final transformation (or at ``T``)."""
        t = np.ascontiguousarray(self.get_final_transformation() if T is None else T, dtype=np.float32).reshape(4, 4)
        s = C.c_double(0.0)
        self._check(self._L.pcm_fitness_score(self._h, t.ctypes.data, float(max_range), C.byref(s)))
        return s.value

    def trace(self):
        """Parity hook: (N, mse) of every iteration that ran in the last align (pcm_icp_trace)."""
        n = C.c_int32(0)
        self._check(self._L.pcm_icp_trace(self._h, 0, None, None, C.byref(n)))
        N, mse = np.zeros(max(1, n.value), np.uint64), np.zeros(max(1, n.value))
        self._check(self._L.pcm_icp_trace(self._h, n.value, N.ctypes.data, mse.ctypes.data, C.byref(n)))
        return N[:n.value].astype(np.int64), mse[:n.value]
