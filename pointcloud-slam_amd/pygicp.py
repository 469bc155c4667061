"""The module-level functions of the reference's ``pygicp`` (fast_gicp/src/python/main.cpp:46-142): ``downsample`` and
``align_points``, and the device operator behind both, pcl::ApproximateVoxelGrid (``approx_voxel_downsample``,
pcm_approx_voxel_downsample; the rules are in include/pcm_amd.h and DESIGN.md section 35).

The registration classes of that module are ``registration``'s (``GicpRegistration`` ...).  These are functions of this module,
not methods and not package names.  Importing it loads nothing; the first call loads the library and fails loudly without it.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi
from ._binding import buffer_arg

METHODS = ("GICP", "VGICP", "VGICP_CUDA", "NDT_CUDA")
_FLT_MAX = float(np.finfo(np.float32).max)
_ctx = None


def _context():
    """The context ``downsample`` runs on: device 0, created by the first call."""
    global _ctx
    if _ctx is None:
        from . import registration
        _ctx = registration.Registration(0)
    return _ctx


def approx_voxel_downsample(reg, points, leaf, out=None):
    """pcl::ApproximateVoxelGrid of ``points`` on ``reg``'s context (pcm_approx_voxel_downsample): one record per run of the
    filter's 512-entry history, in the filter's output order, every float of a record averaged.

    points: (n, 3..16) float32 host array (anything else on the host is converted) or device tensor.
    Without ``out``: -> (records, dropped), the records in the memory of the points (a new array, or a new tensor on the
    points' device).  With ``out`` (same record width; a device tensor, or a host array for host points): the records are
    written there -> (count, dropped); host points with a device ``out`` are uploaded once and filtered on the device.
    A buffer that is too small raises with the needed count in the message."""
    ptr, n, stride, mem, points = buffer_arg(points, (3, 16), convert=True, what="points:")
    cols = stride // 4
    m, d = C.c_size_t(0), C.c_size_t(0)

    def call(ptr, mem, optr, cap):
        reg._check(reg._L.pcm_approx_voxel_downsample(reg.handle, ptr, n, stride, mem, float(leaf), optr, cap, C.byref(m), C.byref(d)))

    if out is not None:
        optr, cap, ostride, omem, _ = buffer_arg(out, (3, 16), write=True, what="out:")
        if ostride != stride:
            raise ValueError("out must have the record width of the points")
        staged = None
        if omem != mem:
            if mem != capi.MEM_HOST:
                raise ValueError("a device cloud needs a device tensor for the records (out=)")
            import torch
            staged = torch.from_numpy(points).to(out.device)
            torch.cuda.synchronize(out.device)   # the context works on a stream of its own
            ptr, mem = staged.data_ptr(), capi.MEM_DEVICE
        call(ptr, mem, optr, cap)
        return m.value, d.value
    if mem == capi.MEM_HOST:
        a = np.empty((n, cols), np.float32)
        call(ptr, mem, a.ctypes.data, n)
        return a[:m.value].copy(), d.value
    import torch
    t = torch.empty((n, cols), dtype=torch.float32, device=points.device)
    call(ptr, mem, t.data_ptr(), n)
    return t[:m.value], d.value


def _xyz32(points, name):
    a = np.asarray(points, dtype=np.float64)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError("%s: expected an (n, 3) float64 array" % name)
    return np.ascontiguousarray(a, dtype=np.float32)   # eigen2pcl: points.row(i).cast<float>()


def downsample(points, downsample_resolution):
    """pygicp.downsample (main.cpp:46-62): (n, 3) float64 -> float32 -> ApproximateVoxelGrid with one leaf -> float64."""
    records, _ = approx_voxel_downsample(_context(), _xyz32(points, "points"), downsample_resolution)
    return records.astype(np.float64)


def _make(method, device, k_correspondences, max_correspondence_distance, voxel_resolution, num_threads, neighbor_search_method, neighbor_search_radius):
    """The object of ``method`` with the setters main.cpp:96-129 calls for it, in that order."""
    from . import registration as R
    if method == "GICP":
        reg = R.GicpRegistration(device)
        reg.set_max_correspondence_distance(min(float(max_correspondence_distance), _FLT_MAX))   # the default is DBL_MAX; the library keeps a float
        reg.set_correspondence_randomness(k_correspondences)
        reg.set_num_threads(num_threads)
    elif method == "VGICP":
        reg = R.VgicpRegistration(device)
        reg.set_correspondence_randomness(k_correspondences)
        reg.set_resolution(voxel_resolution)
        reg.set_neighbor_search_method(neighbor_search_method)
        reg.set_num_threads(num_threads)
    elif method == "VGICP_CUDA":
        reg = R.VgicpCudaRegistration(device)
        reg.set_correspondence_randomness(k_correspondences)
        reg.set_neighbor_search_method(neighbor_search_method, neighbor_search_radius)
        reg.set_resolution(voxel_resolution)
    else:
        reg = R.NdtRegistration(device)
        reg.set_resolution(voxel_resolution)
        reg.set_neighbor_search_method(neighbor_search_method, neighbor_search_radius)
    return reg


def align_points(target, source, method="GICP", downsample_resolution=-1.0, k_correspondences=15, max_correspondence_distance=float(np.finfo(np.float64).max),
                 voxel_resolution=1.0, num_threads=0, neighbor_search_method="DIRECT1", neighbor_search_radius=1.5, initial_guess=None, device=0):
    """pygicp.align_points (main.cpp:64-142): both (n, 3) float64 clouds are cast to float32, filtered by ApproximateVoxelGrid
    when downsample_resolution > 0, and registered by ``method`` ("GICP", "VGICP", "VGICP_CUDA", "NDT_CUDA"; their classes are
    GicpRegistration, VgicpRegistration, VgicpCudaRegistration, NdtRegistration) from ``initial_guess`` (identity) -> the final
    transformation as (4, 4) float64.  The clouds are uploaded once; the filtered clouds stay on the device and are handed to
    set_input_target / set_input_source there.  An unknown method raises ValueError (the reference prints and returns identity).
    ``device``: the HIP device (not an argument of the reference)."""
    if method not in METHODS:
        raise ValueError("unknown registration method %r (one of %s)" % (method, ", ".join(METHODS)))
    tgt, src = _xyz32(target, "target"), _xyz32(source, "source")
    guess = np.eye(4, dtype=np.float32) if initial_guess is None else np.ascontiguousarray(initial_guess, dtype=np.float32)
    if guess.shape != (4, 4):
        raise ValueError("initial_guess: expected a (4, 4) matrix")
    reg = _make(method, device, k_correspondences, max_correspondence_distance, voxel_resolution, num_threads, neighbor_search_method, neighbor_search_radius)
    if downsample_resolution > 0.0:
        import torch
        dev = torch.device("cuda", device)
        tgt, src = torch.from_numpy(tgt).to(dev), torch.from_numpy(src).to(dev)
        torch.cuda.synchronize(dev)   # the context works on a stream of its own
        tgt = approx_voxel_downsample(reg, tgt, downsample_resolution)[0]
        src = approx_voxel_downsample(reg, src, downsample_resolution)[0]
    reg.set_input_target(tgt)
    reg.set_input_source(src)
    return reg.align(guess).T.astype(np.float64)   # getFinalTransformation().cast<double>()
