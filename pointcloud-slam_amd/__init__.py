"""MI355X-native scan-to-submap registration hot path (package root).

Holds only what the path needs: ``csrc/`` (hand-written HIP kernels + the C ABI
of ``include/pcm_amd.h``, built into ``libpcm_amd.so``), the host-side mirror
of the reference's registration interface (``registration.py``, with its subsystems in
``lio.py``, ``loam.py``, ``occ.py`` and ``scan.py`` over the shared ``_binding.py``), the synthetic
Livox-shaped input generator (``synth.py``) and the batch sharding helper
(``sharding.py``).  There is no CPU fallback: loading fails loudly when the HIP
library is missing, and contexts fail when no HIP device is present.
"""
from .capi import PcmError, build_library, library_path, load_library  # noqa: F401
from . import sharding  # noqa: F401
from .registration import (GicpRegistration, NdtRegistration, P2PlaneRegistration, PclNdtRegistration, Registration, VgicpCudaRegistration, VgicpRegistration,  # noqa: F401
                           RegistrationResult, align_batch)
from .registration import LoamRegistration, LoamResult, LoamSubmapResult, LoamLoopResult, loam_align_batch  # noqa: F401
from .registration import loam_extract_features, loam_frame_begin_batch, pack_xyzirt  # noqa: F401
from .registration import OccupancyGrid, OccupancyMap2D, save_map  # noqa: F401
from .registration import LoamGlobalMapResult  # noqa: F401
from .registration import VoxelLargeResult  # noqa: F401
from .registration import LoamMapLoadResult, LoamMapCropResult, read_arealist, write_arealist  # noqa: F401
from .registration import LoamTilesResult  # noqa: F401
from .registration import (ScanSegment, lidar_xyzirt_segment, lidar_xyzi_segment, depth_segment, rs_to_velodyne, hesai_to_velodyne,  # noqa: F401
                           fuse_lidar_cameras)
from .registration import lidar_desc  # noqa: F401
from .registration import LioOdometry, lio_imu_state  # noqa: F401
