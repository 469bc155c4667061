"""2D occupancy map (pcm_occ_*): the occupancy methods of a context, the map in a context of its own,
and the reference's saveMap files."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from ._binding import Context, fill_params
from .scan import _ScanMixin


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


_OCC_FIELDS = {f[0] for f in capi.PcmOccParams._fields_} - {"reserved"}


def _occ_key(p, k, v):
    """Every field takes a float but the two switches; what is no field is left to raise."""
    if k not in _OCC_FIELDS:
        return False
    setattr(p, k, int(bool(v)) if k in ("fill_with_white", "use_nan") else float(v))
    return True


def _occ_unknown(k):
    return TypeError("unknown occupancy parameter %r" % k)


class _OccMixin:
    """pcm_occ_* of the context ``self._h``."""

    def occ_reset(self, **params):
        p = fill_params(capi.PcmOccParams, self._L.pcm_occ_default_params, params, _occ_key, _occ_unknown)
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


class OccupancyMap2D(Context, _OccMixin, _ScanMixin):
    """jueying_slam's 2D occupancy mapping tool on one HIP device, in a context of its own.

    ``insert_scans(clouds, poses)`` = getScan + processScan per cloud, ``map()`` = getGridMap, ``save_map(prefix)`` = saveMap."""

    def __init__(self, device: int = 0, **params):
        super().__init__(device)
        self.occ_reset(**params)

    reset = _OccMixin.occ_reset
    insert_scans = _OccMixin.occ_insert_scans
    scan = _OccMixin.occ_scan
    status = _OccMixin.occ_status
    map = _OccMixin.occ_map
    pgm = _OccMixin.occ_pgm
    counts = _OccMixin.occ_counts
    save_map = _OccMixin.occ_save_map
