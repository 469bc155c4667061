"""3D occupancy map (pcm_octo_*): octomap_server's insertScan, cell and occupied-centre outputs, the projected
2D map and map_saver's files, in a context of its own or on an existing context.  All compute goes through the C ABI (``capi``)."""
from __future__ import annotations

import ctypes as C
import dataclasses

import numpy as np

from . import capi
from ._binding import Context, buffer_arg, fill_params
from .occ import pgm_bytes

_INT_FIELDS = ("filter_speckles", "initial_cells", "max_cells")
CELL_DTYPE = np.dtype([("key", np.int32, 3), ("log_odds", np.float32)])


@dataclasses.dataclass
class ProjectedMap:
    """projected_map as nav_msgs/OccupancyGrid holds it; width = height = 0 while the map has at most one cell."""
    data: np.ndarray        # (height, width) int8: -1 unknown, 0 free, 100 occupied
    resolution: float
    origin_x: float
    origin_y: float
    min_key: tuple          # key of column 0 / row 0

    @property
    def width(self) -> int:
        return int(self.data.shape[1])

    @property
    def height(self) -> int:
        return int(self.data.shape[0])


def _octo_key(p, k, v):
    if k in _INT_FIELDS:
        setattr(p, k, int(v))
        return True
    return False


def _struct_dict(s) -> dict:
    out = {}
    for k, _ in s._fields_:
        if k.startswith("reserved"):
            continue
        v = getattr(s, k)
        out[k] = tuple(v) if hasattr(v, "__len__") else v
    return out


def _cloud(a):
    """(pointer, rows, stride, memory, keep-alive) of a cloud or of None."""
    if a is None:
        return None, 0, None, None, None
    return buffer_arg(a, (3, None), convert=True)


def octo_reset(ctx: Context, **params):
    """An empty 3D map with pcm_octo_params' defaults and the keyword overrides."""
    p = fill_params(capi.PcmOctoParams, ctx._L.pcm_octo_default_params, params, _octo_key)
    ctx._check(ctx._L.pcm_octo_reset(ctx._h, C.byref(p)))


def octo_insert_scan(ctx: Context, nonground=None, origin=(0.0, 0.0, 0.0), ground=None, sensor_to_world=None, allow=(capi.PCM_OK,)) -> dict:
    """insertCloudCallback + insertScan of one cloud.  Clouds are (N,>=3) float32 host arrays or device tensors of one stride and
    one memory kind; ``ground`` clears only.  Returns pcm_octo_insert_result as a dict."""
    gp, gn, gs, gm, gk = _cloud(ground)
    np_, nn, ns, nm, nk = _cloud(nonground)
    if gn and nn and (gs, gm) != (ns, nm):
        raise ValueError("ground and nonground must share the stride and the memory kind")
    stride, mem = (ns, nm) if nn or not gn else (gs, gm)
    if stride is None:
        stride, mem = 12, capi.MEM_HOST
    o = np.ascontiguousarray(origin, np.float32).reshape(3)
    T = None if sensor_to_world is None else np.ascontiguousarray(sensor_to_world, np.float32).reshape(4, 4)
    r = capi.PcmOctoInsertResult()
    rc = ctx._L.pcm_octo_insert_scan(ctx._h, gp, gn, np_, nn, stride, mem, o.ctypes.data, None if T is None else T.ctypes.data, C.byref(r))
    ctx._check(rc, allow)
    return _struct_dict(r)


def octo_insert_keyframes(ctx: Context, first: int, n: int):
    """Key frames first .. first + n - 1 of a LOAM context's store, one scan each, in place under their current poses."""
    ctx._check(ctx._L.pcm_octo_insert_keyframes(ctx._h, int(first), int(n)))


def octo_info(ctx: Context) -> dict:
    s = capi.PcmOctoMapInfo()
    ctx._check(ctx._L.pcm_octo_info(ctx._h, C.byref(s)))
    return _struct_dict(s)


def _records(ctx, call, out, dtype, bound):
    """One call: into ``out``, or into a new host array of ``bound`` records (an upper bound from the statistics), cut to the count."""
    n = C.c_size_t(0)
    if out is not None:
        ptr, cap, _, mem, _ = buffer_arg(out, None, 16, write=True)
        ctx._check(call(ctx._h, ptr, cap, mem, C.byref(n)))
        return n.value
    res = np.zeros(bound, dtype)
    if bound:
        ctx._check(call(ctx._h, res.ctypes.data, bound, capi.MEM_HOST, C.byref(n)))
    return res[:n.value]


def octo_cells(ctx: Context, out=None):
    """The known cells sorted by packed key: a CELL_DTYPE array, or the count when ``out`` (a float32 host array or device tensor
    of 16-byte records) takes them."""
    return _records(ctx, ctx._L.pcm_octo_get_cells, out, CELL_DTYPE, 0 if out is not None else octo_info(ctx)["cells"])


def octo_occupied_points(ctx: Context, out=None):
    """octomap_point_cloud_centers: (n, 4) float32 (x, y, z, log-odds) in the cells' order, or the count with ``out``."""
    r = _records(ctx, ctx._L.pcm_octo_get_occupied, out, np.dtype((np.float32, 4)), 0 if out is not None else octo_info(ctx)["occupied"])
    return r if out is not None else r.reshape(-1, 4)


MARK_VARIANTS = {"lane": 0, "wave": 1, "lane_no_dry_walk": 2, "wave_no_dry_walk": 3}


def octo_debug(ctx: Context, mark_variant="lane", timed: bool = False):
    """Measurement hook (pcm_octo_debug): the mark kernel's variant (one of MARK_VARIANTS; "lane" and "wave" give the same map, the
    others are for measuring only) and event timing of the phases."""
    ctx._check(ctx._L.pcm_octo_debug(ctx._h, MARK_VARIANTS[mark_variant], int(bool(timed))))


def octo_phase_ms(ctx: Context) -> dict:
    """The phases of the last insert (pcm_octo_phase_ms): mark and apply need ``octo_debug(timed=True)``."""
    ms = (C.c_float * 4)()
    ctx._check(ctx._L.pcm_octo_phase_ms(ctx._h, ms))
    return {"mark_ms": ms[0], "apply_ms": ms[1], "growth_ms": ms[2], "mark_passes": int(ms[3])}


def octo_project(ctx: Context) -> ProjectedMap:
    g = capi.PcmOctoGridInfo()
    ctx._check(ctx._L.pcm_octo_project(ctx._h, C.byref(g), None, 0, capi.MEM_HOST))
    data = np.zeros((g.height, g.width), np.int8)
    if data.size:
        ctx._check(ctx._L.pcm_octo_project(ctx._h, C.byref(g), data.ctypes.data, data.size, capi.MEM_HOST))
    return ProjectedMap(data, g.resolution, g.origin_x, g.origin_y, (g.min_key_x, g.min_key_y))


def octo_pgm(ctx: Context) -> np.ndarray:
    """(height, width) uint8: the body of map_saver's P5 image, rows top-down."""
    g = capi.PcmOctoGridInfo()
    ctx._check(ctx._L.pcm_octo_project(ctx._h, C.byref(g), None, 0, capi.MEM_HOST))
    out = np.zeros((g.height, g.width), np.uint8)
    if out.size:
        ctx._check(ctx._L.pcm_octo_get_pgm(ctx._h, out.ctypes.data, out.size, capi.MEM_HOST))
    return out


def save_map(path_prefix: str, grid: ProjectedMap, pgm: np.ndarray = None):
    """<prefix>.pgm and <prefix>.yaml in the byte layout of map_saver.cpp:72-84, :115; returns the two paths.  An empty map writes
    nothing and returns None (map_saver never receives one)."""
    if grid.width == 0 or grid.height == 0:
        return None
    p, y = path_prefix + ".pgm", path_prefix + ".yaml"
    with open(p, "wb") as f:
        f.write(("P5\n# CREATOR: map_saver.cpp %.3f m/pix\n%d %d\n255\n" % (grid.resolution, grid.width, grid.height)).encode())
        f.write(pgm_bytes(grid.data) if pgm is None else np.ascontiguousarray(pgm, np.uint8).tobytes())
    with open(y, "wb") as f:
        f.write(("image: %s\nresolution: %f\norigin: [%f, %f, 0.00]\nnegate: 0\noccupied_thresh: 0.65\nfree_thresh: 0.196\n\n"
                 % (p, grid.resolution, grid.origin_x, grid.origin_y)).encode())
    return p, y


def octo_save_map(ctx: Context, path_prefix: str):
    return save_map(path_prefix, octo_project(ctx), octo_pgm(ctx))


class OccupancyMap3D(Context):
    """octomap_server's map on one HIP device, in a context of its own.

    ``insert_scan(nonground, origin, ground=None, sensor_to_world=None)`` = insertCloudCallback + insertScan, ``project()`` =
    projected_map, ``occupied_points()`` = octomap_point_cloud_centers, ``save_map(prefix)`` = map_saver."""

    def __init__(self, device: int = 0, **params):
        super().__init__(device)
        octo_reset(self, **params)

    reset = octo_reset
    insert_scan = octo_insert_scan
    info = octo_info
    cells = octo_cells
    occupied_points = octo_occupied_points
    project = octo_project
    pgm = octo_pgm
    debug = octo_debug
    phase_ms = octo_phase_ms
    save_map = octo_save_map
