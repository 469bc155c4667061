"""What every module of the binding shares: the context base class, the parameter filler and the buffer helpers.

All compute goes through the C ABI of include/pcm_amd.h (``capi``); nothing here touches oracle/."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import capi


def default_config(model: str) -> capi.PcmConfig:
    """pcm_default_config with the model set."""
    cfg = capi.PcmConfig()
    capi.load_library().pcm_default_config(C.byref(cfg))
    cfg.model = capi.MODEL[model]
    return cfg


class Context:
    """One ``pcm_ctx`` on a HIP device: the library, the handle, the error check and the release."""

    def __init__(self, device: int, cfg: capi.PcmConfig = None):
        self._L = capi.load_library()
        self._h = self._L.pcm_create(device, C.byref(cfg) if cfg is not None else None)
        if not self._h:
            raise capi.PcmError(-3, "pcm_create failed")

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

    def _stored(self, attr: str, message: str):
        """The result struct an earlier call left in ``attr``, or PCM_ERR_NO_INPUT with ``message`` ("X_result before X")."""
        r = getattr(self, attr, None)
        if r is None:
            raise capi.PcmError(-2, message)
        return r

    def _counted(self, call, out=None, cols=None, shape=(4,), dtype=np.float32, store=None):
        """Count, allocate, fill.  ``call(ptr, capacity, memory, n) -> rc`` writes up to ``capacity`` records and sets the
        ``c_size_t`` n.  Without ``out``: asked once with no buffer for the count (an error that still names a count passes),
        then with a new (n, *shape) host array, which returns cut to the n of the second call.  With ``out``: the caller's
        buffer (``buffer_arg(out, cols, write=True)``; cols None = flat 16-byte records) is filled and the count returns; a
        buffer that is too small raises, with the needed count in the message and, where ``store`` names one, in that attribute."""
        n = C.c_size_t(0)
        if out is not None:
            ptr, cap, _, mem, _ = buffer_arg(out, cols, None if cols else 16, write=True)
            rc = call(ptr, cap, mem, n)
            if store:
                setattr(self, store, n.value)
            self._check(rc)
            return n.value
        rc = call(None, 0, capi.MEM_HOST, n)
        if rc != capi.PCM_OK and n.value == 0:
            self._check(rc)
        res = np.zeros((n.value,) + shape, dtype)
        if n.value:
            self._check(call(res.ctypes.data, n.value, capi.MEM_HOST, n))
        return res[:n.value]


def fill_params(cls, default, params: dict, hook=None, unknown=KeyError):
    """A ``cls`` parameter struct as the library's ``default(pointer)`` fills it, with the keyword overrides ``params``.
    ``hook(p, key, value)`` returns True for a key it has dealt with (a flag bit, a table to keep alive, a value to coerce).
    Every other key names a field; an unknown name or a ``reserved*`` field raises ``unknown(key)``."""
    p = cls()
    default(C.byref(p))
    for k, v in params.items():
        if hook is not None and hook(p, k, v):
            continue
        if k.startswith("reserved") or not hasattr(p, k):
            raise unknown(k)
        setattr(p, k, v)
    return p


def buffer_arg(a, cols=None, record=None, f32=True, convert=False, write=False, what="expected"):
    """Classify ``a`` as device memory (a CUDA tensor, used in place) or host memory (anything else) and check it against
    what the call site states -> (pointer, rows, row bytes, memory, keep-alive).

    cols = (lo, hi): a 2-D float32 buffer of lo..hi columns (hi None: no upper bound); its rows are the rows.
    record = bytes: a flat buffer of records of that many bytes, whatever its shape; rows = its bytes // record.  With
    f32=False the elements may be of any type and the bytes must be a whole number of records.
    convert: host input goes through ``np.ascontiguousarray`` (lists, other dtypes, strided arrays and host torch tensors
    pass); without it, it must be a contiguous ndarray of the element type already -- what a buffer the library writes has
    to be.
    write: the library writes the buffer, so a read-only host array is refused."""
    if hasattr(a, "data_ptr") and getattr(a, "is_cuda", False):
        mem, ptr, shape, nbytes = capi.MEM_DEVICE, a.data_ptr(), a.shape, a.numel() * a.element_size()
        ok = a.is_contiguous() and (not f32 or a.dtype.__str__() == "torch.float32")
    else:
        if convert:
            a = np.ascontiguousarray(a, dtype=np.float32 if f32 else None)
        elif not isinstance(a, np.ndarray):
            raise ValueError(_rule(what, cols, record, f32))
        mem, ptr, shape, nbytes = capi.MEM_HOST, a.ctypes.data, a.shape, a.nbytes
        ok = a.flags.c_contiguous and (not f32 or a.dtype == np.float32)
        if write and not a.flags.writeable:
            raise ValueError(_rule(what, cols, record, f32) + " (this one is read-only)")
    if cols is not None:
        if not ok or len(shape) != 2 or shape[1] < cols[0] or (cols[1] is not None and shape[1] > cols[1]):
            raise ValueError(_rule(what, cols, record, f32))
        return ptr, shape[0], shape[1] * 4, mem, a
    if not ok or (not f32 and nbytes % record):
        raise ValueError(_rule(what, cols, record, f32))
    return ptr, nbytes // record, record, mem, a


def _rule(what, cols, record, f32) -> str:
    if cols is None:
        shape = "buffer of %d-byte records" % record
    else:
        lo, hi = cols
        shape = "(N,%s)" % (">=%d" % lo if hi is None else str(lo) if lo == hi else "%d..%d" % (lo, hi))
    return "%s a contiguous %s%s array or device tensor" % (what, "float32 " if f32 else "", shape)
