"""The device side every other module of the mirror starts from: the Context (one GPU and its stream, or the lead of a device group),
resident Scans and pinned host buffers."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ElmError, check
from ._marshal import _Owned, _fp


class Context(_Owned):
    """One GPU, one HIP stream -- or, Context.multi([0, 1, ...]), the LEAD context of a device group: N GPUs inside this process, maps
    replicated, scans sharded, one all-reduce of the packed sums per ICP iteration (elm_ctx_create_multi).  elm_ctx_create fails without a
    gfx950 device."""

    def __init__(self, device_id=0, _devices=None):
        self._h = C.c_void_p()
        if _devices is None:
            check(_lib.lib().elm_ctx_create(device_id, C.byref(self._h)), None, "elm_ctx_create")
        else:
            ids = (C.c_int * len(_devices))(*[int(d) for d in _devices])
            check(_lib.lib().elm_ctx_create_multi(ids, len(_devices), C.byref(self._h)), None, "elm_ctx_create_multi")
            device_id = int(_devices[0])
        self.device_id = device_id
        self._hook_ref = None

    @classmethod
    def multi(cls, device_ids):
        """the lead context of a device group over device_ids (an id may repeat: ranks sharing a GPU exchange through host memory)"""
        return cls(_devices=list(device_ids))

    def group_info(self):
        """(ranks, exchange, device ids): exchange 0 = a plain context, 1 = RCCL, 2 = host memory"""
        n, ex = C.c_int(0), C.c_int(0)
        ids = (C.c_int * 64)()
        check(_lib.lib().elm_ctx_group_info(self._h, C.byref(n), C.byref(ex), ids, 64), self._h, "elm_ctx_group_info")
        return n.value, ex.value, [ids[i] for i in range(n.value)]

    def _destroy(self, h):
        _lib.lib().elm_ctx_destroy(h)

    def synchronize(self):
        check(_lib.lib().elm_ctx_synchronize(self._h), self._h, "elm_ctx_synchronize")

    @property
    def stream(self):
        return _lib.lib().elm_ctx_stream(self._h)

    def set_work_counters(self, on=True):
        """n_cand_total / n_occ_total / n_tested_total / fallback_blocks of the results: off by default (they read 0), on = instrumented kernels."""
        check(_lib.lib().elm_ctx_set_work_counters(self._h, int(bool(on))), self._h, "elm_ctx_set_work_counters")

    def set_profiling(self, on=True):
        check(_lib.lib().elm_ctx_set_profiling(self._h, int(bool(on))), self._h, "elm_ctx_set_profiling")

    def get_profile(self, reset=False):
        p = _lib.Profile()
        check(_lib.lib().elm_ctx_get_profile(self._h, C.byref(p), int(bool(reset))), self._h, "elm_ctx_get_profile")
        return dict(accumulate_launches=int(p.accumulate_launches), solve_steps=int(p.solve_steps),
                    accumulate_ms=float(p.accumulate_ms), solve_ms=float(p.solve_ms))

    def measure_h2d(self, host_ptr, nbytes, reps=5):
        """GB/s of a plain host-to-device copy from host_ptr on this box (the PCIe rate a host-fed stream sits under)."""
        g = C.c_double(0.0)
        check(_lib.lib().elm_ctx_measure_h2d(self._h, C.c_void_p(host_ptr), int(nbytes), int(reps), C.byref(g)), self._h, "elm_ctx_measure_h2d")
        return g.value

    # ---- multi-GPU (RCCL over xGMI): one small all-reduce of the packed normal equations per iteration
    @staticmethod
    def comm_unique_id():
        buf = (C.c_char * _lib.COMM_ID_BYTES)()
        check(_lib.lib().elm_comm_get_unique_id(C.cast(buf, C.c_void_p)), None, "elm_comm_get_unique_id")
        return bytes(buf)

    def comm_init(self, rank, nranks, id_bytes):
        buf = (C.c_char * _lib.COMM_ID_BYTES).from_buffer_copy(id_bytes)
        check(_lib.lib().elm_comm_init(self._h, rank, nranks, C.cast(buf, C.c_void_p)), self._h, "elm_comm_init")

    def comm_destroy(self):
        check(_lib.lib().elm_comm_destroy(self._h), self._h, "elm_comm_destroy")

    def comm_info(self):
        """(rank, nranks) as the RCCL communicator reports them (ncclCommUserRank / ncclCommCount); (0, 0) without one."""
        r, n = C.c_int(0), C.c_int(0)
        check(_lib.lib().elm_comm_info(self._h, C.byref(r), C.byref(n)), self._h, "elm_comm_info")
        return r.value, n.value

    def set_allreduce_hook(self, fn):
        """fn(dev_ptr:int, n_doubles:int, hip_stream:int) -> 0 on success; None removes the hook."""
        if fn is None:
            self._hook_ref = _lib.ALLREDUCE_FN(0)
        else:
            self.hook_error = None

            def call(p, n, s, u):
                # an exception must not escape a ctypes callback (it would be printed and swallowed, the exchange reported as done): the
                # call that is exchanging ends with ELM_ERR_COMM "allreduce hook failed" and the exception is kept in hook_error
                try:
                    return int(fn(p, n, s))
                except BaseException as e:  # noqa: BLE001
                    self.hook_error = e
                    return 1
            self._hook_ref = _lib.ALLREDUCE_FN(call)
        check(_lib.lib().elm_comm_set_hook(self._h, self._hook_ref, None), self._h, "elm_comm_set_hook")


_default_ctx = None


def default_context():
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context(0)
    return _default_ctx


class Scan(_Owned):
    """A device-resident source scan (sensor frame)."""

    def __init__(self, ctx, xyz, n_total=None):
        self.ctx = ctx
        pts = np.ascontiguousarray(xyz, dtype=np.float32).reshape(-1, 3)
        self.n = pts.shape[0]
        self._h = C.c_void_p()
        check(_lib.lib().elm_scan_upload(ctx._h, _fp(pts), self.n, self.n if n_total is None else int(n_total),
                                         C.byref(self._h)), ctx._h, "elm_scan_upload")

    def points(self):
        """The resident points in device order (elm_scan_download) -> float32 [n, 3]."""
        out = np.zeros((max(self.n, 1), 3), np.float32)
        check(_lib.lib().elm_scan_download(self._h, _fp(out), self.n), self.ctx._h, "elm_scan_download")
        return out[:self.n]

    def _destroy(self, h):
        _lib.lib().elm_scan_destroy(h)


def _resident(ctx, scan):
    """a Scan, or (m, 3) points uploaded for the call"""
    return scan if isinstance(scan, Scan) else Scan(ctx, scan)


def _callers_order(sc, given):
    """The index that puts the per-beam outputs of the resident scan sc back into the order of `given`, the points it was uploaded from;
    None for a Scan (it is answered in its resident order) or an empty scan.  Equal points are equal beams with equal outputs, so the
    points are matched by their bytes."""
    if isinstance(given, Scan) or not sc.n:
        return None
    key = np.dtype((np.void, 12))
    res = np.ascontiguousarray(sc.points()).view(key).ravel()
    own = np.ascontiguousarray(given, dtype=np.float32).reshape(-1, 3).view(key).ravel()
    order = np.argsort(res, kind="stable")
    return order[np.searchsorted(res[order], own)]


class PinnedBuffer(_Owned):
    """Page-locked host memory (elm_host_alloc) viewed as a float32 numpy array."""

    def __init__(self, n_floats):
        self.ptr = _lib.lib().elm_host_alloc(4 * int(n_floats))
        if not self.ptr:
            raise ElmError("elm_host_alloc failed")
        self.array = np.ctypeslib.as_array((C.c_float * int(n_floats)).from_address(self.ptr))

    _attr = "ptr"

    def _destroy(self, ptr):
        self.array = None
        _lib.lib().elm_host_free(ptr)
