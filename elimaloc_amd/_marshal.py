"""What every module of the Python mirror needs to cross the C ABI: numpy arrays as C pointers, poses as column-major blocks, config
structs made from keywords, result structs as dicts, owned handles."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import check


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _fp(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _colmajor16(T):
    return np.ascontiguousarray(np.asarray(T, dtype=np.float64).reshape(4, 4).T).ravel()


def _ptr(a):
    """a numpy array as the C pointer to its element type (None stays None)"""
    return None if a is None else a.ctypes.data_as(C.POINTER(np.ctypeslib.as_ctypes_type(a.dtype)))


def _pose_block(poses):
    """poses [n, 4, 4] (or one [4, 4]) -> the column-major flat float64 block the C calls read"""
    return np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4).transpose(0, 2, 1)).reshape(-1)


def _coerce(ctype, v):
    """v as a value of a struct field of type ctype: float() for the floating types, a filled array for c_double * n, a nested struct as
    it is, int() for the rest (the integer types)"""
    if issubclass(ctype, C.Array):
        return ctype(*[float(x) for x in v])
    if issubclass(ctype, (C.c_double, C.c_float)):
        return float(v)
    return v if issubclass(ctype, C.Structure) else int(v)


def _apply(cfg, kw, no_field):
    """Set the keywords kw on the struct cfg, each coerced by its field's type; a name that is no field, or a `_` padding field, raises
    AttributeError(no_field.format(k=name)) -> cfg."""
    ctypes_of = dict(cfg._fields_)
    for k, v in kw.items():
        if k.startswith("_") or k not in ctypes_of:
            raise AttributeError(no_field.format(k=k))
        setattr(cfg, k, _coerce(ctypes_of[k], v))
    return cfg


def _config(name, Struct, default, kw):
    """The config factory `name`: a Struct filled by the C call `default`, then the keywords kw."""
    cfg = Struct()
    getattr(_lib.lib(), default)(C.byref(cfg))
    return _apply(cfg, kw, name + " has no field {k}")


def _counts(st):
    """a struct of counters as a dict of ints, in field order, without the `_` padding"""
    return {k: int(getattr(st, k)) for k, _ in st._fields_ if not k.startswith("_")}


def _sized(ctx, name, call, make, limit=None):
    """The size-then-fill pair of a C call that answers into buffers of the caller's: call(None, 0, byref(n)) asks for the size,
    make(rows) makes the buffers (never empty), call(buffers, m, byref(n)) fills them -> (m, buffers), m the size or `limit` if less."""
    n = C.c_size_t(0)
    check(call(None, 0, C.byref(n)), ctx._h, name)
    m = n.value if limit is None else min(n.value, int(limit))
    bufs = make(max(m, 1))
    check(call(bufs, m, C.byref(n)), ctx._h, name)
    return m, bufs


class _Owned:
    """An object that owns one C handle, kept in the attribute _attr: close() hands it to _destroy and forgets it, garbage collection
    closes quietly."""
    _attr = "_h"

    def close(self):
        h = getattr(self, self._attr, None)
        if h:
            self._destroy(h)
            setattr(self, self._attr, None)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _result_dict(r, trace=None):
    d = dict(T=np.array(r.T).reshape(4, 4).T.copy(), is_success=bool(r.is_success), iterations=int(r.iterations),
             gate=int(r.gate), path=int(r.path), fitness_score=float(r.fitness_score), d_fitness=float(r.d_fitness),
             local_cov=np.array(r.local_cov).reshape(6, 6).T.copy(), n_corr_last=float(r.n_corr_last),
             point_iterations=float(r.point_iterations), n_cand_total=float(r.n_cand_total),
             n_occ_total=float(r.n_occ_total), fallback_blocks=float(r.fallback_blocks), n_tested_total=float(r.n_tested_total))
    if trace is not None:
        its = []
        for k in range(min(r.iterations, _lib.MAX_ITER_TRACE)):
            t = trace[k]
            its.append(dict(n_corr=t.n_corr, JTJ=np.array(t.JTJ).reshape(6, 6).T.copy(), JTr=np.array(t.JTr),
                            residual_sum=t.residual_sum, x=np.array(t.x), step_norm=t.step_norm,
                            T=np.array(t.T).reshape(4, 4).T.copy()))
        d["iters"] = its
    return d
