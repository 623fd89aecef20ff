"""Host-side mirror of the reference's operator interface for the registration hot path.

Same names, argument meaning and error behaviour as
  pcm_matching/include/registration.hpp      (IcpMethod :60, RegistrationConfig :62-85, Registration :101-230)
  pcm_matching/include/voxel_hash_map.hpp    (VoxelHashMap :89-335)
so that parity tests read like calls into the reference.  Everything numerical happens in the C-ABI library
(HIP kernels); this file only marshals numpy arrays.  Out-params of the C++ signatures are returned as tuples.
"""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import (ElmError, EvidenceConfigC, EvidenceRuleC, EvidenceStatsC, GrowthConfigC, GrowthObjectC, GrowthObjectRuleC, GrowthObjectStatsC, GrowthRuleC, GrowthStatsC, FreeSpaceConfigC, FreeSpaceStatsC, RayCastConfigC, RayCastStatsC, GlobalRelocConfigC, GlobalRelocStats, RegConfig, RegResult, IterTrace, MapInfo, RelocCandidate, RelocConfigC,
                   check)


class IcpMethod(enum.IntEnum):  # reg.hpp:60
    P2P = 0
    GICP = 1
    VGICP = 2
    AVGICP = 3


def RegistrationConfig(**kw):
    """RegistrationConfig with the shipped defaults of config/localization.ini:80-105."""
    cfg = RegConfig()
    _lib.lib().elm_reg_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"RegistrationConfig has no field {k}")
        setattr(cfg, k, int(v) if k in ("icp_method", "max_iteration", "i_max_thread", "use_radar_cov") else v)
    return cfg


def RelocConfig(**kw):
    """elm_reloc_config with its defaults (5 m / 0.5 m xy window, 180 deg / 2 deg yaw, 50 m score range, 8192 score points, top 16 after
    non-maximum suppression at 1.0 m / 6 deg, 64 KiB LDS / 64 MiB bitmap budgets)."""
    cfg = RelocConfigC()
    _lib.lib().elm_reloc_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"RelocConfig has no field {k}")
        setattr(cfg, k, int(v) if k in ("max_score_points", "top_k", "lds_budget_bytes", "bitmap_max_bytes") else float(v))
    return cfg


def GlobalRelocConfig(**kw):
    """elm_reloc_global_config with its defaults (the map's xy bounds (NaN rectangle), 0.5 m / 2 deg lattice, 50 m score range, counted points
    1.0 m or more above the ground, 8192 score points, top 16 after non-maximum suppression at 1.0 m / 6 deg, pool 64, kz span 64, 256 MiB)."""
    cfg = GlobalRelocConfigC()
    _lib.lib().elm_reloc_global_config_default(C.byref(cfg))
    for k, v in kw.items():
        if not hasattr(cfg, k):
            raise AttributeError(f"GlobalRelocConfig has no field {k}")
        setattr(cfg, k, int(v) if k in ("max_score_points", "top_k", "pool_min", "max_kz_span", "bitmap_max_bytes") else float(v))
    return cfg


def FreeSpaceConfig(**kw):
    """elm_freespace_config with its defaults (sub 4, step_m 0 = cell / 2 of the map, start 1 m, range 2 .. 50 m, end margins 1 m / 0.2 L,
    min_hits 2, max_samples 1024, origin 0)."""
    cfg = FreeSpaceConfigC()
    _lib.lib().elm_freespace_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(cfg, k):
            raise AttributeError(f"FreeSpaceConfig has no field {k}")
        if k == "origin":
            cfg.origin = (C.c_double * 3)(*[float(x) for x in v])
        else:
            setattr(cfg, k, int(v) if k in ("sub", "min_hits", "max_samples") else float(v))
    return cfg


_FREE_FIELDS = ("n_counted", "n_pierced", "n_end_occupied", "n_supported", "n_samples", "n_hit_samples")


def FreeSpaceStats(st):
    """elm_freespace_stats of one pose as a dict (+ pierced_share = n_pierced / n_counted, 0 without counted rays)."""
    d = {k: int(getattr(st, k)) for k in _FREE_FIELDS}
    d["pierced_share"] = d["n_pierced"] / d["n_counted"] if d["n_counted"] else 0.0
    return d


def RayCastConfig(**kw):
    """elm_raycast_config with its defaults (sub 4, max_steps 4096, range 1 .. 100 m, compared 2 .. 50 m, tol_m 0.5, tol_frac 0.02,
    origin 0)."""
    cfg = RayCastConfigC()
    _lib.lib().elm_raycast_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(cfg, k):
            raise AttributeError(f"RayCastConfig has no field {k}")
        if k == "origin":
            cfg.origin = (C.c_double * 3)(*[float(x) for x in v])
        else:
            setattr(cfg, k, int(v) if k in ("sub", "max_steps") else float(v))
    return cfg


_RAY_FIELDS = ("n_cast", "n_hit", "n_miss", "n_truncated", "n_compared", "n_match", "n_through", "n_front", "n_steps")


def RayCastStats(st):
    """elm_raycast_stats of one pose as a dict (+ match_share / through_share / front_share of the compared beams, 0 without any)."""
    d = {k: int(getattr(st, k)) for k in _RAY_FIELDS}
    for k in ("match", "through", "front"):
        d[k + "_share"] = d["n_" + k] / d["n_compared"] if d["n_compared"] else 0.0
    return d


def EvidenceConfig(**kw):
    """elm_evidence_config with its defaults (sub 4, max_steps 4096, walk from 1 m, observing 2 .. 50 m, end margins 1 m / 0.2 L, origin 0)."""
    cfg = EvidenceConfigC()
    _lib.lib().elm_evidence_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(cfg, k):
            raise AttributeError(f"EvidenceConfig has no field {k}")
        if k == "origin":
            cfg.origin = (C.c_double * 3)(*[float(x) for x in v])
        else:
            setattr(cfg, k, int(v) if k in ("sub", "max_steps") else float(v))
    return cfg


def EvidenceRule(**kw):
    """elm_evidence_rule with its defaults (min_through 3, through_per_hit 4): a cell is stale when through >= min_through and
    through >= through_per_hit * hit.  A starting point, not a measured optimum."""
    rule = EvidenceRuleC()
    _lib.lib().elm_evidence_rule_default(C.byref(rule))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(rule, k):
            raise AttributeError(f"EvidenceRule has no field {k}")
        setattr(rule, k, int(v))
    return rule


_EVID_FIELDS = ("n_cast", "n_observing", "n_walked", "n_truncated", "n_through_beams", "n_end_hit", "n_end_free", "n_through_events", "n_steps")


def EvidenceStats(st):
    """elm_evidence_stats of one observation as a dict."""
    return {k: int(getattr(st, k)) for k in _EVID_FIELDS}


def GrowthConfig(**kw):
    """elm_growth_config with its defaults: the EvidenceConfig defaults and clearance_cells 1 (an end point within that many cells of an
    occupied cell is the old surface, not new structure; 0, 1 or 2 -- a starting point, not a measured optimum)."""
    cfg = GrowthConfigC()
    _lib.lib().elm_growth_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(cfg, k):
            raise AttributeError(f"GrowthConfig has no field {k}")
        if k == "origin":
            cfg.origin = (C.c_double * 3)(*[float(x) for x in v])
        else:
            setattr(cfg, k, int(v) if k in ("sub", "max_steps", "clearance_cells") else float(v))
    return cfg


def GrowthRule(**kw):
    """elm_growth_rule with its defaults (min_hit 3, hit_per_through 4): a candidate cell has appeared when hit >= min_hit and
    hit >= hit_per_through * through.  A starting point, not a measured optimum."""
    rule = GrowthRuleC()
    _lib.lib().elm_growth_rule_default(C.byref(rule))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(rule, k):
            raise AttributeError(f"GrowthRule has no field {k}")
        setattr(rule, k, int(v))
    return rule


_GROWTH_FIELDS = ("n_cast", "n_observing", "n_walked", "n_truncated", "n_end_hit", "n_end_near", "n_end_new", "n_end_out", "n_through_beams",
                  "n_dropped", "n_through_events", "n_steps")


def GrowthStats(st):
    """elm_growth_stats of one observation as a dict."""
    return {k: int(getattr(st, k)) for k in _GROWTH_FIELDS}


def GrowthObjectRule(**kw):
    """elm_growth_object_rule with its defaults (min_hit 3, hit_per_through 4, connectivity 26, min_cells 1): which candidate cells are
    members (GrowthRule's rule), which of them are adjacent (6, 18 or 26) and how many cells make an object.  Starting points, not
    measured optima."""
    rule = GrowthObjectRuleC()
    _lib.lib().elm_growth_object_rule_default(C.byref(rule))
    for k, v in kw.items():
        if k.startswith("_") or not hasattr(rule, k):
            raise AttributeError(f"GrowthObjectRule has no field {k}")
        setattr(rule, k, int(v))
    return rule


_GROWTH_OBJECT_FIELDS = ("n_members", "n_objects", "n_small", "n_small_cells", "max_cells")


def _global_stats_dict(st):
    L = int(st.levels)
    return dict(lattice_poses=int(st.lattice_poses), valid_leaves=int(st.valid_leaves), nx=int(st.nx), ny=int(st.ny), n_yaw=int(st.n_yaw),
                levels=L, n_counted=int(st.n_counted), passes=int(st.passes), tau=int(st.tau),
                nodes_bounded=[int(st.nodes_bounded[l]) for l in range(L + 1)], nodes_kept=[int(st.nodes_kept[l]) for l in range(L + 1)],
                leaves_scored=int(st.leaves_scored), point_evals=int(st.point_evals), ms_ground=float(st.ms_ground),
                ms_search=float(st.ms_search), ms_refine=float(st.ms_refine))


def MakeHypotheses(guess, reloc=None):
    """The relocalization hypotheses around guess (elm_reloc_make_hypotheses) -> [n, 4, 4], index h = (k W + (i + m)) W + (j + m)."""
    cfg = reloc if reloc is not None else RelocConfig()
    T = _colmajor16(guess)
    n = C.c_size_t(0)
    check(_lib.lib().elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), None, 0, C.byref(n)), None, "elm_reloc_make_hypotheses")
    out = np.empty((n.value, 16))
    check(_lib.lib().elm_reloc_make_hypotheses(_dp(T), C.byref(cfg), _dp(out), n.value, C.byref(n)), None, "elm_reloc_make_hypotheses")
    return out.reshape(-1, 4, 4).transpose(0, 2, 1).copy()


def _candidate_dict(c):
    return dict(T0=np.array(c.T0).reshape(4, 4).T.copy(), T=np.array(c.T).reshape(4, 4).T.copy(), score=int(c.score),
                hyp_index=int(c.hyp_index), is_success=bool(c.is_success), iterations=int(c.iterations), fitness_score=float(c.fitness_score))


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


class _MapChild(_Owned):
    """An owned handle (_h) made for a map as it was built then (map, _map_h): _handle() gives it while both stand."""

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ElmError(f"{type(self).__name__}: closed")
        if self.map._h is not self._map_h:
            raise ElmError(f"{type(self).__name__}: its map was rebuilt or cleared")
        return self._h


def _accumulate(obj, single, batch, StatsC, stats_dict, scans, poses, cfg, events):
    """MapEvidence.Accumulate and MapGrowth.Accumulate: `single` / `batch` name the two C entry points."""
    h, L, who = obj._handle(), _lib.lib(), type(obj).__name__
    if isinstance(scans, Scan) or (isinstance(scans, np.ndarray) and scans.ndim == 2):
        sc = _resident(obj.ctx, scans)
        st = StatsC()
        ev = np.zeros(max(sc.n, 1), np.uint16) if events else None
        check(getattr(L, single)(obj.ctx._h, h, sc._h, _dp(_colmajor16(poses)), C.byref(cfg), C.byref(st), _ptr(ev)), obj.ctx._h, single)
        if not events:
            return stats_dict(st)
        ev, back = ev[:sc.n], _callers_order(sc, scans)
        return stats_dict(st), (ev if back is None else np.ascontiguousarray(ev[back]))
    if events:
        raise ElmError(f"{who}.Accumulate: events are returned for a single scan only")
    scs = [_resident(obj.ctx, s) for s in scans]
    P = _pose_block(poses)
    n = len(scs)
    if P.size // 16 != n:
        raise ElmError(f"{who}.Accumulate: one pose per scan")
    hs = (C.c_void_p * max(n, 1))(*[s._h.value for s in scs])
    st = (StatsC * max(n, 1))()
    check(getattr(L, batch)(obj.ctx._h, h, hs, _dp(P), n, C.byref(cfg), st), obj.ctx._h, batch)
    return [stats_dict(st[j]) for j in range(n)]


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


class VoxelHashMap:
    """vhm.hpp:89-335.  Points are (n,3) float32 arrays (the PCD map and the LiDAR are float32, pcm.hpp:205-215)."""

    def __init__(self, voxel_size=1.0, max_points_per_voxel=30, ctx=None, device_build=False, device_index=False):
        """device_build: the map is built by elm_map_build_device (the same map, byte for byte) instead of the host build.
        device_index: the map's P2P / GICP cell grid is laid out on the device (elm_map_set_index_build; the same grid, byte for byte);
        maps derived from this one (Updated, WithoutStale(device=True), WithAppeared(device=True)) keep the preference."""
        self.ctx = ctx or default_context()
        self.voxel_size_ = float(voxel_size)
        self.max_points_per_voxel_ = int(max_points_per_voxel)
        self.device_build_ = bool(device_build)
        self.device_index_ = bool(device_index)
        self._pending = []
        self._derived = False  # made from a base map on the device: _pending is filled from a download when it is first needed
        self._h = None
        self._want_voxel_cov = False
        self._want_point_cov = None

    def Init(self, voxel_size, max_points_per_voxel):  # vhm.cpp:26-29
        self.voxel_size_ = float(voxel_size)
        self.max_points_per_voxel_ = int(max_points_per_voxel)

    def Clear(self):  # vhm.hpp:324
        self._release()
        self._pending = []
        self._derived = False

    def _release(self):
        if self._h is not None:
            _lib.lib().elm_map_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self._release()
        except Exception:
            pass

    def AddPoints(self, points):  # vhm.cpp:270-285
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        if pts.shape[0] == 0:
            return
        if self._derived:  # stored points replay to themselves: stored ++ points builds what AddPoints(points) makes of this map
            self._pending = [self.Pointcloud().astype(np.float32)] if not self.Empty() else []
            self._derived = False
        self._pending.append(pts)
        self._release()  # rebuilt on next use; sequential AddPoints == one AddPoints of the concatenation

    def Update(self, points, origin=None):  # vhm.cpp:268
        self.AddPoints(points)

    def _handle(self):
        if self._h is None:
            allp = (np.concatenate(self._pending, axis=0) if len(self._pending) > 1 else
                    (self._pending[0] if self._pending else np.zeros((0, 3), np.float32)))
            self._pending = [allp] if allp.shape[0] else []
            h = C.c_void_p()
            if self.device_build_:
                check(_lib.lib().elm_map_build_device(self.ctx._h, None, None, _fp(allp), allp.shape[0], self.voxel_size_,
                                                      self.max_points_per_voxel_, C.byref(h)), self.ctx._h, "elm_map_build_device")
            else:
                check(_lib.lib().elm_map_build(self.ctx._h, _fp(allp), allp.shape[0], self.voxel_size_,
                                               self.max_points_per_voxel_, C.byref(h)), self.ctx._h, "elm_map_build")
            self._h = h
            self._set_index_build()
            if self._want_voxel_cov:
                check(_lib.lib().elm_map_cal_voxel_cov_all(self._h), self.ctx._h, "elm_map_cal_voxel_cov_all")
            if self._want_point_cov is not None:
                check(_lib.lib().elm_map_cal_point_cov_all(self._h, self._want_point_cov), self.ctx._h,
                      "elm_map_cal_point_cov_all")
        return self._h

    def _set_index_build(self):
        if self.device_index_:
            check(_lib.lib().elm_map_set_index_build(self._h, _lib.INDEX_BUILD_DEVICE), self.ctx._h, "elm_map_set_index_build")

    def _derive(self, drop, extra):
        """A new map (same voxel size, cap, context and build path) built on the device from this map's stored points without those that
        drop (uint8 [n_points], None: none) marks, followed by extra [k, 3]: the stored points stay in HBM."""
        extra = np.ascontiguousarray(extra, dtype=np.float32).reshape(-1, 3)
        out = VoxelHashMap(self.voxel_size_, self.max_points_per_voxel_, self.ctx, self.device_build_, self.device_index_)
        dptr = None
        if drop is not None:
            drop = np.ascontiguousarray(drop, dtype=np.uint8)
            if drop.shape != (int(self.info().n_points),):
                raise ElmError("one drop flag per stored point")
            dptr = drop.ctypes.data_as(C.POINTER(C.c_uint8))
        h = C.c_void_p()
        check(_lib.lib().elm_map_build_device(self.ctx._h, self._handle(), dptr, _fp(extra), extra.shape[0], self.voxel_size_,
                                              self.max_points_per_voxel_, C.byref(h)), self.ctx._h, "elm_map_build_device")
        out._h = h
        out._derived = True
        out._set_index_build()
        return out

    def Updated(self, points):
        """A new map equal to this one after AddPoints(points) (the reference's Update, vhm.cpp:268), built on the device: this map stays
        as it is and resident, and only `points` cross the bus."""
        return self._derive(None, points)

    def UpdatedFromScans(self, scans, poses, keep_center=None, keep_radius=None, stats=False):
        """A new map (same voxel size, cap, context and build path) built on the device from inputs that are already there
        (elm_map_build_device_from): this map's stored points -- all of them, or with keep_center [3] and keep_radius those within the
        closed sphere -- followed by the resident scans (a list of Scan; the same Scan may repeat) at their poses [n, 4, 4] (map <- scan
        frame), each point float32(R p + t).  Nothing but the job table crosses the bus; this map stays as it is.  A map without points
        (never built) gives a build from the scans alone.  stats=True: also the dict of elm_build_sources_stats."""
        if (keep_center is None) != (keep_radius is None):
            raise ElmError("UpdatedFromScans: keep_center and keep_radius go together")
        scans = list(scans)
        for sc in scans:
            if not isinstance(sc, Scan):
                raise ElmError("UpdatedFromScans: the scans are resident Scan objects")
        P = _pose_block(poses) if len(scans) else np.zeros(0)
        if P.size // 16 != len(scans):
            raise ElmError("UpdatedFromScans: one pose per scan")
        out = VoxelHashMap(self.voxel_size_, self.max_points_per_voxel_, self.ctx, self.device_build_, self.device_index_)
        has_base = self._h is not None or bool(self._pending) or keep_center is not None
        src = _lib.BuildSourcesC()
        src.base = self._handle() if has_base else None
        src.keep_within = 0 if keep_center is None else 1
        if keep_center is not None:
            src.keep_center = (C.c_double * 3)(*[float(x) for x in np.asarray(keep_center, dtype=np.float64).reshape(3)])
            src.keep_radius_m = float(keep_radius)
        hs = (C.c_void_p * max(len(scans), 1))(*[sc._h.value for sc in scans])
        src.scans = hs
        src.poses16 = _dp(P) if len(scans) else None
        src.n_jobs = len(scans)
        st = _lib.BuildSourcesStatsC()
        h = C.c_void_p()
        check(_lib.lib().elm_map_build_device_from(self.ctx._h, C.byref(src), self.voxel_size_, self.max_points_per_voxel_, C.byref(h),
                                                   C.byref(st)), self.ctx._h, "elm_map_build_device_from")
        out._h = h
        out._derived = True
        out._set_index_build()
        return (out, {n: int(getattr(st, n)) for n, _ in st._fields_}) if stats else out

    def CalVoxelCovAll(self):  # vhm.hpp:183-193
        self._want_voxel_cov = True
        if self._h is not None:
            check(_lib.lib().elm_map_cal_voxel_cov_all(self._h), self.ctx._h, "elm_map_cal_voxel_cov_all")
        else:
            self._handle()

    def CalPointCovAll(self, d_search_dist):  # vhm.hpp:252-257
        self._want_point_cov = float(d_search_dist)
        if self._h is not None:
            check(_lib.lib().elm_map_cal_point_cov_all(self._h, float(d_search_dist)), self.ctx._h,
                  "elm_map_cal_point_cov_all")
        else:
            self._handle()

    def BuildNeighbourhoods(self):
        """Pay the neighbourhood-list build (P2P/GICP streaming layout) now instead of on the first registration."""
        check(_lib.lib().elm_map_build_neighbourhoods(self._handle()), self.ctx._h, "elm_map_build_neighbourhoods")

    def CellGrid(self):
        """The P2P / GICP cell grid as it lies on the device (elm_map_download_cell_grid; it is not built by this call: ElmError when the
        map has none) -> dict: desc (dict of the descriptor's fields), start uint32 [entries + 4], blocks float32 [n_blocks, 3, 4]
        (x[4] y[4] z[4]), slot_point uint32 [4 n_blocks], tiles uint32 [n_tiles, 2]."""
        L = _lib.lib()
        d = _lib.CellGridDesc()
        check(L.elm_map_download_cell_grid(self._handle(), C.byref(d), None, 0, None, 0, None, 0, None, 0), self.ctx._h,
              "elm_map_download_cell_grid")
        start = np.zeros(int(d.n_start_words), np.uint32)
        blocks = np.zeros((int(d.n_blocks), 3, 4), np.float32)
        slot_point = np.zeros(4 * int(d.n_blocks), np.uint32)
        tiles = np.zeros((int(d.n_tiles), 2), np.uint32)
        u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
        check(L.elm_map_download_cell_grid(self._handle(), C.byref(d), u32(start), start.size, _fp(blocks), blocks.shape[0], u32(slot_point),
                                           slot_point.size, u32(tiles), tiles.shape[0]), self.ctx._h, "elm_map_download_cell_grid")
        return {"desc": {n: int(getattr(d, n)) for n, _ in d._fields_}, "start": start, "blocks": blocks, "slot_point": slot_point,
                "tiles": tiles}

    def IndexBuildStages(self):
        """Device milliseconds of the stages of this map's device index build (elm_map_index_build_stages): box, entries and counts, sort,
        block starts, padding and fill."""
        ms = np.zeros(_lib.INDEX_STAGES)
        check(_lib.lib().elm_map_index_build_stages(self._handle(), _dp(ms)), self.ctx._h, "elm_map_index_build_stages")
        return ms

    def Empty(self):  # vhm.hpp:325
        return bool(_lib.lib().elm_map_empty(self._handle()))

    def info(self):
        mi = MapInfo()
        check(_lib.lib().elm_map_get_info(self._handle(), C.byref(mi)), self.ctx._h, "elm_map_get_info")
        return mi

    def Pointcloud(self, with_cov=False):  # vhm.cpp:245-255
        n = int(self.info().n_points)
        xyz = np.empty((n, 3))
        if not with_cov:
            check(_lib.lib().elm_map_download_points(self._handle(), _dp(xyz), None, None, n), self.ctx._h,
                  "elm_map_download_points")
            return xyz
        cov = np.empty((n, 9)); mean = np.empty((n, 3))
        check(_lib.lib().elm_map_download_points(self._handle(), _dp(xyz), _dp(cov), _dp(mean), n), self.ctx._h,
              "elm_map_download_points")
        return xyz, cov.reshape(n, 3, 3).transpose(0, 2, 1).copy(), mean

    def Voxels(self):
        """(stored keys, point counts, covs, means) of every voxel."""
        n = int(self.info().n_voxels)
        key = np.empty((n, 3), np.int32); npts = np.empty(n, np.int32)
        cov = np.empty((n, 9)); mean = np.empty((n, 3))
        check(_lib.lib().elm_map_download_voxels(self._handle(), key.ctypes.data_as(C.POINTER(C.c_int32)),
                                                 npts.ctypes.data_as(C.POINTER(C.c_int32)), _dp(cov), _dp(mean), n),
              self.ctx._h, "elm_map_download_voxels")
        return key, npts, cov.reshape(n, 3, 3).transpose(0, 2, 1).copy(), mean

    def Covariances(self):  # vhm.cpp:257-265: voxels with more than 2 points
        key, npts, cov, mean = self.Voxels()
        sel = npts > 2
        return cov[sel], mean[sel]

    def FindGroundHeight(self, position):  # vhm.hpp:285-322 -> (found, ground_z)
        z = C.c_double(0.0); found = C.c_int(0)
        check(_lib.lib().elm_map_find_ground_height(self._handle(), float(position[0]), float(position[1]),
                                                    C.byref(z), C.byref(found)), self.ctx._h,
              "elm_map_find_ground_height")
        return bool(found.value), z.value

    def _correspondences(self, what, points, max_dist):
        q = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = q.shape[0]
        cap = n * (7 if what == 2 else 1)
        src = np.empty(max(cap, 1), np.uint32); tgt = np.empty(max(cap, 1), np.int32)
        k = C.c_size_t(0)
        check(_lib.lib().elm_map_get_correspondences(self.ctx._h, self._handle(), int(what), _dp(q), n, float(max_dist),
                                                     src.ctypes.data_as(C.POINTER(C.c_uint32)), tgt.ctypes.data_as(C.POINTER(C.c_int32)),
                                                     cap, C.byref(k)), self.ctx._h, "elm_map_get_correspondences")
        return q, src[:k.value].astype(np.int64), tgt[:k.value].astype(np.int64)

    def GetCorrespondencePoints(self, points, max_correspondence_dist, indices=False):
        """vhm.cpp:31-88 -> (source points [k, 3], target points [k, 3]) in input order; a point with no neighbour bucket at all pairs
        with the reference's default PointStruct at the origin when that is within range (QUIRK, vhm.cpp:37).  indices=True also returns
        (source index, target index in Pointcloud() order or -1)."""
        q, src, tgt = self._correspondences(0, points, max_correspondence_dist)
        mp = self.Pointcloud()
        target = np.where((tgt >= 0)[:, None], mp[np.maximum(tgt, 0)], 0.0) if tgt.size else np.zeros((0, 3))
        return (q[src], target, src, tgt) if indices else (q[src], target)

    def GetCorrespondencesCov(self, points, max_correspondence_dist, indices=False):
        """vhm.cpp:90-151 -> (source points, target means, target covariances [k, 3, 3]): the nearest voxel MEAN among the occupied
        neighbours; none at all: the default CovStruct (mean 0, covariance I) when the origin is within range."""
        return self._cov_pairs(1, points, max_correspondence_dist, indices)

    def GetCorrespondencesAllCov(self, points, max_correspondence_dist, indices=False):
        """vhm.cpp:153-206 -> one pair per occupied FACE neighbour (and the point's own voxel) whose mean is within range, in the
        reference's neighbour order (vhm.cpp:224-230)."""
        return self._cov_pairs(2, points, max_correspondence_dist, indices)

    def _cov_pairs(self, what, points, max_dist, indices):
        q, src, tgt = self._correspondences(what, points, max_dist)
        _, _, cov, mean = self.Voxels()
        ok = tgt >= 0
        tm = np.where(ok[:, None], mean[np.maximum(tgt, 0)], 0.0) if tgt.size else np.zeros((0, 3))
        tc = np.where(ok[:, None, None], cov[np.maximum(tgt, 0)], np.eye(3)) if tgt.size else np.zeros((0, 3, 3))
        return (q[src], tm, tc, src, tgt) if indices else (q[src], tm, tc)

    def ScorePoses(self, scan, poses, cfg=None):
        """Voxel-occupancy scores (elm_map_score_poses) of poses [n, 4, 4] for a scan (a resident Scan, or (m, 3) points uploaded for the
        call): per pose the number of scan points within cfg.score_max_range_m whose stored key under the pose is a voxel of the map."""
        cfg = cfg if cfg is not None else RelocConfig()
        sc = _resident(self.ctx, scan)
        P = _pose_block(poses)
        n = P.size // 16
        out = np.zeros(max(n, 1), np.uint32)
        check(_lib.lib().elm_map_score_poses(self.ctx._h, self._handle(), sc._h, _dp(P), n, C.byref(cfg),
                                             out.ctypes.data_as(C.POINTER(C.c_uint32))), self.ctx._h, "elm_map_score_poses")
        return out[:n]

    def FineCells(self, sub=4):
        """The occupied fine cells (elm_map_fine_cells): floor(stored point / (voxel_size / sub)) -> int32 [n, 3], ascending (x, y, z)."""
        m, out = _sized(self.ctx, "elm_map_fine_cells",
                        lambda b, cap, n: _lib.lib().elm_map_fine_cells(self.ctx._h, self._handle(), int(sub), _ptr(b), cap, n),
                        lambda rows: np.zeros((rows, 3), np.int32))
        return out[:m]

    def CheckFreeSpace(self, scan, poses, cfg=None, hits=False):
        """Free-space check (elm_map_check_free_space) of poses [n, 4, 4] for a scan (a resident Scan, or (m, 3) points uploaded for the
        call): per pose a FreeSpaceStats dict -- the counted rays, those that pass through occupied fine cells of the map before their end
        point (pierced), the end points in / next to an occupied cell, the samples and the occupied samples.  hits=True: also the occupied
        samples of every ray, uint16 [n, m]; in the caller's point order for an array, in the resident order (Scan.points()) for a Scan."""
        cfg = cfg if cfg is not None else FreeSpaceConfig()
        sc = _resident(self.ctx, scan)
        P = _pose_block(poses)
        n = P.size // 16
        st = (FreeSpaceStatsC * max(n, 1))()
        H = np.zeros((max(n, 1), sc.n), np.uint16) if hits else None
        check(_lib.lib().elm_map_check_free_space(self.ctx._h, self._handle(), sc._h, _dp(P), n, C.byref(cfg), st, _ptr(H)), self.ctx._h,
              "elm_map_check_free_space")
        out = [FreeSpaceStats(st[h]) for h in range(n)]
        if not hits:
            return out
        back = _callers_order(sc, scan)
        return out, (H[:n] if back is None else H[:n][:, back])

    def RayCast(self, beams, poses, cfg=None, ranges=False, cells=False, flags=False):
        """Ray cast (elm_map_raycast) of beams at poses [n, 4, 4]: beam i runs from cfg.origin through point i of `beams` (a resident Scan,
        or (m, 3) points uploaded for the call; unit vectors for a sensor model, a real scan to compare its measured ranges).  Per pose a
        RayCastStats dict: the cast beams, those that hit / miss the map / are truncated, the compared beams and how their measured range
        lies to the expected one (match / through / front), the steps walked.  With ranges / cells / flags also a dict of the per-beam
        arrays asked for -- "range_in", "range_out" float64 [n, m] (-1 without a hit), "cell" int32 [n, m, 3] (the hit cell), "flag" uint8
        [n, m] (0 not cast, 1 hit, 2 miss, 3 truncated) -- in the caller's beam order for an array, in the resident order (Scan.points())
        for a Scan."""
        cfg = cfg if cfg is not None else RayCastConfig()
        sc = _resident(self.ctx, beams)
        P = _pose_block(poses)
        n = P.size // 16
        st = (RayCastStatsC * max(n, 1))()
        rows = max(n, 1)
        arr = {}
        if ranges:
            arr["range_in"] = np.full((rows, sc.n), -1.0)
            arr["range_out"] = np.full((rows, sc.n), -1.0)
        if cells:
            arr["cell"] = np.zeros((rows, sc.n, 3), np.int32)
        if flags:
            arr["flag"] = np.zeros((rows, sc.n), np.uint8)
        check(_lib.lib().elm_map_raycast(self.ctx._h, self._handle(), sc._h, _dp(P), n, C.byref(cfg), st, _ptr(arr.get("range_in")),
                                         _ptr(arr.get("range_out")), _ptr(arr.get("cell")), _ptr(arr.get("flag"))), self.ctx._h,
              "elm_map_raycast")
        out = [RayCastStats(st[h]) for h in range(n)]
        if not arr:
            return out
        back = _callers_order(sc, beams)
        return out, {k: v[:n] if back is None else np.ascontiguousarray(v[:n][:, back]) for k, v in arr.items()}

    def RenderScan(self, pose, beams, cfg=None, noise=0.0, seed=None, return_index=False):
        """The scan a sensor at `pose` [4, 4] would record with the beam model `beams` (an (m, 3) array or a resident Scan): one RayCast,
        then for every beam that hits the STORED map point of the hit cell that lies nearest to the beam, expressed in the sensor frame
        (R^T (q - t)), plus N(0, noise) per coordinate (seed) -> float32 [k, 3], k = the beams that hit, in beam order.  The points are
        real map points (as synth.make_scan's), but one per beam and the first surface only.
        Nearest: with s / w the beam's world origin / direction of the ray-casting contract, e = q - s, a = (e_x w_x + e_y w_y) + e_z w_z,
        r = e - w a, the smallest (r_x r_x + r_y r_y) + r_z r_z; the lowest Pointcloud() index on a tie.
        The cell -> point lookup runs on the host from Pointcloud() (numpy; not a hot path).  On grazing ground the first occupied cell
        lies before the true surface point, so the rendered ground rings are somewhat tighter than a real sensor's.
        return_index: also the beam index and the Pointcloud() index of every returned point."""
        cfg = cfg if cfg is not None else RayCastConfig()
        T = np.asarray(pose, dtype=np.float64).reshape(4, 4)
        _, arr = self.RayCast(beams, T[None], cfg, cells=True, flags=True)
        b = (beams.points() if isinstance(beams, Scan) else np.ascontiguousarray(beams, dtype=np.float32).reshape(-1, 3)).astype(np.float64)
        hit = np.flatnonzero(arr["flag"][0] == 1)
        stored = self.Pointcloud() if hit.size else np.zeros((0, 3))

        def codes(k):
            k = np.asarray(k, dtype=np.int64) + (1 << 20)
            return (k[:, 0] << 42) | (k[:, 1] << 21) | k[:, 2]

        cell = self.voxel_size_ / float(cfg.sub)
        pc = codes(np.floor(stored / cell))
        order = np.argsort(pc, kind="stable")
        hc = codes(arr["cell"][0][hit])
        lo, hi = np.searchsorted(pc[order], hc, "left"), np.searchsorted(pc[order], hc, "right")
        cnt = hi - lo
        which = np.repeat(np.arange(hit.size), cnt)                                   # the hit a candidate belongs to
        cand = order[np.repeat(lo, cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
        o = np.array(list(cfg.origin))
        d = b[hit] - o
        with np.errstate(divide="ignore", invalid="ignore"):
            u = d / np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])[:, None]
        s = np.array([((T[r, 0] * o[0] + T[r, 1] * o[1]) + T[r, 2] * o[2]) + T[r, 3] for r in range(3)])
        w = np.stack([(T[r, 0] * u[:, 0] + T[r, 1] * u[:, 1]) + T[r, 2] * u[:, 2] for r in range(3)], 1)
        e = stored[cand] - s
        wc = w[which]
        a = (e[:, 0] * wc[:, 0] + e[:, 1] * wc[:, 1]) + e[:, 2] * wc[:, 2]
        r = e - wc * a[:, None]
        d2 = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        best = np.lexsort((cand, d2, which))                                          # per hit: smallest d2, then lowest index
        first = best[np.flatnonzero(np.r_[True, which[best][1:] != which[best][:-1]])] if best.size else best
        pick = cand[first]
        q = stored[pick] - T[:3, 3]
        R = T[:3, :3]
        local = np.stack([(q[:, 0] * R[0, j] + q[:, 1] * R[1, j]) + q[:, 2] * R[2, j] for j in range(3)], 1)
        if noise > 0.0:
            local = local + np.random.default_rng(seed).normal(0.0, noise, local.shape)
        scan = np.ascontiguousarray(local.astype(np.float32)).reshape(-1, 3)
        return (scan, hit[which[first]], pick) if return_index else scan

    def Evidence(self, sub=4):
        """A MapEvidence of this map: per occupied fine cell (FineCells(sub)) the beams seen through it and the beams that ended in it,
        kept on the device and fed by Accumulate.  It belongs to the map as built now: AddPoints / Clear afterwards invalidate it."""
        return MapEvidence(self, sub)

    def WithoutStale(self, evidence, rule=None, device=False):
        """A new map (same voxel size and cap, same context) built by the usual build from the stored points that evidence.StalePoints(rule)
        does not flag.  device: the same map by the device build; only the flags cross the bus."""
        if evidence.map is not self:
            raise ElmError("WithoutStale: the evidence belongs to another map")
        flags = evidence.StalePoints(rule)
        if device:
            return self._derive(flags.astype(np.uint8), np.zeros((0, 3), np.float32))
        keep = self.Pointcloud()[~flags] if flags.size else np.zeros((0, 3))
        out = VoxelHashMap(self.voxel_size_, self.max_points_per_voxel_, self.ctx)
        out.AddPoints(keep.astype(np.float32))  # stored coordinates are float32 values: the conversion is exact
        return out

    def Growth(self, capacity, sub=4):
        """A MapGrowth of this map: per candidate fine cell -- a cell the map does not occupy and in which beams ended -- the beams that
        ended in it, the beams that later passed through it and where in it the end points lay, kept on the device and fed by Accumulate.
        capacity: the most candidate cells it can hold (a call needs room for one candidate per beam).  It belongs to the map as built now:
        AddPoints / Clear afterwards invalidate it."""
        return MapGrowth(self, capacity, sub)

    def WithAppeared(self, growth, rule=None, device=False):
        """A new map (same voxel size and cap, same context) built by the usual build from this map's stored points followed by
        growth.AppearedPoints(rule) in cell order: the spacing rule and the voxel cap apply to the new points as to any others.
        device: the same map by the device build; only the appeared points cross the bus."""
        if growth.map is not self:
            raise ElmError("WithAppeared: the growth object belongs to another map")
        new = growth.AppearedPoints(rule)
        if device:
            return self._derive(None, new.astype(np.float32))
        old = self.Pointcloud() if not self.Empty() else np.zeros((0, 3))
        out = VoxelHashMap(self.voxel_size_, self.max_points_per_voxel_, self.ctx)
        out.AddPoints(np.concatenate([old, new]).astype(np.float32))  # stored coordinates are float32 values: their conversion is exact
        return out

    def FindGroundHeights(self, xy):
        """FindGroundHeight of many xy positions [n, 2] on the device (elm_map_ground_heights, bit for bit the single query) -> (found bool
        [n], z [n]; 0 where not found)."""
        q = np.ascontiguousarray(np.asarray(xy, dtype=np.float64).reshape(-1, 2))
        n = q.shape[0]
        z = np.zeros(max(n, 1))
        found = np.zeros(max(n, 1), np.int32)
        check(_lib.lib().elm_map_ground_heights(self.ctx._h, self._handle(), _dp(q), n, _dp(z), found.ctypes.data_as(C.POINTER(C.c_int32))),
              self.ctx._h, "elm_map_ground_heights")
        return found[:n] != 0, z[:n]

    def GlobalHypotheses(self, T_tilt, cfg=None, max_poses=None):
        """The lattice poses of a global relocalization (elm_reloc_global_hypotheses) -> (poses [n, 4, 4], valid bool [n]), index
        hyp = (k NX + i) NY + j; a pose without ground under it is not valid.  max_poses: only the first ones."""
        cfg = cfg if cfg is not None else GlobalRelocConfig()
        T = _colmajor16(T_tilt)
        m, (out, valid) = _sized(self.ctx, "elm_reloc_global_hypotheses",
                                 lambda b, cap, n: _lib.lib().elm_reloc_global_hypotheses(self.ctx._h, self._handle(), _dp(T), C.byref(cfg),
                                                                                          *map(_ptr, b or (None, None)), cap, n),
                                 lambda rows: (np.empty((rows, 16)), np.zeros(rows, np.int32)), max_poses)
        return out[:m].reshape(-1, 4, 4).transpose(0, 2, 1).copy(), valid[:m] != 0

    def GetAdjacentVoxels(self, point, search_range):  # vhm.cpp:208-243: keys only, whether or not such voxels exist
        v = self.PointToVoxel(point, self.voxel_size_).astype(np.int64)
        if search_range == 0:
            return v[None, :].copy()
        if search_range == 1:
            off = np.array([[0, 0, 0], [1, 0, 0], [-1, 0, 0], [0, 1, 0], [0, -1, 0], [0, 0, 1], [0, 0, -1]])
        else:  # any other range: the 27 of the 3 x 3 x 3 block, x slowest (voxel_neighbor = 1 whatever `range` says)
            r = np.arange(-1, 2)
            off = np.stack(np.meshgrid(r, r, r, indexing="ij"), -1).reshape(-1, 3)
        return v[None, :] + off

    @staticmethod
    def PointToVoxel(point, voxel_size):  # vhm.hpp:176-180
        return np.floor(np.asarray(point, dtype=np.float64) / voxel_size).astype(np.int32)

    @staticmethod
    def VoxelDownsample(points, voxel_size):  # vhm.hpp:260-283: first point of every floor-keyed voxel
        pts = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 3)
        keys = np.floor(pts.astype(np.float64) / voxel_size).astype(np.int64)
        _, first = np.unique(keys, axis=0, return_index=True)
        first.sort()
        return pts[first]


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


class MapEvidence(_MapChild):
    """Map change evidence (elm_evidence, include/elimaloc_hip.h "map evidence"): two uint32 counters per occupied fine cell of a map,
    resident on the device.  Made by VoxelHashMap.Evidence(sub)."""

    def __init__(self, voxel_map, sub=4):
        self.map, self.ctx, self.sub = voxel_map, voxel_map.ctx, int(sub)
        self._map_h = voxel_map._handle()
        self._h = C.c_void_p()
        check(_lib.lib().elm_evidence_create(self.ctx._h, self._map_h, self.sub, C.byref(self._h)), self.ctx._h, "elm_evidence_create")

    def Accumulate(self, scans, poses, cfg=None, events=False):
        """Accumulate observations (elm_evidence_accumulate / _batch).  scans: one scan (a resident Scan, or (m, 3) points uploaded for the
        call) with one pose [4, 4] -> its EvidenceStats dict; or a list of scans with poses [n, 4, 4] -> a list of dicts, all jobs in one
        launch (the same Scan may appear several times).  events=True (one scan only): also the through events of every beam, uint16 [m],
        in the resident order (Scan.points()) for a Scan, in the caller's order for an array."""
        return _accumulate(self, "elm_evidence_accumulate", "elm_evidence_accumulate_batch", EvidenceStatsC, EvidenceStats, scans, poses,
                           cfg if cfg is not None else EvidenceConfig(sub=self.sub), events)

    def Counts(self):
        """(through, hit): uint32 [n_cells] each, entry for entry with map.FineCells(sub)."""
        h = self._handle()
        m, (t, hit) = _sized(self.ctx, "elm_evidence_counts",
                             lambda b, cap, n: _lib.lib().elm_evidence_counts(self.ctx._h, h, *map(_ptr, b or (None, None)), cap, n),
                             lambda rows: (np.zeros(rows, np.uint32), np.zeros(rows, np.uint32)))
        return t[:m], hit[:m]

    def Reset(self):
        check(_lib.lib().elm_evidence_reset(self.ctx._h, self._handle()), self.ctx._h, "elm_evidence_reset")

    def StalePoints(self, rule=None):
        """bool [n_points] in map.Pointcloud() order: the stored points whose fine cell is stale by `rule` (EvidenceRule())."""
        rule = rule if rule is not None else EvidenceRule()
        h = self._handle()
        m, f = _sized(self.ctx, "elm_evidence_stale_points",
                      lambda b, cap, n: _lib.lib().elm_evidence_stale_points(self.ctx._h, h, C.byref(rule), _ptr(b), cap, n),
                      lambda rows: np.zeros(rows, np.uint8))
        return f[:m].astype(bool)

    def _destroy(self, h):
        _lib.lib().elm_evidence_destroy(h)


class MapGrowth(_MapChild):
    """Map growth (elm_growth, include/elimaloc_hip.h "map growth"): a device-resident table of candidate fine cells that the map does not
    hold, filled by the observations themselves.  Made by VoxelHashMap.Growth(capacity, sub)."""

    def __init__(self, voxel_map, capacity, sub=4):
        self.map, self.ctx, self.sub, self.capacity = voxel_map, voxel_map.ctx, int(sub), int(capacity)
        self._map_h = voxel_map._handle()
        self._h = C.c_void_p()
        check(_lib.lib().elm_growth_create(self.ctx._h, self._map_h, self.sub, self.capacity, C.byref(self._h)), self.ctx._h, "elm_growth_create")

    def Accumulate(self, scans, poses, cfg=None, events=False):
        """One accumulate call (elm_growth_accumulate / _batch).  scans: one scan (a resident Scan, or (m, 3) points uploaded for the call)
        with one pose [4, 4] -> its GrowthStats dict; or a list of scans with poses [n, 4, 4] -> a list of dicts, all jobs in ONE call: the
        end points of all jobs are recorded before any beam walks (the same Scan may appear several times).  events=True (one scan only):
        also the through events of every beam, uint16 [m], in the resident order (Scan.points()) for a Scan, in the caller's order for an
        array."""
        return _accumulate(self, "elm_growth_accumulate", "elm_growth_accumulate_batch", GrowthStatsC, GrowthStats, scans, poses,
                           cfg if cfg is not None else GrowthConfig(sub=self.sub), events)

    def Count(self):
        """The candidate cells held now (known on the host after every call: no download)."""
        n = C.c_size_t(0)
        check(_lib.lib().elm_growth_cells(self.ctx._h, self._handle(), None, None, None, None, 0, C.byref(n)), self.ctx._h, "elm_growth_cells")
        return int(n.value)

    def Cells(self):
        """(cells int32 [m, 3] ascending (x, y, z), hit uint32 [m], through uint32 [m], sums uint64 [m, 3]) of the candidate cells."""
        m = self.Count()
        cells, hit, through = np.zeros((max(m, 1), 3), np.int32), np.zeros(max(m, 1), np.uint32), np.zeros(max(m, 1), np.uint32)
        sums = np.zeros((max(m, 1), 3), np.uint64)
        n = C.c_size_t(0)
        u32 = C.POINTER(C.c_uint32)
        check(_lib.lib().elm_growth_cells(self.ctx._h, self._handle(), cells.ctypes.data_as(C.POINTER(C.c_int32)), hit.ctypes.data_as(u32),
                                          through.ctypes.data_as(u32), sums.ctypes.data_as(C.POINTER(C.c_uint64)), m, C.byref(n)), self.ctx._h,
              "elm_growth_cells")
        return cells[:m], hit[:m], through[:m], sums[:m]

    def AppearedPoints(self, rule=None):
        """float64 [k, 3]: the mean end point of every candidate cell that `rule` (GrowthRule()) calls appeared, in cell order."""
        rule = rule if rule is not None else GrowthRule()
        h = self._handle()
        m, out = _sized(self.ctx, "elm_growth_appeared_points",
                        lambda b, cap, n: _lib.lib().elm_growth_appeared_points(self.ctx._h, h, C.byref(rule), _ptr(b), cap, n),
                        lambda rows: np.zeros((rows, 3)))
        return out[:m]

    def FindObjects(self, rule=None):
        """The appeared cells grouped into objects on the device (elm_growth_find_objects; `rule`: GrowthObjectRule()) -> the stats dict
        (n_members, n_objects, n_small, n_small_cells, max_cells).  The result is held until the next Accumulate, Reset or FindObjects;
        Objects, CellObjects and BeamObjects read it."""
        rule = rule if rule is not None else GrowthObjectRule()
        st = GrowthObjectStatsC()
        check(_lib.lib().elm_growth_find_objects(self.ctx._h, self._handle(), C.byref(rule), C.byref(st)), self.ctx._h, "elm_growth_find_objects")
        return {k: int(getattr(st, k)) for k in _GROWTH_OBJECT_FIELDS}

    def Objects(self):
        """The objects in ascending label order, as a dict of arrays: label int32 [m, 3], n_cells uint32 [m], lo / hi int32 [m, 3] (the
        bounding box in cells, inclusive), hit / through uint64 [m], cell_sum uint64 [m, 3] (the sum of e + 2^20 over the member cells)."""
        h = self._handle()
        m, buf = _sized(self.ctx, "elm_growth_objects", lambda b, cap, n: _lib.lib().elm_growth_objects(self.ctx._h, h, b, cap, n),
                        lambda rows: (GrowthObjectC * rows)())
        a = np.frombuffer(buf, dtype=np.dtype([("label", np.int32, 3), ("n_cells", np.uint32), ("lo", np.int32, 3), ("hi", np.int32, 3),
                                               ("hit", np.uint64), ("through", np.uint64), ("cell_sum", np.uint64, 3)]))[:m]
        return {k: np.ascontiguousarray(a[k]) for k in a.dtype.names}

    def CellObjects(self):
        """int32 [count], one value per candidate cell in Cells()' order: the index of its object, -2 for a member of a small component,
        -1 for a cell that is not a member."""
        h = self._handle()
        m, out = _sized(self.ctx, "elm_growth_cell_objects",
                        lambda b, cap, n: _lib.lib().elm_growth_cell_objects(self.ctx._h, h, _ptr(b), cap, n),
                        lambda rows: np.full(rows, -1, np.int32))
        return out[:m]

    def BeamObjects(self, scan, pose, cfg=None):
        """int32 [n], one value per beam of the scan (a resident Scan: its resident order, Scan.points(); (m, 3) points are uploaded for the
        call and answered in the resident order of that upload) at the pose [4, 4]: the index of the object the beam ends on, -2 for a
        small component, -1 for anything else (elm_growth_beam_objects)."""
        cfg = cfg if cfg is not None else GrowthConfig(sub=self.sub)
        h = self._handle()
        sc = _resident(self.ctx, scan)
        out = np.full(max(sc.n, 1), -1, np.int32)
        check(_lib.lib().elm_growth_beam_objects(self.ctx._h, h, sc._h, _dp(_colmajor16(pose)), C.byref(cfg), out.ctypes.data_as(C.POINTER(C.c_int32))),
              self.ctx._h, "elm_growth_beam_objects")
        return out[:sc.n]

    def Reset(self):
        check(_lib.lib().elm_growth_reset(self.ctx._h, self._handle()), self.ctx._h, "elm_growth_reset")

    def _destroy(self, h):
        _lib.lib().elm_growth_destroy(h)


def OdometryConfig(**kw):
    """elm_odometry_config with its defaults (voxel 1.0 m, cap 30, max_range_m 100, both keyframe thresholds 0 = every scan is inserted,
    reg = RegistrationConfig()).  reg: a RegistrationConfig; any other keyword that is a field of it is set on reg."""
    cfg = _lib.OdometryConfigC()
    _lib.lib().elm_odometry_config_default(C.byref(cfg))
    for k, v in kw.items():
        if k == "reg":
            cfg.reg = v
        elif k == "max_points_per_voxel":
            cfg.max_points_per_voxel = int(v)
        elif k in ("voxel_size", "max_range_m", "key_min_trans_m", "key_min_rot_rad"):
            setattr(cfg, k, float(v))
        elif hasattr(cfg.reg, k):
            setattr(cfg.reg, k, int(v) if k in ("icp_method", "max_iteration", "i_max_thread", "use_radar_cov") else v)
        else:
            raise AttributeError(f"OdometryConfig has no field {k}")
    return cfg


class _BorrowedMap(VoxelHashMap):
    """A VoxelHashMap view of a map handle that another object owns (LidarOdometry.Map()): read it, register against it; it is never
    rebuilt or destroyed from here, and it is good until its owner replaces it."""

    def _release(self):
        self._h = None

    def AddPoints(self, points):
        raise ElmError("the local map belongs to its LidarOdometry: derive a new map from it (Updated, UpdatedFromScans) instead")


class LidarOdometry(_Owned):
    """LiDAR odometry on a rolling local map kept on the device (elm_odometry, include/elimaloc_hip.h): every scan is registered against
    the local map and, when it is a keyframe, inserted by one device build that also forgets what is farther than max_range_m from the
    new pose.  No point crosses the bus after the scan's own upload."""

    def __init__(self, cfg=None, ctx=None):
        self.ctx = ctx or default_context()
        self.cfg = cfg if cfg is not None else OdometryConfig()
        self._h = C.c_void_p()
        check(_lib.lib().elm_odometry_create(self.ctx._h, C.byref(self.cfg), C.byref(self._h)), self.ctx._h, "elm_odometry_create")

    def Step(self, scan, guess=None):
        """One scan (a resident Scan, or (m, 3) points uploaded for the call) from guess [4, 4] (None: Predict()) -> dict: T [4, 4],
        registered, is_success, inserted (bools), reg (the registration's result dict, None for the first scan), build (the insert's
        elm_build_sources_stats as a dict, None without an insert)."""
        sc = _resident(self.ctx, scan)
        st = _lib.OdometryStepC()
        g = None if guess is None else _colmajor16(guess)
        check(_lib.lib().elm_odometry_step_scan(self._h, sc._h, None if g is None else _dp(g), C.byref(st)), self.ctx._h,
              "elm_odometry_step_scan")
        return dict(T=np.array(st.T).reshape(4, 4).T.copy(), registered=bool(st.registered), is_success=bool(st.is_success),
                    inserted=bool(st.inserted), reg=_result_dict(st.reg) if st.registered else None,
                    build={n: int(getattr(st.build, n)) for n, _ in st.build._fields_} if st.inserted else None)

    def Predict(self):
        """The constant-velocity guess of the next pose [4, 4]: T_{k-1} (T_{k-2}^-1 T_{k-1}); the last pose with one, identity with none."""
        T = np.empty(16)
        check(_lib.lib().elm_odometry_predict(self._h, _dp(T)), self.ctx._h, "elm_odometry_predict")
        return T.reshape(4, 4).T.copy()

    def Map(self):
        """The local map as a VoxelHashMap view (None before the first scan): owned by this object, valid until the next inserting Step,
        Reset or close."""
        h = _lib.lib().elm_odometry_map(self._h)
        if not h:
            return None
        m = _BorrowedMap(float(self.cfg.voxel_size), int(self.cfg.max_points_per_voxel), self.ctx)
        m._h = C.c_void_p(h)
        m._derived = True
        return m

    def Reset(self):
        check(_lib.lib().elm_odometry_reset(self._h), self.ctx._h, "elm_odometry_reset")

    def _destroy(self, h):
        _lib.lib().elm_odometry_destroy(h)


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


def results_from_raw(res):
    return [_result_dict(r) for r in res]


def _trace_buffer(B, trace):
    """The iteration-trace array of B registrations the C ABI fills (None without trace)."""
    return (IterTrace * (_lib.MAX_ITER_TRACE * B))() if trace else None


def _result_dicts(res, tr, B):
    """Result dicts of B registrations, each with its slice of the trace array tr (or none)."""
    T = _lib.MAX_ITER_TRACE
    return [_result_dict(res[b], tr[b * T:(b + 1) * T] if tr is not None else None) for b in range(B)]


class Registration:
    """reg.hpp:101-230."""

    def __init__(self, config=None, ctx=None):
        self.ctx = ctx or default_context()
        self.config_ = config if config is not None else RegistrationConfig()
        self.d_fitness_score_ = 0.0

    def Init(self, config):  # reg.hpp:104
        self.config_ = config

    def RunRegister(self, source_local, voxel_map, initial_guess, m_config=None, trace=False):
        """reg.cpp:274-418.  Returns (pose 4x4, is_success, fitness_score, local_cov 6x6[, details]).

        fitness_score is None on failure (the reference leaves its out-param untouched, reg.cpp:415)."""
        cfg = m_config if m_config is not None else self.config_
        scan = np.ascontiguousarray(source_local, dtype=np.float32).reshape(-1, 3)
        T0 = _colmajor16(initial_guess)
        Tout = np.empty(16); ok = C.c_int(0); fit = C.c_double(float("nan")); cov = np.empty(36)
        res = RegResult()
        tr = (IterTrace * _lib.MAX_ITER_TRACE)() if trace else None
        check(_lib.lib().elm_register(self.ctx._h, voxel_map._handle(), _fp(scan), scan.shape[0], _dp(T0),
                                      C.byref(cfg), _dp(Tout), C.byref(ok), C.byref(fit), _dp(cov), C.byref(res),
                                      tr), self.ctx._h, "elm_register")
        self.d_fitness_score_ = res.d_fitness
        pose = Tout.reshape(4, 4).T.copy()
        out = (pose, bool(ok.value), (fit.value if ok.value else None), cov.reshape(6, 6).T.copy())
        if trace:
            return out + (_result_dict(res, tr),)
        return out

    @staticmethod
    def _with_free_space(cands, scan, voxel_map, free_space):
        """The candidates' refined poses checked in ONE CheckFreeSpace call; each dict gains "free_space" (its FreeSpaceStats)."""
        if free_space is None or not cands:
            return cands
        stats = voxel_map.CheckFreeSpace(scan, np.stack([c["T"] for c in cands]), free_space)
        return [dict(c, free_space=st) for c, st in zip(cands, stats)]

    def Relocalize(self, source_local, voxel_map, guess, reloc=None, m_config=None, free_space=None):
        """Relocalization from a coarse pose (elm_relocalize): occupancy scores of the xy x yaw hypotheses around guess on the device, non-maximum
        suppression, ICP from the best top_k in one batch.  Returns (pose 4x4, is_success, fitness_score or None, local_cov 6x6, candidates):
        the winner's result and the kept hypotheses in rank order (dicts: T0, T, score, hyp_index, is_success, iterations, fitness_score).
        The winner's full result dict is kept in last_relocalize_.  free_space: a FreeSpaceConfig -- every candidate also
        carries "free_space", the free-space statistics of its refined pose (one CheckFreeSpace call); the winner rule does not change."""
        cfg = m_config if m_config is not None else self.config_
        rc = reloc if reloc is not None else RelocConfig()
        scan = np.ascontiguousarray(source_local, dtype=np.float32).reshape(-1, 3)
        T0 = _colmajor16(guess)
        Tout = np.empty(16)
        res = RegResult()
        cap = int(rc.top_k)
        cands = (RelocCandidate * cap)()
        nc = C.c_int(0)
        check(_lib.lib().elm_relocalize(self.ctx._h, voxel_map._handle(), _fp(scan), scan.shape[0], _dp(T0), C.byref(rc), C.byref(cfg),
                                        _dp(Tout), C.byref(res), cands, cap, C.byref(nc)), self.ctx._h, "elm_relocalize")
        self.d_fitness_score_ = res.d_fitness
        self.last_relocalize_ = _result_dict(res)
        ok = bool(res.is_success)
        return (Tout.reshape(4, 4).T.copy(), ok, (res.fitness_score if ok else None), np.array(res.local_cov).reshape(6, 6).T.copy(),
                self._with_free_space([_candidate_dict(cands[b]) for b in range(min(nc.value, cap))], scan, voxel_map, free_space))

    def RelocalizeGlobal(self, source_local, voxel_map, T_tilt=None, reloc=None, m_config=None, free_space=None):
        """Global relocalization without a guess (elm_relocalize_global): branch-and-bound over an xy lattice of the map x the whole turn of
        yaw, every pose standing on the map's ground (T_tilt = [R0 | (0, 0, h)]: sensor roll / pitch and height; identity by default), then
        ICP from the best top_k.  Returns (pose 4x4, is_success, fitness_score or None, local_cov 6x6, candidates, stats); candidates as
        Relocalize's (hyp_index = the lattice index), stats the search's counters and timings; free_space as Relocalize's."""
        cfg = m_config if m_config is not None else self.config_
        rc = reloc if reloc is not None else GlobalRelocConfig()
        scan = np.ascontiguousarray(source_local, dtype=np.float32).reshape(-1, 3)
        T0 = _colmajor16(np.eye(4) if T_tilt is None else T_tilt)
        Tout = np.empty(16)
        res = RegResult()
        cap = int(rc.top_k)
        cands = (RelocCandidate * cap)()
        nc = C.c_int(0)
        st = GlobalRelocStats()
        check(_lib.lib().elm_relocalize_global(self.ctx._h, voxel_map._handle(), _fp(scan), scan.shape[0], _dp(T0), C.byref(rc), C.byref(cfg),
                                               _dp(Tout), C.byref(res), cands, cap, C.byref(nc), C.byref(st)), self.ctx._h,
              "elm_relocalize_global")
        self.d_fitness_score_ = res.d_fitness
        self.last_relocalize_ = _result_dict(res)
        ok = bool(res.is_success)
        return (Tout.reshape(4, 4).T.copy(), ok, (res.fitness_score if ok else None), np.array(res.local_cov).reshape(6, 6).T.copy(),
                self._with_free_space([_candidate_dict(cands[b]) for b in range(min(nc.value, cap))], scan, voxel_map, free_space),
                _global_stats_dict(st))

    def _align(self, method, source_local, target_xyz, target_cov, last_icp_pose, trans_th, m_config, source_cov=None):
        cfg = m_config if m_config is not None else self.config_
        src = np.ascontiguousarray(source_local, dtype=np.float64).reshape(-1, 3)
        tgt = np.ascontiguousarray(target_xyz, dtype=np.float64).reshape(-1, 3)
        n = src.shape[0]
        colmajor = lambda c: None if c is None else np.ascontiguousarray(np.asarray(c, dtype=np.float64).reshape(n, 3, 3).transpose(0, 2, 1)).reshape(n, 9)
        tc, sc = colmajor(target_cov), colmajor(source_cov)
        T = _colmajor16(last_icp_pose)
        Tout = np.empty(16); cov = np.zeros(36); fit = C.c_double(float("nan"))
        check(_lib.lib().elm_align_clouds_local(self.ctx._h, int(method), _dp(src), _dp(tgt), None if tc is None else _dp(tc),
                                                None if sc is None else _dp(sc), n, _dp(T), float(trans_th), C.byref(cfg), _dp(Tout),
                                                _dp(cov), C.byref(fit)), self.ctx._h, "elm_align_clouds_local")
        self.d_fitness_score_ = fit.value
        return Tout.reshape(4, 4).T.copy(), cov.reshape(6, 6)

    @staticmethod
    def CalFramePointCov(points, range_var_m, azim_var_deg, ele_var_deg):
        """reg.hpp:186-217: the covariance term R S of every point (from its position: the MAP frame under the initial guess at the
        reference's call site, reg.cpp:302-305) -> [n, 3, 3], not symmetric.  Host arithmetic (elm_cal_frame_point_cov)."""
        q = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = q.shape[0]
        cov = np.empty((max(n, 1), 9))
        rc = _lib.lib().elm_cal_frame_point_cov(_dp(q), n, float(range_var_m), float(azim_var_deg), float(ele_var_deg), _dp(cov))
        if rc != 0:
            raise ElmError("elm_cal_frame_point_cov failed")
        return cov[:n].reshape(n, 3, 3).transpose(0, 2, 1).copy()

    def AlignCloudsLocal(self, source_local, target_pose, last_icp_pose, trans_th, m_config=None):
        """reg.cpp:15-66 on explicit pairs (source PointStruct::local, target PointStruct::pose) -> the step as a 4x4."""
        return self._align(IcpMethod.P2P, source_local, target_pose, None, last_icp_pose, trans_th, m_config)[0]

    def AlignCloudsLocalPointCov(self, source_local, target_mean, target_cov, last_icp_pose, trans_th, m_config=None, source_cov=None):
        """reg.cpp:68-152 (targets' covariance.mean / covariance.cov) -> (step 4x4, local_cov 6x6)."""
        return self._align(IcpMethod.GICP, source_local, target_mean, target_cov, last_icp_pose, trans_th, m_config, source_cov)

    def AlignCloudsLocalVoxelCov(self, source_local, target_mean, target_cov, last_icp_pose, trans_th, m_config=None, source_cov=None):
        """reg.cpp:154-225 (CovStruct targets) -> the step as a 4x4."""
        return self._align(IcpMethod.VGICP, source_local, target_mean, target_cov, last_icp_pose, trans_th, m_config, source_cov)[0]

    def RunRegisterBatch(self, scans, voxel_map, initial_guesses, m_config=None, trace=False):
        """Many resident scans against one map, iterated together. Returns a list of result dicts."""
        cfg = m_config if m_config is not None else self.config_
        B = len(scans)
        arr, T0 = self.pack_inputs(scans, initial_guesses)
        res = (RegResult * B)()
        tr = _trace_buffer(B, trace)
        check(_lib.lib().elm_register_batch(self.ctx._h, voxel_map._handle(), arr, B, _dp(T0), C.byref(cfg), res, tr), self.ctx._h, "elm_register_batch")
        return _result_dicts(res, tr, B)

    @staticmethod
    def pack_inputs(scans, initial_guesses):
        """(ctypes array of scan handles, contiguous column-major float64 guesses) as the C ABI takes them."""
        arr = (C.c_void_p * len(scans))(*[s._h for s in scans])
        T0 = _pose_block(initial_guesses)
        return arr, T0

    def RunRegisterStream(self, scans, voxel_map, initial_guesses, slots=32, m_config=None, trace=False, raw=False):
        """Continuous batching (elm_register_stream): len(scans) registrations through `slots` device slots that are
        refilled on the device as registrations finish.  Same results as RunRegisterBatch, in input order."""
        cfg = m_config if m_config is not None else self.config_
        arr, T0 = scans, initial_guesses
        if not isinstance(scans, C.Array):  # pack_inputs() lets a caller marshal once and call many times
            arr, T0 = self.pack_inputs(scans, initial_guesses)
        B = len(arr)
        res = (RegResult * B)()
        tr = _trace_buffer(B, trace)
        check(_lib.lib().elm_register_stream(self.ctx._h, voxel_map._handle(), arr, B, _dp(T0), C.byref(cfg), int(slots), res, tr),
              self.ctx._h, "elm_register_stream")
        if raw:  # the elm_reg_result array as the library filled it; results_from_raw() turns it into dicts later
            return res
        return _result_dicts(res, tr, B)

    @staticmethod
    def pack_host_inputs(scans_host, initial_guesses, pinned=None):
        """Marshal HOST scans for RunRegisterStreamHost once: (pointer array, point counts, column-major guesses, keep-alive).

        pinned: optional PinnedBuffer holding all scans back to back (page-locked: the DMA engines read it directly)."""
        B = len(scans_host)
        keep = [np.ascontiguousarray(s, dtype=np.float32).reshape(-1, 3) for s in scans_host]
        npts = (C.c_uint32 * B)(*[k.shape[0] for k in keep])
        if pinned is not None:
            o = 0
            ptrs = []
            for k in keep:
                pinned.array[o:o + k.size] = k.ravel()
                ptrs.append(pinned.ptr + 4 * o)
                o += k.size
            keep = [pinned]
        else:
            ptrs = [k.ctypes.data for k in keep]
        arr = (C.c_void_p * B)(*ptrs)
        T0 = _pose_block(initial_guesses)
        return arr, npts, T0, keep

    def RunRegisterStreamHost(self, packed, voxel_map, slots=32, m_config=None, trace=False, raw=False):
        """elm_register_stream_host: the scans are in host memory when the call starts; uploads, device-side ordering and the
        iterations of earlier registrations overlap.  packed = pack_host_inputs(...)."""
        cfg = m_config if m_config is not None else self.config_
        arr, npts, T0, _keep = packed
        B = len(arr)
        res = (RegResult * B)()
        tr = _trace_buffer(B, trace)
        check(_lib.lib().elm_register_stream_host(self.ctx._h, voxel_map._handle(), arr, npts, B, _dp(T0), C.byref(cfg), int(slots), res, tr),
              self.ctx._h, "elm_register_stream_host")
        if raw:
            return res
        return _result_dicts(res, tr, B)

    def EnqueueBatch(self, scans, voxel_map, initial_guesses, m_config=None, trace=False):
        cfg = m_config if m_config is not None else self.config_
        B = len(scans)
        arr, T0 = self.pack_inputs(scans, initial_guesses)
        self._pending = (B, trace)
        check(_lib.lib().elm_register_batch_enqueue(self.ctx._h, voxel_map._handle(), arr, B, _dp(T0),
                                                    C.byref(cfg), int(bool(trace))), self.ctx._h,
              "elm_register_batch_enqueue")

    def FinishBatch(self):
        B, trace = self._pending
        res = (RegResult * B)()
        tr = _trace_buffer(B, trace)
        check(_lib.lib().elm_register_batch_finish(self.ctx._h, res, tr), self.ctx._h, "elm_register_batch_finish")
        return _result_dicts(res, tr, B)

    @staticmethod
    def TransformPoints(T, points):  # reg.hpp:126-148 (host-side convenience, float64)
        p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
        T = np.asarray(T, dtype=np.float64)
        return p @ T[:3, :3].T + T[:3, 3]
