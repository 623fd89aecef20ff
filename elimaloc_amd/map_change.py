"""Map change on the device: evidence that stored structure is gone (MapEvidence) and that new structure appeared (MapGrowth, with its
objects), both fed by scans at their poses, with their configs, rules and statistics."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ElmError, EvidenceConfigC, EvidenceRuleC, EvidenceStatsC, GrowthConfigC, GrowthObjectC, GrowthObjectRuleC,
                   GrowthObjectStatsC, GrowthRuleC, GrowthStatsC, check)
from ._marshal import _Owned, _colmajor16, _config, _counts, _dp, _pose_block, _ptr, _sized
from .context import Scan, _callers_order, _resident


def EvidenceConfig(**kw):
    """elm_evidence_config with its defaults (sub 4, max_steps 4096, walk from 1 m, observing 2 .. 50 m, end margins 1 m / 0.2 L, origin 0)."""
    return _config("EvidenceConfig", EvidenceConfigC, "elm_evidence_config_default", kw)


def EvidenceRule(**kw):
    """elm_evidence_rule with its defaults (min_through 3, through_per_hit 4): a cell is stale when through >= min_through and
    through >= through_per_hit * hit.  A starting point, not a measured optimum."""
    return _config("EvidenceRule", EvidenceRuleC, "elm_evidence_rule_default", kw)


def EvidenceStats(st):
    """elm_evidence_stats of one observation as a dict."""
    return _counts(st)


def GrowthConfig(**kw):
    """elm_growth_config with its defaults: the EvidenceConfig defaults and clearance_cells 1 (an end point within that many cells of an
    occupied cell is the old surface, not new structure; 0, 1 or 2 -- a starting point, not a measured optimum)."""
    return _config("GrowthConfig", GrowthConfigC, "elm_growth_config_default", kw)


def GrowthRule(**kw):
    """elm_growth_rule with its defaults (min_hit 3, hit_per_through 4): a candidate cell has appeared when hit >= min_hit and
    hit >= hit_per_through * through.  A starting point, not a measured optimum."""
    return _config("GrowthRule", GrowthRuleC, "elm_growth_rule_default", kw)


def GrowthStats(st):
    """elm_growth_stats of one observation as a dict."""
    return _counts(st)


def GrowthObjectRule(**kw):
    """elm_growth_object_rule with its defaults (min_hit 3, hit_per_through 4, connectivity 26, min_cells 1): which candidate cells are
    members (GrowthRule's rule), which of them are adjacent (6, 18 or 26) and how many cells make an object.  Starting points, not
    measured optima."""
    return _config("GrowthObjectRule", GrowthObjectRuleC, "elm_growth_object_rule_default", kw)


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
        return _counts(st)

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
