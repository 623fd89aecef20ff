"""The voxel map (pcm_matching/include/voxel_hash_map.hpp, VoxelHashMap :89-335) and the queries it answers on the device: pose scores,
ground heights, free space, ray casts, with the configs and statistics of those queries."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (ElmError, FreeSpaceConfigC, FreeSpaceStatsC, GlobalRelocConfigC, MapInfo, RayCastConfigC, RayCastStatsC, RelocConfigC,
                   check)
from ._marshal import _colmajor16, _config, _counts, _dp, _fp, _pose_block, _ptr, _sized
from .context import Scan, _callers_order, _resident, default_context
from .map_change import MapEvidence, MapGrowth


def RelocConfig(**kw):
    """elm_reloc_config with its defaults (5 m / 0.5 m xy window, 180 deg / 2 deg yaw, 50 m score range, 8192 score points, top 16 after
    non-maximum suppression at 1.0 m / 6 deg, 64 KiB LDS / 64 MiB bitmap budgets)."""
    return _config("RelocConfig", RelocConfigC, "elm_reloc_config_default", kw)


def GlobalRelocConfig(**kw):
    """elm_reloc_global_config with its defaults (the map's xy bounds (NaN rectangle), 0.5 m / 2 deg lattice, 50 m score range, counted points
    1.0 m or more above the ground, 8192 score points, top 16 after non-maximum suppression at 1.0 m / 6 deg, pool 64, kz span 64, 256 MiB)."""
    return _config("GlobalRelocConfig", GlobalRelocConfigC, "elm_reloc_global_config_default", kw)


def FreeSpaceConfig(**kw):
    """elm_freespace_config with its defaults (sub 4, step_m 0 = cell / 2 of the map, start 1 m, range 2 .. 50 m, end margins 1 m / 0.2 L,
    min_hits 2, max_samples 1024, origin 0)."""
    return _config("FreeSpaceConfig", FreeSpaceConfigC, "elm_freespace_config_default", kw)


def FreeSpaceStats(st):
    """elm_freespace_stats of one pose as a dict (+ pierced_share = n_pierced / n_counted, 0 without counted rays)."""
    d = _counts(st)
    d["pierced_share"] = d["n_pierced"] / d["n_counted"] if d["n_counted"] else 0.0
    return d


def RayCastConfig(**kw):
    """elm_raycast_config with its defaults (sub 4, max_steps 4096, range 1 .. 100 m, compared 2 .. 50 m, tol_m 0.5, tol_frac 0.02,
    origin 0)."""
    return _config("RayCastConfig", RayCastConfigC, "elm_raycast_config_default", kw)


def RayCastStats(st):
    """elm_raycast_stats of one pose as a dict (+ match_share / through_share / front_share of the compared beams, 0 without any)."""
    d = _counts(st)
    for k in ("match", "through", "front"):
        d[k + "_share"] = d["n_" + k] / d["n_compared"] if d["n_compared"] else 0.0
    return d


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
        return (out, _counts(st)) if stats else out

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
        return {"desc": _counts(d), "start": start, "blocks": blocks, "slot_point": slot_point,
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
