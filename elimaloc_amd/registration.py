"""Host-side mirror of the reference's operator interface for the registration hot path.

Same names, argument meaning and error behaviour as
  pcm_matching/include/registration.hpp      (IcpMethod :60, RegistrationConfig :62-85, Registration :101-230)
  pcm_matching/include/voxel_hash_map.hpp    (VoxelHashMap :89-335, in voxel_map.py)
so that parity tests read like calls into the reference.  Everything numerical happens in the C-ABI library
(HIP kernels); this file only marshals numpy arrays.  Out-params of the C++ signatures are returned as tuples.

The context and scans (context.py), the map (voxel_map.py), map evidence and growth (map_change.py) and LiDAR odometry (odometry.py)
have modules of their own; their names are importable from here as before (the block at the end).
"""
import ctypes as C
import enum

import numpy as np

from . import _lib
from ._lib import ElmError, GlobalRelocStats, IterTrace, RegConfig, RegResult, RelocCandidate, check
from ._marshal import _colmajor16, _config, _dp, _fp, _pose_block, _result_dict
from .context import default_context
from .voxel_map import GlobalRelocConfig, RelocConfig


class IcpMethod(enum.IntEnum):  # reg.hpp:60
    P2P = 0
    GICP = 1
    VGICP = 2
    AVGICP = 3


def RegistrationConfig(**kw):
    """RegistrationConfig with the shipped defaults of config/localization.ini:80-105."""
    return _config("RegistrationConfig", RegConfig, "elm_reg_config_default", kw)


def RegInfoConfig(**kw):
    """elm_reginfo_config with its defaults: the method's metric, sigma2 = chi2 / dof, the scan's own length scale, nothing dropped."""
    return _config("RegInfoConfig", _lib.RegInfoConfigC, "elm_reginfo_config_default", kw)


def _reginfo_dict(r):
    m = lambda a: np.array(a).reshape(6, 6).copy()
    return dict(information=m(r.information), H=m(r.H), g=np.array(r.g), chi2=float(r.chi2), sigma2=float(r.sigma2),
                length_scale=float(r.length_scale), eigenvalues=np.array(r.eigenvalues), eigenvectors=m(r.eigenvectors),
                n_points=int(r.n_points), n_pairs=int(r.n_pairs), n_default=int(r.n_default), dof=int(r.dof), rank=int(r.rank),
                status=int(r.status), no_pairs=bool(r.status & _lib.REGINFO_NO_PAIRS), no_dof=bool(r.status & _lib.REGINFO_NO_DOF),
                degenerate=bool(r.status & _lib.REGINFO_DEGENERATE), non_finite=bool(r.status & _lib.REGINFO_NON_FINITE))


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

    def Information(self, scans, voxel_map, poses, cfg=None, m_config=None, raw=False):
        """Registration information (elm_register_information): for every (resident scan, pose) job the 6 x 6 Gauss-Newton information of
        the registration at that pose in the pose graph's tangent [v; w] -- an `information` for PoseGraph.AddEdges / AddPriors as it
        is --, the variance factor and the eigen-analysis that names the directions the scan does not constrain.  cfg: a RegInfoConfig.
        Returns a list of dicts (raw: the elm_reginfo_result array as the library filled it)."""
        reg = m_config if m_config is not None else self.config_
        rc = cfg if cfg is not None else RegInfoConfig()
        B = len(scans)
        arr, T = self.pack_inputs(scans, poses)
        res = (_lib.RegInfoResultC * max(B, 1))()
        check(_lib.lib().elm_register_information(self.ctx._h, voxel_map._handle(), arr, _dp(T), B, C.byref(reg), C.byref(rc), res),
              self.ctx._h, "elm_register_information")
        return res if raw else [_reginfo_dict(res[b]) for b in range(B)]

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


# Every other name this module used to define, where it lives now.
from ._lib import (EvidenceConfigC, EvidenceRuleC, EvidenceStatsC, FreeSpaceConfigC, FreeSpaceStatsC, GlobalRelocConfigC,  # noqa: E402,F401
                   GrowthConfigC, GrowthObjectC, GrowthObjectRuleC, GrowthObjectStatsC, GrowthRuleC, GrowthStatsC, MapInfo, RayCastConfigC,
                   RayCastStatsC, RelocConfigC)
from ._marshal import _Owned, _ptr, _sized  # noqa: E402,F401
from .context import Context, PinnedBuffer, Scan, _callers_order, _resident  # noqa: E402,F401
from .map_change import (EvidenceConfig, EvidenceRule, EvidenceStats, GrowthConfig, GrowthObjectRule, GrowthRule, GrowthStats,  # noqa: E402,F401
                         MapEvidence, MapGrowth, _MapChild, _accumulate)
from .voxel_map import FreeSpaceConfig, FreeSpaceStats, RayCastConfig, RayCastStats, VoxelHashMap  # noqa: E402,F401
from .odometry import LidarOdometry, OdometryConfig, _BorrowedMap  # noqa: E402,F401
