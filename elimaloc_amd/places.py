"""Place recognition (include/elimaloc_hip.h "place recognition"): rotation-aware binary scan descriptors computed on the
GPU, a database of them resident on the GPU, the exact search of a query against every entry at all 64 yaw shifts -- and, on top of
the existing public calls only, the step from a candidate to a loop constraint (LoopCloser)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ElmError, PlaceCandidateC, PlaceMatchC, PlacesConfigC, PlacesQueryConfigC, PlacesStatsC, check
from ._marshal import _Owned, _config, _counts, _dp, _pose_block, _ptr
from .context import Scan, _resident, default_context
from .registration import IcpMethod, RegistrationConfig
from .voxel_map import RelocConfig, VoxelHashMap

SECTORS, MAX_TOP_K = _lib.PLACES_SECTORS, _lib.PLACES_MAX_TOP_K
MATCH_DTYPE = np.dtype([("dice_q16", np.uint32), ("inter", np.uint16), ("shift", np.uint16)])


def PlaceConfig(**kw):
    """elm_places_config with its defaults (16 rings over 2 .. 42 m, 8 layers over -3 .. 9 m)."""
    return _config("PlaceConfig", PlacesConfigC, "elm_places_config_default", kw)


def PlaceTables(cfg=None):
    """(ring_edge2 [n_rings + 1], z_edge [n_layers + 1], dir [64, 2]) of a config: the library's own float64 tables (host only)."""
    cfg = cfg if cfg is not None else PlaceConfig()
    re, ze, d = np.zeros(max(cfg.n_rings, 0) + 1), np.zeros(max(cfg.n_layers, 0) + 1), np.zeros((SECTORS, 2))
    if not (1 <= cfg.n_rings <= 32 and 1 <= cfg.n_layers <= 16):
        raise ElmError("PlaceTables: n_rings in 1 .. 32 and n_layers in 1 .. 16")
    check(_lib.lib().elm_places_tables(C.byref(cfg), _dp(re), _dp(ze), _dp(d)), None, "elm_places_tables")
    return re, ze, d


def PlaceStats(st):
    """elm_places_stats of one described scan as a dict."""
    return _counts(st)


def _candidate(c):
    return dict(entry=int(c.entry), dice_q16=int(c.dice_q16), id=int(c.id), inter=int(c.inter), shift=int(c.shift), yaw_rad=float(c.yaw_rad))


def _one_or_many(scans):
    return isinstance(scans, Scan) or (isinstance(scans, np.ndarray) and scans.ndim == 2)


class PlaceDatabase(_Owned):
    """A database of scan descriptors resident on the device (elm_places), of a capacity fixed at creation (1 .. 65536)."""

    def __init__(self, cfg=None, capacity=1024, ctx=None):
        self.ctx = ctx if ctx is not None else default_context()
        self.cfg = cfg if cfg is not None else PlaceConfig()
        self.capacity = int(capacity)
        self.n_words = int(self.cfg.n_rings) * int(self.cfg.n_layers)
        self._h = C.c_void_p()
        check(_lib.lib().elm_places_create(self.ctx._h, C.byref(self.cfg), self.capacity, C.byref(self._h)), self.ctx._h, "elm_places_create")

    def _handle(self):
        if not getattr(self, "_h", None):
            raise ElmError("PlaceDatabase: closed")
        return self._h

    def _jobs(self, scans, levels, what):
        scs = [_resident(self.ctx, s) for s in ([scans] if _one_or_many(scans) else list(scans))]
        n = len(scs)
        P = None if levels is None else _pose_block(levels)
        if P is not None and P.size // 16 != n:
            raise ElmError(f"PlaceDatabase.{what}: one level per scan")
        hs = (C.c_void_p * max(n, 1))(*[s._h.value for s in scs])
        return scs, n, hs, (None if P is None else _dp(P)), P

    def Tables(self):
        return PlaceTables(self.cfg)

    def Size(self):
        n = C.c_size_t(0)
        check(_lib.lib().elm_places_size(self.ctx._h, self._handle(), C.byref(n)), self.ctx._h, "elm_places_size")
        return int(n.value)

    def Reset(self):
        check(_lib.lib().elm_places_reset(self.ctx._h, self._handle()), self.ctx._h, "elm_places_reset")

    def Describe(self, scans, levels=None):
        """The descriptors of resident scans (or (m, 3) arrays uploaded for the call), each levelled by its pose of levels [n, 4, 4] (None:
        identity), in one launch; the database is not touched -> (words uint64 [n, W], [PlaceStats dicts]); for one scan (words [W], dict)."""
        scs, n, hs, lp, _keep = self._jobs(scans, levels, "Describe")
        words = np.zeros((max(n, 1), self.n_words), np.uint64)
        st = (PlacesStatsC * max(n, 1))()
        check(_lib.lib().elm_places_describe(self.ctx._h, self._handle(), hs, lp, n, _ptr(words), st), self.ctx._h, "elm_places_describe")
        if _one_or_many(scans):
            return words[0], PlaceStats(st[0])
        return words[:n], [PlaceStats(st[j]) for j in range(n)]

    def Add(self, scans, levels=None, ids=None):
        """The same descriptors appended as entries in job order; ids: int64 per scan (default: the entry indices) -> [PlaceStats dicts]
        (one dict for one scan)."""
        scs, n, hs, lp, _keep = self._jobs(scans, levels, "Add")
        if ids is None:
            first = self.Size()
            ids = np.arange(first, first + n, dtype=np.int64)
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        if ids.size != n:
            raise ElmError("PlaceDatabase.Add: one id per scan")
        st = (PlacesStatsC * max(n, 1))()
        check(_lib.lib().elm_places_add(self.ctx._h, self._handle(), hs, lp, _ptr(ids), n, st), self.ctx._h, "elm_places_add")
        return PlaceStats(st[0]) if _one_or_many(scans) else [PlaceStats(st[j]) for j in range(n)]

    def AddDescriptors(self, words, ids):
        """Descriptors from the host, words uint64 [n, W] with ids int64 [n], appended (a saved database loaded again)."""
        words = np.ascontiguousarray(np.asarray(words, dtype=np.uint64).reshape(-1, self.n_words))
        ids = np.ascontiguousarray(np.asarray(ids, dtype=np.int64).reshape(-1))
        if ids.size != words.shape[0]:
            raise ElmError("PlaceDatabase.AddDescriptors: one id per descriptor")
        check(_lib.lib().elm_places_add_words(self.ctx._h, self._handle(), _ptr(words) if ids.size else None, _ptr(ids) if ids.size else None,
                                              ids.size), self.ctx._h, "elm_places_add_words")

    def Download(self, first=0, count=None):
        """Entries first .. first + count - 1 (default: to the end) -> (words uint64 [count, W], ids int64 [count], n_bits uint32 [count])."""
        count = self.Size() - int(first) if count is None else int(count)
        if first < 0 or count < 0:
            raise ElmError("PlaceDatabase.Download: beyond the database's size")
        m = max(count, 1)
        words, ids, bits = np.zeros((m, self.n_words), np.uint64), np.zeros(m, np.int64), np.zeros(m, np.uint32)
        check(_lib.lib().elm_places_download(self.ctx._h, self._handle(), int(first), count, _ptr(words), _ptr(ids), _ptr(bits)), self.ctx._h,
              "elm_places_download")
        return words[:count], ids[:count], bits[:count]

    def _query_configs(self, n, top_k, min_dice_q16, exclude_ids):
        cfgs = (PlacesQueryConfigC * max(n, 1))()
        per_query = isinstance(exclude_ids, (list, np.ndarray)) and np.asarray(exclude_ids).ndim == 2
        for q in range(n):
            lo, hi = (exclude_ids[q] if per_query else exclude_ids) if exclude_ids is not None else (0, -1)
            cfgs[q].top_k, cfgs[q].min_dice_q16 = int(top_k), int(min_dice_q16)
            cfgs[q].exclude_id_lo, cfgs[q].exclude_id_hi = int(lo), int(hi)
        return cfgs

    def _answer(self, n, cands, nc, matches, single):
        out = [[_candidate(cands[q * MAX_TOP_K + c]) for c in range(nc[q])] for q in range(n)]
        res = out[0] if single else out
        if matches is None:
            return res
        return res, (matches[0] if single else matches[:n])

    def Match(self, words, top_k=1, min_dice_q16=0, exclude_ids=None, matches=False):
        """Query descriptors words uint64 [n, W] (or one [W]) against every entry at every yaw shift (elm_places_match_words) -> per query
        the list of candidate dicts (entry, dice_q16, id, inter, shift, yaw_rad) in rank order; exclude_ids: a closed id range (lo, hi),
        or one per query [n, 2]; matches=True: also every (query, entry) pair, a structured array [n, size] of MATCH_DTYPE."""
        words = np.asarray(words, dtype=np.uint64)
        single = words.ndim == 1
        words = np.ascontiguousarray(words.reshape(-1, self.n_words))
        n = words.shape[0]
        cfgs = self._query_configs(n, top_k, min_dice_q16, exclude_ids)
        cands = (PlaceCandidateC * (max(n, 1) * MAX_TOP_K))()
        nc = (C.c_int32 * max(n, 1))()
        m = np.zeros((max(n, 1), max(self.Size(), 1)), MATCH_DTYPE)[:, :self.Size()].copy() if matches else None
        check(_lib.lib().elm_places_match_words(self.ctx._h, self._handle(), _ptr(words), n, cfgs, cands, nc,
                                                None if m is None else C.cast(m.ctypes.data, C.POINTER(PlaceMatchC))), self.ctx._h,
              "elm_places_match_words")
        return self._answer(n, cands, nc, m, single)

    def Query(self, scans, levels=None, top_k=1, min_dice_q16=0, exclude_ids=None, matches=False):
        """The same on scans (elm_places_query): described into scratch, then matched; one scan or a list, as Describe takes them."""
        scs, n, hs, lp, _keep = self._jobs(scans, levels, "Query")
        cfgs = self._query_configs(n, top_k, min_dice_q16, exclude_ids)
        cands = (PlaceCandidateC * (max(n, 1) * MAX_TOP_K))()
        nc = (C.c_int32 * max(n, 1))()
        m = np.zeros((max(n, 1), max(self.Size(), 1)), MATCH_DTYPE)[:, :self.Size()].copy() if matches else None
        check(_lib.lib().elm_places_query(self.ctx._h, self._handle(), hs, lp, n, cfgs, cands, nc,
                                          None if m is None else C.cast(m.ctypes.data, C.POINTER(PlaceMatchC)), None), self.ctx._h,
              "elm_places_query")
        return self._answer(n, cands, nc, m, _one_or_many(scans))

    def _destroy(self, h):
        _lib.lib().elm_places_destroy(h)


def _rz(yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    return T


def LoopRegConfig(**kw):
    """The registration a LoopCloser runs by default: the shipped RegistrationConfig with P2P, run to convergence (up to 50 iterations,
    stopping at a step of 2 mm).  The shipped stop at a 2 cm step is set for tracking; a loop constraint is judged against guesses that
    can be good to a few hundredths of a degree, and 0.02 deg at 20 m is 7 mm.  The method was chosen by measurement on ONE fixture (24
    entries on a 35 m circle of the synthetic field world, 4 096-point scans, 12 revisits) and is not validated
    beyond it: with real scans, denser submaps or another spacing of the entries, pass the m_config that fits."""
    cfg = dict(icp_method=IcpMethod.P2P, max_iteration=50, icp_termination_threshold_m=0.002)
    cfg.update(kw)
    return RegistrationConfig(**cfg)


class LoopCloser:
    """From a place candidate to a loop constraint, on public calls only: Insert keeps every resident scan with its pose and adds its
    descriptor (id = entry index); Detect queries; Verify builds a submap of the entries around the candidate on the device and
    relocalizes the query scan in it from the candidate's yaw.

    window: the submap takes entries max(e - window, 0) .. min(e + window, last): a window along the log, clipped at its ends and not
    wrapped around, so near the ends it holds fewer scans.  It should reach every kept scan that can overlap the query, since the
    registration is only as exact as the submap is dense.  Without m_config / registration the closer registers with LoopRegConfig().
    registration (beyond the issue's signature): a Registration to use instead of making one from m_config."""

    def __init__(self, places, voxel_size=1.0, max_points_per_voxel=30, window=2, reloc=None, m_config=None, registration=None):
        from .registration import Registration
        self.places, self.ctx = places, places.ctx
        self.voxel_size, self.max_points_per_voxel, self.window = float(voxel_size), int(max_points_per_voxel), int(window)
        # the candidate's yaw is good to a sector and a half (8.4 deg) and says nothing of the position: a window of 2 m and 10 deg
        self.reloc = reloc if reloc is not None else RelocConfig(radius_xy_m=2.0, yaw_range_deg=10.0, top_k=4)
        if m_config is None and registration is None:
            m_config = LoopRegConfig()
        self.m_config = m_config
        self.reg = registration if registration is not None else Registration(m_config, ctx=self.ctx)
        self.scans, self.poses = [], []
        self.loops = []  # AddLoop: (entry_a, entry_b, T_a_b, information)
        self.priors = []  # AddPosePrior / AddPositionPrior: (entry, Z, information 6 x 6, lever)

    def Insert(self, scan, T_world_sensor, T_level=None):
        sc = _resident(self.ctx, scan)
        entry = len(self.scans)
        st = self.places.Add(sc, None if T_level is None else np.asarray(T_level)[None], ids=[entry])
        self.scans.append(sc)
        self.poses.append(np.array(T_world_sensor, dtype=np.float64).reshape(4, 4))
        return entry, st

    def Detect(self, scan, T_level=None, exclude_last=0, top_k=1, min_dice_q16=0):
        n = len(self.scans)
        rng = (n - int(exclude_last), n - 1) if exclude_last > 0 else None
        return self.places.Query(_resident(self.ctx, scan), None if T_level is None else np.asarray(T_level)[None], top_k=top_k,
                                 min_dice_q16=min_dice_q16, exclude_ids=rng)

    def Submap(self, entry):
        """The map of the kept scans of entries entry - window .. entry + window at their poses (a whole-log device build), with the
        covariances the registration method needs."""
        lo, hi = max(entry - self.window, 0), min(entry + self.window, len(self.scans) - 1)
        base = VoxelHashMap(self.voxel_size, self.max_points_per_voxel, self.ctx, device_build=True)
        m = base.UpdatedFromScans(self.scans[lo:hi + 1], np.stack(self.poses[lo:hi + 1]))
        cfg = self.m_config if self.m_config is not None else self.reg.config_
        if cfg.icp_method == IcpMethod.GICP:
            m.CalPointCovAll(cfg.gicp_cov_search_dist)
        elif cfg.icp_method in (IcpMethod.VGICP, IcpMethod.AVGICP):
            m.CalVoxelCovAll()
        return m

    def Guess(self, candidate):
        return self.poses[candidate["entry"]] @ _rz(candidate["yaw_rad"])

    def Verify(self, scan, candidate, information=None):
        """-> dict(T, is_success, fitness_score, local_cov, candidates: Registration.Relocalize's result from the guess T_e Rz(yaw) in the
        submap around the candidate's entry; T_entry_query = T_e^-1 T).
        information: a RegInfoConfig -- the dict also carries "reginfo", Registration.Information's result for the scan at T in that
        submap, and "information", its 6 x 6 matrix in the tangent of T: the information of the edge T_entry_query as AddLoop takes it
        (DESIGN.md section 29).  The plane metric on a submap without point covariances computes them first."""
        pts = scan.points() if isinstance(scan, Scan) else np.ascontiguousarray(scan, dtype=np.float32).reshape(-1, 3)
        m = self.Submap(candidate["entry"])
        T, ok, fit, cov, cands = self.reg.Relocalize(pts, m, self.Guess(candidate), self.reloc, self.m_config)
        out = dict(T=T, is_success=ok, fitness_score=fit, local_cov=cov, candidates=cands,
                   T_entry_query=np.linalg.inv(self.poses[candidate["entry"]]) @ T)
        if information is not None:
            cfg = self.m_config if self.m_config is not None else self.reg.config_
            if information.metric == _lib.REGINFO_METRIC_PLANE and not m.info().has_point_cov:
                m.CalPointCovAll(cfg.gicp_cov_search_dist)
            out["reginfo"] = self.reg.Information([_resident(self.ctx, scan)], m, T[None], information, self.m_config)[0]
            out["information"] = out["reginfo"]["information"]
        return out

    def AddLoop(self, entry_a, entry_b, T_a_b, information=None):
        """A loop constraint for Close: T_a_b ~ T_a^-1 T_b between two entries (Verify's T_entry_query, with the query inserted as an
        entry); information: 6 x 6 symmetric in the order [translation; rotation] (default: the identity)."""
        n = len(self.scans)
        a, b = int(entry_a), int(entry_b)
        if not (0 <= a < n and 0 <= b < n) or a == b:
            raise ElmError("LoopCloser.AddLoop: two different entries")
        info = np.eye(6) if information is None else np.array(information, dtype=np.float64).reshape(6, 6)
        self.loops.append((a, b, np.array(T_a_b, dtype=np.float64).reshape(4, 4), info))

    def _add_prior(self, what, entry, Z, info, lever):
        e = int(entry)
        if not 0 <= e < len(self.scans):
            raise ElmError(f"LoopCloser.{what}: no such entry")
        lv = np.zeros(3) if lever is None else np.array(lever, dtype=np.float64).reshape(3)
        self.priors.append((e, Z, info, lv))

    def AddPosePrior(self, entry, T_world_sensor, information=None, lever=None):
        """An absolute pose measurement of an entry for Close (a match against an existing map, a GNSS pose): T_world_sensor 4 x 4,
        information 6 x 6 symmetric in the order [translation; rotation] (default: the identity), lever: the measured point in the
        entry's frame (default: its origin).  PoseGraph.AddPriors' factor."""
        info = np.eye(6) if information is None else np.array(information, dtype=np.float64).reshape(6, 6)
        self._add_prior("AddPosePrior", entry, np.array(T_world_sensor, dtype=np.float64).reshape(4, 4), info, lever)

    def AddPositionPrior(self, entry, position, information=None, lever=None):
        """An absolute position measurement of an entry for Close (a GNSS fix at the antenna `lever`): position [3] in the world,
        information 3 x 3 symmetric (default: the identity).  PoseGraph.AddPositionPriors' factor."""
        Z = np.eye(4)
        Z[:3, 3] = np.asarray(position, dtype=np.float64).reshape(3)
        info = np.zeros((6, 6))
        info[:3, :3] = np.eye(3) if information is None else np.asarray(information, dtype=np.float64).reshape(3, 3)
        self._add_prior("AddPositionPrior", entry, Z, info, lever)

    def ConsistentLoops(self, cfg=None, var_t=None, var_r=None, odom_covariance=None):
        """The loops of AddLoop that agree with one another over the inserted poses (loops.LoopConsistency on self.poses and
        self.loops; cfg: a LoopConsistencyConfig, whose q_t and q_r say how good the odometry is per entry) -> its dict.  var_t,
        var_r: one number for all loops or one per loop; by default 3 / trace(Omega_vv) and 3 / trace(Omega_ww) of each loop's
        information, the weights of PoseGraph.Initialize inverted.
        odom_covariance: the 6 x 6 covariance of one odometry step (or [n - 1, 6, 6], one per step); then the covariance model runs
        (loops.LoopConsistencyCov), each loop's covariance being the symmetrised inverse of its information, cfg's q_t and q_r stay 0
        and var_t, var_r are not used.  Without it every result is what it was."""
        from .loops import LoopConsistency, LoopConsistencyCov
        info = np.stack([l[3] for l in self.loops]) if self.loops else np.zeros((0, 6, 6))
        if odom_covariance is not None:
            cov = np.linalg.inv(info) if self.loops else info
            cov = 0.5 * (cov + cov.transpose(0, 2, 1))
            Z = np.stack([l[2] for l in self.loops]) if self.loops else np.zeros((0, 4, 4))
            return LoopConsistencyCov(np.stack(self.poses), [l[0] for l in self.loops], [l[1] for l in self.loops], Z, cov, odom_covariance, cfg,
                                      self.ctx)
        if var_t is None:
            var_t = 3.0 / ((info[:, 0, 0] + info[:, 1, 1]) + info[:, 2, 2])
        if var_r is None:
            var_r = 3.0 / ((info[:, 3, 3] + info[:, 4, 4]) + info[:, 5, 5])
        Z = np.stack([l[2] for l in self.loops]) if self.loops else np.zeros((0, 4, 4))
        return LoopConsistency(np.stack(self.poses), [l[0] for l in self.loops], [l[1] for l in self.loops], Z, var_t, var_r, cfg, self.ctx)

    def Close(self, cfg=None, odom_information=None, fixed=(0,), apply=False, preconditioner="block_jacobi", initialize=False,
              consistency=None, odom_covariance=None, marginals=None, prior_huber_k=0.0):
        """The corrected poses of all entries: a PoseGraph over the entries at their inserted poses, the odometry edges
        Z = T_k^-1 T_k+1 of those poses (information odom_information, one 6 x 6 for all), the loops of AddLoop, and Optimize(cfg)
        -> (poses [n, 4, 4], PoseGraph.Optimize's result).  apply=True replaces self.poses (Submap, Guess and Map then use them).
        The default informations are the identity, which weighs a metre like a radian and an odometry step like a verified loop: a
        caller with real data passes informations that say how good its odometry and its loops are.  preconditioner: PoseGraph's
        ("block_jacobi" | "chain"); the entries are a chain by construction, which is what "chain" is made for.
        initialize=True runs PoseGraph.Initialize (rotations first, then translations, both linear) before Optimize and puts its result
        under "initialize" in the returned dict: the start that a long loop needs, whose drift is far outside Gauss-Newton's reach.  A
        false loop pulls a linear initialization as hard as a true one: Huber acts only in Optimize, so verify loops before adding
        them.  consistency: a LoopConsistencyConfig; then only the members of ConsistentLoops(consistency) are added to the graph, in
        their original order, and its dict is put under "consistency"; odom_covariance is handed to ConsistentLoops with it (the
        covariance model) and is not used otherwise.  marginals: node indices; then one Linearize at the final poses with cfg's huber_k
        and PoseGraph.Marginals(marginals) put the covariances [m, 6, 6] under "marginals" and the call's stats under
        "marginals_stats", solved with the same preconditioner.  The priors of AddPosePrior / AddPositionPrior are added in the order
        they were given, under the Huber threshold prior_huber_k of their own (0: off); with at least one, fixed=() is legal: the priors
        tie the graph to the world.  initialize=True ignores them (and refuses fixed=()); initialize="priors" runs
        PoseGraph.InitializeWithPriors instead, which uses them and needs no fixed node: the start for a long log held by GNSS positions
        or map matches alone.  The defaults, without priors, leave every result as it was."""
        from .posegraph import PoseGraph
        n = len(self.scans)
        if n < 2:
            raise ElmError("LoopCloser.Close: at least two entries")
        with_priors = isinstance(initialize, str)
        if with_priors and initialize != "priors":
            raise ElmError(f"LoopCloser.Close: initialize is False, True or \"priors\", not {initialize!r}")
        P = np.stack(self.poses)
        kept = self.ConsistentLoops(consistency, odom_covariance=odom_covariance) if consistency is not None else None
        loops = self.loops if kept is None else [self.loops[k] for k in kept["members"]]
        pg = PoseGraph(n, n - 1 + max(len(loops), 1), self.ctx, prior_capacity=len(self.priors))
        try:
            fx = np.zeros(n, bool)
            fx[list(fixed)] = True
            pg.SetPreconditioner(preconditioner)
            pg.AddNodes(P, fx)
            Z = np.linalg.inv(P[:-1]) @ P[1:]
            pg.AddEdges(np.arange(n - 1), np.arange(1, n), Z, None if odom_information is None else np.asarray(odom_information, dtype=np.float64))
            if loops:
                pg.AddEdges([l[0] for l in loops], [l[1] for l in loops], np.stack([l[2] for l in loops]), np.stack([l[3] for l in loops]))
            if self.priors:
                pg.SetPriorHuber(prior_huber_k)
                pg.AddPriors([q[0] for q in self.priors], np.stack([q[1] for q in self.priors]), np.stack([q[2] for q in self.priors]),
                             np.stack([q[3] for q in self.priors]))
            init = pg.InitializeWithPriors() if with_priors else pg.Initialize() if initialize else None
            res = pg.Optimize(cfg)
            if initialize:
                res["initialize"] = init
            if kept is not None:
                res["consistency"] = kept
            out = pg.Poses()
            if marginals is not None:
                pg.Linearize(0.0 if cfg is None else float(cfg.huber_k))
                res["marginals"], res["marginals_stats"] = pg.Marginals(marginals, return_stats=True)
        finally:
            pg.close()
        if apply:
            self.poses = [out[k].copy() for k in range(n)]
        return out, res

    def Map(self, poses=None):
        """The whole-log device build of the kept scans at the current (or the given) poses."""
        P = np.stack(self.poses) if poses is None else np.asarray(poses, dtype=np.float64).reshape(-1, 4, 4)
        if P.shape[0] != len(self.scans):
            raise ElmError("LoopCloser.Map: one pose per entry")
        base = VoxelHashMap(self.voxel_size, self.max_points_per_voxel, self.ctx, device_build=True)
        return base.UpdatedFromScans(self.scans, P)
