"""LiDAR odometry on a rolling local map kept on the device (elm_odometry, include/elimaloc_hip.h)."""
import ctypes as C

import numpy as np

from . import _lib
from ._lib import ElmError, OdometryConfigC, RegConfig, check
from ._marshal import _Owned, _apply, _colmajor16, _config, _counts, _dp, _result_dict
from .context import _resident, default_context
from .voxel_map import VoxelHashMap


def OdometryConfig(**kw):
    """elm_odometry_config with its defaults (voxel 1.0 m, cap 30, max_range_m 100, both keyframe thresholds 0 = every scan is inserted,
    reg = RegistrationConfig()).  reg: a RegistrationConfig; any other keyword that is a field of it is set on reg."""
    cfg = _config("OdometryConfig", OdometryConfigC, "elm_odometry_config_default", {})
    of_reg = dict(RegConfig._fields_)
    for k, v in kw.items():  # one at a time, in the caller's order: a later reg= replaces what an earlier keyword set on reg
        _apply(cfg.reg if k in of_reg else cfg, {k: v}, "OdometryConfig has no field {k}")
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
                    build=_counts(st.build) if st.inserted else None)

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
