"""CPU checks of the Python binding itself: the ctypes signature tables of elimaloc_amd/_lib.py against the prototypes of the three
headers, the config factories against the C defaults and their structs' field types, the statistics dicts against their structs."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from elimaloc_amd import _lib, _marshal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADERS = {"elimaloc_hip.h": _lib.DECLS, "elimaloc_hip_posegraph_precond.h": _lib.DECLS_PRECOND,
           "elimaloc_hip_posegraph_init.h": _lib.DECLS_INIT}


def _prototypes(header):
    """{name: (return type as written, number of parameters)} of every function a header declares."""
    src = open(os.path.join(ROOT, "include", header)).read()
    src = re.sub(r"/\*.*?\*/", " ", src, flags=re.S)
    src = re.sub(r"//[^\n]*", " ", src)
    src = re.sub(r"^\s*#[^\n]*", " ", src, flags=re.M)
    out = {}
    for m in re.finditer(r"(?:^|[;{}])\s*([A-Za-z_][\w\s]*?[\s*]+)(elm_[a-z0-9_]+)\s*\(", src):
        depth, commas, k = 1, 0, m.end()
        while depth:  # to the parenthesis that closes the parameter list; the commas at depth 0 of it separate the parameters
            c = src[k]
            depth += (c in "([") - (c in ")]")
            commas += c == "," and depth == 1
            k += 1
        params = src[m.end():k - 1].strip()
        assert src[k:].lstrip().startswith(";"), m.group(2)
        assert m.group(2) not in out, m.group(2)
        out[m.group(2)] = (" ".join(m.group(1).split()), 0 if params in ("", "void") else commas + 1)
    return out


@pytest.mark.parametrize("header", list(HEADERS))
def test_signature_tables_match_the_headers(header):
    protos, table = _prototypes(header), HEADERS[header]
    assert "elm_allreduce_fn" not in protos  # a typedef, not a function
    assert set(protos) == set(table), set(protos) ^ set(table)
    for name, (ret, n_params) in protos.items():
        restype, argtypes = table[name]
        assert len(argtypes) == n_params, name
        assert (restype is None) == (ret == "void"), name
        if ret == "int":
            assert restype is C.c_int, name
        elif ret != "void":  # a pointer or a size_t: read as an int it would be cut to 32 bits
            assert "*" in ret or ret == "size_t", (name, ret)
            assert restype is not C.c_int and C.sizeof(restype) == C.sizeof(C.c_void_p), name


def test_signature_tables_are_the_whole_surface():
    assert sum(len(_prototypes(h)) for h in HEADERS) == 158
    assert [len(_lib.EXPORTS), len(_lib.EXPORTS_PRECOND), len(_lib.EXPORTS_INIT)] == [154, 2, 2]
    for names, table in ((_lib.EXPORTS, _lib.DECLS), (_lib.EXPORTS_PRECOND, _lib.DECLS_PRECOND), (_lib.EXPORTS_INIT, _lib.DECLS_INIT)):
        assert isinstance(names, list) and names == list(table)
    L = _lib.lib()  # what the tables say is what the loaded functions carry
    for table in HEADERS.values():
        for name, (restype, argtypes) in table.items():
            assert getattr(L, name).restype is restype and list(getattr(L, name).argtypes) == argtypes, name


def _factories():
    from elimaloc_amd import ekf, map_change, odometry, places, posegraph, registration, voxel_map
    return {
        "RegistrationConfig": (registration.RegistrationConfig, _lib.RegConfig, "elm_reg_config_default"),
        "RelocConfig": (voxel_map.RelocConfig, _lib.RelocConfigC, "elm_reloc_config_default"),
        "GlobalRelocConfig": (voxel_map.GlobalRelocConfig, _lib.GlobalRelocConfigC, "elm_reloc_global_config_default"),
        "FreeSpaceConfig": (voxel_map.FreeSpaceConfig, _lib.FreeSpaceConfigC, "elm_freespace_config_default"),
        "RayCastConfig": (voxel_map.RayCastConfig, _lib.RayCastConfigC, "elm_raycast_config_default"),
        "EvidenceConfig": (map_change.EvidenceConfig, _lib.EvidenceConfigC, "elm_evidence_config_default"),
        "EvidenceRule": (map_change.EvidenceRule, _lib.EvidenceRuleC, "elm_evidence_rule_default"),
        "GrowthConfig": (map_change.GrowthConfig, _lib.GrowthConfigC, "elm_growth_config_default"),
        "GrowthRule": (map_change.GrowthRule, _lib.GrowthRuleC, "elm_growth_rule_default"),
        "GrowthObjectRule": (map_change.GrowthObjectRule, _lib.GrowthObjectRuleC, "elm_growth_object_rule_default"),
        "PoseGraphConfig": (posegraph.PoseGraphConfig, _lib.PoseGraphConfigC, "elm_posegraph_config_default"),
        "PoseGraphInitConfig": (posegraph.PoseGraphInitConfig, _lib.PoseGraphInitConfigC, "elm_posegraph_init_config_default"),
        "PlaceConfig": (places.PlaceConfig, _lib.PlacesConfigC, "elm_places_config_default"),
        "EkfConfig": (lambda **kw: ekf.EkfConfig(**kw).c, _lib.EkfConfig, "elm_ekf_config_default"),
        "OdometryConfig": (odometry.OdometryConfig, _lib.OdometryConfigC, "elm_odometry_config_default"),
    }


FACTORIES = ["RegistrationConfig", "RelocConfig", "GlobalRelocConfig", "FreeSpaceConfig", "RayCastConfig", "EvidenceConfig", "EvidenceRule",
             "GrowthConfig", "GrowthRule", "GrowthObjectRule", "PoseGraphConfig", "PoseGraphInitConfig", "PlaceConfig", "EkfConfig"]
INTEGERS = (C.c_int32, C.c_uint32, C.c_int64, C.c_uint64)


def _default(Struct, default):
    ref = Struct()
    getattr(_lib.lib(), default)(C.byref(ref))
    return ref


@pytest.mark.parametrize("name", FACTORIES)
def test_config_factory(name):
    make, Struct, default = _factories()[name]
    assert bytes(make()) == bytes(_default(Struct, default))
    for k, ctype in Struct._fields_:
        if k.startswith("_"):
            continue
        if issubclass(ctype, C.Array):
            assert ctype._type_ is C.c_double
            vals = [0.5 + j for j in range(ctype._length_)]
            tries = [(v, vals) for v in (tuple(vals), list(vals), np.array(vals))]
        elif ctype in (C.c_double, C.c_float):
            tries = [(0.75, 0.75), (2, 2.0), (np.float32(0.3), float(np.float32(0.3)))]
        else:
            assert ctype in INTEGERS, (k, ctype)
            tries = [(3, 3), (True, 1), (np.int64(5), 5)]
        for given, stored in tries:
            cfg, ref = make(**{k: given}), _default(Struct, default)
            setattr(ref, k, ctype(*stored) if issubclass(ctype, C.Array) else stored)
            got = getattr(cfg, k)
            assert (list(got) if issubclass(ctype, C.Array) else got) == stored, (k, given)
            assert bytes(cfg) == bytes(ref), (k, given)  # ... and nothing else moved
    refusal = "unknown EKF config key {}" if name == "EkfConfig" else name + " has no field {}"
    for bad in ["no_such_field"] + (["_pad"] if "_pad" in dict(Struct._fields_) else []):
        with pytest.raises(AttributeError, match=re.escape(refusal.format(bad))):
            make(**{bad: 1})


def test_padding_fields_are_where_the_test_expects_them():
    """the `_pad` refusals above run for these four, and no config struct hides another underscore field"""
    padded = [n for n in FACTORIES if "_pad" in dict(_factories()[n][1]._fields_)]
    assert padded == ["FreeSpaceConfig", "GrowthConfig", "PoseGraphConfig", "EkfConfig"]
    for n in FACTORIES:
        assert [k for k, _ in _factories()[n][1]._fields_ if k.startswith("_")] in ([], ["_pad"])


def test_odometry_config_routes_registration_fields():
    make, Struct, default = _factories()["OdometryConfig"]
    from elimaloc_amd.registration import RegistrationConfig
    assert bytes(make()) == bytes(_default(Struct, default))
    cfg = make(max_iteration=7, voxel_size=0.5)
    ref = _default(Struct, default)
    ref.reg.max_iteration, ref.voxel_size = 7, 0.5
    assert (cfg.reg.max_iteration, cfg.voxel_size) == (7, 0.5) and bytes(cfg) == bytes(ref)
    cfg = make(max_points_per_voxel=np.int64(12), key_min_rot_rad=1, ego_to_lidar_trans=[1, 2, 3], lm_lambda=np.float32(0.25))
    assert (cfg.max_points_per_voxel, cfg.key_min_rot_rad, list(cfg.reg.ego_to_lidar_trans), cfg.reg.lm_lambda) == (12, 1.0, [1.0, 2.0, 3.0], 0.25)
    reg = RegistrationConfig(icp_method=0, max_search_dist=2.5)
    assert bytes(make(reg=reg).reg) == bytes(reg)
    # keywords apply in the caller's order: a whole reg replaces what came before it, a field after it lands in it
    assert make(max_iteration=7, reg=reg).reg.max_iteration == reg.max_iteration
    assert make(reg=reg, max_iteration=7).reg.max_iteration == 7
    for bad in ("no_such_field", "_pad"):
        with pytest.raises(AttributeError, match=re.escape("OdometryConfig has no field " + bad)):
            make(**{bad: 1})


def _filled(Struct):
    """a struct of counters with a different value in every field"""
    st = Struct()
    for j, (k, _) in enumerate(Struct._fields_):
        setattr(st, k, 10 + j)
    return st


def _stats():
    from elimaloc_amd import map_change, places, voxel_map
    return {
        "FreeSpaceStats": (voxel_map.FreeSpaceStats, _lib.FreeSpaceStatsC,
                           ["n_counted", "n_pierced", "n_end_occupied", "n_supported", "n_samples", "n_hit_samples"], ["pierced_share"]),
        "RayCastStats": (voxel_map.RayCastStats, _lib.RayCastStatsC,
                         ["n_cast", "n_hit", "n_miss", "n_truncated", "n_compared", "n_match", "n_through", "n_front", "n_steps"],
                         ["match_share", "through_share", "front_share"]),
        "EvidenceStats": (map_change.EvidenceStats, _lib.EvidenceStatsC,
                          ["n_cast", "n_observing", "n_walked", "n_truncated", "n_through_beams", "n_end_hit", "n_end_free",
                           "n_through_events", "n_steps"], []),
        "GrowthStats": (map_change.GrowthStats, _lib.GrowthStatsC,
                        ["n_cast", "n_observing", "n_walked", "n_truncated", "n_end_hit", "n_end_near", "n_end_new", "n_end_out",
                         "n_through_beams", "n_dropped", "n_through_events", "n_steps"], []),
        "GrowthObjectStats": (_marshal._counts, _lib.GrowthObjectStatsC,  # MapGrowth.FindObjects answers with it as it is
                              ["n_members", "n_objects", "n_small", "n_small_cells", "max_cells"], []),
        "PlaceStats": (places.PlaceStats, _lib.PlacesStatsC, ["n_points", "n_used", "n_bits"], []),
    }


@pytest.mark.parametrize("name", ["FreeSpaceStats", "RayCastStats", "EvidenceStats", "GrowthStats", "GrowthObjectStats", "PlaceStats"])
def test_stats_dict(name):
    to_dict, Struct, keys, derived = _stats()[name]
    assert keys == [k for k, _ in Struct._fields_ if not k.startswith("_")]
    st = _filled(Struct)
    d = to_dict(st)
    assert list(d) == keys + derived
    for k in keys:
        assert type(d[k]) is int and d[k] == getattr(st, k)
    zero = to_dict(Struct())
    for k in derived:
        assert type(zero[k]) is float and zero[k] == 0.0  # no count to share out
    if name == "FreeSpaceStats":
        assert d["pierced_share"] == st.n_pierced / st.n_counted
    if name == "RayCastStats":
        assert [d[k] for k in derived] == [st.n_match / st.n_compared, st.n_through / st.n_compared, st.n_front / st.n_compared]
