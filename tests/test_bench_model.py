"""bench.py's roofline model as plain functions (no GPU): no utilisation above 1 is ever printed, a counter pass speaks only for its
own operating point (per GPU, at every N), and the N > 1 default keeps the N = 1 operating point."""
import glob
import json
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402


def test_pmc_key_names_the_operating_point():
    assert bench.pmc_key("k_accumulate_grid<P2P>", 131072, 10_000_000, "easy") == "k_accumulate_grid<P2P>"
    assert bench.pmc_key("k_accumulate_grid<P2P>", 131072, 10_000_000, "hard") == "k_accumulate_grid<P2P>@hard"
    assert bench.pmc_key("k_accumulate_vnbr<VGICP>", 32768, 50_000_000, "easy") == "k_accumulate_vnbr<VGICP>@32768/50000000"
    assert bench.pmc_key("k_accumulate_grid<GICP>", 131072, 10_000_000, "easy", "field") == "k_accumulate_grid<GICP>@field"


def test_index_is_charged_at_most_its_touched_part():
    # the round-4 failure: 32 slots of 262144-point scans on the 50 M-point map were charged the whole 3.5 GB index per launch
    idx = 3.5e9
    b = bench.index_touch_bound(idx, 32 * 262144, 250.0, 32, 50_000_000)
    assert b < 0.3 * idx
    # the headline: 256 scans cover the 10 M-point map several times over -> the whole index, once
    assert 0.2499e9 - bench.L2_TOTAL_BYTES < bench.index_touch_bound(0.25e9, 256 * 131072 * 0.9, 250.0, 230, 10_000_000) <= 0.25e9 - bench.L2_TOTAL_BYTES
    # never more than the points request
    assert bench.index_touch_bound(1e9, 1000, 100.0, 1, 10_000_000) <= 1e5


@pytest.mark.parametrize("path", sorted(glob.glob(os.path.join(ROOT, "profiles", "r04*_bench.json")) + glob.glob(os.path.join(ROOT, "profiles", "r05*_bench*.json"))))
def test_no_recorded_operating_point_yields_a_fraction_above_one(path):
    """every bench line committed under profiles/ re-priced with the current model: the compulsory stream stays below the HBM peak"""
    r = json.load(open(path))
    if "roofline" not in r or "config" not in r or r["config"].get("slots_per_gpu", 0) <= 0:
        pytest.skip("not a stream bench line")
    rf = r["roofline"]
    hv = rf.get("hbm", rf)
    method = {"P2P": 0, "GICP": 1, "VGICP": 2, "AVGICP": 3}[rf["kernel"].split("<")[1].rstrip(">")]
    sp = int(r["config"].get("scan_points", 262144 if "262144" in r["config"]["workload"] else 131072))
    mp = int(r["config"].get("map_points", 50_000_000 if "50000000" in r["config"]["workload"] else 10_000_000))
    upl, sec = rf["units_per_launch"], rf["avg_launch_ms"] * 1e-3
    h = bench.hbm_object(method, rf["index_bytes"], upl, sec, hv["requested_bytes_per_unit"], hv["algorithmic_ref_bytes_per_unit"], upl / sp, mp)
    assert h["frac"] <= 1.05 and h["compulsory_frac"] <= 1.05, (path, h["frac"])
    bench.assert_fractions({"roofline": bench.build_roofline(method, rf["kernel"], h, None, upl, rf["avg_launch_ms"])})


def test_assert_fractions_refuses_a_utilisation_above_one():
    bench.assert_fractions({"roofline": {"frac": 0.93, "hbm": {"frac": 0.26, "compulsory_frac": 0.11}}})
    with pytest.raises(AssertionError):
        bench.assert_fractions({"configs": {"C4_shard": {"roofline": {"frac": 4.997}}}})


def test_counter_pass_speaks_for_its_own_operating_point_at_any_n(tmp_path, monkeypatch):
    """per-GPU batch / slots and units per launch decide, not the number of ranks (round 4 refused every pass at N > 1)"""
    prof = tmp_path / "profiles"
    prof.mkdir()
    entry = {"batch": 4096, "slots": 256, "guess": "easy", "scan_points": 131072, "map_points": 10_000_000, "units_per_launch_profiled": 30.0e6,
             "hbm_bytes_per_unit": 58.7, "valu_insts_per_simd_cycle": 0.2448, "ta_busy": 0.81}
    (prof / "pmc_latest.json").write_text(json.dumps({"k_accumulate_grid<P2P>": entry}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    k = "k_accumulate_grid<P2P>"
    assert bench.load_counter_pass(k, 131072, 10_000_000, "easy", 4096, 256, 30.1e6) is not None
    assert bench.load_counter_pass(k, 131072, 10_000_000, "easy", 4096, 256, 29.0e6) is not None  # a rank of an 8-GPU run: same per-GPU point
    assert bench.load_counter_pass(k, 131072, 10_000_000, "easy", 1024, 256, 30.1e6) is None       # another batch: another launch mix
    assert bench.load_counter_pass(k, 131072, 10_000_000, "easy", 4096, 256, 8.0e6) is None        # a quarter of the work per launch
    assert bench.load_counter_pass(k, 131072, 10_000_000, "hard", 4096, 256, 30.1e6) is None
    assert bench.load_counter_pass(k, 32768, 50_000_000, "easy", 4096, 256, 30.1e6) is None
    assert bench.load_counter_pass(k, 131072, 10_000_000, "easy", 4096, 256, 30.1e6, "field") is None   # another world: another pass
    pm = bench.load_counter_pass(k, 131072, 10_000_000, "easy", 4096, 256, 30.1e6)
    h = bench.hbm_object(0, 0.25e9, 30.1e6, 0.84e-3, 303.0, 3348.0, 230, 10_000_000, pm["hbm_bytes_per_unit"] * 30.1e6, "test")
    rf = bench.build_roofline(0, k, h, pm, 30.1e6, 0.84)
    assert rf["bound"] == "valu_issue" and 0.9 < rf["frac"] < 0.95 and 0.2 < rf["hbm"]["frac"] < 0.3


def test_default_operating_point_is_the_same_at_every_n():
    """bench.py --batch 0: 4096 registrations per GPU at N = 1 and at N > 1 (round 4: 4096 vs 1024 -- the first step of the scaling curve
    compared two different launch mixes)"""
    src = open(os.path.join(ROOT, "bench.py")).read()
    assert "args.batch = 4096  # the SAME per-GPU operating point at every N" in src
    assert "4096 if world_size == 1 else 1024" not in src


def test_c_caller_numbers_never_raise():
    """bench.py's c_caller object: compiles the two plain-C examples and runs them as child processes; without a GPU (here) both exit with
    an error -- reported inside the object, never raised (an auxiliary leg must not cost the line its timed numbers)."""
    import bench
    out = bench.c_caller_numbers(timeout_s=30)
    assert isinstance(out, dict) and "what" in out
    for key in ("register", "config5"):
        assert key in out or "error" in out
        if key in out:
            assert isinstance(out[key], dict)


# ---- the driver line (round 5's 45 KB line was not parsed) ----
REQUIRED_TOP = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data",
                "config", "roofline")
REQUIRED_ROOFLINE = ("bound", "achieved", "peak", "unit", "frac", "traffic", "hbm_frac", "compulsory_bytes_per_unit", "kernel", "avg_launch_ms",
                     "units_per_launch")


def _strings(obj, path=""):
    if isinstance(obj, dict):
        for k, v in obj.items():
            yield from _strings(v, f"{path}.{k}")
    elif isinstance(obj, list):
        for i, v in enumerate(obj):
            yield from _strings(v, f"{path}[{i}]")
    elif isinstance(obj, str):
        yield path, obj


@pytest.mark.parametrize("name", ["r05_final_default_bench.json", "r05_final_dist1_bench.json"])
def test_driver_line_is_small_and_complete(name):
    """the ONE stdout line, built from a committed full record: below the hard size limit, one line, every contract key present, numbers only
    under `configs`, and the top-level roofline is the HBM one (north_star) with the busiest unit beside it"""
    full = json.load(open(os.path.join(ROOT, "profiles", name)))
    text = bench.driver_line(full)
    assert len(text) < bench.LINE_LIMIT <= 6000 and "\n" not in text
    line = json.loads(text)
    for k in REQUIRED_TOP:
        assert k in line, k
    for k in REQUIRED_ROOFLINE:
        assert line["roofline"].get(k) is not None, k
    rf = line["roofline"]
    assert rf["bound"] == "hbm" and rf["unit"] == "GB/s" and rf["peak"] == 8000.0
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-4 and rf["frac"] == rf["hbm_frac"]
    assert abs(rf["achieved"] - rf["traffic"] / (rf["avg_launch_ms"] * 1e-3) / 1e9) < 0.01 * rf["achieved"]
    assert rf["limiter"] in ("valu_issue", "vector_memory_issue", "hbm") and rf["limiter_frac"] <= 1.05
    assert abs(line["value"] - full["value"]) < 1e-5 * full["value"] and line["steps"] == full["steps"] and line["warmup"] == full["warmup"]
    assert "workload" in line["config"] and line["config"]["iterations_mean"] > 1
    if "cpu_baseline" in full:
        for k in ("value", "unit", "cores", "kind", "sample", "cpu_model", "value_all_cores"):
            assert k in line["cpu_baseline"], k
        assert line["pose_err_vs_cpu"]["max_trans_m"] < 1e-4 and line["pose_err_vs_cpu"]["max_rot_rad"] < 1e-5
        assert line["pose_err_vs_cpu"]["pair_mismatches"] == 0
    if "configs" in full:
        assert set(line["configs"]) == set(full["configs"])
        for path, s in _strings(line["configs"]):
            assert len(s) <= 24, (path, s)          # unit names only: no prose
        for leg in ("C3_gicp", "vgicp", "avgicp", "C4_shard"):
            assert len(json.dumps(line["configs"][leg])) < 400
    long_strings = [(p, s) for p, s in _strings(line) if len(s) > 130]
    assert not long_strings, long_strings


def test_driver_line_sheds_optional_blocks_rather_than_break_the_limit():
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_final_default_bench.json")))
    full["configs"] = {f"leg{i}": dict(full["configs"]["C3_gicp"]) for i in range(40)}   # a future builder adds legs
    text = bench.driver_line(full)
    line = json.loads(text)
    assert len(text) < bench.LINE_LIMIT and "configs" not in line and "roofline" in line and "cpu_baseline" in line


def test_emit_writes_the_full_record_beside_the_line(tmp_path, capsys):
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_final_default_bench.json")))
    path = tmp_path / "bench_full.json"
    text = bench.emit(full, str(path))
    out = capsys.readouterr()
    assert out.out.strip() == text and out.out.count("\n") == 1
    assert json.load(open(path)) == full and json.loads(out.err) == full


def test_compulsory_is_a_lower_bound_or_the_line_is_refused():
    """measured traffic below the compulsory bound means the model charges bytes the kernel does not read"""
    ok = {"roofline": {"unit": "GB/s", "achieved": 2100.0, "traffic": 1.8e9, "compulsory_gbs": 750.0, "frac": 0.26}}
    bench.assert_fractions(ok)
    bad = {"configs": {"vgicp": {"roofline": {"hbm": {"unit": "GB/s", "achieved": 1100.0, "traffic": 1.2e9, "compulsory_gbs": 1700.0, "frac": 0.14}}}}}
    with pytest.raises(AssertionError):
        bench.assert_fractions(bad)
    # no counter pass (traffic None): `achieved` IS the compulsory figure, nothing to compare
    bench.assert_fractions({"roofline": {"unit": "GB/s", "achieved": 750.0, "traffic": None, "compulsory_gbs": 750.0, "frac": 0.09}})


def test_a_shard_covers_its_share_of_the_footprint():
    """locality-aware shards: 256 shards of 1 / 8 of a scan's footprint lie over an eighth of the index a whole scan's footprint would"""
    L2 = bench.L2_TOTAL_BYTES
    whole = bench.index_touch_bound(1.0e9, 7.8e6, 300.0, 64, 50_000_000) + L2
    shard = bench.index_touch_bound(1.0e9, 7.8e6, 300.0, 64, 50_000_000, shard_of=8) + L2
    assert 0.12 * whole < shard < 0.16 * whole  # ~1 / 8 of it (the 64 whole footprints overlap a little more than the 64 shard footprints)
    h1 = bench.hbm_object(2, 5.2e8, 7.8e6, 0.15e-3, 273.0, 584.0, 238, 50_000_000, 60.0 * 7.8e6, "test", shard_of=8)
    assert h1["compulsory_bytes_per_unit"] < 60.0 and h1["achieved"] >= 0.95 * h1["compulsory_gbs"]


def test_counter_pass_of_another_shard_shape_is_refused(tmp_path, monkeypatch):
    prof = tmp_path / "profiles"
    prof.mkdir()
    k = "k_accumulate_vnbr<VGICP>"
    entry = {"batch": 2048, "slots": 256, "guess": "easy", "scan_points": 32768, "map_points": 50_000_000, "units_per_launch_profiled": 7.8e6, "shard_of": 8,
             "hbm_bytes_per_unit": 60.0}
    (prof / "pmc_latest.json").write_text(json.dumps({bench.pmc_key(k, 32768, 50_000_000, "easy"): entry}))
    monkeypatch.setattr(bench, "ROOT", str(tmp_path))
    assert bench.load_counter_pass(k, 32768, 50_000_000, "easy", 2048, 256, 7.8e6, "lattice", 8) is not None
    assert bench.load_counter_pass(k, 32768, 50_000_000, "easy", 2048, 256, 7.8e6, "lattice", 1) is None  # thinned-out scans: another traffic pattern


def test_a_model_error_never_costs_the_line():
    """main() sanitises instead of raising: the offending figures are dropped and the error is listed; the line still builds"""
    full = json.load(open(os.path.join(ROOT, "profiles", "r05_final_default_bench.json")))
    h = full["configs"]["C4_shard"]["roofline"]["hbm"]
    h["compulsory_gbs"] = 2.0 * h["achieved"]
    errs = bench.sanitize_fractions(full)  # (round 5's record also holds the vnbr legs whose bound exceeded the measurement: VERDICT r5 weak 8)
    assert errs and any("C4_shard" in e for e in errs) and h["compulsory_gbs"] is None and "model_error" in h
    line = json.loads(bench.driver_line(full))
    assert line["model_errors"] == len(errs) and line["configs"]["C4_shard"]["value"] > 0
    bench.assert_fractions(full)  # nothing left to complain about


def test_footprints_overlap_before_they_tile_the_map():
    a = bench.index_touch_bound(1.0e9, 1e12, 1e6, 235, 50_000_000, shard_of=8)
    assert 0.18e9 < a + bench.L2_TOTAL_BYTES < 0.20e9  # 1 - exp(-0.214), not 0.214 (minus what the L2s keep between launches)
    assert bench.index_touch_bound(0.25e9, 1e12, 1e6, 235, 10_000_000) > 0.249e9 - bench.L2_TOTAL_BYTES


def test_dump_outputs_writes_float64_rows_and_samples_a_large_batch(tmp_path, monkeypatch):
    """--dump-outputs: one row per registration in input order, float64; above the size limit a fixed sample of rows (the same every run)"""
    rng = np.random.default_rng(5)
    out = [dict(T=rng.standard_normal((4, 4)), local_cov=rng.standard_normal((6, 6)), fitness_score=0.1 * i, d_fitness=0.0, is_success=i % 3 > 0,
                iterations=i % 7, gate=0, path=1, n_corr_last=100.0 + i, point_iterations=1e3 * i) for i in range(50)]
    bench.dump_outputs(str(tmp_path / "all"), out)
    a = {f.stem: np.load(f) for f in (tmp_path / "all").glob("*.npy")}
    assert set(a) == {"registration", "T", "local_cov", "fitness_score", "d_fitness", "is_success", "iterations", "gate", "path", "n_corr_last",
                      "point_iterations"}
    assert all(v.dtype == np.float64 and v.shape[0] == 50 for v in a.values())
    assert np.array_equal(a["T"][7], out[7]["T"]) and a["iterations"][13] == 6 and a["is_success"][3] == 0.0
    per_reg = 8 * (1 + 16 + 36 + 8)
    monkeypatch.setattr(bench, "DUMP_LIMIT_BYTES", 20 * per_reg)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / f"s{k}"), out)
    s0, s1 = ({f.stem: np.load(f) for f in (tmp_path / f"s{k}").glob("*.npy")} for k in range(2))
    idx = s0["registration"].astype(int)
    assert len(idx) == 20 and np.all(np.diff(idx) > 0) and sum(v.nbytes for v in s0.values()) <= 20 * per_reg
    assert np.array_equal(s0["T"], np.stack([out[i]["T"] for i in idx]))
    assert all(np.array_equal(s0[k], s1[k]) for k in s0)
