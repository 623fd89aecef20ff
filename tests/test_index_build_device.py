"""The device index build on the GPU (elm_map_set_index_build): for every case two maps from the same points, one with the host index and
one with the device index -- layout_flags bit 9 on the second only; the descriptor, block starts, slot points, tile table and the blocks
(as bit patterns) np.array_equal between the two and equal to the numpy mirror (tests/grid_ref.py); elm_map_get_info equal field by
field but for bit 9.  Families: the block, wave, workgroup and scan-chunk edges of the point count; hundreds of points in one cell; the
cell faces and their float32 neighbours, voxel 0.3, a cloud 1e5 m out; boxes of one, two and four radix passes and of one entry more
than a scan chunk; the same under the two-level form, forced and after a refused dense form, with its tile shapes; the wide form;
repeats; registrations, correspondences and the derived maps; refusals and no-ops; the 1 M world once."""
import ctypes as C
import functools

import numpy as np
import pytest

import grid_ref  # tests/ is on sys.path via conftest
from elimaloc_amd import _lib, synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.registration import (Context, EvidenceConfig, GrowthConfig, IcpMethod, Registration, RegistrationConfig, Scan,
                                        VoxelHashMap)

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -5
BIT9 = 512
f32 = np.float32


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


# ---------------------------------------------------------------- the clouds
def _own_voxel(n):
    """n points, each alone in its voxel (a 16 x 16 x k lattice of voxels around the origin): all are stored, in input order"""
    i = np.arange(n)
    base = np.stack([i % 16 - 8, (i // 16) % 16 - 8, i // 256 - 2], 1).astype(np.float64)
    return (base + np.random.default_rng(n).uniform(0.05, 0.95, (n, 3))).astype(f32)


def _one_cell(n):
    """n <= 8 points of ONE half-voxel cell, 0.25 m apart (more than the spacing rule's 0.18 m at cap 30)"""
    c = np.array([[x, y, z] for z in (0.1, 0.35) for y in (0.1, 0.35) for x in (0.1, 0.35)])
    return c[:n].astype(f32)


def _crowded_cell():
    """1 500 points in the cell [0, 0.5)^3 of one voxel, cap 400 (spacing 0.05 m): what is stored is well over a wavefront, in one cell"""
    return np.random.default_rng(400).uniform(0.0, 0.4999, (1500, 3)).astype(f32)


def _faces():
    """every combination of values on and next to the cell faces, per axis"""
    v = [0.5, -0.5, 0.999, -0.999, -0.0, 0.0, 1.0, -1.0, 1.5, -1.5, 2.0, -2.0]
    v += [np.nextafter(f32(a), f32(s)) for a in (0.5, -0.5, 1.0, -1.0, 1.5, -1.5) for s in (-9, 9)]
    v = np.array(v, f32)
    rng = np.random.default_rng(5)
    return np.stack([v[rng.permutation(len(v))] for _ in range(3)], 1), v


def _faces_cloud():
    cols, v = _faces()
    rng = np.random.default_rng(6)
    more = v[rng.integers(0, len(v), (300, 3))]
    return np.concatenate([cols, more]).astype(f32)


def _two_clusters(far):
    rng = np.random.default_rng(24)
    a = rng.uniform(0.0, 3.0, (300, 3))
    return np.concatenate([a, rng.uniform(0.0, 3.0, (300, 3)) + far]).astype(f32)


def _tiles_cloud():
    """cells 0 .. 17 in x and y (3 x 3 tiles, the corner point in the last row and column): tile (1, 1) empty between occupied ones, tile
    (2, 2) with every point in one z cell, a tower of 30 m in tile (0, 0)"""
    rng = np.random.default_rng(33)
    p = rng.uniform([0.0, 0.0, 0.0], [8.9, 8.9, 2.9], (2500, 3))
    hole = (p[:, 0] >= 3.0) & (p[:, 0] < 7.0) & (p[:, 1] >= 3.0) & (p[:, 1] < 7.0)
    p = p[~hole]
    flat = (p[:, 0] >= 7.0) & (p[:, 1] >= 7.0)
    p[flat, 2] = rng.uniform(0.05, 0.45, int(flat.sum()))
    tower = np.stack([rng.uniform(0.5, 2.5, 200), rng.uniform(0.5, 2.5, 200), rng.uniform(0.0, 30.0, 200)], 1)
    ends = np.array([[0.1, 0.1, 0.2], [8.6, 8.6, 0.2]])
    return np.concatenate([ends, p, tower]).astype(f32)


CLOUDS = {
    **{"one_cell_%d" % n: (lambda n=n: _one_cell(n), 1.0, 30) for n in (1, 3, 4, 5)},
    **{"own_voxel_%d" % n: (lambda n=n: _own_voxel(n), 1.0, 30) for n in (63, 64, 65, 255, 256, 257, 1023, 1024, 1025)},
    "crowded_cell": (_crowded_cell, 1.0, 400),
    "faces": (_faces_cloud, 1.0, 30),
    "voxel_03": (lambda: np.random.default_rng(3).uniform(-2.0, 2.0, (3000, 3)).astype(f32), 0.3, 30),
    "offset_1e5": (lambda: (np.random.default_rng(4).uniform(-5.0, 5.0, (3000, 3)) + (1e5, -1e5, 50.0)).astype(f32), 1.0, 30),
    "cells_2_24": (lambda: _two_clusters((150.0, 150.0, 90.0)), 1.0, 30),       # ~17.5 M cells: four radix passes, 70 MB of block starts
    "scan_chunk": (lambda: np.concatenate([[[0.1, 0.1, 0.1], [49.1, 48.1, 48.1]], np.random.default_rng(8).uniform(0, 48, (500, 3))]).astype(f32), 1.0, 30),
    "tiles": (_tiles_cloud, 1.0, 30),
}
DENSE = list(CLOUDS)
TILED = ["one_cell_1", "one_cell_5", "own_voxel_64", "own_voxel_257", "own_voxel_1025", "crowded_cell", "faces", "voxel_03", "offset_1e5", "tiles"]


@functools.lru_cache(maxsize=None)
def _cloud(name):
    make, vs, cap = CLOUDS[name]
    return make(), vs, cap


# ---------------------------------------------------------------- the comparison
def _map(c, pts, vs, cap, device_index, build=True):
    vm = VoxelHashMap(vs, cap, c, device_index=device_index)
    vm.AddPoints(pts)
    if build:
        vm.BuildNeighbourhoods()
    return vm


def _info(vm):
    mi = vm.info()
    out = {}
    for n, _ in mi._fields_:
        v = getattr(mi, n)
        out[n] = tuple(v) if hasattr(v, "__len__") else v
    return out


def _same_grids(a, b):
    assert a["desc"] == b["desc"], (a["desc"], b["desc"])
    for k in ("start", "slot_point", "tiles"):
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
    assert a["blocks"].shape == b["blocks"].shape and np.array_equal(a["blocks"].view(np.uint32), b["blocks"].view(np.uint32))


def _compare(host, dev, tiled, narrow_limit=0xFFFFFF00):
    ih, idv = _info(host), _info(dev)
    assert idv["layout_flags"] & BIT9 and not ih["layout_flags"] & BIT9, (ih["layout_flags"], idv["layout_flags"])
    idv["layout_flags"] &= ~BIT9
    assert ih == idv, {k: (ih[k], idv[k]) for k in ih if ih[k] != idv[k]}
    assert bool(ih["layout_flags"] & 4) == tiled
    gh, gd = host.CellGrid(), dev.CellGrid()
    _same_grids(gh, gd)
    ref = grid_ref.grid(host.Pointcloud().astype(f32), host.voxel_size_, tiled, narrow_limit)
    for k, v in ref["desc"].items():
        assert gd["desc"][k] == v, (k, gd["desc"][k], v)
    for k in ("start", "slot_point", "tiles"):
        assert np.array_equal(gd[k], ref[k]), k
    assert np.array_equal(gd["blocks"].view(np.uint32), ref["blocks"].view(np.uint32))
    return gd


def _pair(c, name, tiled, narrow_limit=0xFFFFFF00):
    pts, vs, cap = _cloud(name)
    host, dev = _map(c, pts, vs, cap, False), _map(c, pts, vs, cap, True)
    return _compare(host, dev, tiled, narrow_limit)


@pytest.mark.parametrize("name", DENSE)
def test_device_grid_is_the_host_grid_dense(ctx, name):
    g = _pair(ctx, name, False)
    cells, n = g["desc"]["n_start_words"] - 4, int((g["slot_point"] != grid_ref.PAD_POINT).sum())
    per_cell = np.diff(g["start"][:cells + 1].astype(np.int64)).max() * 4
    print(f"{name}: {n} stored points, {cells} cells, {g['desc']['n_blocks']} blocks, at most {per_cell} slots in a cell")
    if name.startswith("one_cell_") or name.startswith("own_voxel_"):
        assert n == int(name.rsplit("_", 1)[1])  # the edge is the STORED count
    if name.startswith("one_cell_"):
        assert cells < 256 and g["desc"]["n_blocks"] == 1 + (n + 3) // 4  # one radix pass; all points in one cell
    if name.startswith("own_voxel_"):
        assert 256 <= cells < 65536  # two radix passes
    if name == "crowded_cell":
        assert n > 128 and g["desc"]["n_blocks"] == 1 + (n + 3) // 4  # one cell, well over a wavefront
    if name == "cells_2_24":
        assert cells > 2 ** 24  # four radix passes
    if name == "scan_chunk":
        assert 1024 * 1024 < cells <= 1024 * 1024 + 4096  # the workgroup sums are one chunk and a few entries
    if name == "faces":
        assert n >= 100


@pytest.mark.parametrize("grid", ["tiled", "max_cells=100"])
@pytest.mark.parametrize("name", TILED)
def test_device_grid_is_the_host_grid_tiled(ctx, monkeypatch, name, grid):
    """forced, and after the dense form was refused (every box here has at least 125 cells)"""
    monkeypatch.setenv("ELM_GRID", grid)
    g = _pair(ctx, name, True)
    if name == "tiles":
        t = g["tiles"].reshape(3, 3, 2)
        nz = t[:, :, 1] >> 16
        assert not t[1, 1].any() and all(t[i, j].any() for i in range(3) for j in range(3) if (i, j) != (1, 1))  # the hole, between occupied tiles
        assert nz[2, 2] == 1 and nz[0, 0] >= 40  # one z cell; the tower


def test_wide_form_and_its_registration(ctx, monkeypatch):
    monkeypatch.setenv("ELM_GRID", "max_block_bytes=48")
    pts, vs, cap = _cloud("tiles")
    host, dev = _map(ctx, pts, vs, cap, False), _map(ctx, pts, vs, cap, True)
    g = _compare(host, dev, False, 48)
    assert g["desc"]["grid_wide"] == 1
    assert _register(ctx, host, pts, IcpMethod.P2P) == _register(ctx, dev, pts, IcpMethod.P2P)


def test_five_repeats_of_the_densest_case_are_byte_identical(ctx):
    pts, vs, cap = _cloud("crowded_cell")
    first = _map(ctx, pts, vs, cap, True).CellGrid()
    for _ in range(4):
        vm = _map(ctx, pts, vs, cap, True)
        assert vm.info().layout_flags & BIT9
        _same_grids(vm.CellGrid(), first)


# ---------------------------------------------------------------- downstream
def _register(c, vm, world, method, seed=7):
    scan, T = synth.make_scan(world, 2000, seed=seed)
    T0 = np.array(T)
    T0[:3, 3] += (0.2, -0.1, 0.05)
    pose, ok, fit, cov, d = Registration(RegistrationConfig(icp_method=method), c).RunRegister(scan, vm, T0, trace=True)
    return (pose.tobytes(), ok, fit, cov.tobytes(), d["iterations"], d["gate"], d["path"], d["n_corr_last"])


@pytest.fixture(scope="module")
def world100k():
    return synth.make_world(100000, seed=1001)


@pytest.mark.parametrize("cov_first", [True, False])
def test_registrations_and_correspondences_on_the_100k_world(ctx, world100k, cov_first):
    """CalPointCovAll before the index exists (the commit gathers the GICP records) and after (the covariance call refreshes them)"""
    out = []
    for device_index in (False, True):
        vm = _map(ctx, world100k, 1.0, 30, device_index, build=False)
        if cov_first:
            vm.CalPointCovAll(0.4)
        res = [_register(ctx, vm, world100k, IcpMethod.P2P)]  # the lazy build
        if not cov_first:
            vm.CalPointCovAll(0.4)
        res.append(_register(ctx, vm, world100k, IcpMethod.GICP))
        q = synth.make_scan(world100k, 3000, seed=11)[0]
        src, tgt, si, ti = vm.GetCorrespondencePoints(np.asarray(q, np.float64), 1.0, indices=True)
        res.append((src.tobytes(), tgt.tobytes(), np.asarray(si).tobytes(), np.asarray(ti).tobytes()))
        assert bool(vm.info().layout_flags & BIT9) == device_index
        out.append((res, vm.CellGrid(), _info(vm)))
    assert out[0][0] == out[1][0]
    _same_grids(out[0][1], out[1][1])
    out[1][2]["layout_flags"] &= ~BIT9
    assert out[0][2] == out[1][2]
    print([(r[1], r[4], r[5], r[6]) for r in out[1][0][:2]], len(out[1][0][2][2]) // 4, "pairs")


def test_derived_maps_keep_the_preference(ctx):
    """Updated, WithoutStale(device=True) and WithAppeared(device=True) on the box scene of tests/test_map_build_device.py: the derived map
    builds its grid on the device and registers to the bytes of a host-index twin (a map built from its stored points, which replay
    to themselves)"""
    from test_map_build_device import _box
    field = synth.make_field_world(300_000, seed=4242)
    vm_a = VoxelHashMap(1.0, 20, ctx, device_index=True)
    vm_a.AddPoints(field)
    box, poses = _box(vm_a, np.random.default_rng(1))
    vm_b = VoxelHashMap(1.0, 20, ctx, device_index=True)
    vm_b.AddPoints(np.concatenate([field, box]))
    beams = synth.lidar_beams(32, 512)
    ev = vm_b.Evidence()
    ev.Accumulate([Scan(ctx, vm_a.RenderScan(P, beams)) for P in poses], poses, EvidenceConfig())
    scans_b = [Scan(ctx, vm_b.RenderScan(P, beams)) for P in poses]
    g = vm_a.Growth(sum(s.n for s in scans_b))
    g.Accumulate(scans_b, poses, GrowthConfig())
    derived = {"updated": vm_a.Updated(box), "pruned": vm_b.WithoutStale(ev, device=True), "grown": vm_a.WithAppeared(g, device=True)}
    ev.close()
    g.close()
    for name, dev in derived.items():
        assert dev._derived and dev.device_index_
        stored = dev.Pointcloud().astype(f32)
        twin = _map(ctx, stored, 1.0, 20, False)
        assert np.array_equal(twin.Pointcloud(), dev.Pointcloud())
        assert _register(ctx, dev, stored, IcpMethod.P2P) == _register(ctx, twin, stored, IcpMethod.P2P), name
        assert dev.info().layout_flags & BIT9 and not twin.info().layout_flags & BIT9, name
        _same_grids(dev.CellGrid(), twin.CellGrid())


# ---------------------------------------------------------------- refusals and no-ops
def test_refusals_and_no_ops(ctx, monkeypatch):
    L = _lib.lib()
    pts, vs, cap = _cloud("tiles")
    ref = _map(ctx, pts, vs, cap, False).CellGrid()

    def still_good(c=ctx):
        vm = _map(c, pts, vs, cap, True)
        assert vm.info().layout_flags & BIT9
        _same_grids(vm.CellGrid(), ref)

    vm = _map(ctx, pts, vs, cap, False, build=False)
    h = vm._handle()
    assert L.elm_map_set_index_build(h, 2) == INVALID and L.elm_map_set_index_build(h, -1) == INVALID
    # no grid yet: the read-back refuses and builds nothing
    d = _lib.CellGridDesc()
    assert L.elm_map_download_cell_grid(h, C.byref(d), None, 0, None, 0, None, 0, None, 0) == UNSUPPORTED
    assert vm.info().index_bytes == 0
    with pytest.raises(ElmError):
        vm.CellGrid()
    still_good()
    # the preference after the grid is built changes nothing
    vm.BuildNeighbourhoods()
    before = _info(vm)
    assert L.elm_map_set_index_build(h, 1) == 0
    vm.BuildNeighbourhoods()
    assert _info(vm) == before and not before["layout_flags"] & BIT9
    _same_grids(vm.CellGrid(), ref)
    # caps smaller than the counts: only the caps are written, desc has the full counts
    n_s, n_b = len(ref["start"]), len(ref["blocks"])
    start, blocks, slots = np.full(n_s, 0xABABABAB, np.uint32), np.full((n_b, 3, 4), -3.0, f32), np.full(4 * n_b, 0xABABABAB, np.uint32)
    u32 = lambda a: a.ctypes.data_as(C.POINTER(C.c_uint32))
    assert L.elm_map_download_cell_grid(h, C.byref(d), u32(start), 10, blocks.ctypes.data_as(C.POINTER(C.c_float)), 2, u32(slots), 5, None, 99) == 0
    assert (d.n_start_words, d.n_blocks, d.n_tiles) == (n_s, n_b, 0)
    assert np.array_equal(start[:10], ref["start"][:10]) and (start[10:] == 0xABABABAB).all()
    assert np.array_equal(blocks[:2].view(np.uint32), ref["blocks"][:2].view(np.uint32)) and (blocks[2:] == -3.0).all()
    assert np.array_equal(slots[:5], ref["slot_point"][:5]) and (slots[5:] == 0xABABABAB).all()
    # a hook attached; a device group's lead and its replicated map
    other = Context(0)
    vo = _map(other, pts, vs, cap, False, build=False)
    other.set_allreduce_hook(lambda p, n_, s: 0)
    assert L.elm_map_set_index_build(vo._handle(), 1) == UNSUPPORTED and "one rank" in L.elm_last_error(other._h).decode()
    other.set_allreduce_hook(None)
    assert L.elm_map_set_index_build(vo._handle(), 1) == 0
    vo.BuildNeighbourhoods()
    assert vo.info().layout_flags & BIT9
    _same_grids(vo.CellGrid(), ref)
    del vo
    other.close()
    grp = Context.multi([0, 0])
    vg = _map(grp, pts, vs, cap, False, build=False)
    assert L.elm_map_set_index_build(vg._handle(), 1) == UNSUPPORTED and "one rank" in L.elm_last_error(grp._h).decode()
    with pytest.raises(ElmError):
        _map(grp, pts, vs, cap, True, build=False)._handle()
    del vg
    grp.close()
    still_good()
    # ELM_KERNEL=lists: the lists are built, bit 9 stays clear, there is no grid to read back
    monkeypatch.setenv("ELM_KERNEL", "lists")
    lists = Context(0)
    monkeypatch.delenv("ELM_KERNEL")
    vl = _map(lists, pts, vs, cap, True)
    il = _info(vl)
    assert not il["layout_flags"] & BIT9 and il["index_part_bytes"][3] > 0 and il["index_part_bytes"][0] == 0
    with pytest.raises(ElmError):
        vl.CellGrid()
    del vl
    lists.close()
    still_good()


def test_the_1m_lattice_world_once(ctx):
    world = synth.make_world(1_000_000, seed=1001)
    host, dev = _map(ctx, world, 1.0, 30, False), _map(ctx, world, 1.0, 30, True)
    assert dev.info().layout_flags & BIT9 and not host.info().layout_flags & BIT9
    _same_grids(host.CellGrid(), dev.CellGrid())
    print("stages ms", dev.IndexBuildStages().round(3).tolist(), "points", dev.info().n_points)
