"""The device index build (include/elimaloc_hip.h, device index build) on the CPU: the numpy mirror of the cell grid (tests/grid_ref.py)
against grid_block_layout itself (tests/grid_layout_dump.cpp, a program of its own built with the address and undefined-behaviour
sanitizers) and against grid_cell_of's cases worked out by hand; the box, the dense entry and the tile table on a hand-made cloud; the
symbols and values in the header; argument errors without a device; and the C++ shim's BuildIndexOnDevice call lines compiling."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import grid_ref  # tests/ is on sys.path via conftest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(ROOT, "elimaloc_amd", "csrc")
INVALID = -1


@pytest.fixture(scope="module")
def L():
    import __graft_entry__ as g
    from elimaloc_amd import _lib
    if not os.path.exists(_lib.LIB_PATH):
        g.build()
    return _lib.lib()


# ---------------------------------------------------------------- the mirror's layout against grid_block_layout
@pytest.fixture(scope="module")
def dump(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/grid_layout_dump.cpp")
    exe = str(tmp_path_factory.mktemp("grid_layout_dump") / "grid_layout_dump")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            "-static-libasan", "-static-libubsan", "-I", CSRC, os.path.join(HERE, "grid_layout_dump.cpp"), "-o", exe],
                           capture_output=True, text=True)
    assert build.returncode == 0, build.stdout + build.stderr
    return exe


def _layout_cases():
    rng = np.random.default_rng(1901)
    per_entry = [0, 1, 3, 4, 5, 8, 9]
    # every count, in an order that puts empty entries at both ends and between occupied ones
    counts = [0, 0, 9, 1, 0, 3, 4, 0, 5, 8, 0, 0]
    mixed = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    return {
        "counts_0_1_3_4_5_8_9": (mixed, len(counts)),
        "each_count_alone": (np.repeat(np.arange(len(per_entry)), per_entry), len(per_entry)),
        "random_1000_in_300": (rng.integers(0, 300, 1000), 300),
        "random_sparse": (rng.integers(5, 4000, 700), 5000),
        "all_in_one": (np.full(400, 3), 7),
        "first_and_last_only": (np.array([0, 6, 6, 0, 6]), 7),
        "descending": (np.arange(50)[::-1].copy(), 50),
        "no_points": (np.zeros(0, np.int64), 9),
        "one_entry_one_point": (np.zeros(1, np.int64), 1),
    }


@pytest.mark.parametrize("name", list(_layout_cases()))
def test_the_mirrors_layout_is_grid_block_layout(dump, tmp_path, name):
    entry, entries = _layout_cases()[name]
    n = len(entry)
    xyz = np.random.default_rng(7).uniform(-100, 100, (n, 3)).astype(np.float32)
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(np.array([n, entries], np.uint64).tobytes() + entry.astype(np.uint32).tobytes() + xyz.tobytes())
    run = subprocess.run([dump, fin, fout], capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout + run.stderr
    raw = open(fout, "rb").read()
    n_blk = int(np.frombuffer(raw, np.uint64, 1)[0])
    start = np.frombuffer(raw, np.uint32, entries + 4, 8)
    blocks = np.frombuffer(raw, np.float32, 12 * n_blk, 8 + 4 * (entries + 4)).reshape(n_blk, 3, 4)
    slot_point = np.frombuffer(raw, np.uint32, 4 * n_blk, 8 + 4 * (entries + 4) + 48 * n_blk)
    ms, mb, mi = grid_ref.layout(xyz, entry, entries)
    assert len(mb) == n_blk and np.array_equal(ms, start) and np.array_equal(mi, slot_point)
    assert np.array_equal(mb.view(np.uint32), blocks.view(np.uint32))
    # and the properties themselves: block 0 and every unused slot padded, every point once, input order inside an entry
    assert (blocks[0] == grid_ref.PAD_COORD).all() and (slot_point[:4] == grid_ref.PAD_POINT).all()
    used = slot_point != grid_ref.PAD_POINT
    assert sorted(slot_point[used].tolist()) == list(range(n))
    assert (blocks.transpose(0, 2, 1).reshape(-1, 3)[~used] == grid_ref.PAD_COORD).all()
    assert (start[entries:] == n_blk).all()
    for e in range(entries):
        pts = slot_point[4 * start[e]:4 * start[e + 1]]
        pts = pts[pts != grid_ref.PAD_POINT]
        assert pts.tolist() == np.flatnonzero(entry == e).tolist()


# ---------------------------------------------------------------- the mirror's cells, box, entries and tiles by hand
def test_cell_of_at_the_faces():
    f32 = np.float32
    cases = {0.0: 0, -0.0: 0, 0.5: 1, -0.5: -2, 0.4999999: 0, -0.4999999: -1, 1.0: 2, -1.0: -3, 1.5: 3, -1.5: -4, 0.999: 1, -0.999: -2,
             2.0: 4, -2.0: -5, 2.25: 4, -2.25: -5, 2.5: 5, -2.5: -6, 2.75: 5, -2.75: -6}
    for t, want in cases.items():
        assert int(grid_ref.cell_of(f32(t), 1.0)) == want, (t, want)
    # the float32 neighbours of a half-voxel face: the face itself belongs to the cell away from zero
    for face, below, at in ((0.5, 0, 1), (1.0, 1, 2), (1.5, 2, 3), (7.5, 14, 15)):
        lo, hi = np.nextafter(f32(face), f32(0)), np.nextafter(f32(face), f32(100))
        assert [int(grid_ref.cell_of(v, 1.0)) for v in (lo, f32(face), hi)] == [below, at, at]
        assert [int(grid_ref.cell_of(-v, 1.0)) for v in (lo, f32(face), hi)] == [-below - 1, -at - 1, -at - 1]
    # another voxel size: the quotient is taken in float64 from the float32 value
    assert int(grid_ref.cell_of(f32(0.15), 0.3)) == (1 if float(f32(0.15)) / 0.3 >= 0.5 else 0)
    assert grid_ref.cell_of(np.array([0.3, 0.6, -0.3], f32), 0.3).tolist() == [
        2 * int(float(f32(0.3)) / 0.3) + (float(f32(0.3)) / 0.3 % 1 >= 0.5), 2 * int(float(f32(0.6)) / 0.3) + (float(f32(0.6)) / 0.3 % 1 >= 0.5),
        -3 if float(f32(0.3)) / 0.3 >= 1.0 else -2]


def test_box_entries_and_tiles_on_a_hand_made_cloud():
    # cells (0,0,0) (1,0,0) (9,0,3) and (0,17,1): box lo = -2, dim = (14, 22, 8)
    xyz = np.array([[0.1, 0.1, 0.1], [0.6, 0.2, 0.3], [4.6, 0.1, 1.6], [0.2, 8.6, 0.7]], np.float32)
    cells = grid_ref.cell_of(xyz, 1.0)
    assert cells.tolist() == [[0, 0, 0], [1, 0, 0], [9, 0, 3], [0, 17, 1]]
    lo, dim = grid_ref.box(cells)
    assert lo.tolist() == [-2, -2, -2] and dim.tolist() == [14, 22, 8]
    assert grid_ref.dense_entry(cells, lo, dim).tolist() == [(2 * 22 + 2) * 8 + 2, (3 * 22 + 2) * 8 + 2, (11 * 22 + 2) * 8 + 5, (2 * 22 + 19) * 8 + 3]
    tiles, entries, tnx, tny = grid_ref.tile_table(cells, lo, dim)
    assert (tnx, tny) == (2, 3) and len(tiles) == 6
    # box-relative cells (2,2,2) (3,2,2) -> tile 0 (z 2..2); (11,2,5) -> tile 3 (z 5); (2,19,3) -> tile 2 (z 3): each owns 64 * 2 entries
    assert tiles.tolist() == [[64, 2 | 1 << 16], [0, 0], [192, 3 | 1 << 16], [320, 5 | 1 << 16], [0, 0], [0, 0]] and entries == 448
    assert grid_ref.tiled_entry(cells, lo, tiles, tny).tolist() == [64 + (2 * 8 + 2) * 2, 64 + (3 * 8 + 2) * 2, 320 + (3 * 8 + 2) * 2, 192 + (2 * 8 + 3) * 2]
    g = grid_ref.grid(xyz, 1.0, True)
    assert (g["start"][:64] == 0).all() and g["desc"]["gnx"] == 16 and g["desc"]["gny"] == 24 and g["desc"]["n_start_words"] == 452
    d = grid_ref.grid(xyz, 1.0, False)["desc"]
    assert (d["vx0"], d["vy0"], d["vz0"], d["vnx"], d["vny"], d["vnz"]) == (-1, -1, -1, 7, 11, 4) and d["n_blocks"] == 5


# ---------------------------------------------------------------- header, arguments, shim
def test_the_symbols_and_values_are_in_the_header(L):
    raw = open(os.path.join(ROOT, "include", "elimaloc_hip.h")).read()
    src = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+ELM_INDEX_BUILD_HOST\s+0\b", src) and re.search(r"#define\s+ELM_INDEX_BUILD_DEVICE\s+1\b", src)
    assert re.search(r"int\s+elm_map_set_index_build\s*\(\s*elm_map\*\s*map,\s*int where\)", src)
    assert re.search(r"int\s+elm_map_download_cell_grid\s*\(\s*const elm_map\*\s*map,\s*elm_cell_grid_desc\*\s*desc,\s*uint32_t\*\s*start,\s*size_t start_cap,"
                     r"\s*float\*\s*blocks12,\s*size_t block_cap,\s*uint32_t\*\s*slot_point,\s*size_t slot_cap,\s*uint32_t\*\s*tiles2,\s*size_t tile_cap\)", src)
    assert "bit 9" in raw and "device index build" in raw
    from elimaloc_amd import _lib
    assert (_lib.INDEX_BUILD_HOST, _lib.INDEX_BUILD_DEVICE) == (0, 1)
    for s in ("elm_map_set_index_build", "elm_map_download_cell_grid", "elm_map_index_build_stages"):
        assert hasattr(L, s) and s in _lib.EXPORTS
    # the descriptor as the header declares it: 15 int32, one uint32, three uint64
    body = re.search(r"typedef struct elm_cell_grid_desc \{(.*?)\} elm_cell_grid_desc;", src, flags=re.S).group(1)
    names = [n.strip() for line in body.split(";") for n in re.sub(r"^\s*\w+\s", "", line.strip()).split(",") if n.strip()]
    assert names == [n for n, _ in _lib.CellGridDesc._fields_] and C.sizeof(_lib.CellGridDesc) == 16 * 4 + 3 * 8


def test_argument_errors_without_a_device(L):
    from elimaloc_amd import _lib
    assert L.elm_map_set_index_build(None, 0) == INVALID and L.elm_map_set_index_build(None, 1) == INVALID
    d = _lib.CellGridDesc()
    assert L.elm_map_download_cell_grid(None, C.byref(d), None, 0, None, 0, None, 0, None, 0) == INVALID
    ms = (C.c_double * _lib.INDEX_STAGES)()
    assert L.elm_map_index_build_stages(None, ms) == INVALID


def test_shim_index_call_lines_compile_and_link(L, tmp_path):
    """tests/shim_harness/index_calls.cpp, built as tests/test_map_build_device_abi.py builds build_calls.cpp"""
    exe = tmp_path / "index_calls"
    libdir = os.path.join(ROOT, "elimaloc_amd")
    for std in ("c++14", "c++17"):
        subprocess.check_call(["g++", "-std=" + std, "-Wall", "-Wextra", "-Werror", "-I", os.path.join(ROOT, "tests", "fake_eigen"),
                               "-I", os.path.join(ROOT, "include", "elimaloc"), "-I", os.path.join(ROOT, "include"),
                               os.path.join(ROOT, "tests", "shim_harness", "index_calls.cpp"), "-L", libdir, "-lelimaloc_hip",
                               "-Wl,-rpath," + libdir, "-o", str(exe)])
        assert subprocess.run([str(exe)]).returncode == 0
