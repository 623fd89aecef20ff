"""The host side of the search indices -- which index a map gets on each form, its byte accounting, the order of the points inside a
cell (it decides every tie) -- must not move when the index builders are rearranged.  Every (map, index form) of
tests/index_form_cases.py is compared, exactly, with tests/golden/index_forms_parent.npz: the same calls recorded on the library of the
parent commit (tools/record_index_golden.py; the hash is in the fixture).  Compared: the map's info once the index is built and after
every call, the (source index, target index) pairs of GetCorrespondencePoints / GetCorrespondencesCov / GetCorrespondencesAllCov on
about 2000 seeded queries, and one traced registration each for P2P, GICP, VGICP and AVGICP, as bit patterns."""
import os

import numpy as np
import pytest

import index_form_cases as ic

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_forms_parent.npz")
CALLS = ("GetCorrespondencePoints", "GetCorrespondencesCov", "GetCorrespondencesAllCov")


# ---- CPU: the inputs are what they claim ------------------------------------------------------------------------------------------------
def test_straddle_map_has_the_tiles_it_claims():
    """Several tiles in x and y, negative and positive coordinates, an empty tile with occupied tiles on both sides in x and in y, tiles of
    one and of several layers of cells."""
    pts = ic.straddle_map()
    assert 2900 <= len(pts) <= 3100 and (pts.min(axis=0) < -1.0).all() and (pts.max(axis=0) > 1.0).all()
    tiles = ic.tiles_of(pts)
    xs, ys = {t[0] for t in tiles}, {t[1] for t in tiles}
    assert len(xs) >= 3 and len(ys) >= 3
    empty = [(x, y) for x in xs for y in ys if (x, y) not in tiles]
    assert any({(x - 1, y), (x + 1, y), (x, y - 1), (x, y + 1)} <= set(tiles) for x, y in empty), (empty, sorted(tiles))
    layers = [hi - lo + 1 for lo, hi in tiles.values()]
    assert min(layers) == 1 and max(layers) >= 4, layers


def test_query_sets_hold_exact_ties():
    """The straddle map's queries: a few hundred with two map points at exactly the same, smallest, distance."""
    assert len(ic.queries("straddle")) == ic.N_QUERY
    assert ic.exact_ties("straddle") >= 100


def test_small_maps_are_what_they_claim():
    assert len(ic.single_map()) == 1
    c = ic.crowded_map()
    keys = np.unique(np.floor(c).astype(int), axis=0)
    assert len(keys) == 27 and len(c) == 27 * 64 and 27 * ic.MAP_MAX_POINTS["crowded"] > 1024
    s = ic.sheet_map()
    _, counts = np.unique(np.floor(s[:, :2]).astype(int), axis=0, return_counts=True)
    assert set(counts) == {2, 3} and len(s) <= 300


# ---- GPU: every map on every index form, against the parent -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def golden():
    with np.load(GOLDEN) as z:
        return {k: z[k] for k in z.files}


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(ic.FORMS))
@pytest.mark.parametrize("name", ic.MAPS)
def test_index_form_matches_parent(golden, name, form):
    rec = ic.run_case(name, form)
    want_fields = {k.split("/", 3)[3] for k in golden if k.startswith(f"case/{name}/{form}/")}
    assert want_fields == set(rec), (sorted(want_fields ^ set(rec)))
    print(f"{name} {form}: info {dict(zip(('flags', 'dev', 'n_query', 'entries', 'index', 'p0', 'p1', 'p2', 'p3', 'n_list'), rec['info_end'].tolist()))}")
    for field in ("info_index", "info_end") + tuple(f"{c}/{w}" for c in CALLS for w in ("src", "tgt")) + \
            tuple(f"{m}/{f}" for m, _ in ic.METHODS for f in ic.FIELDS):
        want, got = golden["blob/" + str(golden[f"case/{name}/{form}/{field}"])], rec[field]
        assert got.shape == want.shape and got.dtype == want.dtype, (name, form, field, got.shape, want.shape)
        assert np.array_equal(_bits(got), _bits(want)), (name, form, field, got, want)
