"""The hand-built relocalization cases (tests/reloc_cases.py) must bite: conditions on the INPUTS, checked on the CPU with the numpy mirror
(tests/reloc_ref.py) alone.  The mirror's bound is admissible on every node of every case, its search returns what exhaustive scoring
returns, no case prunes nothing, every rule of the bound is taken (in the case built for it and often enough over the set), and the
points of the score cases sit exactly on the edge they are named after.  tests/test_reloc_edges.py then holds the kernels to the mirror."""
import numpy as np
import pytest

import reloc_cases as rc
import reloc_ref as rr


def _tag_counts(name):
    """per rule tag, the number of (node, point) pairs of the case's levels 1 .. top that took it"""
    m = rc.mirror(name)
    hist = np.zeros(256, np.int64)
    for l in range(1, m.top + 1):
        hist += np.bincount(m.bounds(l, m.all_nodes(l))[1].ravel(), minlength=256)
    return {t: int(sum(hist[v] for v in range(256) if v & bit)) for t, bit in rr.TAGS.items()}


@pytest.mark.parametrize("name", rc.GLOBAL_NAMES)
def test_global_case_bites(name):
    c, m, st = rc.global_case(name), rc.mirror(name), rc.searched(name)
    assert m.nS <= 300 and 100 <= len(c.map) <= 5000 and m.K * m.NX * m.NY <= 80_000 and (m.K, m.NX, m.NY) == c.dims
    assert np.array_equal(c.map.astype(np.float64).astype(np.float32), c.map) and c.scan.dtype == np.float32
    # admissible: no node's bound is below the best leaf under it
    for l in range(1, m.top + 1):
        nodes = m.all_nodes(l)
        b, _ = m.bounds(l, nodes)
        lm = m.leaf_max(l)[nodes[:, 0], nodes[:, 1], nodes[:, 2]]
        assert lm.min() >= 0 and np.all(b >= lm), (l, nodes[b < lm][:5])
    # the search is the exhaustive answer
    assert st.kept == m.exhaustive() and len(st.kept) > 0
    assert [h for h, _ in st.leaves] == sorted((h for h, _ in st.leaves), key=lambda h: (-dict(st.leaves)[h], h))
    # not vacuous
    assert st.tau >= 1, st
    strict = [st.nodes_kept[l] < st.nodes_bounded[l] for l in range(1, m.top + 1)]
    assert any(strict) and (name not in rc.MULTI_LEVEL or all(strict)), (st.nodes_kept, st.nodes_bounded)
    assert st.point_evals == m.nS * (sum(st.nodes_bounded) + st.leaves_scored)
    # the rules this case is built for
    tc = _tag_counts(name)
    assert all(tc[t] >= 1 for t in c.targets), (c.targets, tc)


def test_every_rule_is_taken():
    total = {t: 0 for t in rr.TAGS}
    for name in rc.GLOBAL_NAMES:
        for t, n in _tag_counts(name).items():
            total[t] += n
    assert all(n >= 8 for n in total.values()), total
    assert {t for name in rc.GLOBAL_NAMES for t in rc.global_case(name).targets} == set(rr.TAGS)


def test_a_threshold_tie_decides_somewhere():
    """in at least one case a leaf with score >= tau lies under a node whose bound equals tau exactly: `bound >= tau` keeps it, `>` would not"""
    assert any(rc.searched(name).tau_bound_leaf for name in rc.GLOBAL_NAMES)


def test_levels_and_lattice_shapes():
    tops = {name: rc.mirror(name).top for name in rc.GLOBAL_NAMES}
    assert tops["top2_33x33"] == 2 and tops["top3_33x33"] == 3 and tops["width_w2_eq_w1"] == 2
    assert all(t == 1 for n, t in tops.items() if n not in rc.MULTI_LEVEL)
    assert rc.mirror("nx1_line").NX == 1 and rc.global_case("top1_k4_9x7").dims == (4, 9, 7)
    m = rc.mirror("top2_33x33")  # holes: invalid leaves, and whole level-1 nodes without a valid leaf
    assert 0 < m.valid.sum() < m.valid.size and np.any(m.zmin[1] > m.zmax[1])
    ragged = [n for n in rc.GLOBAL_NAMES if rc.mirror(n).NX & (rc.mirror(n).NX - 1) or rc.mirror(n).NY & (rc.mirror(n).NY - 1)]
    assert len(ragged) >= 10


def _keys_wide(name):
    """the set of x and of y key-range widths (in keys) that the pairs of the case's level-1 nodes and points take, per yaw"""
    m = rc.mirror(name)
    nodes = m.all_nodes(1)
    kx0, kx1, ky0, ky1, _, _ = m.key_ranges(1, nodes)
    return m.w[1], {(int(k), ax, int(v)) for ax, d in (("x", kx1 - kx0 + 1), ("y", ky1 - ky0 + 1)) for k in range(m.K)
                    for v in np.unique(d[nodes[:, 0] == k])}


def test_window_widths():
    assert rc.mirror("width_05_05").w == [1, 3] and rc.mirror("width_025_05").w == [1, 2] and rc.mirror("width_075_05").w == [1, 3]
    assert rc.mirror("width_w2_eq_w1").w == [1, 2, 2] and rc.mirror("width_vs03").w == [1, 3] and rc.mirror("width_floor_under").w == [1, 4]
    assert rc.mirror("top3_33x33").w == [1, 3, 5, 9]
    # key ranges exactly w - 1 and exactly w keys wide, on x and on y, under each of the four quarter-turn yaws
    for name in ("width_025_05", "width_075_05", "width_vs03"):
        w, got = _keys_wide(name)
        assert all((k, ax, v) in got for k in range(4) for ax in "xy" for v in (w - 1, w)), (name, w, sorted(got))
        assert max(v for _, _, v in got) == w
    # an exact-integer ratio (0.5 / 0.5): w - 1 keys everywhere; the window's last key is used only where the rounding of a + t (the
    # 6e-17 entries of a quarter turn's cos) puts the low end just below a key face
    w, got = _keys_wide("width_05_05")
    assert max(v for _, _, v in got) <= w and all((k, ax, w - 1) in got for k in range(4) for ax in "xy")
    # the floor of 0.6 / 0.2 is 2, not 3: ranges of w + 1 keys exist, which only the wide rule keeps in the bound
    w, got = _keys_wide("width_floor_under")
    assert max(v for _, _, v in got) == w + 1 and _tag_counts("width_floor_under")["wide"] >= 8


def test_z_words_and_cap():
    m = rc.mirror("zwords_cap64")
    assert list(m.dims)[2] == 128 and m.vox[:, 2].max() - m.k0[2] == 127
    col = m.vox[(m.vox[:, 0] == -4) & (m.vox[:, 1] == 20)][:, 2] - m.k0[2]  # the structure column at (-1.125, 5.125)
    assert {0, 31, 32, 63, 64, 127} <= set(col.tolist())
    nodes = m.all_nodes(1)
    _, _, _, _, kz0, kz1 = m.key_ranges(1, nodes)
    _, tags = m.bounds(1, nodes)
    look = (tags & (rr.W1 | rr.W2 | rr.W3)) != 0
    c0, c1 = kz0 - m.k0[2], kz1 - m.k0[2]
    for seam in (31, 63):
        assert np.any(look & (c0 < seam) & (c1 == seam)), seam        # the range ends exactly on the word's last bit
        assert np.any(look & (c0 == seam + 1) & (c1 > seam + 1)), seam  # ... starts exactly on the next word's first bit
        assert np.any(look & (c0 <= seam) & (c1 > seam)), seam        # ... straddles the seam
    assert np.any(look & (c0 < 31) & (c1 > 63))  # three words
    # the cap flips between adjacent cases: the same world, different nodes kept
    span = c1.clip(None, 127) - c0.clip(0, None)
    for lo, hi in ((1, 1), (2, 32), (33, 63)):  # the spans that count under the smaller cap and are looked up under the larger
        assert np.any((span >= lo) & (span <= hi)), (lo, hi)
    kept = [rc.searched(f"zwords_cap{cap}").nodes_kept for cap in (1, 2, 33, 64)]
    assert len({tuple(k) for k in kept}) == 4, kept


def test_box_edges_and_origin():
    m, c = rc.mirror("box_overhang"), rc.global_case("box_overhang")
    lo, hi = m.k0, m.k0 + m.dims - 1
    assert c.cfg.x_min / c.vs < lo[0] and c.cfg.x_max / c.vs > hi[0] and c.cfg.y_min / c.vs < lo[1] and c.cfg.y_max / c.vs > hi[1]
    have = {tuple(k) for k in m.vox.tolist()}
    zs = (lo[2], m.vox[:, 2].max())
    assert all((x, y, z) in have for x in (lo[0], hi[0]) for y in (lo[1], hi[1]) for z in zs)
    # leaves whose points leave the map's key box: the leaf score's probe fallback inside the bitmap form
    k = rr.pose_keys(m.S, m.H[m.valid_flat][::7], m.vs)
    assert np.any((k < lo) | (k > hi))
    assert rc.mirror("thin_y").dims[1] == 2
    o = rc.mirror("origin_band")
    assert o.k0[0] < 0 < (o.k0 + o.dims)[0] and o.k0[1] < 0 and o.k0[2] < 0 and o.xs[0] < 0 < o.xs[-1] and o.ys[0] < 0 < o.ys[-1]
    k = rr.pose_keys(o.S, o.H[o.valid_flat], o.vs)
    for ax in range(3):
        assert {-1, 0, 1} <= set(np.unique(k[..., ax]).tolist())
    assert o.gz.min() < 0.0 < o.gz.max() + 2.0


def test_pruning_pressure():
    pools = {int(rc.global_case(n).cfg.pool_min) for n in rc.GLOBAL_NAMES}
    assert {1, 4, 64} <= pools
    st = rc.searched("pool_64_topk_1024")
    assert len(st.kept) == 1024 and st.kept == st.leaves[:1024]  # no NMS: the output is the prefix of the exhaustive order
    assert rc.searched("nms_wide_passes").passes >= 2 and rc.searched("pool_1").passes >= 2


# ---------------------------------------------------------------------------------------------------------------- score cases
def _moved(scan, i, ax, up):
    s = scan.copy()
    s[i, ax] = np.nextafter(s[i, ax], np.float32(np.inf if up else -np.inf))
    return s


@pytest.mark.parametrize("name", [n for n in rc.SCORE_NAMES if not n.startswith("blocks") and n != "tight_box"])
def test_score_case_sits_on_its_edge(name):
    """moving a targeted point by one float32 ulp across its face (or across the r_max sphere) changes the mirror's scores"""
    c, ref = rc.score_case(name), rc.score_ref(name)
    assert len(c.edge_points) >= 5 and ref.max() > 0
    axes = []
    for i in c.edge_points:
        moves = [rr.mirror_scores(c.map, c.vs, _moved(c.scan, i, ax, up), c.poses, c.r_max) for ax in range(3) for up in (False, True)]
        changed = [not np.array_equal(mv, ref) for mv in moves]
        assert any(changed), (name, i, c.scan[i])
        axes += [changed[2 * ax] or changed[2 * ax + 1] for ax in range(3) if c.scan[i, ax] != 0.0]
    if name.startswith("faces") and c.vs != 0.3:
        # every non-zero coordinate is on a face (0 lies inside the wide key 0): a move along it changes a key, and the score unless the
        # voxel behind the face happens to be occupied as well
        assert np.mean(axes) >= 0.9, np.mean(axes)


def test_band_reads_the_wide_key_zero():
    c = rc.score_case("band_vs0.5")
    k = rr.pose_keys(c.scan, c.poses, c.vs)
    assert set(np.unique(k[0]).tolist()) == {-1, 0, 1} and set(np.unique(k).tolist()) == {-2, -1, 0, 1, 2}
    q = c.scan.astype(np.float64)
    assert np.any((q > -0.5) & (q < 0.0)) and np.any((q > 0.0) & (q < 0.5)) and np.any(q == 0.5) and np.any(q == -0.5)


def test_tight_box_margin():
    c = rc.score_case("tight_box")
    S = rr.in_range(c.scan, c.r_max)
    k0, d = rr.score_box(S, c.poses, c.vs)
    assert int(np.prod(d)) % 64 != 0 and int(np.prod(d)) % 256 != 0
    hi = k0 + d - 1
    have = {tuple(k) for k in rr.voxel_keys(c.map, c.vs).tolist()}
    for k in c.margin:  # occupied, inside the box, on its outermost layer, read by no point
        assert tuple(k) in have and np.all(np.array(k) >= k0) and np.all(np.array(k) <= hi) and (np.any(np.array(k) == k0) or np.any(np.array(k) == hi))
    for k in c.outside:  # occupied, outside the box
        assert tuple(k) in have and (np.any(np.array(k) < k0) or np.any(np.array(k) > hi))
    assert sum(1 for k in c.outside if np.all(np.array(k) >= k0 - 1) and np.all(np.array(k) <= hi + 1)) >= 6  # exactly one key outside
    keys = rr.pose_keys(S, c.poses, c.vs)
    read = {tuple(k) for k in keys.reshape(-1, 3).tolist()}
    assert not read & {tuple(k) for k in c.margin + c.outside}
    # the scan's outermost keys are occupied and read: the layer next to the margin
    assert np.any(keys[0, :, 0] == k0[0] + 1) and (int(k0[0]) + 1 in {k[0] for k in have & read})
    # The box is the union over the whole pose set, margin included, so under ScorePoses no counted point can leave it: the probe
    # fallback inside the bitmap forms is reached from the global search's leaf scores (test_box_edges_and_origin), not from here
    assert np.all(keys >= k0 + 1) and np.all(keys <= hi - 1)


@pytest.mark.parametrize("n", rc.N_COUNTED)
def test_block_cases_count(n):
    for p in rc.N_POSES:
        c, ref = rc.score_case(f"blocks_n{n}_p{p}"), rc.score_ref(f"blocks_n{n}_p{p}")
        assert rr.in_range(c.scan, c.r_max).shape[0] == n == c.n_counted and c.scan.shape[0] == n + 3 and len(c.poses) == p
        assert ref[0] == n and ref[-1] == n  # every counted point reads a voxel under the first and the last pose
