"""Place recognition on the GPU (elm_places_*): every descriptor word and stats field, every (query, entry) match
and every selection against the numpy mirror of the contract (tests/places_ref.py), in bytes; the capacity and misuse; and the loop of
tests/places_cases.py: the candidates of the committed fixture, and LoopCloser.Verify against the hand composition of the public calls
it is made of."""
import math

import numpy as np
import pytest

import places_cases as cases
import places_ref as ref
from elimaloc_amd import synth
from elimaloc_amd._lib import ElmError
from elimaloc_amd.places import LoopCloser, PlaceConfig, PlaceDatabase
from elimaloc_amd.registration import Context, IcpMethod, Registration, RegistrationConfig, Scan, VoxelHashMap

pytestmark = pytest.mark.gpu

CONFIGS = {"1x1": dict(n_rings=1, n_layers=1), "16x8": dict(), "32x16": dict(n_rings=32, n_layers=16)}


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def _db(ctx, name="16x8", capacity=300):
    kw = CONFIGS[name]
    return PlaceDatabase(PlaceConfig(**kw), capacity, ctx), ref.Cfg(**kw)


def _mirror(scans, levels, cfg, dirs):
    out = [ref.describe(s, cfg, dirs, None if levels is None else levels[j]) for j, s in enumerate(scans)]
    return np.stack([w for w, _ in out]), [st for _, st in out]


def _check_describe(db, cfg, scans, levels=None):
    dirs = db.Tables()[2]
    want_w, want_st = _mirror(scans, levels, cfg, dirs)
    words, st = db.Describe(list(scans), levels)
    assert words.tobytes() == want_w.tobytes() and st == want_st
    return words, st


# ---------------------------------------------------------------- describe
@pytest.mark.parametrize("name", list(CONFIGS))
def test_describe_sizes_jobs_and_levels(ctx, name):
    db, cfg = _db(ctx, name)
    scans = [cases.random_scan(n, 100 + n) for n in (0, 1, 255, 256, 257, 1025)]
    for s in scans:  # one job each
        _check_describe(db, cfg, [s])
    empty = scans[0]
    _check_describe(db, cfg, [empty, scans[5]])  # a zero-point job first, in the middle, last
    _check_describe(db, cfg, [scans[4], empty, scans[2], empty, scans[3]])
    _check_describe(db, cfg, [scans[3], scans[1], scans[5], scans[2], empty])
    resident = Scan(ctx, scans[5])
    words, st = db.Describe([resident, resident])  # one scan twice
    assert words[0].tobytes() == words[1].tobytes() == ref.describe(scans[5], cfg, db.Tables()[2])[0].tobytes() and st[0] == st[1]
    levels = np.stack([np.eye(4), cases.tilted_level(), cases.far_level(), cases.tilted_level(-3.0, 2.5, -0.7), np.eye(4)])
    words, st = _check_describe(db, cfg, [scans[5], scans[5], scans[5], scans[4], scans[2]], levels)
    assert st[2] == dict(n_points=1025, n_used=0, n_bits=0) and not words[2].any()  # carried 1e5 m away: every point is dropped
    assert st[0]["n_used"] > 300 and st[1]["n_used"] > 300
    assert name == "1x1" or words[0].tobytes() != words[1].tobytes()  # (one word of 64 sectors is full either way)
    assert db.Size() == 0  # Describe leaves the database alone


def test_describe_boundary_family(ctx):
    for name in ("16x8", "32x16"):
        db, cfg = _db(ctx, name)
        re, ze, dirs = db.Tables()
        sectors = cases.sector_boundary_points(dirs)
        edges = cases.edge_points(cfg, re, ze)
        assert len(sectors) == 64 * 2 * 9
        words, st = _check_describe(db, cfg, [sectors, edges, np.concatenate([edges, sectors])])
        assert st[0]["n_used"] == len(sectors)  # every boundary point has a sector, a ring and a layer
        assert 0 < st[1]["n_used"] < len(edges)  # below the first and at the last edge there is no ring / layer
        # the same points one per job: a bit per point, where the family stands on its bits
        for p in sectors[::37]:
            w, s = db.Describe(p[None])
            assert w.tobytes() == ref.describe(p[None], cfg, dirs)[0].tobytes() and s["n_bits"] == 1


def test_describe_all_dropped_and_quarter_turn(ctx):
    db, cfg = _db(ctx)
    dirs = db.Tables()[2]
    dropped = np.array([(0, 0, 0), (0, 0, 3), (np.nan, 1, 1), (1, np.nan, 1), (5, 5, np.nan), (1, 1, 0), (100, 0, 0), (10, 0, 50), (np.inf, 0, 0)],
                       np.float32)
    words, st = _check_describe(db, cfg, [dropped])
    assert st[0] == dict(n_points=9, n_used=0, n_bits=0) and not words.any()
    pts = np.concatenate([cases.random_scan(3000, 21), cases.sector_boundary_points(dirs)])
    turned = np.ascontiguousarray(np.stack([-pts[:, 1], pts[:, 0], pts[:, 2]], axis=1))
    words, st = _check_describe(db, cfg, [pts, turned])
    assert st[0] == st[1] and words[1].tobytes() == ref.rotl(words[0], 16).tobytes()


def test_describe_repeats_and_add_download(ctx):
    db, cfg = _db(ctx, capacity=8)
    scans = [cases.random_scan(n, 300 + n) for n in (1025, 0, 257, 4096)]
    levels = np.stack([cases.tilted_level(), np.eye(4), np.eye(4), cases.tilted_level(0.5, 0.5, 2.0)])
    words, st = _check_describe(db, cfg, scans, levels)
    for _ in range(4):  # five byte-identical runs
        w2, s2 = db.Describe(scans, levels)
        assert w2.tobytes() == words.tobytes() and s2 == st
    ids = np.array([7, -3, 1 << 40, 0], np.int64)
    assert db.Add(scans, levels, ids) == st and db.Size() == 4
    w, i, b = db.Download()
    assert w.tobytes() == words.tobytes() and i.tolist() == ids.tolist() and b.tolist() == [s["n_bits"] for s in st]
    assert db.Add(scans[2], None, ids=[99]) == ref.describe(scans[2], cfg, db.Tables()[2])[1]  # a second add appends
    w, i, b = db.Download(3, 2)
    assert w[0].tobytes() == words[3].tobytes() and w[1].tobytes() == ref.describe(scans[2], cfg, db.Tables()[2])[0].tobytes() and i.tolist() == [0, 99]
    # the query on scans is the match on their descriptors
    got = db.Query(scans[:3], levels[:3], top_k=16, matches=True)
    want = db.Match(words[:3], top_k=16, matches=True)
    assert got[0] == want[0] and got[1].tobytes() == want[1].tobytes()
    assert got[0][0][0]["entry"] == 0 and got[0][0][0]["dice_q16"] == 65536 and got[0][2][0]["entry"] == 2  # (entry 4 repeats entry 2: the smaller first)


# ---------------------------------------------------------------- match
def _entries(W, seed):
    """257 entries: random at densities 1 %, 20 % and 100 %, an all-zero one, and duplicates"""
    parts = [cases.random_words(100, W, 0.01, seed), cases.random_words(100, W, 0.2, seed + 1), cases.random_words(2, W, 1.0, seed + 2),
             np.zeros((1, W), np.uint64), cases.random_words(54, W, 0.5, seed + 3)]
    e = np.concatenate(parts)
    e[250], e[256], e[3] = e[120], e[120], e[5]
    return np.ascontiguousarray(e)


def _check_match(db, queries, entries_words, ids, mirror, **kw):
    got, m = db.Match(queries, matches=True, **kw)
    n = len(entries_words)
    assert m.shape == (len(queries), n) and m.tobytes() == np.ascontiguousarray(mirror[:, :n]).tobytes()
    ex = kw.get("exclude_ids")
    want = [ref.select(mirror[q, :n], ids[:n], kw.get("top_k", 1), kw.get("min_dice_q16", 0), ex) for q in range(len(queries))]
    assert got == want
    return got


@pytest.mark.parametrize("name", list(CONFIGS))
def test_match_against_the_mirror(ctx, name):
    db, cfg = _db(ctx, name)
    W = cfg.n_words
    entries = _entries(W, 40 + W)
    ids = (np.arange(257, dtype=np.int64) * 3) - 100
    queries = np.ascontiguousarray(np.stack([entries[120], cases.random_words(1, W, 0.2, 7)[0], ref.rotl(entries[150], 37)]))
    mirror = ref.match_all(queries, entries)
    for n in (0, 1, 3, 4, 5, 257):  # four pairs per workgroup: 3 / 4 / 5 is the seam
        db.Reset()
        db.AddDescriptors(entries[:n], ids[:n])
        assert db.Size() == n
        for q in (queries, queries[:1]):
            for top_k in (1, 16):  # (16 is above n for the small databases)
                got = _check_match(db, q, entries[:n], ids, mirror[:len(q)], top_k=top_k)
                assert all(len(c) == min(top_k, n) for c in got)
    # with all 257: the duplicate entries 120, 250 and 256 tie at the top of query 0, the smaller index first; the rotated query finds its turn
    got = _check_match(db, queries, entries, ids, mirror, top_k=5)
    assert [c["entry"] for c in got[0][:3]] == [120, 250, 256] and all(c["dice_q16"] == 65536 and c["shift"] == 0 for c in got[0][:3])
    if W > 1:
        assert got[2][0]["entry"] == 150 and got[2][0]["shift"] == 37 and got[2][0]["dice_q16"] == 65536
    # the threshold at a realised dice and one above it
    d = got[1][2]["dice_q16"]
    at = _check_match(db, queries, entries, ids, mirror, top_k=16, min_dice_q16=d)
    above = _check_match(db, queries, entries, ids, mirror, top_k=16, min_dice_q16=d + 1)
    assert all(c["dice_q16"] >= d for c in at[1]) and all(c["dice_q16"] > d for c in above[1]) and len(at[1]) >= 3
    assert _check_match(db, queries, entries, ids, mirror, top_k=16, min_dice_q16=65537) == [[], [], []]
    # the closed id range around entry 120 (id 260): at lo, at hi, and one either side of each
    for lo, hi in ((260, 260), (261, 300), (200, 259), (257, 263), (260, 650), (650, 668), (669, 700), (668, 668), (300, 200), (-1000, 1000)):
        got = _check_match(db, queries, entries, ids, mirror, top_k=3, exclude_ids=(lo, hi))
        assert (120 in [c["entry"] for c in got[0]]) == (not (lo <= 260 <= hi))
        assert (256 in [c["entry"] for c in got[0]]) == (not (lo <= 668 <= hi))
    # one range per query
    per = db.Match(queries, top_k=2, exclude_ids=np.array([[260, 260], [0, -1], [350, 350]]))
    assert per == [ref.select(mirror[q], ids, 2, 0, r) for q, r in enumerate(((260, 260), None, (350, 350)))]


def test_match_every_shift_and_the_special_patterns(ctx):
    db, cfg = _db(ctx)
    W = cfg.n_words
    q = cases.random_words(1, W, 0.2, 99)[0]
    bits = ref.popcount(q)
    # entry k = rotl(query, k): the pair's shift s has rotl(entry, s) = query, s = (64 - k) mod 64
    entries = np.stack([ref.rotl(q, k) for k in range(64)])
    db.AddDescriptors(entries, np.arange(64))
    got, m = db.Match(q, top_k=16, matches=True)
    assert m.tobytes() == ref.match_all(q[None], entries)[0].tobytes()
    assert m["shift"].tolist() == [(64 - k) % 64 for k in range(64)] and (m["inter"] == bits).all() and (m["dice_q16"] == 65536).all()
    assert [c["entry"] for c in got] == list(range(16)) and [c["yaw_rad"] for c in got] == [ref.yaw_of_shift((64 - k) % 64) for k in range(16)]
    # the other way round: query = rotl(entry 0, k) finds shift k
    for k in (0, 1, 31, 32, 33, 63):
        c = db.Match(ref.rotl(q, k), top_k=1, exclude_ids=(1, 63))[0]
        assert (c["entry"], c["shift"], c["inter"], c["dice_q16"], c["yaw_rad"]) == (0, k, bits, 65536, ref.yaw_of_shift(k))
    # all zero on both sides: dice 0 at shift 0, still a candidate under a zero threshold, none under a threshold of 1
    db.Reset()
    db.AddDescriptors(np.zeros((5, W), np.uint64), np.arange(5))
    got, m = db.Match(np.zeros(W, np.uint64), top_k=16, matches=True)
    assert not m["dice_q16"].any() and not m["shift"].any() and [c["entry"] for c in got] == [0, 1, 2, 3, 4]
    assert db.Match(np.zeros(W, np.uint64), top_k=16, min_dice_q16=1) == []
    # a pattern of period 16: inter is the same at k, k + 16, k + 32, k + 48 and the smallest wins
    p = np.full(W, 0x0001000100010001, np.uint64)
    db.Reset()
    db.AddDescriptors(np.stack([p, ref.rotl(p, 5), ref.rotl(p, 59)]), np.arange(3))
    got, m = db.Match(p, top_k=3, matches=True)
    assert m["shift"].tolist() == [0, 11, 5] and (m["dice_q16"] == 65536).all() and m.tobytes() == ref.match_all(p[None], db.Download()[0])[0].tobytes()


def test_match_dice_at_the_64_bit_edge(ctx):
    db, cfg = _db(ctx, "32x16")
    full = np.full(512, ref.M64, np.uint64)
    db.AddDescriptors(full[None], [5])
    c = db.Match(full)[0]
    assert (c["inter"], c["shift"], c["dice_q16"], c["id"]) == (1 << 15, 0, 65536, 5)  # (inter << 17 = 2^32 in 32 bits would be 0)
    assert db.Download()[2].tolist() == [1 << 15]


# ---------------------------------------------------------------- capacity and misuse
def test_capacity_reset_and_misuse(ctx):
    db, cfg = _db(ctx, capacity=4)
    W = cfg.n_words
    words = cases.random_words(6, W, 0.2, 5)
    scans = [Scan(ctx, cases.random_scan(300, 900 + k)) for k in range(3)]
    db.AddDescriptors(words[:3], [1, 2, 3])
    before = db.Download()
    with pytest.raises(ElmError, match=r"\(-5\).*capacity"):  # two more would overfill: refused, nothing changes
        db.Add(scans[:2], None, [4, 5])
    with pytest.raises(ElmError, match=r"\(-5\).*capacity"):
        db.AddDescriptors(words[3:5], [4, 5])
    after = db.Download()
    assert db.Size() == 3 and all(a.tobytes() == b.tobytes() for a, b in zip(before, after))
    db.Add(scans[0], None, [4])  # to capacity
    assert db.Size() == 4
    with pytest.raises(ElmError, match=r"\(-5\)"):
        db.AddDescriptors(words[5:6], [6])
    with pytest.raises(ElmError, match=r"\(-5\)"):
        db.Add(scans[1], None, [6])
    assert db.Size() == 4 and db.Download()[1].tolist() == [1, 2, 3, 4]
    assert db.Match(words[1])[0]["id"] == 2
    db.Reset()
    assert db.Size() == 0 and db.Match(words[1], top_k=16) == [] and db.Query(scans[0], top_k=3) == []  # an empty database: no candidates
    db.AddDescriptors(words[4:6], [8, 9])
    assert db.Download()[1].tolist() == [8, 9] and db.Match(words[5])[0]["id"] == 9
    # misuse, each followed by a correct call
    for bad in (lambda: db.Match(words[0], top_k=0), lambda: db.Match(words[0], top_k=17), lambda: db.Query(scans[0], top_k=17),
                lambda: db.Download(1, 2), lambda: db.Download(3, 0),
                lambda: db.Describe(scans[0], np.full((1, 4, 4), np.nan)), lambda: db.Add(scans[0], np.full((1, 4, 4), np.inf), [1])):
        with pytest.raises(ElmError, match=r"\(-1\)"):
            bad()
        assert db.Match(words[4])[0]["id"] == 8 and db.Size() == 2
    other = Context(0)
    try:
        foreign = Scan(other, cases.random_scan(10, 1))
        odb = PlaceDatabase(PlaceConfig(), 2, other)
        with pytest.raises(ElmError, match=r"\(-1\)"):
            db.Describe([scans[0], foreign])  # a scan of another context
        with pytest.raises(ElmError, match=r"\(-1\)"):
            _ = C_size(other, db)  # an object of another context
        assert odb.Size() == 0 and db.Describe(scans[0])[1]["n_points"] == 300
        odb.close()
        foreign.close()
    finally:
        other.close()
    # a batch in flight: every call that takes ctx is refused, and works again once the batch is finished
    vm = VoxelHashMap(1.0, 30, ctx)
    vm.AddPoints(cases.random_scan(2000, 77, scale=5.0))
    reg = Registration(RegistrationConfig(icp_method=IcpMethod.P2P), ctx)
    reg.EnqueueBatch([scans[1]], vm, [np.eye(4)])
    for bad in (lambda: db.Size(), lambda: db.Reset(), lambda: db.Describe(scans[0]), lambda: db.Add(scans[0], None, [3]),
                lambda: db.AddDescriptors(words[:1], [3]), lambda: db.Download(), lambda: db.Match(words[4]), lambda: db.Query(scans[0]),
                lambda: PlaceDatabase(PlaceConfig(), 4, ctx)):
        with pytest.raises(ElmError, match=r"\(-1\)"):
            bad()
    reg.FinishBatch()
    assert db.Size() == 2 and db.Download()[1].tolist() == [8, 9] and db.Match(words[4])[0]["id"] == 8
    with pytest.raises(ElmError, match=r"\(-1\)"):
        PlaceDatabase(PlaceConfig(r_min_m=50.0), 4, ctx)
    with pytest.raises(ElmError, match=r"\(-1\)"):
        PlaceDatabase(PlaceConfig(), 65537, ctx)
    db.close()
    with pytest.raises(ElmError, match="closed"):
        db.Size()


def C_size(ctx, db):
    import ctypes as C
    from elimaloc_amd import _lib
    n = C.c_size_t(0)
    _lib.check(_lib.lib().elm_places_size(ctx._h, db._h, C.byref(n)), ctx._h, "elm_places_size")
    return n.value


# ---------------------------------------------------------------- the loop
# The submap reaches every kept scan that can overlap the query: two scans of 45 m range overlap up to 90 m apart, and no two entries of
# the 35 m circle are farther apart than 70 m.  Submap() takes entries e - window .. e + window clipped at the ends of the log (it does
# not wrap around), so only a window of 24 gives every revisit all 24 scans, whichever entry it revisits.  The registration is the
# closer's own default (LoopRegConfig: P2P run to a 2 mm step).
WINDOW = 24


@pytest.fixture(scope="module")
def loop(ctx):
    Lp = cases.loop_inputs()
    lc = LoopCloser(PlaceDatabase(PlaceConfig(), 64, ctx), 1.0, 30, window=WINDOW)
    assert (lc.reg.config_.icp_method, lc.reg.config_.max_iteration, lc.reg.config_.icp_termination_threshold_m) == (IcpMethod.P2P, 50, 0.002)
    for e in range(cases.N_ENTRIES):
        entry, _ = lc.Insert(Lp["entry_scans"][e], Lp["entry_poses"][e])
        assert entry == e
    return Lp, lc, [Scan(ctx, s) for s in Lp["revisit_scans"]]


def test_loop_candidates_are_the_fixture(loop):
    Lp, lc, revisits = loop
    gold = np.load(cases.GOLDEN)
    words, ids, _ = lc.places.Download()
    assert words.tobytes() == gold["entry_words"].tobytes() and ids.tolist() == list(range(24))
    for i, sc in enumerate(revisits):
        got = lc.Detect(sc, top_k=3)
        assert [c["entry"] for c in got] == gold["cand_entry"][i].tolist() and [c["dice_q16"] for c in got] == gold["cand_dice"][i].tolist()
        assert [c["inter"] for c in got] == gold["cand_inter"][i].tolist() and [c["shift"] for c in got] == gold["cand_shift"][i].tolist()
        assert got[0]["entry"] == Lp["revisit_entry"][i] and got[0]["id"] == got[0]["entry"]
    got, m = lc.places.Query(revisits, top_k=3, matches=True)
    assert m.tobytes() == gold["matches"].tobytes()
    # the exclusion of the last n ids: with the last 24 excluded nothing is left, with the last 3 entries 21 .. 23 are not answered
    assert lc.Detect(revisits[11], exclude_last=24, top_k=3) == []
    assert [c["entry"] for c in lc.Detect(revisits[11], exclude_last=3, top_k=3)] == [e for e in ref_top(gold, 11) if e < 21][:3]


def ref_top(gold, i):
    row = gold["matches"][i]
    return [c["entry"] for c in ref.select(row, np.arange(24), 24)]


@pytest.fixture(scope="module")
def verified(loop):
    """every revisit's first candidate verified once: (candidate, guess, Verify's result) per revisit"""
    Lp, lc, revisits = loop
    out = []
    for i in range(cases.N_REVISITS):
        cand = lc.Detect(revisits[i])[0]
        out.append((cand, lc.Guess(cand), lc.Verify(revisits[i], cand)))
    return out


def test_loop_verify_is_the_hand_composition_and_succeeds(loop, verified):
    """Verify is the hand composition of the public calls it is made of, in pose bytes, and the registration succeeds for every revisit."""
    Lp, lc, revisits = loop
    for i, (cand, guess, res) in enumerate(verified):
        e = cand["entry"]
        assert e == Lp["revisit_entry"][i] and guess.tobytes() == (Lp["entry_poses"][e] @ _rz(cand["yaw_rad"])).tobytes()
        assert res["is_success"], i
        # by hand, for every revisit
        lo, hi = max(e - WINDOW, 0), min(e + WINDOW, 23)
        assert (lo, hi) == (0, 23)
        m = VoxelHashMap(1.0, 30, lc.ctx, device_build=True).UpdatedFromScans(lc.scans[lo:hi + 1], Lp["entry_poses"][lo:hi + 1])
        T, ok, fit, cov, _ = lc.reg.Relocalize(Lp["revisit_scans"][i], m, guess, lc.reloc, lc.m_config)  # (P2P: no covariances)
        assert T.tobytes() == res["T"].tobytes() and ok == res["is_success"] and fit == res["fitness_score"]
        assert cov.tobytes() == res["local_cov"].tobytes()
        assert res["T_entry_query"].tobytes() == (np.linalg.inv(Lp["entry_poses"][e]) @ T).tobytes()


def test_loop_verify_improves_on_the_guess(loop, verified):
    """The condition as the issue sets it: for every revisit, Verify's pose is closer to the truth than the guess T_e Rz(yaw) it started
    from, in translation AND in rotation.  Two revisits decide it: revisit 4 was drawn 0.152 m from its entry and revisit 9's yaw 0.021 deg
    from a sector centre, so the registration has to be good to that.  The measured errors are in DESIGN.md section 21."""
    Lp, lc, revisits = loop
    misses = []
    for i, (cand, guess, res) in enumerate(verified):
        dt0, dr0 = synth.pose_error(Lp["revisit_poses"][i], guess)
        dt, dr = synth.pose_error(Lp["revisit_poses"][i], res["T"])
        print(f"revisit {i}: entry {cand['entry']} guess error {dt0:.3f} m {math.degrees(dr0):.3f} deg -> {dt:.3f} m {math.degrees(dr):.3f} deg "
              f"fitness {res['fitness_score']}")
        if not (dt < dt0 and dr < dr0):
            misses.append((i, round(dt0, 3), round(math.degrees(dr0), 3), round(dt, 3), round(math.degrees(dr), 3)))
    assert not misses, misses


def _rz(yaw):
    T = np.eye(4)
    c, s = np.cos(yaw), np.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    return T
