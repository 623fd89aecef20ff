"""Inputs of the place-recognition tests (tests/test_places_abi.py on the CPU, tests/test_places.py on the GPU): the boundary family of
the descriptor, random scans and descriptors, and the loop of 24 entries and 12 revisits in the field world whose mirror results are
committed as tests/golden/places_loop.npz (written by `python tests/places_cases.py`)."""
import math
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "places_loop.npz")


def f32_steps(v, k):
    """the float32 k representable steps above (k > 0) or below (k < 0) v"""
    v = np.float32(v)
    for _ in range(abs(k)):
        v = np.nextafter(v, np.float32(np.inf if k > 0 else -np.inf), dtype=np.float32)
    return v


def sector_boundary_points(dirs, radii=(5.0, 30.0), z=0.5):
    """every sector boundary at the given radii: the float32 point on the direction and its neighbours up to 2 ulps either side in x
    and in y -> float32 [64 * len(radii) * 9, 3]"""
    out = []
    for r in radii:
        for k in range(64):
            x, y = np.float32(r * dirs[k, 0]), np.float32(r * dirs[k, 1])
            out.append((x, y, z))
            for s in (-2, -1, 1, 2):
                out.append((f32_steps(x, s), y, z))
                out.append((x, f32_steps(y, s), z))
    return np.array(out, np.float32)


def edge_points(cfg_ref, ring_edge2, z_edge):
    """every ring edge (along +x and along the diagonal) and every layer edge with its float32 neighbours up to 2 steps either side"""
    out = []
    z_mid = np.float32(0.5 * (z_edge[0] + z_edge[1]))
    for e2 in ring_edge2:
        e = math.sqrt(e2)
        for s in (-2, -1, 0, 1, 2):
            out.append((f32_steps(e, s), 0.0, z_mid))
            out.append((0.0, -f32_steps(e, s), z_mid))
            d = f32_steps(e / math.sqrt(2.0), s)
            out.append((d, d, z_mid))
    r_mid = np.float32(math.sqrt(0.5 * (ring_edge2[0] + ring_edge2[1])))
    for ze in z_edge:
        for s in (-2, -1, 0, 1, 2):
            out.append((r_mid, 0.25, f32_steps(ze, s)))
    return np.array(out, np.float32)


def random_scan(n, seed, scale=25.0):
    """n points of a rough cylinder around the sensor: ranges 0 .. 2 scale, heights -5 .. 12 (some outside every ring and layer)"""
    rng = np.random.default_rng(seed)
    az = rng.uniform(-math.pi, math.pi, n)
    r = rng.uniform(0.0, 2.0 * scale, n)
    return np.ascontiguousarray(np.stack([r * np.cos(az), r * np.sin(az), rng.uniform(-5.0, 12.0, n)], axis=1).astype(np.float32))


def tilted_level(roll_deg=1.5, pitch_deg=-2.0, height=1.9):
    from elimaloc_amd import synth
    T = np.eye(4)
    T[:3, :3] = synth.rot_zyx(math.radians(roll_deg), math.radians(pitch_deg), 0.0)
    T[2, 3] = height
    return T


def far_level(offset=1e5):
    """a level that carries the scan 1e5 m away in x and y: nothing of it lies in a ring"""
    T = np.eye(4)
    T[0, 3] = T[1, 3] = offset
    return T


def random_words(n, W, density, seed):
    """n descriptors of W words with each bit set with probability `density` (1.0: all ones)"""
    rng = np.random.default_rng(seed)
    bits = (rng.random((n, W, 64)) < density).astype(np.uint8)
    return np.ascontiguousarray(np.packbits(bits, axis=-1, bitorder="little").view(np.uint64).reshape(n, W))


# ---- the loop: 24 entries on a circle of radius 35 m in the field world, 12 revisits
LOOP_SEED = 20261019
N_ENTRIES, N_REVISITS, RADIUS, HEIGHT, SCAN_POINTS, MAX_RANGE = 24, 12, 35.0, 2.1, 4096, 45.0
_LOOP = {}


def _pose(x, y, yaw):
    T = np.eye(4)
    c, s = math.cos(yaw), math.sin(yaw)
    T[:2, :2] = [[c, -s], [s, c]]
    T[:3, 3] = (x, y, HEIGHT)
    return T


def loop_inputs():
    """dict(world, entry_poses [24, 4, 4], entry_scans [24][4096, 3], revisit_entry [12], revisit_yaw [12], revisit_poses, revisit_scans):
    deterministic in LOOP_SEED, built once per process"""
    if _LOOP:
        return _LOOP
    from elimaloc_amd import synth
    world = synth.make_field_world(400_000, 1001)
    rng = np.random.default_rng(LOOP_SEED)
    ang = 2.0 * math.pi * np.arange(N_ENTRIES) / N_ENTRIES
    entry_poses = np.stack([_pose(RADIUS * math.cos(a), RADIUS * math.sin(a), a + 0.5 * math.pi) for a in ang])
    entry_scans = [synth.make_scan(world, SCAN_POINTS, 5000 + e, T_true=entry_poses[e], max_range=MAX_RANGE)[0] for e in range(N_ENTRIES)]
    rev_entry = rng.integers(0, N_ENTRIES, N_REVISITS)
    off = rng.uniform(-1.0, 1.0, (N_REVISITS, 2))
    rev_yaw = rng.uniform(-math.pi, math.pi, N_REVISITS)  # relative to the entry's sensor
    rev_poses = np.stack([_pose(entry_poses[e][0, 3] + off[i, 0], entry_poses[e][1, 3] + off[i, 1], ang[e] + 0.5 * math.pi + rev_yaw[i])
                          for i, e in enumerate(rev_entry)])
    rev_scans = [synth.make_scan(world, SCAN_POINTS, 7000 + i, T_true=rev_poses[i], max_range=MAX_RANGE)[0] for i in range(N_REVISITS)]
    _LOOP.update(world=world, entry_poses=entry_poses, entry_scans=entry_scans, revisit_entry=rev_entry, revisit_yaw=rev_yaw,
                 revisit_poses=rev_poses, revisit_scans=rev_scans)
    return _LOOP


def expected_shift(yaw):
    """round(-yaw 64 / 2 pi) mod 64"""
    return int(round(-yaw * 64.0 / (2.0 * math.pi))) % 64


def mirror_loop(dirs):
    """the mirror's descriptors and top-3 candidates of the loop -> dict of arrays (the content of the golden file)"""
    import places_ref
    L = loop_inputs()
    cfg = places_ref.Cfg()
    ew = np.stack([places_ref.describe(s, cfg, dirs)[0] for s in L["entry_scans"]])
    rw = np.stack([places_ref.describe(s, cfg, dirs)[0] for s in L["revisit_scans"]])
    m = places_ref.match_all(rw, ew)
    ids = np.arange(N_ENTRIES)
    top = [places_ref.select(m[i], ids, 3) for i in range(N_REVISITS)]
    return dict(entry_words=ew, revisit_words=rw, matches=m,
                cand_entry=np.array([[c["entry"] for c in t] for t in top], np.int32),
                cand_dice=np.array([[c["dice_q16"] for c in t] for t in top], np.uint32),
                cand_inter=np.array([[c["inter"] for c in t] for t in top], np.uint16),
                cand_shift=np.array([[c["shift"] for c in t] for t in top], np.uint16),
                revisit_entry=L["revisit_entry"].astype(np.int32), revisit_yaw=L["revisit_yaw"])


if __name__ == "__main__":
    import sys
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from elimaloc_amd.places import PlaceTables
    g = mirror_loop(PlaceTables()[2])
    ok = True
    for i in range(N_REVISITS):
        want = expected_shift(g["revisit_yaw"][i])
        d = (int(g["cand_shift"][i, 0]) - want) % 64
        first = int(g["cand_entry"][i, 0]) == int(g["revisit_entry"][i])
        ok &= first and d in (0, 1, 63)
        print(i, "true", int(g["revisit_entry"][i]), "cands", g["cand_entry"][i].tolist(), "dice", g["cand_dice"][i].tolist(), "shift",
              int(g["cand_shift"][i, 0]), "want", want)
    print("condition met:", ok)
    if ok:
        np.savez_compressed(GOLDEN, **g)
