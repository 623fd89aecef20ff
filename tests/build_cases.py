"""The inputs that tests/test_map_build_device_abi.py (mirror against oracle, CPU) and tests/test_map_build_device.py (device build against
host build against mirror, GPU) share: case(name) -> (points float32 [n, 3], voxel_size, cap), NAMES all of them."""
import numpy as np

SIZES = (0, 1, 63, 64, 65, 255, 256, 257, 1023, 1024, 1025)
ONE_VOXEL_CAPS = (1, 30, 64, 65, 100)
SPARSE_N = 1024 * 1024 + 1  # one entry beyond one chunk of the workgroup-sum scan (1024 workgroups of 1024 entries)


def _f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, 3))


def dense3():
    """60 000 points in +-3 m: at voxel 1, cap 30 every voxel ends at the cap"""
    return _f32(np.random.default_rng(5).uniform(-3.0, 3.0, size=(60000, 3)))


def extra5000():
    return _f32(np.random.default_rng(6).uniform(-3.5, 3.5, size=(5000, 3)))


def _axis_points(vals):
    out = []
    for v in vals:
        for axis in range(3):
            p = [0.25, 0.25, 0.25]
            p[axis] = v
            out.append(p)
        out.append([v, v, v])
        out.append([v, -v, 0.125])
    return out


# A = (1/8, 1/4, 1/4), B = (1/2, ..) 0.375 from A, C = (3/4, ..) 0.25 from B and 0.625 from A; map_resolution = 0.5 (voxel 1, cap 4)
_A, _B, _C = [0.125, 0.25, 0.25], [0.5, 0.25, 0.25], [0.75, 0.25, 0.25]
_CLOSER = float(np.nextafter(np.float32(0.75), np.float32(0.0)))  # the next float32 below 0.75: 0.5 - 2^-24 from (1/4, 1/4, 1/4)

_FIXED = {
    # truncation: voxel 0 is two wide (-1, 1); -0.0f; points exactly on the faces +-1, +-2
    "keys": (lambda: _f32(_axis_points([0.5, -0.5, 0.999, -0.999, -0.0, 0.0, 1.0, -1.0, 2.0, -2.0, 1.5, -1.5])), 1.0, 30),
    "keys_vs03": (lambda: _f32(np.concatenate([_axis_points([0.5, -0.5, 0.999, -0.999, -0.0, 0.3, -0.3, 0.6, -0.6, 0.29999998, 1.0, -1.0, 2.0, -2.0]),
                                                 np.random.default_rng(9).uniform(-2.0, 2.0, size=(3000, 3))])), 0.3, 30),
    "offset_1e5": (lambda: _f32(np.random.default_rng(10).uniform(-3.0, 3.0, size=(20000, 3)) + 1e5), 1.0, 30),
    # the spacing rule at its threshold: dyadic coordinates, the float64 distance is exact
    "exactly_res_apart": (lambda: _f32([[0.25, 0.25, 0.25], [0.75, 0.25, 0.25]]), 1.0, 4),        # 0.5 < 0.5 is false: both kept
    "one_ulp_closer": (lambda: _f32([[0.25, 0.25, 0.25], [_CLOSER, 0.25, 0.25]]), 1.0, 4),       # the second is rejected
    "chain_abc": (lambda: _f32([_A, _B, _C]), 1.0, 4),   # B is near A: rejected; C is not near A: kept
    "chain_cba": (lambda: _f32([_C, _B, _A]), 1.0, 4),   # C, then A
    "chain_bac": (lambda: _f32([_B, _A, _C]), 1.0, 4),   # B alone
    "duplicates": (lambda: _f32([[0.25, 0.5, 0.75]] * 5 + [[0.75, 0.5, 0.25]] * 3 + [[0.25, 0.5, 0.75]]), 1.0, 4),
    "dense3": (dense3, 1.0, 30),
    "dense3_vs05": (dense3, 0.5, 30),
    # 20 000 points in +-8 m: almost purely the spacing rule
    "spacing8": (lambda: _f32(np.random.default_rng(7).uniform(-8.0, 8.0, size=(20000, 3))), 1.0, 30),
    "own_voxel_4097": (lambda: _f32(np.random.default_rng(11).permutation(
        np.stack([np.arange(4097) % 64 + 0.5, np.arange(4097) // 64 + 0.5, np.full(4097, 0.5)], 1))), 1.0, 30),
    "pairs_512": (lambda: _f32(np.random.default_rng(12).permutation(np.concatenate(
        [np.stack([np.arange(512) + 0.25, np.full(512, 0.25), np.full(512, -7.25)], 1),
         np.stack([np.arange(512) + 0.75, np.full(512, 0.75), np.full(512, -7.75)], 1)]))), 1.0, 30),
    # beyond 64 kept points without reaching the cap at once
    "one_voxel_1500_cap400": (lambda: _f32(np.random.default_rng(14).uniform(0.05, 0.95, size=(1500, 3))), 1.0, 400),
    "sparse_%d" % SPARSE_N: (lambda: _f32(np.random.default_rng(15).uniform(-500.0, 500.0, size=(SPARSE_N, 3))), 1.0, 30),
}


def case(name):
    if name.startswith("n_"):
        n = int(name[2:])
        return _f32(np.random.default_rng(100 + n).uniform(-2.0, 2.0, size=(n, 3))), 1.0, 30
    if name.startswith("one_voxel_cap"):
        return _f32(np.random.default_rng(13).uniform(0.05, 0.95, size=(5000, 3))), 1.0, int(name[len("one_voxel_cap"):])
    make, vs, cap = _FIXED[name]
    return make(), vs, cap


NAMES = ["n_%d" % n for n in SIZES] + ["one_voxel_cap%d" % c for c in ONE_VOXEL_CAPS] + list(_FIXED)
