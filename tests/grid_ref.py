"""The numpy mirror of the P2P / GICP cell grid (include/elimaloc_hip.h, "device index build"; DevMap::grid_* in csrc/elm_internal.hpp),
written from the description of the layout, not from the builders:

  cell      a stored coordinate a lies in half-voxel cell c of its axis.  With t = (double)a / voxel_size and k = t truncated toward zero
            (the stored key): cells 2k and 2k + 1 split voxel k > 0 at t - k >= 0.5; voxel k < 0 is split into 2k - 2 and 2k - 1 at
            t - k > -0.5; voxel 0 holds FOUR cells, -2 | -1 | 0 | 1, split at t > -0.5, t >= 0 (so -0.0 is in cell 0) and t >= 0.5
  box       lowest cell - 2 .. highest cell + 2 per axis
  dense     entry = ((cx - x0) * ny + (cy - y0)) * nz + (cz - z0)
  two-level tiles of 8 x 8 columns, tile t = (cx >> 3) * tny + (cy >> 3) over box-relative cells; an occupied tile with cells z0 .. z0 + nz - 1
            owns 64 * (nz + 1) entries, the tiles in ascending t from entry 64 on (entries 0 .. 63: the run every empty tile shares);
            tiles[t] = {first entry, z0 | nz << 16}, {0, 0} when empty; entry = first + ((cx & 7) << 3 | (cy & 7)) * (nz + 1) + (cz - z0)
  layout    the points of an entry in input order, every entry in whole blocks of four slots from block 1 on (block 0 is padding);
            start[e] = first block of e (an empty entry: where its blocks would begin), four trailing words = n_blk, the two-level form's
            first 64 words = 0; a block is x[4] y[4] z[4]; padding is 1e18 / 0xFFFFFFFF
"""
import numpy as np

PAD_COORD = np.float32(1e18)
PAD_POINT = np.uint32(0xFFFFFFFF)
TILE_SHIFT, TILE = 3, 8


def cell_of(a, voxel_size):
    """half-voxel cell of every float32 coordinate in a (any shape) -> int64"""
    t = np.asarray(a, np.float32).astype(np.float64) / np.float64(voxel_size)
    k = np.trunc(t)
    f = t - k
    pos = 2 * k + (f >= 0.5)
    neg = 2 * k - 2 + (f > -0.5)
    zero = np.where(t >= 0.0, np.where(t >= 0.5, 1, 0), np.where(t > -0.5, -1, -2))
    return np.where(k > 0, pos, np.where(k < 0, neg, zero)).astype(np.int64)


def box(cells):
    """cells [n, 3] -> (lo [3], dim [3]) with the margin of two cells on every side"""
    lo = cells.min(axis=0) - 2
    hi = cells.max(axis=0) + 2
    return lo, hi - lo + 1


def dense_entry(cells, lo, dim):
    c = cells - lo
    return (c[:, 0] * dim[1] + c[:, 1]) * dim[2] + c[:, 2]


def tile_table(cells, lo, dim):
    """-> (tiles uint32 [n_tiles, 2], entries, tnx, tny)"""
    c = cells - lo
    tnx, tny = (int(dim[0]) + TILE - 1) // TILE, (int(dim[1]) + TILE - 1) // TILE
    t = (c[:, 0] >> TILE_SHIFT) * tny + (c[:, 1] >> TILE_SHIFT)
    n_tiles = tnx * tny
    zmin = np.full(n_tiles, 1 << 40, np.int64)
    zmax = np.full(n_tiles, -1, np.int64)
    np.minimum.at(zmin, t, c[:, 2])
    np.maximum.at(zmax, t, c[:, 2])
    occ = zmax >= 0
    nz = np.where(occ, zmax - zmin + 1, 0)
    own = np.where(occ, TILE * TILE * (nz + 1), 0)
    first = TILE * TILE + np.concatenate([[0], np.cumsum(own)[:-1]])
    tiles = np.zeros((n_tiles, 2), np.uint32)
    tiles[occ, 0] = first[occ]
    tiles[occ, 1] = zmin[occ] | (nz[occ] << 16)
    return tiles, int(TILE * TILE + own.sum()), tnx, tny


def tiled_entry(cells, lo, tiles, tny):
    c = cells - lo
    te = tiles[(c[:, 0] >> TILE_SHIFT) * tny + (c[:, 1] >> TILE_SHIFT)].astype(np.int64)
    z0, nz = te[:, 1] & 0xFFFF, te[:, 1] >> 16
    return te[:, 0] + (((c[:, 0] & (TILE - 1)) << TILE_SHIFT) | (c[:, 1] & (TILE - 1))) * (nz + 1) + (c[:, 2] - z0)


def layout(xyz, entry, entries, zero_head=0):
    """xyz float32 [n, 3], entry [n] -> (start uint32 [entries + 4], blocks float32 [n_blk, 3, 4], slot_point uint32 [4 n_blk])"""
    xyz = np.asarray(xyz, np.float32).reshape(-1, 3)
    entry = np.asarray(entry, np.int64)
    n = len(entry)
    cnt = np.bincount(entry, minlength=entries).astype(np.int64)
    nblk = (cnt + 3) // 4
    first_blk = 1 + np.concatenate([[0], np.cumsum(nblk)[:-1]]) if entries else np.zeros(0, np.int64)
    n_blk = 1 + int(nblk.sum())
    start = np.concatenate([first_blk, [n_blk] * 4]).astype(np.uint32)
    start[:zero_head] = 0
    order = np.argsort(entry, kind="stable")  # by entry, input order inside
    first_pos = np.concatenate([[0], np.cumsum(cnt)[:-1]]) if entries else np.zeros(0, np.int64)
    e_sorted = entry[order]
    slot = 4 * first_blk[e_sorted] + (np.arange(n) - first_pos[e_sorted])
    blocks = np.full((n_blk, 3, 4), PAD_COORD, np.float32)
    slot_point = np.full(4 * n_blk, PAD_POINT, np.uint32)
    blocks[slot >> 2, :, slot & 3] = xyz[order]
    slot_point[slot] = order
    return start, blocks, slot_point


def grid(stored_xyz, voxel_size, tiled, narrow_limit=0xFFFFFF00):
    """The whole grid of a map's stored points (float32 values, in stored order) -> the dict VoxelHashMap.CellGrid() returns, with the
    descriptor fields this mirror knows (the dense form's statistics box from the stored keys; not the two-level form's, which has none)."""
    xyz = np.asarray(stored_xyz, np.float32).reshape(-1, 3)
    cells = cell_of(xyz, voxel_size)
    lo, dim = box(cells)
    desc = {"gx0": int(lo[0]), "gy0": int(lo[1]), "gz0": int(lo[2]), "grid_tiled": int(bool(tiled))}
    if tiled:
        tiles, entries, tnx, tny = tile_table(cells, lo, dim)
        start, blocks, slot_point = layout(xyz, tiled_entry(cells, lo, tiles, tny), entries, TILE * TILE)
        desc.update(gnx=tnx * TILE, gny=tny * TILE, gnz=int(dim[2]), gtny=tny, n_tiles=tnx * tny)
    else:
        tiles = np.zeros((0, 2), np.uint32)
        entries = int(dim[0] * dim[1] * dim[2])
        start, blocks, slot_point = layout(xyz, dense_entry(cells, lo, dim), entries)
        keys = np.trunc(xyz.astype(np.float64) / np.float64(voxel_size)).astype(np.int64)
        klo, khi = keys.min(axis=0), keys.max(axis=0)
        desc.update(gnx=int(dim[0]), gny=int(dim[1]), gnz=int(dim[2]), n_tiles=0, vx0=int(klo[0]) - 1, vy0=int(klo[1]) - 1, vz0=int(klo[2]) - 1,
                    vnx=int(khi[0] - klo[0]) + 3, vny=int(khi[1] - klo[1]) + 3, vnz=int(khi[2] - klo[2]) + 3)
    desc.update(n_start_words=entries + 4, n_blocks=len(blocks), grid_nslots=4 * len(blocks), grid_wide=int(len(blocks) * 48 > narrow_limit))
    return {"desc": desc, "start": start, "blocks": blocks, "slot_point": slot_point, "tiles": tiles}
