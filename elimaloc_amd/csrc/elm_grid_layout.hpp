// elm_grid_layout.hpp -- the block layout of the cell grids (DevMap::grid_blk / grid_idx / grid_start), said once for the dense and the
// two-level form.  Plain C++17, no HIP: tests/test_grid_layout.py compiles it on its own.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <vector>

namespace elm_host {

constexpr float kGridPadCoord = 1e18f;        // a padding slot's coordinates: never the nearest, never within range
constexpr uint32_t kGridPadPoint = 0xFFFFFFFFu; // a padding slot's point number

// Lays n points out in blocks of four slots, entry by entry.  xyz4: the points, x y z at a stride of four floats.  entry[i] < entries: the
// entry (cell) of point i; the vector is CONSUMED (released as soon as the order is known, before the blocks are allocated).  Blk: twelve
// floats x[4] y[4] z[4] (GridBlk).  Out:
//   start  entries + 4 words: start[e] = the first block of entry e (an empty entry: where its blocks would begin, so start[e + 1] is always
//          the end of e); the four trailing words = n_blk
//   gb     n_blk blocks; block 0 is four padding slots (read by masked-off loads), as is every slot past an entry's last point
//   gi     4 * n_blk words: the point in every slot, kGridPadPoint in padding
// A point's slot is 4 * start[entry] + its rank among the entry's points in input order (so an entry keeps the caller's order).
// Returns n_blk; beyond max_blocks nothing but the count is computed and the outputs are not to be used.
// ONE table of entries + 4 words serves in turn as the counts, the running cursors of the stable scatter and -- rewritten entry by entry
// while the blocks are laid out -- the block starts; beside it only the scatter's order (n words) is alive while the blocks are written.
template <class Blk>
uint64_t grid_block_layout(const float* xyz4, size_t n, std::vector<uint32_t>& entry, uint64_t entries, uint64_t max_blocks,
                           std::vector<uint32_t>& start, std::vector<Blk>& gb, std::vector<uint32_t>& gi) {
    static_assert(sizeof(Blk) == 12 * sizeof(float), "a block is x[4] y[4] z[4]");
    start.assign(entries + 4, 0u);
    for (size_t i = 0; i < n; ++i) start[(uint64_t)entry[i] + 1]++;
    uint64_t n_blk = 1; // block 0: four padding slots
    for (uint64_t c = 0; c < entries; ++c) n_blk += (start[c + 1] + 3) / 4;
    if (n_blk > max_blocks) return n_blk;
    for (uint64_t c = 0; c < entries; ++c) start[c + 1] += start[c]; // start[c] = first position of entry c in the (unpadded) sorted order
    std::vector<uint32_t> perm(n);
    for (size_t i = 0; i < n; ++i) perm[start[entry[i]]++] = (uint32_t)i; // input order in, so an entry keeps its points in input order
    std::vector<uint32_t>().swap(entry);
    // the cursors now hold every entry's END: start[c] = end(c) = begin(c + 1)
    gb.resize(n_blk);
    gi.assign(4 * n_blk, kGridPadPoint);
    for (auto& b : gb)
        for (int u = 0; u < 4; ++u) b.x[u] = b.y[u] = b.z[u] = kGridPadCoord;
    uint64_t blk = 1;
    uint32_t begin = 0;
    for (uint64_t c = 0; c < entries; ++c) {
        const uint32_t end = start[c];
        start[c] = (uint32_t)blk;
        for (uint32_t k = begin; k < end; ++k) {
            const uint32_t i = perm[k];
            const uint64_t pos = blk * 4 + (k - begin);
            gb[pos >> 2].x[pos & 3] = xyz4[4 * (size_t)i]; gb[pos >> 2].y[pos & 3] = xyz4[4 * (size_t)i + 1]; gb[pos >> 2].z[pos & 3] = xyz4[4 * (size_t)i + 2];
            gi[pos] = i;
        }
        blk += (end - begin + 3) / 4;
        begin = end;
    }
    for (uint64_t c = entries; c < entries + 4; ++c) start[c] = (uint32_t)blk;
    return n_blk;
}

} // namespace elm_host
