// The stand-alone program of tests/test_index_build_device_abi.py: elm_host::grid_block_layout (csrc/elm_grid_layout.hpp, nothing else of
// the library) run on the caller's points and entries, its outputs written out for the numpy mirror (tests/grid_ref.py) to be compared
// with.  Built with the address and undefined-behaviour sanitizers.
//   grid_layout_dump IN OUT
//   IN:  uint64 n, uint64 entries, uint32 entry[n], float32 xyz[n][3]
//   OUT: uint64 n_blk, uint32 start[entries + 4], float32 blocks[n_blk][12], uint32 slot_point[4 * n_blk]
#include <stdint.h>
#include <stdio.h>

#include <vector>

#include "elm_grid_layout.hpp"

struct Blk {
    float x[4], y[4], z[4];
};
static_assert(sizeof(Blk) == 48, "x[4] y[4] z[4]");

int main(int argc, char** argv) {
    if (argc != 3) return 2;
    FILE* in = fopen(argv[1], "rb");
    if (!in) return 3;
    uint64_t n = 0, entries = 0;
    if (fread(&n, 8, 1, in) != 1 || fread(&entries, 8, 1, in) != 1) return 4;
    std::vector<uint32_t> entry(n);
    std::vector<float> xyz(3 * n), xyz4(4 * n);
    if (n && (fread(entry.data(), 4, n, in) != n || fread(xyz.data(), 12, n, in) != n)) return 4;
    fclose(in);
    for (uint64_t i = 0; i < n; ++i) {
        if (entry[i] >= entries) return 5;
        for (int a = 0; a < 3; ++a) xyz4[4 * i + a] = xyz[3 * i + a];
        xyz4[4 * i + 3] = -7.f; // the fourth float of a stored point is not a coordinate
    }
    std::vector<uint32_t> start, gi;
    std::vector<Blk> gb;
    const uint64_t n_blk = elm_host::grid_block_layout(xyz4.data(), (size_t)n, entry, entries, 0x1FFFFFF0ull, start, gb, gi);
    if (start.size() != entries + 4 || gb.size() != n_blk || gi.size() != 4 * n_blk) return 6;
    FILE* out = fopen(argv[2], "wb");
    if (!out) return 3;
    fwrite(&n_blk, 8, 1, out);
    fwrite(start.data(), 4, start.size(), out);
    fwrite(gb.data(), sizeof(Blk), gb.size(), out);
    fwrite(gi.data(), 4, gi.size(), out);
    return fclose(out) == 0 ? 0 : 7;
}
