// The stand-alone program of tests/test_grid_layout.py: elm_host::grid_block_layout (csrc/elm_grid_layout.hpp, nothing else of the
// library) against a naive reference -- a stable sort of (entry, input index) -- on seeded inputs.  Built with the address and
// undefined-behaviour sanitizers; prints one line per case and exits non-zero at the first difference.
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <algorithm>
#include <random>
#include <string>
#include <utility>
#include <vector>

#include "elm_grid_layout.hpp"

struct Blk {
    float x[4], y[4], z[4];
};
static_assert(sizeof(Blk) == 48, "x[4] y[4] z[4]");

static int g_failed = 0;
#define EXPECT(cond, ...)                                  \
    do {                                                   \
        if (!(cond)) {                                     \
            printf("  FAILED %s: ", #cond);                \
            printf(__VA_ARGS__);                           \
            printf("\n");                                  \
            ++g_failed;                                    \
            return;                                        \
        }                                                  \
    } while (0)

static bool is_pad(float v) { return v == 1e18f; }

// entry[i] of every point; the points themselves are seeded, distinct, and carry a fourth float that the layout must not read as a coordinate
static void check(const char* name, const std::vector<uint32_t>& entry, uint64_t entries, uint32_t seed) {
    const size_t n = entry.size();
    std::mt19937 rng(seed);
    std::uniform_real_distribution<float> u(-100.f, 100.f);
    std::vector<float> xyz4(4 * n);
    for (size_t i = 0; i < n; ++i) {
        xyz4[4 * i] = u(rng); xyz4[4 * i + 1] = u(rng); xyz4[4 * i + 2] = u(rng);
        xyz4[4 * i + 3] = -7.f;
    }
    // the reference: points in (entry, input index) order; every entry starts a fresh block, block 0 is padding
    std::vector<std::pair<uint32_t, uint32_t>> order(n);
    for (size_t i = 0; i < n; ++i) order[i] = {entry[i], (uint32_t)i};
    std::stable_sort(order.begin(), order.end(), [](const std::pair<uint32_t, uint32_t>& a, const std::pair<uint32_t, uint32_t>& b) { return a.first < b.first; });
    std::vector<uint32_t> cnt(entries, 0), want_start(entries + 4, 0);
    for (size_t i = 0; i < n; ++i) cnt[entry[i]]++;
    uint64_t blk = 1;
    for (uint64_t e = 0; e < entries; ++e) {
        want_start[e] = (uint32_t)blk;
        blk += (cnt[e] + 3) / 4;
    }
    const uint64_t want_blk = blk;
    for (uint64_t e = entries; e < entries + 4; ++e) want_start[e] = (uint32_t)want_blk;
    std::vector<uint32_t> want_slot(4 * want_blk, 0xFFFFFFFFu);
    {
        size_t k = 0;
        for (uint64_t e = 0; e < entries; ++e)
            for (uint32_t r = 0; r < cnt[e]; ++r, ++k) want_slot[4 * (size_t)want_start[e] + r] = order[k].second;
    }

    std::vector<uint32_t> ent(entry), start, gi;
    std::vector<Blk> gb;
    const uint64_t n_blk = elm_host::grid_block_layout(xyz4.data(), n, ent, entries, ~0ull, start, gb, gi);
    printf("%-28s n %5zu entries %5llu n_blk %5llu\n", name, n, (unsigned long long)entries, (unsigned long long)n_blk);
    EXPECT(n_blk == want_blk, "n_blk %llu, want %llu", (unsigned long long)n_blk, (unsigned long long)want_blk);
    EXPECT(ent.empty() && ent.capacity() == 0, "the entry numbers are released");
    EXPECT(start.size() == entries + 4 && gb.size() == n_blk && gi.size() == 4 * n_blk, "sizes %zu %zu %zu", start.size(), gb.size(), gi.size());
    for (uint64_t e = 0; e < entries + 4; ++e) EXPECT(start[e] == want_start[e], "start[%llu] = %u, want %u", (unsigned long long)e, start[e], want_start[e]);
    for (uint64_t e = entries; e < entries + 4; ++e) EXPECT(start[e] == n_blk, "trailing entry %llu = %u", (unsigned long long)e, start[e]);
    std::vector<uint32_t> seen(n, 0);
    for (size_t s = 0; s < gi.size(); ++s) {
        const Blk& b = gb[s >> 2];
        const float x = b.x[s & 3], y = b.y[s & 3], z = b.z[s & 3];
        EXPECT(gi[s] == want_slot[s], "slot %zu holds point %u, want %u", s, gi[s], want_slot[s]);
        if (gi[s] == 0xFFFFFFFFu) {
            EXPECT(is_pad(x) && is_pad(y) && is_pad(z), "unused slot %zu is not padding: %g %g %g", s, x, y, z);
        } else {
            const uint32_t i = gi[s];
            EXPECT(i < n, "slot %zu: point %u of %zu", s, i, n);
            EXPECT(s >= 4, "a point in block 0");
            EXPECT(memcmp(&x, &xyz4[4 * i], 4) == 0 && memcmp(&y, &xyz4[4 * i + 1], 4) == 0 && memcmp(&z, &xyz4[4 * i + 2], 4) == 0, "slot %zu: coordinates of point %u", s, i);
            seen[i]++;
        }
    }
    for (int s = 0; s < 4; ++s) EXPECT(gi[s] == 0xFFFFFFFFu && is_pad(gb[0].x[s]) && is_pad(gb[0].y[s]) && is_pad(gb[0].z[s]), "block 0, slot %d", s);
    for (size_t i = 0; i < n; ++i) EXPECT(seen[i] == 1, "point %zu appears %u times", i, seen[i]);
    // a point's slot = 4 * start[entry] + its rank among the entry's points in input order
    std::vector<uint32_t> rank(entries, 0);
    for (size_t i = 0; i < n; ++i) {
        const size_t s = 4 * (size_t)start[entry[i]] + rank[entry[i]]++;
        EXPECT(gi[s] == i, "point %zu is not at slot %zu", i, s);
    }
    // a block limit below n_blk: the count alone
    if (n_blk > 1) {
        std::vector<uint32_t> ent2(entry), start2, gi2;
        std::vector<Blk> gb2;
        EXPECT(elm_host::grid_block_layout(xyz4.data(), n, ent2, entries, n_blk - 1, start2, gb2, gi2) == n_blk, "the count beyond the block limit");
    }
}

int main() {
    std::mt19937 rng(20240607);
    { // entries holding 0, 1, 3, 4, 5 and 9 points, in shuffled input order
        const uint32_t sizes[] = {0, 1, 3, 4, 5, 9, 0, 4, 1};
        std::vector<uint32_t> e;
        for (uint32_t k = 0; k < 9; ++k)
            for (uint32_t r = 0; r < sizes[k]; ++r) e.push_back(k);
        std::shuffle(e.begin(), e.end(), rng);
        check("sizes 0 1 3 4 5 9", e, 9, 1);
    }
    check("all points in one entry", std::vector<uint32_t>(37, 5u), 11, 2);
    check("all points in entry 0", std::vector<uint32_t>(8, 0u), 1, 3);
    check("no points", {}, 6, 4);
    check("no points, no entries", {}, 0, 5);
    { // the last entry occupied (and the first empty)
        std::vector<uint32_t> e = {6, 2, 6, 6, 2, 6, 6};
        check("last entry occupied", e, 7, 6);
    }
    { // entry numbers in descending input order
        std::vector<uint32_t> e;
        for (uint32_t k = 40; k-- > 0;)
            for (uint32_t r = 0; r < 1 + k % 6; ++r) e.push_back(k);
        check("descending entries", e, 40, 7);
    }
    { // many entries, random occupancy: most empty, some with several blocks
        std::uniform_int_distribution<uint32_t> pick(0, 999);
        std::vector<uint32_t> e(3000);
        for (auto& v : e) v = pick(rng) < 300 ? pick(rng) % 7 * 13 : pick(rng);
        check("random, 1000 entries", e, 1000, 8);
    }
    if (g_failed) {
        printf("%d case(s) failed\n", g_failed);
        return 1;
    }
    printf("all cases passed\n");
    return 0;
}
