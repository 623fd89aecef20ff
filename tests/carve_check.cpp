// carve_check.cpp -- the carver of csrc/elm_carve.hpp on the CPU (tests/test_carve.py builds this against that header alone, with the
// address and undefined-behaviour sanitizers).  A mixed list of arrays is carved twice, on a null base and on a real allocation: the
// offsets of both passes agree, every pointer is 256-byte aligned relative to the base, no two arrays overlap, carved_size is the last
// offset, and a null base yields null pointers.  Every array is then written from end to end, so an array that reached past the
// allocation would trip the address sanitizer.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "elm_carve.hpp"

using elm_carve::carved_size;
using elm_carve::Carver;

namespace {

int failures = 0;
#define CHECK(cond)                                                     \
    do {                                                                \
        if (!(cond)) {                                                  \
            printf("FAILED line %d: %s\n", __LINE__, #cond);            \
            ++failures;                                                 \
        }                                                               \
    } while (0)

struct Span { // one carved array: where it starts (null on the size pass), the offset before and after its take, its bytes
    char* p;
    size_t off0, off1, bytes;
};

template <class T>
void take(Carver& c, size_t count, std::vector<Span>& out) {
    const size_t off0 = c.off;
    T* p = c.take<T>(count);
    out.push_back({(char*)p, off0, c.off, count * sizeof(T)});
}

// counts of 0 and 1, arrays of 255, 256 and 257 bytes, a uint8_t array between two double arrays, and a struct of an odd size
struct Odd {
    char b[12];
};
void carve(Carver& c, std::vector<Span>& out) {
    out.clear();
    take<double>(c, 0, out);
    take<double>(c, 1, out);
    take<uint8_t>(c, 255, out);
    take<uint8_t>(c, 256, out);
    take<uint8_t>(c, 257, out);
    take<double>(c, 33, out);
    take<uint8_t>(c, 3, out);
    take<double>(c, 32, out);
    take<uint32_t>(c, 64, out); // exactly 256 bytes
    take<uint32_t>(c, 65, out);
    take<Odd>(c, 43, out); // 516 bytes
    take<unsigned long long>(c, 1000, out);
    take<uint8_t>(c, 0, out);
    take<int32_t>(c, 1, out); // the last array
}

} // namespace

int main() {
    std::vector<Span> size_pass, real_pass;
    Carver sizer{nullptr};
    carve(sizer, size_pass);
    const size_t total = sizer.off;
    CHECK(total > 0 && total % 256 == 0);
    CHECK(carved_size([&](Carver& c) {
              std::vector<Span> tmp;
              carve(c, tmp);
          }) == total);
    for (const Span& s : size_pass) CHECK(s.p == nullptr); // a null base yields null pointers

    // the allocation is exactly `total` bytes and deliberately not 256-aligned itself: alignment is relative to the base
    std::vector<char> mem(total + 1);
    char* base = mem.data() + 1;
    Carver real{base};
    carve(real, real_pass);
    CHECK(real.off == total);
    CHECK(real_pass.size() == size_pass.size());
    size_t expect = 0;
    for (size_t k = 0; k < real_pass.size(); ++k) {
        const Span &r = real_pass[k], &s = size_pass[k];
        CHECK(r.off0 == s.off0 && r.off1 == s.off1 && r.bytes == s.bytes); // both passes agree
        CHECK(r.off0 == expect);                                           // arrays follow one another
        CHECK(r.p == base + r.off0);
        CHECK((size_t)(r.p - base) % 256 == 0);
        CHECK(r.off1 % 256 == 0 && r.off1 - r.off0 >= r.bytes && r.off1 - r.off0 < r.bytes + 256); // padded to the next 256, no further
        CHECK(r.off1 <= total);
        expect = r.off1;
    }
    CHECK(expect == total); // carved_size equals the last offset
    for (size_t k = 0; k < real_pass.size(); ++k)
        for (size_t j = k + 1; j < real_pass.size(); ++j) {
            const Span &a = real_pass[k], &b = real_pass[j];
            CHECK(a.p + a.bytes <= b.p || b.p + b.bytes <= a.p || !a.bytes || !b.bytes); // no two arrays overlap
        }
    // every array written from end to end with its own byte, then read back: nothing reached into a neighbour or past the allocation
    for (size_t k = 0; k < real_pass.size(); ++k) memset(real_pass[k].p, (int)(k + 1), real_pass[k].bytes);
    for (size_t k = 0; k < real_pass.size(); ++k)
        for (size_t q = 0; q < real_pass[k].bytes; ++q) CHECK((unsigned char)real_pass[k].p[q] == k + 1);

    // an empty carve takes nothing
    CHECK(carved_size([](Carver&) {}) == 0);
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("all cases passed (%zu arrays, %zu bytes)\n", real_pass.size(), total);
    return 0;
}
