// elm_carve.hpp -- the arrays of one allocation: a carve function takes them from a Carver one after another, each aligned to 256 bytes,
// and runs twice with the same counts -- on a null base for the size (carved_size), on the allocation for the pointers
// (elm_call.hpp's DeviceBlob does both).  Nothing of HIP is included: a CPU program can test it (tests/carve_check.cpp).  C++17.
#pragma once
#include <stddef.h>

namespace elm_carve {

constexpr size_t kCarveAlign = 256;

struct Carver {
    char* base; // nullptr: the size pass, every take() is nullptr
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (count * sizeof(T) + kCarveAlign - 1) / kCarveAlign * kCarveAlign;
        return p;
    }
};

// the bytes that carve(Carver&) takes
template <class F>
size_t carved_size(F carve) {
    Carver c{nullptr};
    carve(c);
    return c.off;
}

} // namespace elm_carve
