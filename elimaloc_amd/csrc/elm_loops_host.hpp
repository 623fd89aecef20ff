// elm_loops_host.hpp -- what the two loop consistency calls share on the host (elm_loops.cpp, elm_loopcov.cpp): the one device allocation
// of a call and its carving, the call's stream events, the checks on the loops themselves, and the greedy loop that queues
// steps_per_batch steps between two reads of the device's state.  Host-side C++17, everything inline.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "elm_dev_loops.hpp"
#include "elm_query.hpp"

namespace elm_loops_host {

constexpr size_t kLcMaxPoses = (size_t)1 << 20;

// the device arrays of one call carved from one allocation, each aligned to 256 bytes (base == nullptr: the size alone)
struct Carver {
    char* base;
    size_t off = 0;
    template <class T>
    T* take(size_t count) {
        T* p = base ? (T*)(base + off) : nullptr;
        off += (count * sizeof(T) + 255) / 256 * 256;
        return p;
    }
};

struct Blob { // the call's one device allocation, released when the call ends however it ends (its stream joined first)
    char* p = nullptr;
    hipStream_t st = nullptr;
    ~Blob() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        (void)hipFree(p);
    }
};

template <int N>
struct Events { // the marks of a call on its stream
    hipEvent_t ev[N] = {};
    ~Events() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
};

// the greedy arrays of an LcDev (adj aside) from the carver
inline void carve_greedy(elm::LcDev& d, Carver& c, size_t L) {
    const size_t W = elm::lc_words((uint32_t)L);
    d.cand = c.take<unsigned long long>(2 * W);
    d.deg0 = c.take<int32_t>(L);
    d.deg = c.take<int32_t>(L);
    d.member = c.take<uint8_t>(L);
    d.state = c.take<elm::LcState>(1);
    d.L = (uint32_t)L;
    d.W = (uint32_t)W;
}

// every loop a candidate, no member, the state cleared (cand0: [W] host words that live until the stream is joined)
inline hipError_t greedy_reset(hipStream_t st, const elm::LcDev& d, std::vector<unsigned long long>& cand0) {
    cand0.assign(d.W, ~0ull);
    if (d.L & 63u) cand0[d.W - 1] = (1ull << (d.L & 63u)) - 1ull; // the padding bits clear
    hipError_t e = hipMemcpyAsync(d.cand, cand0.data(), d.W * sizeof(unsigned long long), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemsetAsync(d.member, 0, d.L, st);
    if (e == hipSuccess) e = hipMemsetAsync(d.state, 0, sizeof(elm::LcState), st);
    return e;
}

// The greedy loop: a clique has at most L members, and the step after the last pick would only set the stop word.  The stream is joined
// after every batch; state holds the device's when it returns.
inline hipError_t greedy_run(hipStream_t st, const elm::LcDev& d, int32_t steps_per_batch, elm::LcState& state) {
    const size_t L = d.L;
    hipError_t e = hipSuccess;
    uint32_t it = 0;
    while (e == hipSuccess) {
        const uint32_t upto = (uint32_t)std::min<uint64_t>((uint64_t)it + (uint64_t)steps_per_batch, L);
        e = elm_query::launched([&] {
            for (; it < upto; ++it) elm::launch_lc_step(st, d, it);
        });
        if (e == hipSuccess) e = hipMemcpyAsync(&state, d.state, sizeof(elm::LcState), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess || state.stop[it & 1u] || it >= L) break;
    }
    return e;
}

} // namespace elm_loops_host
