// elm_loops_host.hpp -- what the two loop consistency calls share on the host (elm_loops.cpp, elm_loopcov.cpp) beyond the call skeleton
// of elm_call.hpp: the limit on the poses, the greedy arrays' carving and reset, and the greedy loop as a run_batched of steps_per_batch
// steps between two reads of the device's state.  Host-side C++17, everything inline.
#pragma once
#include <hip/hip_runtime.h>

#include <vector>

#include "elm_dev_loops.hpp"
#include "elm_query.hpp"

namespace elm_loops_host {

using elm_query::Carver;

constexpr size_t kLcMaxPoses = (size_t)1 << 20;

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
    return elm_query::run_batched(
        st, steps_per_batch, d.L, [&](uint32_t it) { elm::launch_lc_step(st, d, it); }, (const elm::LcState*)d.state, &state,
        [&](uint32_t it) { return state.stop[it & 1u] != 0; });
}

} // namespace elm_loops_host
