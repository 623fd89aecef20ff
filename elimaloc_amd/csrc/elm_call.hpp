// elm_call.hpp -- the skeleton of a host call, in this file (elm_query.hpp includes it and adds what only the map queries share): who
// may call (check_plain, check_call), the body on the context's stream under the host-allocation guard (guard_alloc, on_stream), what the
// launches and the stream say (launched, join, dev_error), the one device allocation of a call (DeviceBlob on elm_carve.hpp's Carver),
// the marks of a call on its stream (StreamEvents), the loop that queues a batch of steps between two reads of the device's state
// (run_batched) and the refusal of a full object (refuse_full).  Host-side C++17, everything inline.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <new>
#include <string>

#include "elm_carve.hpp"
#include "elm_host_types.hpp"

namespace elm_query {

using elm_carve::carved_size;
using elm_carve::Carver;

// one rank, no exchange: a device group's lead or a context with a communicator / hook attached is refused
inline int check_plain(elm_ctx* ctx, const char* what) {
    if ((ctx->group && !elm_multi::in_worker()) || ctx->comm || ctx->hook) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": one rank only (not on a device group, nor with a communicator or hook attached)");
        return ELM_ERR_UNSUPPORTED;
    }
    return ELM_OK;
}
// a call without an object: one rank, and no batch in flight (the context's stream and scratch belong to it)
inline int check_call(elm_ctx* ctx, const char* what) {
    const int rc = check_plain(ctx, what);
    if (rc != ELM_OK) return rc;
    return ctx->in_flight ? ELM_ERR_INVALID : ELM_OK;
}

inline int dev_error(elm_ctx* ctx, const char* what, hipError_t e) {
    elm_host::ctx_set_error(ctx, std::string(what) + ": " + hipGetErrorString(e));
    return ELM_ERR_DEVICE;
}

// the refusal of n items more than an object of capacity cap, holding have, can take
inline int refuse_full(elm_ctx* ctx, const char* what, const char* items, size_t have, size_t n, size_t cap) {
    elm_host::ctx_set_error(ctx, std::string(what) + ": " + std::to_string(have) + " + " + std::to_string(n) + " " + items + " exceed the capacity of " +
                                     std::to_string(cap));
    return ELM_ERR_UNSUPPORTED;
}

// body(), with a failed host allocation turned into ELM_ERR_ALLOC
template <class Body>
int guard_alloc(elm_ctx* ctx, const char* what, Body body) {
    try {
        return body();
    } catch (const std::bad_alloc&) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": host allocation failed");
        return ELM_ERR_ALLOC;
    }
}

// The device work of an entry point: the context's device current, body(stream) on the context's stream, a failed host allocation
// anywhere in it turned into ELM_ERR_ALLOC.
template <class Body>
int on_stream(elm_ctx* ctx, const char* what, Body body) {
    return guard_alloc(ctx, what, [&]() -> int {
        if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
        return body((hipStream_t)elm_ctx_stream(ctx));
    });
}

// launch(), and what its launches say: an error left behind by an earlier call is dropped first
template <class Launch>
hipError_t launched(Launch launch) {
    (void)hipGetLastError();
    launch();
    return hipGetLastError();
}

// the stream joined unless e already holds a failure; the call's return code
inline int join(elm_ctx* ctx, hipStream_t st, hipError_t e, const char* what) {
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? (int)ELM_OK : dev_error(ctx, what, e);
}

// The one device allocation of a call, released when the call ends however it ends: the stream is joined first, so nothing queued still
// reads or writes it.  alloc(carve) is the size pass, the hipMalloc and the real pass of carve(Carver&); its error is the hipMalloc's.
struct DeviceBlob {
    char* p = nullptr;
    size_t bytes = 0;
    hipStream_t st;
    explicit DeviceBlob(hipStream_t stream) : st(stream) {}
    DeviceBlob(const DeviceBlob&) = delete;
    DeviceBlob& operator=(const DeviceBlob&) = delete;
    ~DeviceBlob() {
        if (!p) return;
        (void)hipStreamSynchronize(st);
        (void)hipFree(p);
    }
    template <class F>
    hipError_t alloc(F carve) {
        bytes = carved_size(carve);
        const hipError_t e = hipMalloc((void**)&p, bytes);
        if (e != hipSuccess) {
            p = nullptr;
            return e;
        }
        Carver real{p};
        carve(real);
        return hipSuccess;
    }
    char* release() { // the allocation leaves with an owner that outlives the call
        char* q = p;
        p = nullptr;
        return q;
    }
};

// Up to N marks of a call on its stream, each event created when it is recorded.  ms(k) is the time between marks k and k + 1; a mark
// that was never made (or past the N-th) reads as 0.0 ms.  Read after the stream has been joined.
template <int N>
struct StreamEvents {
    hipEvent_t ev[N] = {};
    int n = 0;
    StreamEvents() = default;
    StreamEvents(const StreamEvents&) = delete;
    StreamEvents& operator=(const StreamEvents&) = delete;
    ~StreamEvents() {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t mark(hipStream_t st) {
        if (n >= N) return hipSuccess;
        hipError_t e = hipEventCreate(&ev[n]);
        if (e == hipSuccess) e = hipEventRecord(ev[n], st);
        ++n;
        return e;
    }
    double ms(int k) const {
        float f = 0.0f;
        return (k >= 0 && k + 1 < n && ev[k] && ev[k + 1] && hipEventElapsedTime(&f, ev[k], ev[k + 1]) == hipSuccess) ? (double)f : 0.0;
    }
};

// The batched device loop: queue(it) for per_batch steps (the last batch ends at max_steps), one copy of the device's state *d_state
// into *h_state, the stream joined, then stopped(it) on that state -- it being the number of steps queued so far -- or it >= max_steps
// ends it.  One copy and one join per batch; *h_state holds the device's state when it returns hipSuccess.
template <class State, class Queue, class Stopped>
hipError_t run_batched(hipStream_t st, int64_t per_batch, int64_t max_steps, Queue queue, const State* d_state, State* h_state, Stopped stopped) {
    hipError_t e = hipSuccess;
    uint32_t it = 0;
    while (e == hipSuccess) {
        const uint32_t upto = (uint32_t)std::min<int64_t>((int64_t)it + per_batch, max_steps);
        e = launched([&] {
            for (; it < upto; ++it) queue(it);
        });
        if (e == hipSuccess) e = hipMemcpyAsync(h_state, d_state, sizeof(State), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess || stopped(it) || it >= (uint32_t)max_steps) break;
    }
    return e;
}

} // namespace elm_query
