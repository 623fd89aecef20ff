// elm_build.cpp -- the device map build (include/elimaloc_hip.h, "device map build"): the argument checks, the
// scratch arrays, the stages of elm_k_build.hip queued on the context's stream with the few read-backs that size what follows (kept base
// points, voxels, kept points), the stage times (elm_call.hpp's StreamEvents), and the hand-over of the finished arrays to a map handle
// (elm_host::map_adopt).  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_query;

namespace {

constexpr uint64_t kBuildMaxPoints = 0x7FFFFFFFull; // 32-bit indices with all ones as "no point"

// device arrays of one call: released at its end unless handed on
struct Scratch {
    std::vector<void*> ptrs;
    Scratch() { ptrs.reserve(32); }
    ~Scratch() {
        for (void* p : ptrs)
            if (p) (void)hipFree(p);
    }
    template <class T>
    hipError_t get(T** p, size_t count) {
        void* q = nullptr;
        const hipError_t e = hipMalloc(&q, std::max<size_t>(count * sizeof(T), 256));
        if (e == hipSuccess) ptrs.push_back(q); // (room reserved: no allocation here)
        *p = (T*)q;
        return e;
    }
    void* hand_on(void* p) { // the array leaves with its new owner
        for (void*& q : ptrs)
            if (q == p) q = nullptr;
        return p;
    }
};

// the stage times of this thread's last successful build
thread_local uint64_t t_stage_ctx = 0;
thread_local bool t_stage_valid = false;
thread_local double t_stage_ms[ELM_BUILD_STAGES];

// what was queued has run: the first error of the launches or of the stream
hipError_t join(hipStream_t st) {
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
}
hipError_t read_word(hipStream_t st, const unsigned* d_word, unsigned* out) {
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_word, sizeof(unsigned), hipMemcpyDeviceToHost, st);
    return e == hipSuccess ? hipStreamSynchronize(st) : e;
}

// Who fills d_pos (the kept stored points of base) and d_in + K (the new points): the host's arrays (elm_map_build_device: drop bytes
// and xyz go up), or the device's own producers (elm_map_build_device_from: the sphere and the job table).  n: the new points.
struct BuildInput {
    const char* what = "elm_map_build_device";
    const uint8_t* drop = nullptr; // host
    const float* xyz = nullptr;    // host
    size_t n = 0;
    bool within = false; // device: keep the stored points inside the sphere
    double center[3] = {0.0, 0.0, 0.0}, r2 = 0.0;
    const JobTable* jobs = nullptr; // device: the new points are the jobs' scans at their poses (n = jobs->beams)
    elm_build_sources_stats* stats = nullptr;
};

int build_impl(elm_ctx* ctx, const elm_map* base, const BuildInput& in, double vs, int cap, elm_map** out) {
    const char* what = in.what;
    const uint8_t* drop = in.drop;
    const size_t n = in.n;
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    (void)hipGetLastError(); // drop stale errors of other libraries
    Scratch sc;
    StreamEvents<ELM_BUILD_STAGES + 1> evs; // a mark before the first stage and one after each
    unsigned* d_total = nullptr;            // [0] a scan's sum, [1] the kernels' flags
    hipError_t e = sc.get(&d_total, 2);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    unsigned* d_flags = d_total + 1;

    // ---- the input: base's kept points in bucket order, then xyz
    const unsigned n_base = base ? base->dm.n_pts : 0u;
    unsigned K = n_base;
    unsigned* d_pos = nullptr;
    uint8_t* d_drop = nullptr;
    e = evs.mark(st);
    if (e == hipSuccess && (drop || in.within) && n_base) {
        unsigned* d_blk = nullptr;
        if (drop) e = sc.get(&d_drop, n_base);
        if (e == hipSuccess) e = sc.get(&d_pos, n_base);
        if (e == hipSuccess) e = sc.get(&d_blk, (size_t)n_base / 1024 + 1);
        if (e == hipSuccess && drop) e = hipMemcpyAsync(d_drop, drop, n_base, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) {
            if (drop) launch_bd_keep(st, d_drop, n_base, d_pos);
            else launch_bd_keep_within(st, base->dm.pts, n_base, in.center, in.r2, d_pos);
            launch_bd_scan(st, d_pos, n_base, d_blk, d_total);
            e = read_word(st, d_total, &K);
        }
    }
    if (e != hipSuccess) return dev_error(ctx, what, e);
    if ((uint64_t)K + n > kBuildMaxPoints) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": more than 2^31 - 1 input points");
        return ELM_ERR_UNSUPPORTED;
    }
    const unsigned N = K + (unsigned)n;
    Pt3* d_in = nullptr;
    e = sc.get(&d_in, N);
    if (e == hipSuccess && K) launch_bd_compact(st, base->dm.pts, d_drop, d_pos, n_base, K, d_in);
    std::vector<uint32_t> pt0; // (read by the copy until the stream is joined)
    if (e == hipSuccess && n && in.jobs) {
        const size_t n_jobs = in.jobs->jobs.size();
        EvidJob* d_jobs = nullptr;
        uint32_t* d_pt0 = nullptr;
        pt0.resize(n_jobs);
        uint32_t first = 0;
        for (size_t j = 0; j < n_jobs; ++j) {
            pt0[j] = first;
            first += in.jobs->jobs[j].n;
        }
        e = sc.get(&d_jobs, n_jobs);
        if (e == hipSuccess) e = sc.get(&d_pt0, n_jobs);
        if (e == hipSuccess) e = hipMemcpyAsync(d_jobs, in.jobs->jobs.data(), n_jobs * sizeof(EvidJob), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = hipMemcpyAsync(d_pt0, pt0.data(), n_jobs * sizeof(uint32_t), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) launch_bd_transform(st, d_jobs, (uint32_t)n_jobs, (uint32_t)in.jobs->chunks, d_pt0, d_in + K);
    } else if (e == hipSuccess && n) {
        e = hipMemcpyAsync(d_in + K, in.xyz, n * sizeof(Pt3), hipMemcpyHostToDevice, st); // (Pt3 is three packed floats)
    }
    if (e == hipSuccess) e = evs.mark(st);
    if (e != hipSuccess) return dev_error(ctx, what, e);

    // ---- stage 1: keys into a scratch table sized for one voxel per point at load <= 0.5
    unsigned cap_log2 = 1;
    while (((uint64_t)1 << cap_log2) < 2 * (uint64_t)N) ++cap_log2;
    const size_t T = (size_t)1 << cap_log2;
    unsigned long long* d_table = nullptr;
    unsigned *d_first = nullptr, *d_slot_vid = nullptr, *d_slot = nullptr, *d_key[2] = {nullptr, nullptr}, *d_val[2] = {nullptr, nullptr},
             *d_blk = nullptr, *d_hist = nullptr;
    const size_t hist_words = bd_rx_hist_words(N);
    e = sc.get(&d_table, T);
    if (e == hipSuccess) e = sc.get(&d_first, T);
    if (e == hipSuccess) e = sc.get(&d_slot_vid, T);
    if (e == hipSuccess) e = sc.get(&d_slot, N);
    for (int k = 0; k < 2 && e == hipSuccess; ++k) {
        e = sc.get(&d_key[k], N);
        if (e == hipSuccess) e = sc.get(&d_val[k], N);
    }
    if (e == hipSuccess) e = sc.get(&d_blk, std::max<size_t>(N, hist_words) / 1024 + 1); // the longest array scanned below
    if (e == hipSuccess) e = sc.get(&d_hist, hist_words);
    if (e == hipSuccess) e = hipMemsetAsync(d_table, 0xFF, T * sizeof(unsigned long long), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_first, 0xFF, T * sizeof(unsigned), st);
    if (e == hipSuccess) e = hipMemsetAsync(d_total, 0, 2 * sizeof(unsigned), st);
    unsigned flags = 0;
    if (e == hipSuccess && N) {
        launch_bd_insert(st, d_in, N, vs, d_table, d_first, cap_log2, d_slot, d_flags);
        e = read_word(st, d_flags, &flags);
    }
    if (e == hipSuccess) e = evs.mark(st);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    if (flags & kBdBadInput) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": an input coordinate is not finite, or |x / voxel_size| >= 2^20 (the packed key has 21 bits per axis)");
        return ELM_ERR_UNSUPPORTED;
    }
    if (flags & kBdTableFull) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": the scratch key table is full");
        return ELM_ERR_DEVICE;
    }

    // ---- stage 2: voxel ids in first-seen order
    unsigned n_vox = 0;
    if (N) {
        launch_bd_opens(st, d_first, d_slot, N, d_key[1]);
        launch_bd_scan(st, d_key[1], N, d_blk, d_total);
        e = read_word(st, d_total, &n_vox);
    }
    if (e == hipSuccess) e = evs.mark(st);
    // ---- stage 3: the sort's input, raw counts and group starts
    int32_t* d_keys = nullptr; // (the map's)
    unsigned *d_off = nullptr, *d_kcnt = nullptr, *d_kstart = nullptr;
    if (e == hipSuccess) e = sc.get(&d_keys, (size_t)n_vox * 3);
    if (e == hipSuccess) e = sc.get(&d_off, n_vox);
    if (e == hipSuccess) e = sc.get(&d_kcnt, n_vox);
    if (e == hipSuccess) e = sc.get(&d_kstart, n_vox);
    if (e == hipSuccess && n_vox) e = hipMemsetAsync(d_off, 0, (size_t)n_vox * sizeof(unsigned), st);
    if (e == hipSuccess && N) {
        launch_bd_vid(st, d_first, d_slot, N, d_key[1], d_table, d_slot_vid, d_keys, d_key[0], d_val[0], d_off);
        launch_bd_scan(st, d_off, n_vox, d_blk, d_total);
    }
    if (e == hipSuccess) e = evs.mark(st);
    // ---- stage 4: the indices grouped by voxel id, input order inside a group: as many 8-bit passes as the ids have digits
    int cur = 0;
    if (e == hipSuccess && n_vox > 1) {
        unsigned bits = 0;
        while (bits < 32 && ((uint64_t)1 << bits) < n_vox) ++bits;
        for (unsigned shift = 0; shift < bits; shift += 8, cur ^= 1) {
            launch_bd_rx_hist(st, d_key[cur], N, shift, d_hist);
            launch_bd_scan(st, d_hist, (unsigned)hist_words, d_blk, d_total);
            launch_bd_rx_scatter(st, d_key[cur], d_val[cur], N, shift, d_hist, d_key[cur ^ 1], d_val[cur ^ 1]);
        }
    }
    if (e == hipSuccess) e = evs.mark(st);
    // ---- stage 5: the replay
    unsigned n_pts = 0;
    if (e == hipSuccess && n_vox) {
        const double map_resolution = sqrt(vs * vs / cap); // as build_host
        launch_bd_replay(st, d_in, d_val[cur], d_off, n_vox, N, (unsigned)cap, map_resolution, d_kcnt, d_kstart);
        launch_bd_scan(st, d_kstart, n_vox, d_blk, d_total);
        e = read_word(st, d_total, &n_pts);
    }
    if (e == hipSuccess) e = evs.mark(st);
    // ---- stage 6: the map's arrays
    float4* d_pts = nullptr;
    uint2* d_ranges = nullptr;
    if (e == hipSuccess) e = sc.get(&d_pts, n_pts);
    if (e == hipSuccess) e = sc.get(&d_ranges, n_vox);
    if (e == hipSuccess && n_vox) launch_bd_emit(st, d_in, d_val[cur], d_key[cur], d_off, d_kcnt, d_kstart, n_vox, N, d_pts, d_ranges);
    if (e == hipSuccess) e = evs.mark(st);
    if (e == hipSuccess) e = join(st);
    if (e != hipSuccess) return dev_error(ctx, what, e);
    double ms[ELM_BUILD_STAGES];
    for (int k = 0; k < ELM_BUILD_STAGES; ++k) ms[k] = evs.ms(k);
    const int rc = elm_host::map_adopt(ctx, sc.hand_on(d_pts), sc.hand_on(d_ranges), sc.hand_on(d_keys), n_pts, n_vox, N, vs, cap, out);
    if (rc == ELM_OK) {
        std::copy(ms, ms + ELM_BUILD_STAGES, t_stage_ms);
        t_stage_ctx = ctx->id;
        t_stage_valid = true;
        if (in.stats) *in.stats = elm_build_sources_stats{K, n_base - K, n, n_pts, n_vox};
    }
    return rc;
}

} // namespace

extern "C" int elm_map_build_device(elm_ctx* ctx, const elm_map* base, const uint8_t* drop, const float* xyz, size_t n, double voxel_size,
                                    int max_points_per_voxel, elm_map** out) {
    if (out) *out = nullptr;
    if (!ctx || !out || (!xyz && n) || !(voxel_size > 0.0) || max_points_per_voxel <= 0 || (drop && !base)) return ELM_ERR_INVALID;
    const int rc = check_plain(ctx, "elm_map_build_device");
    if (rc != ELM_OK) return rc;
    if ((base && base->ctx != ctx) || ctx->in_flight) return ELM_ERR_INVALID;
    if (n > kBuildMaxPoints) {
        elm_host::ctx_set_error(ctx, "elm_map_build_device: more than 2^31 - 1 input points");
        return ELM_ERR_UNSUPPORTED;
    }
    BuildInput in;
    in.drop = drop;
    in.xyz = xyz;
    in.n = n;
    return guard_alloc(ctx, "elm_map_build_device", [&] { return build_impl(ctx, base, in, voxel_size, max_points_per_voxel, out); });
}

extern "C" int elm_map_build_device_from(elm_ctx* ctx, const elm_build_sources* src, double voxel_size, int max_points_per_voxel, elm_map** out,
                                         elm_build_sources_stats* stats) {
    const char* what = "elm_map_build_device_from";
    if (out) *out = nullptr;
    if (!ctx || !src || !out || !(voxel_size > 0.0) || max_points_per_voxel <= 0) return ELM_ERR_INVALID;
    if (src->n_jobs < 0 || src->n_jobs > kEvidMaxJobs || (src->n_jobs > 0 && (!src->scans || !src->poses16))) return ELM_ERR_INVALID;
    if ((src->keep_within != 0 && src->keep_within != 1) || (src->keep_within == 1 && !src->base)) return ELM_ERR_INVALID;
    if (!finite3(src->keep_center) || !fin_ge0(src->keep_radius_m)) return ELM_ERR_INVALID;
    for (int j = 0; j < src->n_jobs; ++j)
        if (!src->scans[j]) return ELM_ERR_INVALID;
    if (!poses_finite(src->poses16, (size_t)src->n_jobs)) return ELM_ERR_INVALID;
    const int rc = check_plain(ctx, what);
    if (rc != ELM_OK) return rc;
    if ((src->base && src->base->ctx != ctx) || ctx->in_flight) return ELM_ERR_INVALID;
    for (int j = 0; j < src->n_jobs; ++j)
        if (src->scans[j]->ctx != ctx) return ELM_ERR_INVALID;
    return guard_alloc(ctx, what, [&] {
        const JobTable jobs = build_jobs(src->scans, src->poses16, (uint32_t)src->n_jobs);
        if (jobs.beams > kBuildMaxPoints) {
            elm_host::ctx_set_error(ctx, std::string(what) + ": more than 2^31 - 1 input points");
            return (int)ELM_ERR_UNSUPPORTED;
        }
        BuildInput in;
        in.what = what;
        in.n = (size_t)jobs.beams;
        in.within = src->keep_within == 1;
        std::copy(src->keep_center, src->keep_center + 3, in.center);
        in.r2 = src->keep_radius_m * src->keep_radius_m;
        in.jobs = &jobs;
        in.stats = stats;
        return build_impl(ctx, src->base, in, voxel_size, max_points_per_voxel, out);
    });
}

extern "C" int elm_map_build_device_stages(const elm_ctx* ctx, double ms[ELM_BUILD_STAGES]) {
    if (!ctx || !ms || !t_stage_valid || t_stage_ctx != ctx->id) return ELM_ERR_INVALID;
    std::copy(t_stage_ms, t_stage_ms + ELM_BUILD_STAGES, ms);
    return ELM_OK;
}
