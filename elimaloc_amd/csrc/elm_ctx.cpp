// elm_ctx.cpp -- the context behind the C ABI (include/elimaloc_hip.h): the RCCL loader and the communicator calls, the registry of
// live contexts, the environment tokens, context create / destroy, profiling switches, page-locked host memory.  Host-side C++17.
#include <dlfcn.h>
#include <hip/hip_runtime.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "elm_host_types.hpp"

using namespace elm;
using namespace elm_host;

typedef int (*nccl_get_unique_id_t)(void*);
typedef int (*nccl_comm_init_rank_t)(void**, int, struct elm_nccl_id, int);
typedef int (*nccl_all_reduce_t)(const void*, void*, size_t, int, int, void*, hipStream_t);
typedef int (*nccl_comm_destroy_t)(void*);
typedef const char* (*nccl_get_error_string_t)(int);
typedef int (*nccl_comm_query_t)(const void*, int*);
struct elm_nccl_id {
    char internal[ELM_COMM_ID_BYTES];
};

struct RcclApi {
    void* handle = nullptr;
    nccl_get_unique_id_t get_unique_id = nullptr;
    nccl_comm_init_rank_t comm_init_rank = nullptr;
    nccl_all_reduce_t all_reduce = nullptr;
    nccl_comm_destroy_t comm_destroy = nullptr;
    nccl_get_error_string_t get_error_string = nullptr;
    nccl_comm_query_t comm_count = nullptr, comm_user_rank = nullptr;
};
static RcclApi g_rccl;

static bool load_rccl(std::string* err) {
    if (g_rccl.handle) return true;
    const char* names[] = {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"};
    void* h = nullptr;
    for (const char* n : names) {
        h = dlopen(n, RTLD_NOW | RTLD_GLOBAL);
        if (h) break;
    }
    if (!h) {
        if (err) *err = std::string("cannot dlopen librccl: ") + dlerror();
        return false;
    }
    g_rccl.get_unique_id = (nccl_get_unique_id_t)dlsym(h, "ncclGetUniqueId");
    g_rccl.comm_init_rank = (nccl_comm_init_rank_t)dlsym(h, "ncclCommInitRank");
    g_rccl.all_reduce = (nccl_all_reduce_t)dlsym(h, "ncclAllReduce");
    g_rccl.comm_destroy = (nccl_comm_destroy_t)dlsym(h, "ncclCommDestroy");
    g_rccl.get_error_string = (nccl_get_error_string_t)dlsym(h, "ncclGetErrorString");
    g_rccl.comm_count = (nccl_comm_query_t)dlsym(h, "ncclCommCount");
    g_rccl.comm_user_rank = (nccl_comm_query_t)dlsym(h, "ncclCommUserRank");
    if (!g_rccl.get_unique_id || !g_rccl.comm_init_rank || !g_rccl.all_reduce || !g_rccl.comm_destroy) {
        if (err) *err = "librccl lacks ncclGetUniqueId/ncclCommInitRank/ncclAllReduce/ncclCommDestroy";
        return false;
    }
    g_rccl.handle = h;
    return true;
}

// Contexts that are alive.  Maps and scans hold a pointer to their context; destroying the context first is legal (e.g. Python
// object finalisation order): a child destroyed later finds its context gone and only releases its own device memory.
// A child remembers the context's unique id: a NEW context that happens to be allocated at a destroyed context's address (possibly on
// another device) is not its owner.
static std::mutex g_live_mu;
static std::map<const elm_ctx*, uint64_t> g_live_ctx;
static uint64_t g_next_ctx_id = 1;
bool elm_host::ctx_alive(const elm_ctx* ctx, uint64_t id) {
    std::lock_guard<std::mutex> lk(g_live_mu);
    auto it = g_live_ctx.find(ctx);
    return it != g_live_ctx.end() && it->second == id;
}

// The library's run-time switches are FIVE environment variables (include/elimaloc_hip.h lists them): ELM_KERNEL, ELM_GRID, ELM_CHECK,
// ELM_SCAN_ORDER, ELM_GROUP_EXCHANGE.  ELM_GRID and ELM_CHECK hold comma-separated tokens, `name` or `name=value`.
bool elm_host::env_token(const char* var, const char* name, const char** value) {
    const char* e = getenv(var);
    if (!e) return false;
    const size_t ln = strlen(name);
    for (const char* p = e; *p;) {
        const char* q = strchr(p, ',');
        const size_t len = q ? (size_t)(q - p) : strlen(p);
        if (len >= ln && strncmp(p, name, ln) == 0 && (len == ln || p[ln] == '=')) {
            if (value) *value = (len > ln) ? p + ln + 1 : "";
            return true;
        }
        if (!q) break;
        p = q + 1;
    }
    return false;
}
bool elm_host::check_mode(const char* name) { return env_token("ELM_CHECK", name); } // the in-product checkers of the fast forms (tests)

extern "C" const char* elm_strerror(int status) {
    switch (status) {
    case ELM_OK: return "ok";
    case ELM_ERR_INVALID: return "invalid argument";
    case ELM_ERR_DEVICE: return "HIP runtime error";
    case ELM_ERR_NO_DEVICE: return "no usable gfx950 device";
    case ELM_ERR_COMM: return "RCCL error";
    case ELM_ERR_UNSUPPORTED: return "unsupported configuration";
    case ELM_ERR_IO: return "file missing or unreadable";
    case ELM_ERR_ALLOC: return "host allocation failed";
    default: return "unknown status";
    }
}

extern "C" void elm_reg_config_default(elm_reg_config* c) {
    // config/localization.ini:80-105
    memset(c, 0, sizeof(*c));
    c->i_max_thread = 10;
    c->icp_method = ELM_GICP;
    c->voxel_search_method = 2;
    c->use_radar_cov = 0;
    c->max_iteration = 10;
    c->b_debug_print = 0;
    c->gicp_cov_search_dist = 0.4;
    c->max_search_dist = 5.0;
    c->lm_lambda = 0.5;
    c->icp_termination_threshold_m = 0.02;
    c->min_overlap_ratio = 0.4;
    c->max_fitness_score = 0.5;
    c->doppler_trans_lambda = 0.5;
    c->range_variance_m = 1.0;
    c->azimuth_variance_deg = 0.4;
    c->elevation_variance_deg = 0.4;
    for (int i = 0; i < 3; ++i) c->ego_to_lidar_rot[i * 4] = c->ego_to_imu_rot[i * 4] = 1.0;
}

extern "C" int elm_ctx_create(int device_id, elm_ctx** out) {
    if (!out) return ELM_ERR_INVALID;
    *out = nullptr;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return ELM_ERR_NO_DEVICE;
    if (device_id < 0 || device_id >= count) return ELM_ERR_INVALID;
    hipDeviceProp_t prop;
    if (hipGetDeviceProperties(&prop, device_id) != hipSuccess) return ELM_ERR_NO_DEVICE;
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) return ELM_ERR_NO_DEVICE; // kernels are built for gfx950 only
    elm_ctx* ctx = new elm_ctx();
    ctx->device = device_id;
    if (hipSetDevice(device_id) != hipSuccess || hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) {
        delete ctx;
        return ELM_ERR_DEVICE;
    }
    if (const char* k = getenv("ELM_KERNEL")) ctx->kernel_mode = (strcmp(k, "direct") == 0) ? 2 : (strcmp(k, "lists") == 0) ? 3 : 4;
    if (const char* o = getenv("ELM_SCAN_ORDER")) ctx->scan_order = (strcmp(o, "none") == 0) ? 0 : 1;
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        ctx->id = g_next_ctx_id++;
        g_live_ctx[ctx] = ctx->id;
    }
    *out = ctx;
    return ELM_OK;
}

extern "C" void elm_ctx_destroy(elm_ctx* ctx) {
    if (!ctx) return;
    if (ctx->group && !elm_multi::in_worker()) { // the group first: its workers, communicators and the other ranks' contexts
        elm_group* g = ctx->group;
        elm_multi::destroy(g); // (clears ctx->group)
    }
    {
        std::lock_guard<std::mutex> lk(g_live_mu);
        if (!g_live_ctx.erase(ctx)) return; // not a live context (double destroy)
    }
    (void)hipSetDevice(ctx->device);
    if (ctx->stream) (void)hipStreamSynchronize(ctx->stream);
    if (ctx->comm && g_rccl.comm_destroy) g_rccl.comm_destroy(ctx->comm);
    for (hipStream_t st : {ctx->copy_stream, ctx->order_stream, ctx->poll_stream})
        if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
    for (hipEvent_t e : {ctx->ev_iter[0], ctx->ev_iter[1], ctx->ev_iter[2], ctx->ev_iter[3]})
        if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ctx->ev_groups) (void)hipEventDestroy(e);
    if (ctx->d_hilbert) (void)hipFree(ctx->d_hilbert);
    if (ctx->h_jobs) (void)hipHostFree(ctx->h_jobs);
    DevBuf* bufs[] = {&ctx->d_scans, &ctx->d_state, &ctx->d_partials, &ctx->d_sums, &ctx->d_T0, &ctx->d_trace, &ctx->d_stage_pts, &ctx->d_active, &ctx->d_queue, &ctx->d_ds,
                      &ctx->d_order_jobs, &ctx->d_order_tmp, &ctx->d_arena, &ctx->d_raw, &ctx->d_flagged, &ctx->d_asym, &ctx->d_q0, &ctx->d_q1, &ctx->d_q2, &ctx->d_q3, &ctx->d_q4, &ctx->d_q5};
    if (ctx->h_active) (void)hipHostFree(ctx->h_active);
    for (DevBuf* b : bufs)
        if (b->p) (void)hipFree(b->p);
    for (DevBuf& b : ctx->d_reloc)
        if (b.p) (void)hipFree(b.p);
    for (auto& b : ctx->scan_pool) (void)hipFree(b.first);
    for (elm_scan* f : ctx->scan_free) delete f;
    if (ctx->h_state) (void)hipHostFree(ctx->h_state);
    if (ctx->h_trace) (void)hipHostFree(ctx->h_trace);
    if (ctx->h_stage) (void)hipHostFree(ctx->h_stage);
    if (ctx->h_desc) (void)hipHostFree(ctx->h_desc);
    for (hipEvent_t e : ctx->events) (void)hipEventDestroy(e);
    if (ctx->stream) (void)hipStreamDestroy(ctx->stream);
    delete ctx;
}

extern "C" const char* elm_last_error(const elm_ctx* ctx) { return ctx ? ctx->last_error.c_str() : ""; }
extern "C" void* elm_ctx_stream(elm_ctx* ctx) { return ctx ? (void*)ctx->stream : nullptr; }
extern "C" int elm_ctx_set_work_counters(elm_ctx* ctx, int enable) {
    if (!ctx) return ELM_ERR_INVALID;
    if (ctx->in_flight) return ELM_ERR_INVALID;
    if (group_call(ctx)) return elm_multi::set_work_counters(ctx, enable); // every rank: the counters ride in the exchanged record
    ctx->work_counters = enable != 0;
    return ELM_OK;
}

extern "C" int elm_ctx_set_profiling(elm_ctx* ctx, int enable) {
    if (!ctx) return ELM_ERR_INVALID;
    ctx->profiling = enable != 0;
    return ELM_OK;
}
extern "C" int elm_ctx_get_profile(elm_ctx* ctx, elm_profile* out, int reset) {
    if (!ctx || !out) return ELM_ERR_INVALID;
    *out = ctx->prof;
    if (reset) ctx->prof = elm_profile{};
    return ELM_OK;
}
extern "C" int elm_ctx_synchronize(elm_ctx* ctx) {
    if (!ctx) return ELM_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ELM_OK;
}

int elm_host::exchange(elm_ctx* ctx, double* d_sums, size_t count, hipStream_t stream) {
    if (!stream) stream = ctx->stream;
    if (ctx->hook) {
        int rc = ctx->hook(d_sums, count, (void*)stream, ctx->hook_user);
        if (rc != 0) {
            ctx->last_error = "allreduce hook failed";
            return ELM_ERR_COMM;
        }
        return ELM_OK;
    }
    if (ctx->comm) {
        // ONE sum all-reduce of the packed normal equations of the whole batch per ICP iteration
        int rc = g_rccl.all_reduce(d_sums, d_sums, count, /*ncclDouble*/ 8, /*ncclSum*/ 0, ctx->comm, stream);
        if (rc != 0) {
            ctx->last_error = std::string("ncclAllReduce: ") + (g_rccl.get_error_string ? g_rccl.get_error_string(rc) : "error");
            return ELM_ERR_COMM;
        }
    }
    return ELM_OK;
}

extern "C" void* elm_host_alloc(size_t bytes) {
    void* p = nullptr;
    if (hipHostMalloc(&p, std::max<size_t>(bytes, 64), hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
extern "C" void elm_host_free(void* p) {
    if (p) (void)hipHostFree(p);
}

// Diagnostic for the benches: what one plain hipMemcpyAsync of `bytes` from `host` achieves on this box (median of reps), i.e.
// the PCIe rate a host-fed stream sits under.
extern "C" int elm_ctx_measure_h2d(elm_ctx* ctx, const void* host, size_t bytes, int reps, double* gb_per_s) {
    if (!ctx || !host || !bytes || reps <= 0 || !gb_per_s) return ELM_ERR_INVALID;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    int rc = dev_reserve(ctx, ctx->d_arena, bytes);
    if (rc != ELM_OK) return rc;
    hipEvent_t a, b;
    HIPCHK(ctx, hipEventCreate(&a));
    HIPCHK(ctx, hipEventCreate(&b));
    std::vector<float> ms;
    hipError_t e = hipSuccess;
    for (int r = 0; r < reps + 1 && e == hipSuccess; ++r) { // the first copy warms the path up
        e = hipEventRecord(a, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_arena.p, host, bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) e = hipEventRecord(b, ctx->stream);
        if (e == hipSuccess) e = hipEventSynchronize(b);
        float t = 0.f;
        if (e == hipSuccess) e = hipEventElapsedTime(&t, a, b);
        if (r) ms.push_back(t);
    }
    (void)hipEventDestroy(a);
    (void)hipEventDestroy(b);
    if (e != hipSuccess) {
        ctx->last_error = std::string("h2d probe: ") + hipGetErrorString(e);
        return ELM_ERR_DEVICE;
    }
    std::sort(ms.begin(), ms.end());
    *gb_per_s = (double)bytes / ((double)ms[ms.size() / 2] * 1e-3) / 1e9;
    return ELM_OK;
}

// what the other host units ask of a context (elm_hostapi.hpp)
namespace elm_host {
void ctx_set_error(elm_ctx* ctx, const std::string& text) { if (ctx) ctx->last_error = text; }
void* ctx_reloc_scratch(elm_ctx* ctx, ScratchSlot slot, size_t bytes, int* rc) {
    *rc = dev_reserve(ctx, ctx->d_reloc[slot], bytes);
    return *rc == ELM_OK ? ctx->d_reloc[slot].p : nullptr;
}
bool ctx_is_alive(const elm_ctx* ctx, uint64_t id) { return ctx_alive(ctx, id); }
int free_space_form() { return check_mode("free_wave") ? 1 : 0; }
int ray_pose_block(int dflt) {
    const char* v = nullptr;
    if (!env_token("ELM_CHECK", "ray_poses", &v) || !v) return dflt;
    const int b = atoi(v);
    return b >= 1 && b <= elm::kRayMaxPoses ? b : dflt;
}
} // namespace elm_host

// ------------------------------------------------------------------------------------------------------
// multi-GPU
// ------------------------------------------------------------------------------------------------------
extern "C" int elm_comm_get_unique_id(void* id_bytes) {
    if (!id_bytes) return ELM_ERR_INVALID;
    std::string err;
    if (!load_rccl(&err)) return ELM_ERR_COMM;
    return g_rccl.get_unique_id(id_bytes) == 0 ? ELM_OK : ELM_ERR_COMM;
}

extern "C" int elm_comm_init(elm_ctx* ctx, int rank, int nranks, const void* id_bytes) {
    if (!ctx || !id_bytes || nranks < 1 || rank < 0 || rank >= nranks) return ELM_ERR_INVALID;
    if (group_call(ctx)) { ctx->last_error = "elm_comm_init: a device group exchanges among its own ranks"; return ELM_ERR_INVALID; }
    if (!load_rccl(&ctx->last_error)) return ELM_ERR_COMM;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    elm_nccl_id id;
    memcpy(id.internal, id_bytes, ELM_COMM_ID_BYTES);
    void* comm = nullptr;
    int rc = g_rccl.comm_init_rank(&comm, nranks, id, rank);
    if (rc != 0) {
        ctx->last_error = std::string("ncclCommInitRank: ") + (g_rccl.get_error_string ? g_rccl.get_error_string(rc) : "error");
        return ELM_ERR_COMM;
    }
    ctx->comm = comm;
    ctx->rank = rank;
    ctx->nranks = nranks;
    return ELM_OK;
}

extern "C" int elm_comm_destroy(elm_ctx* ctx) {
    if (!ctx) return ELM_ERR_INVALID;
    if (ctx->comm && g_rccl.comm_destroy) g_rccl.comm_destroy(ctx->comm);
    ctx->comm = nullptr;
    ctx->nranks = 1;
    ctx->rank = 0;
    return ELM_OK;
}

// What the COMMUNICATOR says about itself (ncclCommCount / ncclCommUserRank), not what the caller passed to elm_comm_init: the benches
// print it so that a run labelled N GPUs is known to have formed an N-rank RCCL communicator.  No communicator: 0 ranks.
extern "C" int elm_comm_info(elm_ctx* ctx, int* rank, int* nranks) {
    if (!ctx || !rank || !nranks) return ELM_ERR_INVALID;
    *rank = 0;
    *nranks = 0;
    if (!ctx->comm) return ELM_OK;
    if (!g_rccl.comm_count || !g_rccl.comm_user_rank) {
        ctx->last_error = "librccl lacks ncclCommCount / ncclCommUserRank";
        return ELM_ERR_COMM;
    }
    int rc = g_rccl.comm_count(ctx->comm, nranks);
    if (rc == 0) rc = g_rccl.comm_user_rank(ctx->comm, rank);
    if (rc != 0) {
        ctx->last_error = std::string("ncclCommCount: ") + (g_rccl.get_error_string ? g_rccl.get_error_string(rc) : "error");
        return ELM_ERR_COMM;
    }
    return ELM_OK;
}

extern "C" int elm_comm_set_hook(elm_ctx* ctx, elm_allreduce_fn fn, void* user) {
    if (!ctx) return ELM_ERR_INVALID;
    ctx->hook = fn;
    ctx->hook_user = user;
    return ELM_OK;
}
