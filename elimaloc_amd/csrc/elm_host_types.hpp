// elm_host_types.hpp -- the host-side structs behind the C ABI's opaque handles (elm_ctx, elm_map, elm_scan) and the helpers that cross the
// host translation units.  Needs HIP: units that must build without it include elm_hostapi.hpp alone.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <utility>
#include <vector>

#include "elm_hostapi.hpp"
#include "elm_internal.hpp"

struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
};

struct elm_scan {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0; // the owning context's unique id (a context allocated later at the same address is not the owner)
    elm::Pt3* d_pts = nullptr;
    size_t cap_bytes = 0;
    uint32_t n = 0, n_total = 0;
    std::vector<elm_scan*> shards; // a scan uploaded through a device GROUP (elm_ctx_create_multi): this handle is rank 0's shard, these
                                   // are the shards of ranks 1 .. N-1 (elm_multi.cpp)
};

struct elm_ctx {
    int device = 0;
    uint64_t id = 0; // unique for the life of the process (children compare ids, not pointers)
    hipStream_t stream = nullptr;
    // host-fed streams / ordered uploads: uploads (DMA) and the scan-ordering kernel run beside the iterations on the compute stream
    hipStream_t copy_stream = nullptr, order_stream = nullptr, poll_stream = nullptr;
    hipEvent_t ev_iter[4] = {nullptr, nullptr, nullptr, nullptr};
    std::vector<hipEvent_t> ev_groups; // host-fed streams: per upload group its "copied" and "ordered" events
    uint16_t* d_hilbert = nullptr; // Hilbert index of every cell of the ordering grid (kOrderCells^2 entries)
    DevBuf d_order_jobs, d_order_tmp, d_arena, d_raw, d_flagged, d_asym;
    DevBuf d_q0, d_q1, d_q2, d_q3, d_q4, d_q5; // scratch of elm_map_get_correspondences / elm_align_clouds_local (kept between calls)
    DevBuf d_reloc[elm_host::kScrCount]; // the query scratch, one buffer per ScratchSlot (elm_hostapi.hpp): relocalization and the map
                                         // queries of elm_query.hpp; kept between calls
    bool work_counters = false; // elm_ctx_set_work_counters: the accumulate launches also sum the work counters of
                                // elm_reg_result (n_cand_total, n_occ_total, n_tested_total, fallback_blocks); off: those fields read 0
    void* h_jobs = nullptr; // pinned: ordering job descriptors
    size_t h_jobs_cap = 0;
    std::string last_error;
    // scratch (grow-only; no allocation on the per-scan path after warm-up)
    DevBuf d_scans, d_state, d_partials, d_sums, d_T0, d_trace, d_stage_pts, d_active, d_queue, d_ds;
    int stream_hint_count = 0, stream_hint_slots = 0, stream_hint_iters = 0; // iterations the last elm_register_stream call of that shape needed
    int* h_active = nullptr; // pinned: number of scans still iterating, read back at the early-stop checks
    int iter_hint = 0;       // iterations the longest of the last eight batches needed (0 = unknown): first early-stop check happens there
    int iter_ring[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    unsigned iter_ring_pos = 0;
    const void* iter_key_map = nullptr; // the history belongs to ONE kind of call: (map, method, batch size); another kind starts afresh
    int iter_key_method = -1, iter_key_batch = 0;
    void* h_state = nullptr; // pinned
    size_t h_state_cap = 0;
    void* h_trace = nullptr; // pinned
    size_t h_trace_cap = 0;
    void* h_stage = nullptr; // pinned staging for synchronous uploads (scan points, deskew tables)
    size_t h_stage_cap = 0;
    std::vector<uint32_t> h_key, h_ord, h_tmp; // scratch of the scan ordering (grow-only)
    std::vector<struct elm_scan*> scan_free;   // recycled scan handles
    std::vector<std::pair<void*, size_t>> scan_pool; // device buffers of destroyed scans, reused by the next upload (a scan per
                                                     // LiDAR message: no hipMalloc / hipFree on the per-scan path after warm-up)
    void* h_desc = nullptr; // pinned staging of the batch descriptors (read by an async copy)
    size_t h_desc_cap = 0;
    // in-flight batch
    int batch = 0;
    bool want_trace = false;
    bool in_flight = false;
    void* ds_clean_ptr = nullptr;     // the downsample hash table at this address ...
    unsigned ds_clean_cap_log2 = 0;   // ... of this size is all ones (every pass cleans up the slots it touched)
    bool results_ready = false; // the last early-stop check of the in-flight batch found every scan finished: h_state holds the final states
    elm::RegParams rp{};
    int scan_order = 1;  // 1: order uploaded scans along a Hilbert curve (elm_scan_upload), 0: keep the caller's order (ELM_SCAN_ORDER=none)
    int kernel_mode = 4; // accumulate kernels: 4 = dense cell grid, or cell-indexed neighbourhood lists when the grid does not fit
                         // (P2P/GICP), voxel-mean lists (VGICP/AVGICP): the default; 3 = neighbourhood lists forced (ELM_KERNEL=lists);
                         // 2 = the plain 27-probe walk of k_accumulate_direct (ELM_KERNEL=direct: in-kernel reference for tests)
    // optional hipEvent timing
    bool profiling = false;
    bool keep_iter_ms = false;         // prof_collect also keeps every accumulate span of the call (b_debug_print: the reference's
    std::vector<double> iter_acc_ms;   // per-iteration "Total Correspondence Time for" lines)
    std::vector<hipEvent_t> events;
    int events_used = 0;
    elm_profile prof{};
    // exchange
    void* comm = nullptr;
    int rank = 0, nranks = 1;
    elm_allreduce_fn hook = nullptr;
    void* hook_user = nullptr;
    int path = 0; // ELM_PATH_* of the registration call in progress (elm_reg_result.path)
    elm_group* group = nullptr; // elm_ctx_create_multi: this context LEADS a group of per-device contexts inside this process (elm_multi.cpp);
                                // maps built and scans uploaded through it are replicated / sharded over the group, registrations run on all
};

struct elm_map {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0;
    std::vector<elm_map*> replicas; // built through a device group: the same map on the devices of ranks 1 .. N-1 (this one is rank 0's)
    elm_map_info info{};
    elm::DevMap dm{};
    elm::HashSlot* d_slots = nullptr;
    float4* d_pts = nullptr;
    uint2* d_ranges = nullptr;
    int32_t* d_keys = nullptr; // [n_vox][3] stored keys (for downloads)
    double *d_vox_mean = nullptr, *d_vox_cov = nullptr, *d_vox_cinv = nullptr, *d_vox_nk = nullptr;
    unsigned* d_bad = nullptr;     // covariances outside the compact form I + k n n^T (counted by the covariance kernels)
    double* d_grid_gicp8 = nullptr; // the compact GICP records in grid slot order
    double* d_pt_gicp = nullptr; // [n_pts][16]: mean, inverse covariance, fitness normal (DevMap::pt_gicp)
    double* d_pt_cov = nullptr;  // [n_pts][9]: the covariances themselves (Pointcloud() read-back only)
    elm::HashSlot* d_qslots = nullptr;
    elm::Pt3* d_nbr_pts = nullptr;
    uint32_t* d_nbr_idx = nullptr;
    uint16_t* d_nbr_cell_off = nullptr;
    elm::HashSlot* d_vqslots = nullptr;
    uint32_t* d_vq_dense = nullptr;
    uint32_t* d_vqf_dense = nullptr;
    elm::VoxRec* d_vox_rec = nullptr;   // [n_vox] (DevMap::vox_rec)
    elm::VoxBlk* d_vnbr_blk = nullptr;
    elm::VoxRec* d_vface = nullptr;
    elm::GridBlk* d_grid_blk = nullptr;    // dense cell grid (DevMap::grid_*), the default P2P / GICP search index
    uint32_t* d_grid_idx = nullptr;
    uint32_t* d_grid_start = nullptr;
    uint2* d_grid_tiles = nullptr; // two-level grid only
    uint32_t* d_vox_stat = nullptr;
    double* d_grid_gicp = nullptr; // the GICP records in grid slot order (built with the grid / refreshed by CalPointCovAll)
    size_t grid_slots = 0;
    uint64_t grid_start_words = 0; // words of d_grid_start: entries + 4
    bool has_grid = false;
    bool want_gicp_compact = false; // the grid gets 64-byte GICP records (points outside the compact form are flagged and read pt_gicp)
    unsigned n_bad_pts = 0, n_bad_vox = 0; // covariances outside the compact form (diagnostics)
    unsigned n_asym_pts = 0, n_asym_vox = 0; // ... of which the stored inverse is not symmetric: such a map carries side records (choose_path)
    bool grid_refused = false; // the bounding box needs more cells than the budget: neighbourhood lists instead
    int index_build = 0;       // elm_map_set_index_build: who lays the cell grid out (ELM_INDEX_BUILD_HOST / _DEVICE)
    double index_stage_ms[5] = {0.0, 0.0, 0.0, 0.0, 0.0}; // the device producer's stages (elm_map_index_build_stages)
    bool warned_slow_path = false; // choose_path has said that this map's covariance methods run the per-pair kernels
    bool has_vnbr = false; // voxel-mean lists (VGICP / AVGICP)
    bool has_vface = false, vface_refused = false; // AVGICP's face sublists (built at the first AVGICP call; refused: no dense table / too many records)
    bool has_cells = false; // lists sorted by half-voxel cell + offset tables (every list <= 1024 entries)
    bool has_nbr = false;
    std::vector<int32_t> h_keys;
    std::vector<uint2> h_ranges;
    // the ground field's 2-D bin index (elm_map_ground_heights; built at its first call) and the xy bounds of the stored points
    float4* d_gpts = nullptr;
    uint32_t* d_gstart = nullptr;
    elm::GroundIndex gidx{};
    double pt_bounds[4] = {0.0, 0.0, 0.0, 0.0};
    bool has_gidx = false;
    // the fine-occupancy tables of the free-space check (elm_map_check_free_space; built at the first call per sub = 1, 2, 4)
    int4* d_fine_keys[3] = {nullptr, nullptr, nullptr};
    unsigned long long* d_fine_masks[3] = {nullptr, nullptr, nullptr};
    elm::FineTable fine[3]{};
    double fine_info[3][2] = {{0.0, 0.0}, {0.0, 0.0}, {0.0, 0.0}}; // build ms, device bytes
    bool has_fine[3] = {false, false, false};
};

#define HIPCHK(ctx, call)                                                                              \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            return ELM_ERR_DEVICE;                                                                     \
        }                                                                                              \
    } while (0)

namespace elm_host {
inline int dev_reserve(elm_ctx* ctx, DevBuf& b, size_t bytes) {
    if (bytes <= b.cap) return ELM_OK;
    if (b.p) HIPCHK(ctx, hipFree(b.p));
    b.p = nullptr;
    b.cap = 0;
    size_t cap = std::max<size_t>(bytes, 256);
    HIPCHK(ctx, hipMalloc(&b.p, cap));
    b.cap = cap;
    return ELM_OK;
}
inline int pinned_reserve(elm_ctx* ctx, void** p, size_t* cap, size_t bytes) {
    if (bytes <= *cap) return ELM_OK;
    if (*p) HIPCHK(ctx, hipHostFree(*p));
    *p = nullptr;
    *cap = 0;
    HIPCHK(ctx, hipHostMalloc(p, bytes, hipHostMallocDefault));
    *cap = bytes;
    return ELM_OK;
}

// Contexts that are alive (elm_ctx.cpp): a child handle compares the unique id, not the pointer.
bool ctx_alive(const elm_ctx* ctx, uint64_t id);
// A group's lead context seen from the caller's thread: the public entry points hand the call to elm_multi (which runs it on every
// rank's own context from that rank's worker thread -- where the same entry points take their plain single-device path).
inline bool group_call(const elm_ctx* ctx) { return ctx && ctx->group && !elm_multi::in_worker(); }
// ELM_GRID / ELM_CHECK tokens (elm_ctx.cpp)
bool env_token(const char* var, const char* name, const char** value = nullptr);
bool check_mode(const char* name);
// one sum all-reduce of `count` doubles through the attached hook or communicator; neither: nothing (elm_ctx.cpp)
int exchange(elm_ctx* ctx, double* d_sums, size_t count, hipStream_t stream = nullptr);

// elm_map.cpp
inline uint32_t next_pow2(uint64_t v) {
    uint64_t p = 16;
    while (p < v) p <<= 1;
    return (uint32_t)p;
}
// An open-addressing table of `cap` slots (a power of two above n) over the n keys [n][3], inserted in key order with linear probing
// (hash3): key v gets vid = v and what fields(v, slot) writes into its start / cnt / pad0.  The map's own slot table, the query-voxel
// tables of the neighbourhood lists and of the voxel-mean lists are all filled here.
template <class Fields>
std::vector<elm::HashSlot> fill_slot_table(const int32_t* keys, uint32_t n, uint32_t cap, Fields fields) {
    std::vector<elm::HashSlot> slots(cap);
    for (auto& s : slots) {
        s.kx = s.ky = s.kz = 0;
        s.vid = -1;
        s.start = s.cnt = s.pad0 = s.pad1 = 0;
    }
    for (uint32_t v = 0; v < n; ++v) {
        uint32_t h = elm::hash3(keys[3 * v], keys[3 * v + 1], keys[3 * v + 2]) & (cap - 1);
        while (slots[h].vid >= 0) h = (h + 1) & (cap - 1);
        slots[h].kx = keys[3 * v]; slots[h].ky = keys[3 * v + 1]; slots[h].kz = keys[3 * v + 2];
        slots[h].vid = (int32_t)v;
        fields(v, slots[h]);
    }
    return slots;
}
void map_free(elm_map* m);
int map_finish(elm_ctx* ctx, elm_map* m, uint32_t n_pts, size_t n_input, double voxel_size, int max_points_per_voxel, elm_map** out);
void enumerate_query_keys(const elm_map* m, std::vector<int32_t>& qkeys);

// elm_index.cpp
int refresh_grid_gicp(elm_map* m);
int build_search_index(elm_map* m, bool* use_grid);
int build_voxel_neighbourhoods(elm_map* m, bool want_faces);

// elm_scan.cpp
int ensure_hilbert(elm_ctx* ctx);
int scan_alloc(elm_ctx* ctx, size_t n, elm_scan** out);
int scan_upload_impl(elm_ctx* ctx, const float* xyz, size_t n, size_t n_total, bool order, bool sync, elm_scan** out);
elm::DeskewDev deskew_args(const elm_deskew_tables* tab, const double* d_tab, size_t rows);
int downsample_enqueue(elm_ctx* ctx, const float* d_und, size_t n, double voxel_size, elm_scan** sc_out, unsigned** d_total_out);

// elm_api.cpp
// pcm.cpp:92-100: the covariance methods need their covariances computed (ELM_ERR_INVALID with the text in last_error)
int check_covariances(elm_ctx* ctx, const elm_map* map, int method);
// The device part of elm_map_get_correspondences on n query points that are already in HBM (d_q [n][3] float64, map frame): the search
// that call chooses -- the QUERY instantiation of the production search where the map has its index, the plain walk otherwise -- queued
// on the context's stream, d_out as RegParams::q_out ([n], or [n][8] for what == 2; set to -1 first).  *hd stages the launch's
// descriptor: it is read by an asynchronous copy until the stream is joined.  Takes the context's d_q2 and d_q3.
int query_pairs_enqueue(elm_ctx* ctx, const elm_map* map, int what, const double* d_q, size_t n, double max_dist, int32_t* d_out, elm::ScanDesc* hd);
int batch_enqueue_impl(elm_ctx* ctx, const elm_map* map, elm_scan* const* scans, int batch, const double* T0, const elm_reg_config* cfg,
                       int want_trace, const unsigned* n_dev);

// The 64 bytes behind the ScanState array of a lockstep batch (d_state, h_state): one copy reads the states and these together.
struct StateTail {
    int32_t active;        // scans still iterating (the early-stop counter)
    int32_t rank_mismatch; // the ranks iterated different registrations (rank-agreement check of the exchanged sums)
    int32_t _pad0[2];
    uint32_t ds_kept;      // downsample_enqueue: the points kept, the size of a one-scan batch on the device (launch_init_pack's n_dev)
    int32_t ds_overflow;   // downsample_enqueue: a voxel key does not pack
    int32_t _pad1[10];
};
static_assert(sizeof(StateTail) == 64 && offsetof(StateTail, rank_mismatch) == 4 && offsetof(StateTail, ds_kept) == 16 &&
              offsetof(StateTail, ds_overflow) == 20, "the state tail's layout");
inline StateTail* state_tail(void* states, int n_scans) { return (StateTail*)((char*)states + (size_t)n_scans * sizeof(elm::ScanState)); }
} // namespace elm_host
