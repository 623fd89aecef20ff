// elm_index.cpp -- the search indices of a map: the dense and the two-level (tiled) cell grid, the neighbourhood lists, the voxel-mean
// lists, and the choice among them (build_search_index); the device build's stage times are elm_call.hpp's StreamEvents.  Host-side C++17.
#include <assert.h>
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <initializer_list>
#include <new>
#include <string>
#include <vector>

#include "elm_call.hpp"
#include "elm_grid_layout.hpp"

using namespace elm;
using namespace elm_host;

// The block array of the cell grid: 4 slots per block must number below 2^31 (the kernels carry slot numbers as ints); below
// grid_narrow_limit() bytes stage 1 uses 32-bit byte offsets, beyond it 16-byte units (ELM_GRID=max_block_bytes=N lowers the limit: tests
// force the wide form onto small maps).
constexpr uint64_t kGridMaxBlocks = 0x1FFFFFF0ull;
static uint64_t grid_narrow_limit() {
    const char* v = nullptr;
    if (env_token("ELM_GRID", "max_block_bytes", &v)) return std::min<uint64_t>(strtoull(v, nullptr, 10), 0xFFFFFF00ull);
    return 0xFFFFFF00ull;
}
// The cell budget of the dense tables (the cell grid's offsets, the voxel-mean lists' floor-key box): ELM_GRID=max_cells=N, default
// 1.5e9 = 6 GB of offsets.
static uint64_t grid_max_cells() {
    const char* v = nullptr;
    if (env_token("ELM_GRID", "max_cells", &v)) return strtoull(v, nullptr, 10);
    return 1500000000ull;
}
// Host memory a large temporary may take: MemAvailable of /proc/meminfo (free + reclaimable page cache -- after a big PCD has been read
// most of the RAM is page cache, and MemFree alone would refuse the grid depending on the cache state); unknown: no limit (the
// allocations themselves fail with bad_alloc, which the builders handle).
static uint64_t host_available_bytes() {
    FILE* f = fopen("/proc/meminfo", "r");
    if (!f) return ~0ull;
    char line[256];
    uint64_t kb = 0;
    bool found = false;
    while (fgets(line, sizeof(line), f)) {
        unsigned long long v = 0;
        if (sscanf(line, "MemAvailable: %llu kB", &v) == 1) { kb = v; found = true; break; }
    }
    fclose(f);
    return found ? kb * 1024ull : ~0ull;
}

// The device allocations local to one builder: the builder's own pointer variables, by address.  Whatever they still hold when the
// builder returns -- on any path -- is released; release_all() at the commit leaves them to the map.
struct DevLocals {
    static constexpr int kMax = 8;
    void** held[kMax];
    int n = 0;
    DevLocals(std::initializer_list<void**> ptrs) {
        assert(ptrs.size() <= (size_t)kMax);
        for (void** p : ptrs)
            if (n < kMax) held[n++] = p;
    }
    DevLocals(const DevLocals&) = delete;
    DevLocals& operator=(const DevLocals&) = delete;
    void release_all() { n = 0; }
    ~DevLocals() {
        for (int i = 0; i < n; ++i)
            if (*held[i]) (void)hipFree(*held[i]);
    }
};
// HIPCHK for the grid builders: out of device memory is "this index is not affordable" (the caller builds another), not an error
#define HIPCHK_OOM(ctx, call)                                                                          \
    do {                                                                                               \
        hipError_t e_ = (call);                                                                        \
        if (e_ != hipSuccess) {                                                                        \
            (ctx)->last_error = std::string(#call) + ": " + hipGetErrorString(e_);                     \
            (void)hipGetLastError();                                                                   \
            return e_ == hipErrorOutOfMemory ? ELM_ERR_UNSUPPORTED : ELM_ERR_DEVICE;                   \
        }                                                                                              \
    } while (0)

// The query voxels of a map and the sizes of their lists, for the neighbourhood lists and for the voxel-mean lists: the keys
// (enumerate_query_keys) go to the device, launch_nbr_count counts every query voxel's neighbour points (counts) and occupied neighbour
// voxels (nocc), and the list offsets are the running sums of stride(q) -- the caller's rule -- on the host and on the device.  The device
// arrays live as long as this object.
struct QueryLists {
    std::vector<int32_t> qkeys;
    uint32_t n_q = 0;
    std::vector<uint32_t> counts, nocc, offs;
    uint64_t total = 0;
    int32_t* d_qkeys = nullptr;
    uint32_t *d_counts = nullptr, *d_nocc = nullptr, *d_off = nullptr;
    DevLocals own{(void**)&d_qkeys, (void**)&d_counts, (void**)&d_nocc, (void**)&d_off};
};
template <class Stride>
static int count_query_lists(elm_map* m, QueryLists& ql, Stride stride) {
    elm_ctx* ctx = m->ctx;
    std::vector<int32_t>& qkeys = ql.qkeys;
    enumerate_query_keys(m, qkeys);
    const uint32_t n_q = ql.n_q = (uint32_t)(qkeys.size() / 3);
    int32_t*& d_qkeys = ql.d_qkeys;
    uint32_t *&d_counts = ql.d_counts, *&d_nocc = ql.d_nocc, *&d_off = ql.d_off;
    const size_t nq_alloc = std::max<size_t>(n_q, 1);
    HIPCHK(ctx, hipMalloc((void**)&d_qkeys, nq_alloc * 3 * sizeof(int32_t)));
    HIPCHK(ctx, hipMalloc((void**)&d_counts, nq_alloc * sizeof(uint32_t)));
    HIPCHK(ctx, hipMalloc((void**)&d_nocc, nq_alloc * sizeof(uint32_t)));
    HIPCHK(ctx, hipMalloc((void**)&d_off, nq_alloc * sizeof(uint32_t)));
    std::vector<uint32_t>&counts = ql.counts, &nocc = ql.nocc, &offs = ql.offs;
    counts.resize(n_q); nocc.resize(n_q); offs.resize(n_q);
    uint64_t total = 0;
    if (n_q) { // (deterministic: a later build from the same map finds the offsets the lists were written with)
        HIPCHK(ctx, hipMemcpy(d_qkeys, qkeys.data(), (size_t)n_q * 3 * sizeof(int32_t), hipMemcpyHostToDevice));
        (void)hipGetLastError();
        launch_nbr_count(ctx->stream, m->dm, d_qkeys, n_q, d_counts, d_nocc);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        // (the voxel-mean lists read only nocc on the host; their counts come down too -- n_q words, once per build -- so that the step is one)
        HIPCHK(ctx, hipMemcpy(counts.data(), d_counts, (size_t)n_q * sizeof(uint32_t), hipMemcpyDeviceToHost));
        HIPCHK(ctx, hipMemcpy(nocc.data(), d_nocc, (size_t)n_q * sizeof(uint32_t), hipMemcpyDeviceToHost));
        for (uint32_t q = 0; q < n_q; ++q) {
            offs[q] = (uint32_t)total;
            total += stride(q);
        }
        HIPCHK(ctx, hipMemcpy(d_off, offs.data(), (size_t)n_q * sizeof(uint32_t), hipMemcpyHostToDevice));
    }
    ql.total = total; // (the caller refuses a total beyond what its offsets hold)
    return ELM_OK;
}
// the probe table over the query voxels: query voxel q at its key with what fields(q, slot) writes
template <class Fields>
static int upload_query_slots(elm_ctx* ctx, const QueryLists& ql, uint32_t qcap, HashSlot** d_slots, Fields fields) {
    const std::vector<HashSlot> qs = fill_slot_table(ql.qkeys.data(), ql.n_q, qcap, fields);
    HIPCHK(ctx, hipMalloc((void**)d_slots, (size_t)qcap * sizeof(HashSlot)));
    HIPCHK(ctx, hipMemcpy(*d_slots, qs.data(), (size_t)qcap * sizeof(HashSlot), hipMemcpyHostToDevice));
    return ELM_OK;
}

// Voxel-mean lists for VGICP / AVGICP (DevMap::vnbr_blk, vox_rec): built lazily at the first VGICP / AVGICP registration, after
// CalVoxelCovAll.  The lists hold 16 bytes per slot (float32 mean + voxel id | position code); a voxel's float64 record is stored ONCE in
// vox_rec (round 6: rounds 2-5 copied the 64-byte record into every list, 27 x).  AVGICP's face sublists (whole records, <= 7 per query
// voxel) are built only when an AVGICP call asks for them (want_faces): a VGICP map does not pay their bytes.
int elm_host::build_voxel_neighbourhoods(elm_map* m, bool want_faces) {
    const bool need_lists = !m->has_vnbr;
    // faces exist only beside the dense floor-key table; a map whose lists were built without one never gets them
    const bool need_faces = want_faces && !m->has_vface && !m->vface_refused && (need_lists || m->d_vq_dense != nullptr);
    if (!need_lists && !need_faces) return ELM_OK;
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (m->dm.n_vox > kVidMask) { ctx->last_error = "voxel-mean lists: more than 2^26 voxels"; return ELM_ERR_UNSUPPORTED; }
    QueryLists ql;
    int rc;
    if ((rc = count_query_lists(m, ql, [&](uint32_t q) { return (ql.nocc[q] + 3u) & ~3u; })) != ELM_OK) return rc; // list starts: multiples of four slots
    const std::vector<int32_t>& qkeys = ql.qkeys;
    const std::vector<uint32_t>&nocc = ql.nocc, &offs = ql.offs;
    const uint32_t n_q = ql.n_q;
    const uint64_t total = ql.total;
    int32_t* const d_qkeys = ql.d_qkeys;
    uint32_t *const d_nocc = ql.d_nocc, *const d_off = ql.d_off;
    if (total >= (1ull << 32)) { ctx->last_error = "voxel-mean lists exceed 2^32 slots"; return ELM_ERR_UNSUPPORTED; }
    // the dense box of floor keys (when it fits the cell budget and the packed word holds the offsets): no hash probe in the kernel --
    // one 4-byte load at a computed, spatially coherent address
    int32_t klo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, khi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (uint32_t q = 0; q < n_q; ++q)
        for (int a = 0; a < 3; ++a) {
            klo[a] = std::min(klo[a], qkeys[3 * q + a]);
            khi[a] = std::max(khi[a], qkeys[3 * q + a]);
        }
    const int64_t vd[3] = {n_q ? (int64_t)khi[0] - klo[0] + 1 : 0, n_q ? (int64_t)khi[1] - klo[1] + 1 : 0, n_q ? (int64_t)khi[2] - klo[2] + 1 : 0};
    const uint64_t vcells = (uint64_t)vd[0] * (uint64_t)vd[1] * (uint64_t)vd[2];
    auto dense_index = [&](uint32_t q) {
        return ((uint64_t)(qkeys[3 * q] - klo[0]) * (uint64_t)vd[1] + (uint64_t)(qkeys[3 * q + 1] - klo[1])) * (uint64_t)vd[2] + (uint64_t)(qkeys[3 * q + 2] - klo[2]);
    };
    const bool dense_ok = n_q && total / 4 < (1ull << 27) && vcells <= grid_max_cells() && m->ctx->kernel_mode == 4;
    if (need_lists) {
        const size_t nb = (size_t)(total / 4) + 1; // + one block of padding slots at the end: the target of the filter's loads past a list's last block
        HIPCHK(ctx, hipMalloc((void**)&m->d_vnbr_blk, nb * sizeof(VoxBlk)));
        {
            VoxBlk padblk;
            for (int u = 0; u < 4; ++u) { padblk.g.x[u] = padblk.g.y[u] = padblk.g.z[u] = 1e18f; padblk.vc[u] = -1; }
            HIPCHK(ctx, hipMemcpy(m->d_vnbr_blk + (nb - 1), &padblk, sizeof(VoxBlk), hipMemcpyHostToDevice));
            m->dm.vnbr_pad_blk = (uint32_t)(nb - 1);
        }
        HIPCHK(ctx, hipMalloc((void**)&m->d_vox_rec, std::max<size_t>((size_t)m->dm.n_vox * sizeof(VoxRec), 256)));
        (void)hipGetLastError();
        launch_vox_rec_fill(ctx->stream, m->dm, m->d_vox_rec);
        if (n_q) launch_vnbr_fill(ctx->stream, m->dm, d_qkeys, n_q, d_off, m->d_vnbr_blk);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        const uint32_t qcap = next_pow2((uint64_t)n_q * 2);
        if ((rc = upload_query_slots(ctx, ql, qcap, &m->d_vqslots, [&](uint32_t q, HashSlot& s) { s.start = offs[q]; s.cnt = nocc[q]; })) != ELM_OK) return rc;
        size_t bytes = nb * sizeof(VoxBlk) + (size_t)m->dm.n_vox * sizeof(VoxRec);
        if (dense_ok) {
            std::vector<uint32_t> dense(vcells, 0u);
            for (uint32_t q = 0; q < n_q; ++q) dense[dense_index(q)] = ((offs[q] >> 2) << 5) | nocc[q]; // first block of four slots, nocc <= 27
            HIPCHK(ctx, hipMalloc((void**)&m->d_vq_dense, vcells * sizeof(uint32_t)));
            HIPCHK(ctx, hipMemcpy(m->d_vq_dense, dense.data(), vcells * sizeof(uint32_t), hipMemcpyHostToDevice));
            m->dm.vq_dense = m->d_vq_dense;
            m->dm.vq_x0 = klo[0]; m->dm.vq_y0 = klo[1]; m->dm.vq_z0 = klo[2];
            m->dm.vq_nx = (int32_t)vd[0]; m->dm.vq_ny = (int32_t)vd[1]; m->dm.vq_nz = (int32_t)vd[2];
            bytes += vcells * sizeof(uint32_t);
        } else {
            bytes += (size_t)qcap * sizeof(HashSlot); // (the probe table is read only without the dense one)
        }
        m->dm.vqslots = m->d_vqslots;
        m->dm.vqmask = qcap - 1;
        m->dm.vox_rec = m->d_vox_rec;
        m->dm.vnbr_blk = m->d_vnbr_blk;
        m->has_vnbr = true;
        m->info.device_bytes += bytes + (dense_ok ? (size_t)qcap * sizeof(HashSlot) : 0);
        m->info.index_bytes += bytes + (size_t)m->n_bad_vox * 9 * sizeof(double); // + the stored inverses flagged voxels read
        m->info.index_part_bytes[1] += bytes + (size_t)m->n_bad_vox * 9 * sizeof(double);
        m->info.n_list_voxels = n_q;
    }
    if (need_faces && m->d_vq_dense && n_q) {
        // AVGICP pairs with the face neighbours only (<= 7 of a list's <= 27 slots): their sublists as whole records, addressed like vq_dense
        uint32_t *d_fcnt = nullptr, *d_foff = nullptr;
        DevLocals own{(void**)&d_fcnt, (void**)&d_foff};
        const size_t nq_alloc = n_q;
        HIPCHK(ctx, hipMalloc((void**)&d_fcnt, nq_alloc * sizeof(uint32_t)));
        HIPCHK(ctx, hipMalloc((void**)&d_foff, nq_alloc * sizeof(uint32_t)));
        (void)hipGetLastError();
        // the fused AVGICP walk's record format; flagged voxels (NaN normals) are left to its fix-up launch (ELM_CHECK=avg_inline: such maps
        // keep the nine-entry walk with its in-line fallback)
        // The fix-up launch pays while few workgroups meet a flagged record (round 4: +14 % with 0.3 % of the voxels flagged); when
        // flagged voxels are common -- sparse clutter: two or three points per voxel, rank-deficient -- nearly every workgroup is marked,
        // the second launch repeats the whole walk, and the in-line fallback is the cheaper form: by default the map decides at 1 % of
        // its voxels (ELM_CHECK=avg_fixup / avg_inline force either form).
        const bool fx_inline = check_mode("avg_inline"), fx_fixup = check_mode("avg_fixup"), fx_skip = check_mode("avg_skip");
        const bool fixup_ok = fx_inline ? false : ((fx_fixup || fx_skip) ? true : (uint64_t)m->n_bad_vox * 100ull <= (uint64_t)m->dm.n_vox);
        const int plain = (m->dm.vox_compact && (m->n_bad_vox == 0 || fixup_ok) && !check_mode("avg_nine") && !check_mode("pair_nine")) ? 1 : 0;
        launch_vface(ctx->stream, m->dm, d_off, d_nocc, n_q, d_fcnt, nullptr, nullptr, plain);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
        std::vector<uint32_t> fcnt(n_q), foff(n_q);
        HIPCHK(ctx, hipMemcpy(fcnt.data(), d_fcnt, (size_t)n_q * sizeof(uint32_t), hipMemcpyDeviceToHost));
        uint64_t ftotal = 0;
        for (uint32_t q = 0; q < n_q; ++q) { foff[q] = (uint32_t)ftotal; ftotal += fcnt[q]; }
        if (ftotal < (1ull << 29)) {
            HIPCHK(ctx, hipMemcpy(d_foff, foff.data(), (size_t)n_q * sizeof(uint32_t), hipMemcpyHostToDevice));
            HIPCHK(ctx, hipMalloc((void**)&m->d_vface, std::max<size_t>((size_t)ftotal * sizeof(VoxRec), 256)));
            launch_vface(ctx->stream, m->dm, d_off, d_nocc, n_q, d_fcnt, d_foff, m->d_vface, plain);
            HIPCHK(ctx, hipGetLastError());
            HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
            std::vector<uint32_t> dense(vcells, 0u);
            for (uint32_t q = 0; q < n_q; ++q) dense[dense_index(q)] = (foff[q] << 3) | fcnt[q]; // fcnt <= 7
            HIPCHK(ctx, hipMalloc((void**)&m->d_vqf_dense, vcells * sizeof(uint32_t)));
            HIPCHK(ctx, hipMemcpy(m->d_vqf_dense, dense.data(), vcells * sizeof(uint32_t), hipMemcpyHostToDevice));
            m->dm.vface = m->d_vface;
            m->dm.vqf_dense = m->d_vqf_dense;
            m->dm.vface_plain = plain;
            m->dm.vface_flagged = (plain && m->n_bad_vox != 0) ? (fx_skip ? 2 : 1) : 0; // (2: tests only -- no fix-up launch, the flagged pairs are dropped)
            m->info.layout_flags = (m->info.layout_flags & ~(32 | 64)) | (plain ? 32 : 0) | (m->dm.vface_flagged ? 64 : 0);
            m->info.device_bytes += vcells * sizeof(uint32_t) + (size_t)ftotal * sizeof(VoxRec);
            m->info.index_bytes += vcells * sizeof(uint32_t) + (size_t)ftotal * sizeof(VoxRec);
            m->info.index_part_bytes[2] += vcells * sizeof(uint32_t) + (size_t)ftotal * sizeof(VoxRec);
            m->has_vface = true;
        } else {
            m->vface_refused = true;
        }
    } else if (need_faces) {
        m->vface_refused = true;
    }
    return ELM_OK;
}

// The GICP payload in grid slot order (DevMap::grid_gicp): needs the grid and the point covariances, whichever comes last.
int elm_host::refresh_grid_gicp(elm_map* m) {
    if (!m->has_grid || !m->info.has_point_cov || !m->grid_slots) return ELM_OK;
    elm_ctx* ctx = m->ctx;
    const bool compact = m->want_gicp_compact;
    double** dst = compact ? &m->d_grid_gicp8 : &m->d_grid_gicp;
    const size_t rec_bytes = (compact ? 8 : 16) * sizeof(double);
    if (!*dst) {
        HIPCHK(ctx, hipMalloc((void**)dst, m->grid_slots * rec_bytes));
        m->info.device_bytes += m->grid_slots * rec_bytes;
    }
    (void)hipGetLastError();
    launch_gather_gicp(ctx->stream, m->dm, m->grid_slots, *dst, compact ? 1 : 0);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    m->dm.grid_gicp = m->d_grid_gicp;
    m->dm.grid_gicp8 = m->d_grid_gicp8;
    // 2: no point outside the compact form -- the kernel has no full-record fallback and gathers the pair fused (ELM_CHECK=pair_nine: the
    // nine-entry form with its fallback, as for maps with flagged points; fusing the compact lanes of THOSE kernels too and reading a
    // flagged point's stored inverse row by row measured 15 % slower in round 5: profiles/r05_kernel_ab.txt)
    m->dm.gicp_compact = compact ? ((m->n_bad_pts == 0 && !check_mode("pair_nine")) ? 2 : 1) : 0;
    m->info.layout_flags = (m->info.layout_flags & ~(1 | 8)) | (compact ? 1 : 0) | (m->dm.gicp_compact == 2 ? 8 : 0);
    return ELM_OK;
}

// ------------------------------------------------------------------------------------------------------
// the cell grids: what the dense and the two-level form share
// ------------------------------------------------------------------------------------------------------
static_assert(sizeof(GridBlk) == 48 && offsetof(GridBlk, x) == 0 && offsetof(GridBlk, y) == 16 && offsetof(GridBlk, z) == 32,
              "grid_block_layout writes blocks of x[4] y[4] z[4]");

// The stored points on the host and the box of their half-voxel cells, two cells of margin on every side: a block or ball that reaches
// just past the outermost points stays inside the grid.
struct GridBox {
    std::vector<float4> pts;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX};
    int64_t dim[3] = {0, 0, 0};
};
// box.lo / hi: the outermost cells of the points -> the box with its margin
static void grid_box_margin(GridBox& box, int32_t hi[3]) {
    for (int a = 0; a < 3; ++a) {
        box.lo[a] -= 2; hi[a] += 2;
        box.dim[a] = (int64_t)hi[a] - box.lo[a] + 1;
    }
}
static int grid_box(elm_map* m, GridBox& box) {
    elm_ctx* ctx = m->ctx;
    const size_t n = m->dm.n_pts;
    const double vs = m->dm.voxel_size;
    std::vector<float4>& pts = box.pts;
    pts.resize(n);
    HIPCHK(ctx, hipMemcpy(pts.data(), m->d_pts, n * sizeof(float4), hipMemcpyDeviceToHost));
    int32_t* lo = box.lo;
    int32_t hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (size_t i = 0; i < n; ++i) {
        const float c3[3] = {pts[i].x, pts[i].y, pts[i].z};
        for (int a = 0; a < 3; ++a) {
            const int32_t c = grid_cell_of((double)c3[a], vs);
            lo[a] = std::min(lo[a], c);
            hi[a] = std::max(hi[a], c);
        }
    }
    grid_box_margin(box, hi);
    return ELM_OK;
}
// the same box from the device (k_gb_box): the points stay where they are, six words come down
static int grid_box_device(elm_map* m, GridBox& box, int* d_box) {
    elm_ctx* ctx = m->ctx;
    const int32_t init[6] = {INT32_MAX, INT32_MAX, INT32_MAX, INT32_MIN, INT32_MIN, INT32_MIN};
    int32_t got[6];
    HIPCHK(ctx, hipMemcpyAsync(d_box, init, sizeof(init), hipMemcpyHostToDevice, ctx->stream));
    (void)hipGetLastError();
    launch_gb_box(ctx->stream, m->d_pts, (unsigned)m->dm.n_pts, m->dm.voxel_size, d_box);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, hipMemcpyAsync(got, d_box, sizeof(got), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    int32_t hi[3];
    for (int a = 0; a < 3; ++a) { box.lo[a] = got[a]; hi[a] = got[3 + a]; }
    grid_box_margin(box, hi);
    return ELM_OK;
}

// A laid-out grid (grid_block_layout) on the host, and its copy on the device: the builder's locals until grid_commit.  d_side is the
// form's own table (the dense grid's statistics box, the two-level grid's tile table), allocated by the form.
struct GridHost {
    std::vector<uint32_t> start, gi;
    std::vector<GridBlk> gb;
    uint64_t n_blk = 0;
};
struct GridDev {
    GridBlk* d_blk = nullptr;
    uint32_t *d_idx = nullptr, *d_start = nullptr;
    void* d_side = nullptr;
    DevLocals own{(void**)&d_blk, (void**)&d_idx, (void**)&d_start, &d_side};
};
// What a producer -- the host layout or the device build -- hands to the shared finish of its form: the arrays in d, and their counts.
struct GridCounts {
    uint64_t n_blk = 0;     // blocks (4 * n_blk slots)
    uint64_t n_start = 0;   // words of grid_start: entries + 4
    bool on_device = false; // the device producer ran to the end (layout_flags bit 9)
};
// dm (the builder's copy of the map's view) gets the fields both forms and both producers set alike
static void grid_dm_common(DevMap& dm, const GridDev& d, const GridCounts& c) {
    dm.grid_blk = d.d_blk;
    dm.grid_idx = d.d_idx;
    dm.grid_start = d.d_start;
    dm.grid_wide = c.n_blk * sizeof(GridBlk) > grid_narrow_limit() ? 1 : 0;
    dm.grid_nslots = (uint32_t)(4 * c.n_blk);
}
// the host producer: blocks, slot indices and block starts go up
static int grid_upload(elm_ctx* ctx, const GridHost& g, GridDev& d) {
    const std::vector<GridBlk>& gb = g.gb;
    const std::vector<uint32_t>&gi = g.gi, &start = g.start;
    GridBlk*& d_blk = d.d_blk;
    uint32_t *&d_idx = d.d_idx, *&d_start = d.d_start;
    HIPCHK_OOM(ctx, hipMalloc((void**)&d_blk, gb.size() * sizeof(GridBlk)));
    HIPCHK_OOM(ctx, hipMalloc((void**)&d_idx, gi.size() * sizeof(uint32_t)));
    HIPCHK_OOM(ctx, hipMalloc((void**)&d_start, start.size() * sizeof(uint32_t)));
    HIPCHK_OOM(ctx, hipMemcpy(d_blk, gb.data(), gb.size() * sizeof(GridBlk), hipMemcpyHostToDevice));
    HIPCHK_OOM(ctx, hipMemcpy(d_idx, gi.data(), gi.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    HIPCHK_OOM(ctx, hipMemcpy(d_start, start.data(), start.size() * sizeof(uint32_t), hipMemcpyHostToDevice));
    return ELM_OK;
}
// Every device step has succeeded: dm and the arrays become the map's, and the GICP records are gathered into slot order.  When those do
// not fit the grid is given back (the lists read pt_gicp through their index): the map is as before, d still owns the arrays,
// ELM_ERR_UNSUPPORTED.  ALL the grid's bytes and counts in elm_map_info are accounted here, for both forms and both producers: blocks,
// slot indices and starts, and the form's own table d.d_side -- the dense grid's statistics box (side_cells words; not in
// index_part_bytes[0]: it is read by the instrumented kernels only) or the two-level grid's tile table (side_cells tiles).
static int grid_commit(elm_map* m, const DevMap& dm, const GridCounts& c, GridDev& d, uint64_t side_cells) {
    const DevMap dm_before = m->dm;
    m->dm = dm;
    m->d_grid_blk = d.d_blk; m->d_grid_idx = d.d_idx; m->d_grid_start = d.d_start;
    m->has_grid = true;
    m->grid_slots = (size_t)(4 * c.n_blk);
    m->grid_start_words = c.n_start;
    if (refresh_grid_gicp(m) != ELM_OK) {
        m->d_grid_blk = nullptr; m->d_grid_idx = nullptr; m->d_grid_start = nullptr;
        m->dm = dm_before;
        m->has_grid = false;
        m->grid_slots = 0;
        m->grid_start_words = 0;
        (void)hipGetLastError();
        return ELM_ERR_UNSUPPORTED;
    }
    const bool tiled = dm.grid_tiled != 0;
    if (tiled) m->d_grid_tiles = (uint2*)d.d_side;
    else m->d_vox_stat = (uint32_t*)d.d_side;
    d.own.release_all();
    const size_t searched = (size_t)c.n_blk * sizeof(GridBlk) + (size_t)c.n_start * sizeof(uint32_t);
    const size_t side = (size_t)side_cells * (tiled ? sizeof(uint2) : sizeof(uint32_t));
    m->info.device_bytes += searched + (size_t)(4 * c.n_blk) * sizeof(uint32_t) + side;
    m->info.nbr_entries = m->dm.n_pts;
    m->info.n_query_voxels = side_cells;
    m->info.index_bytes += searched + side;
    m->info.index_part_bytes[0] += searched + (tiled ? side : 0);
    if (tiled) m->info.layout_flags |= 4;
    if (c.on_device) m->info.layout_flags |= 512;
    return ELM_OK;
}

// ---- the decisions both producers share: which boxes and budgets a form accepts (host arithmetic on the box integers and counts)
static bool dense_box_refused(const int64_t dim[3], uint64_t cells, uint64_t max_cells) {
    return dim[0] > 0x7FFFFFF0ll || dim[1] > 0x7FFFFFF0ll || dim[2] > 0x7FFFFFF0ll || cells > max_cells || cells > 0xFFFFFFF0ull;
}
// dense voxel box of floor keys: a query with floor key f walks the stored keys f-1 .. f+1
static uint64_t dense_vox_box(const elm_map* m, int32_t klo[3], int64_t vd[3]) {
    int32_t khi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    klo[0] = klo[1] = klo[2] = INT32_MAX;
    for (uint32_t v = 0; v < m->dm.n_vox; ++v)
        for (int a = 0; a < 3; ++a) {
            klo[a] = std::min(klo[a], m->h_keys[3 * v + a]);
            khi[a] = std::max(khi[a], m->h_keys[3 * v + a]);
        }
    for (int a = 0; a < 3; ++a) vd[a] = (int64_t)khi[a] - klo[a] + 3;
    return (uint64_t)vd[0] * (uint64_t)vd[1] * (uint64_t)vd[2];
}
// Byte budget (the cell count alone says nothing about a sparse or elongated map just under it): host transients = the
// offsets + the sorted copy (blocks of four: at most one block per point) + two index arrays; device = offsets + statistics +
// blocks + slot indices (+ the GICP records in slot order).  Not affordable right now -> the lists.  The device producer has no host
// tables (host_tables = false drops the host term) and adds its scratch (dev_scratch) to the device need.
static int grid_budget(elm_map* m, const char* what, uint64_t host_need, uint64_t dev_need, bool host_tables, uint64_t dev_scratch, bool* ok) {
    elm_ctx* ctx = m->ctx;
    size_t dev_free = 0, dev_total = 0;
    HIPCHK(ctx, hipMemGetInfo(&dev_free, &dev_total));
    const uint64_t host_free = host_available_bytes();
    dev_need += dev_scratch;
    *ok = !((host_tables && host_need > host_free / 10 * 7) || dev_need > (uint64_t)dev_free / 10 * 8);
    if (!*ok)
        ctx->last_error = std::string(what) + ": tables exceed the memory that is free (host " + std::to_string((host_tables ? host_need : 0) >> 20) +
                          " MB, device " + std::to_string(dev_need >> 20) + " MB needed)";
    return ELM_OK;
}
static int dense_budget(elm_map* m, uint64_t cells, uint64_t vcells, bool host_tables, uint64_t dev_scratch, bool* ok) {
    const uint64_t n = m->dm.n_pts;
    const uint64_t worst_blk = std::min<uint64_t>(n, cells) + n / 4 + 2;
    const uint64_t host_need = (cells + 4) * 4 + worst_blk * (sizeof(GridBlk) + 16) + n * 8;
    const uint64_t dev_need = (cells + 4) * 4 + vcells * 4 + worst_blk * (sizeof(GridBlk) + 16) + (m->info.has_point_cov ? worst_blk * 4 * (m->want_gicp_compact ? 64 : 128) : 0);
    return grid_budget(m, "cell grid", host_need, dev_need, host_tables, dev_scratch, ok);
}
// 64 M tiles = 512 MB of tile table (a 32 km x 32 km box at half-metre cells); the z range of a tile is a 16-bit pair
static bool tiled_box_refused(const int64_t dim[3], int64_t tnx, int64_t tny) {
    return tnx * tny > ((int64_t)64 << 20) || dim[2] > 65000 || tnx * kTile > 0x7FFFFFF0ll || tny * kTile > 0x7FFFFFF0ll;
}
// (host_need still counts two tables of entries + 4 words, from before the layout was shared with the dense grid; the build now takes
// one: the formula over-counts and is left as it is -- a changed refusal changes which index a map gets)
static int tiled_budget(elm_map* m, uint64_t entries, uint64_t n_tiles, bool host_tables, uint64_t dev_scratch, bool* ok) {
    const uint64_t n = m->dm.n_pts;
    const uint64_t worst_blk = n + 2;
    const uint64_t host_need = (entries + 4) * 8 + worst_blk * (sizeof(GridBlk) + 16) + n * 8 + n_tiles * 12;
    const uint64_t dev_need = (entries + 4) * 4 + n_tiles * 8 + worst_blk * (sizeof(GridBlk) + 16) + (m->info.has_point_cov ? worst_blk * 4 * (m->want_gicp_compact ? 64 : 128) : 0);
    return grid_budget(m, "tiled cell grid", host_need, dev_need, host_tables, dev_scratch, ok);
}

// ---- the finish both producers share: d holds blocks, slot indices and starts; the form's own table, the map's view, the commit
// Dense form: the statistics box is allocated and filled here (launch_vox_stat reads the grid through dm).
static int dense_grid_finish(elm_map* m, const GridBox& box, const GridCounts& c, GridDev& d, const int32_t klo[3], const int64_t vd[3], uint64_t vcells) {
    elm_ctx* ctx = m->ctx;
    DevMap dm = m->dm;
    grid_dm_common(dm, d, c);
    uint32_t* d_stat = nullptr;
    HIPCHK_OOM(ctx, hipMalloc((void**)&d_stat, std::max<size_t>(vcells * sizeof(uint32_t), 256)));
    d.d_side = d_stat;
    dm.gx0 = box.lo[0]; dm.gy0 = box.lo[1]; dm.gz0 = box.lo[2];
    dm.gnx = (int32_t)box.dim[0]; dm.gny = (int32_t)box.dim[1]; dm.gnz = (int32_t)box.dim[2];
    dm.vox_stat = d_stat;
    dm.vx0 = klo[0] - 1; dm.vy0 = klo[1] - 1; dm.vz0 = klo[2] - 1;
    dm.vnx = (int32_t)vd[0]; dm.vny = (int32_t)vd[1]; dm.vnz = (int32_t)vd[2];
    (void)hipGetLastError();
    launch_vox_stat(ctx->stream, dm, d_stat);
    HIPCHK_OOM(ctx, hipGetLastError());
    HIPCHK_OOM(ctx, hipStreamSynchronize(ctx->stream));
    return grid_commit(m, dm, c, d, vcells);
}
// Two-level form: d.d_side is the tile table, already on the device.
static int tiled_grid_finish(elm_map* m, const GridBox& box, const GridCounts& c, GridDev& d, int64_t tnx, int64_t tny) {
    DevMap dm = m->dm;
    grid_dm_common(dm, d, c);
    dm.grid_tiles = (const uint2*)d.d_side;
    dm.grid_tiled = 1;
    dm.gtny = (int32_t)tny;
    dm.gx0 = box.lo[0]; dm.gy0 = box.lo[1]; dm.gz0 = box.lo[2];
    dm.gnx = (int32_t)(tnx * kTile); dm.gny = (int32_t)(tny * kTile); dm.gnz = (int32_t)box.dim[2];
    dm.vox_stat = nullptr;
    return grid_commit(m, dm, c, d, (uint64_t)(tnx * tny));
}

// ------------------------------------------------------------------------------------------------------
// the device producer (elm_k_gridbuild.hip): opt-in per map (elm_map_set_index_build)
// ------------------------------------------------------------------------------------------------------
constexpr int kTryHost = 1; // not an error: this build is the host producer's (scratch not affordable, out of device memory, a size beyond the device kernels' 32-bit indices)
// the device allocations of one device build, released on every path; get(): hipErrorOutOfMemory -> kTryHost
struct GridScratch {
    std::vector<void*> held;
    GridScratch() = default;
    GridScratch(const GridScratch&) = delete;
    GridScratch& operator=(const GridScratch&) = delete;
    ~GridScratch() {
        for (void* p : held) (void)hipFree(p);
    }
    template <class T>
    int get(elm_ctx* ctx, T** p, size_t count) {
        void* v = nullptr;
        const hipError_t e = hipMalloc(&v, std::max<size_t>(count * sizeof(T), 256));
        if (e != hipSuccess) {
            ctx->last_error = std::string("device index build: hipMalloc: ") + hipGetErrorString(e);
            (void)hipGetLastError();
            return e == hipErrorOutOfMemory ? kTryHost : ELM_ERR_DEVICE;
        }
        held.push_back(v);
        *p = (T*)v;
        return ELM_OK;
    }
};
// hipEvents around the stages (elm_map_index_build_stages)
static_assert(sizeof(elm_map::index_stage_ms) == ELM_INDEX_STAGES * sizeof(double), "one slot per stage");
using GridStageClock = elm_query::StreamEvents<ELM_INDEX_STAGES + 1>; // (a stage whose mark was never made reads as 0.0 ms)
// what the sort and the scans need beside the table of entries + 4 words: 16 bytes per point (key and payload, twice), the histogram
// of one radix pass and the workgroup sums of the longest scan
static uint64_t grid_device_scratch_bytes(uint64_t n, uint64_t entries) {
    const uint64_t hist_words = bd_rx_hist_words((unsigned)n);
    return n * 16 + hist_words * 4 + (std::max<uint64_t>(entries + 4, hist_words) / 1024 + 1) * 4 + 1024;
}
// the sizes the device kernels index with 32 bits (beyond: the host producer)
static bool grid_device_sizes_ok(uint64_t n, uint64_t entries) { return n < 0x7FFFFFFFull && entries + 4 <= 0xF0000000ull; }

// From the counts in d.d_start (entries + 4 words, the trailing four zero) and the unsorted (entry, point number) pairs in key[0] / val[0]:
// the stable sort by entry, the block starts, n_blk down, blocks and slots allocated, padded and filled.  The tail both forms share.
struct GridSortBufs {
    unsigned *key[2] = {nullptr, nullptr}, *val[2] = {nullptr, nullptr}, *hist = nullptr, *blk = nullptr, *total = nullptr;
};
static int grid_device_layout(elm_map* m, GridStageClock& clk, const GridSortBufs& b, uint64_t entries, unsigned zero_head,
                              GridDev& d, GridCounts& c) {
    elm_ctx* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const unsigned n = (unsigned)m->dm.n_pts;
    (void)hipGetLastError();
    // order inside an entry = input order: stable 8-bit passes over the bits the entries have
    unsigned bits = 0, cur = 0;
    while (bits < 32 && ((uint64_t)1 << bits) < entries) ++bits;
    const unsigned hist_words = (unsigned)bd_rx_hist_words(n);
    for (unsigned shift = 0; shift < bits; shift += 8, cur ^= 1) {
        launch_bd_rx_hist(st, b.key[cur], n, shift, b.hist);
        launch_bd_scan(st, b.hist, hist_words, b.blk, b.total);
        launch_bd_rx_scatter(st, b.key[cur], b.val[cur], n, shift, b.hist, b.key[cur ^ 1], b.val[cur ^ 1]);
    }
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, clk.mark(st));
    // block starts
    launch_gb_blocks(st, d.d_start, (unsigned)entries);
    launch_bd_scan(st, d.d_start, (unsigned)entries, b.blk, b.total);
    launch_gb_start_fin(st, d.d_start, (unsigned)entries, zero_head, b.total);
    HIPCHK(ctx, hipGetLastError());
    unsigned blocks = 0;
    HIPCHK(ctx, hipMemcpyAsync(&blocks, b.total, sizeof(unsigned), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    c.n_blk = (uint64_t)blocks + 1; // block 0: four padding slots
    c.n_start = entries + 4;
    HIPCHK(ctx, clk.mark(st));
    if (c.n_blk > kGridMaxBlocks) return ELM_ERR_UNSUPPORTED; // (the host's refusal: the caller marks the map)
    // fill
    for (void** p : {(void**)&d.d_blk, (void**)&d.d_idx}) {
        const size_t bytes = p == (void**)&d.d_blk ? (size_t)c.n_blk * sizeof(GridBlk) : (size_t)c.n_blk * 4 * sizeof(uint32_t);
        const hipError_t e = hipMalloc(p, bytes);
        if (e != hipSuccess) {
            ctx->last_error = std::string("device index build: hipMalloc: ") + hipGetErrorString(e);
            (void)hipGetLastError();
            return e == hipErrorOutOfMemory ? kTryHost : ELM_ERR_DEVICE;
        }
    }
    launch_gb_pad(st, d.d_blk, d.d_idx, c.n_blk);
    launch_gb_fill(st, m->d_pts, b.key[cur], b.val[cur], n, d.d_start, d.d_blk, d.d_idx);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, clk.mark(st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    return ELM_OK;
}
static int grid_sort_bufs(elm_ctx* ctx, GridScratch& sc, GridSortBufs& b, uint64_t n, uint64_t entries) {
    const uint64_t hist_words = bd_rx_hist_words((unsigned)n);
    int rc;
    for (int k = 0; k < 2; ++k) {
        if ((rc = sc.get(ctx, &b.key[k], n)) != ELM_OK) return rc;
        if ((rc = sc.get(ctx, &b.val[k], n)) != ELM_OK) return rc;
    }
    if ((rc = sc.get(ctx, &b.hist, hist_words)) != ELM_OK) return rc;
    if ((rc = sc.get(ctx, &b.blk, std::max<uint64_t>(entries + 4, hist_words) / 1024 + 1)) != ELM_OK) return rc;
    return sc.get(ctx, &b.total, 4);
}
// the table of entries + 4 words, zeroed: the counts, then the block starts (it becomes the map's grid_start)
static int grid_start_table(elm_ctx* ctx, GridDev& d, uint64_t entries) {
    const hipError_t e = hipMalloc((void**)&d.d_start, (entries + 4) * sizeof(uint32_t));
    if (e != hipSuccess) {
        ctx->last_error = std::string("device index build: hipMalloc: ") + hipGetErrorString(e);
        (void)hipGetLastError();
        return e == hipErrorOutOfMemory ? kTryHost : ELM_ERR_DEVICE;
    }
    HIPCHK(ctx, hipMemsetAsync(d.d_start, 0, (entries + 4) * sizeof(uint32_t), ctx->stream));
    return ELM_OK;
}

// The dense form on the device.  ELM_OK; ELM_ERR_UNSUPPORTED exactly where the host producer refuses (same functions, same numbers; the
// caller sets grid_refused as it does for the host's refusals); kTryHost; an error.
static int build_cell_grid_device(elm_map* m, uint64_t max_cells) {
    elm_ctx* ctx = m->ctx;
    const uint64_t n = m->dm.n_pts;
    if (!grid_device_sizes_ok(n, 0)) return kTryHost;
    GridScratch sc;
    GridStageClock clk;
    int rc;
    int* d_box = nullptr;
    if ((rc = sc.get(ctx, &d_box, 8)) != ELM_OK) return rc;
    HIPCHK(ctx, clk.mark(ctx->stream));
    GridBox box;
    if ((rc = grid_box_device(m, box, d_box)) != ELM_OK) return rc;
    HIPCHK(ctx, clk.mark(ctx->stream));
    const int64_t* dim = box.dim;
    const uint64_t cells = (uint64_t)dim[0] * (uint64_t)dim[1] * (uint64_t)dim[2];
    if (dense_box_refused(dim, cells, max_cells)) return ELM_ERR_UNSUPPORTED;
    int32_t klo[3];
    int64_t vd[3];
    const uint64_t vcells = dense_vox_box(m, klo, vd);
    if (vcells > max_cells) return ELM_ERR_UNSUPPORTED;
    if (!grid_device_sizes_ok(n, cells)) return kTryHost;
    bool ok = false;
    if ((rc = dense_budget(m, cells, vcells, false, grid_device_scratch_bytes(n, cells), &ok)) != ELM_OK) return rc;
    if (!ok) return kTryHost; // (the host producer decides with its own terms)
    GridDev d;
    GridSortBufs b;
    if ((rc = grid_start_table(ctx, d, cells)) != ELM_OK) return rc;
    if ((rc = grid_sort_bufs(ctx, sc, b, n, cells)) != ELM_OK) return rc;
    (void)hipGetLastError();
    launch_gb_entry_dense(ctx->stream, m->d_pts, (unsigned)n, m->dm.voxel_size, box.lo, (uint64_t)dim[1], (uint64_t)dim[2], b.key[0], b.val[0], d.d_start);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, clk.mark(ctx->stream));
    GridCounts c;
    if ((rc = grid_device_layout(m, clk, b, cells, 0u, d, c)) != ELM_OK) return rc;
    c.on_device = true;
    rc = dense_grid_finish(m, box, c, d, klo, vd, vcells);
    for (int k = 0; rc == ELM_OK && k < ELM_INDEX_STAGES; ++k) m->index_stage_ms[k] = clk.ms(k);
    return rc;
}
// The two-level form on the device; results as build_cell_grid_device.
static int build_tiled_grid_device(elm_map* m) {
    elm_ctx* ctx = m->ctx;
    hipStream_t st = ctx->stream;
    const uint64_t n = m->dm.n_pts;
    if (!grid_device_sizes_ok(n, 0)) return kTryHost;
    GridScratch sc;
    GridStageClock clk;
    int rc;
    int* d_box = nullptr; // six box words, then the 64-bit total of the tile entries
    if ((rc = sc.get(ctx, &d_box, 8)) != ELM_OK) return rc;
    HIPCHK(ctx, clk.mark(st));
    GridBox box;
    if ((rc = grid_box_device(m, box, d_box)) != ELM_OK) return rc;
    HIPCHK(ctx, clk.mark(st));
    const int64_t* dim = box.dim;
    const int64_t tnx = (dim[0] + kTile - 1) / kTile, tny = (dim[1] + kTile - 1) / kTile;
    if (tiled_box_refused(dim, tnx, tny)) return ELM_ERR_UNSUPPORTED;
    const uint64_t n_tiles = (uint64_t)(tnx * tny);
    // z range and entries per tile; the total in 64 bits before the 32-bit scan is trusted
    unsigned *d_zmin = nullptr, *d_zmax = nullptr, *d_tcnt = nullptr, *d_tblk = nullptr, *d_ttot = nullptr;
    unsigned long long* d_total64 = (unsigned long long*)(d_box + 6);
    GridDev d;
    uint2* d_tiles = nullptr;
    {
        size_t dev_free = 0, dev_total = 0;
        HIPCHK(ctx, hipMemGetInfo(&dev_free, &dev_total));
        if (n_tiles * 20 + n * 16 > (uint64_t)dev_free / 10 * 8) return kTryHost;
    }
    if ((rc = sc.get(ctx, &d_zmin, n_tiles)) != ELM_OK) return rc;
    if ((rc = sc.get(ctx, &d_zmax, n_tiles)) != ELM_OK) return rc;
    if ((rc = sc.get(ctx, &d_tcnt, n_tiles)) != ELM_OK) return rc;
    if ((rc = sc.get(ctx, &d_tblk, n_tiles / 1024 + 1)) != ELM_OK) return rc;
    if ((rc = sc.get(ctx, &d_ttot, 4)) != ELM_OK) return rc;
    {
        const hipError_t e = hipMalloc((void**)&d_tiles, n_tiles * sizeof(uint2));
        if (e != hipSuccess) {
            (void)hipGetLastError();
            return e == hipErrorOutOfMemory ? kTryHost : ELM_ERR_DEVICE;
        }
        d.d_side = d_tiles;
    }
    HIPCHK(ctx, hipMemsetAsync(d_zmin, 0xFF, n_tiles * sizeof(unsigned), st));
    HIPCHK(ctx, hipMemsetAsync(d_zmax, 0, n_tiles * sizeof(unsigned), st));
    HIPCHK(ctx, hipMemsetAsync(d_total64, 0, sizeof(unsigned long long), st));
    (void)hipGetLastError();
    launch_gb_tile_z(st, m->d_pts, (unsigned)n, m->dm.voxel_size, box.lo, (uint64_t)tny, d_zmin, d_zmax);
    launch_gb_tile_cnt(st, d_zmin, d_zmax, (unsigned)n_tiles, d_tcnt, d_total64);
    HIPCHK(ctx, hipGetLastError());
    unsigned long long tile_entries = 0;
    HIPCHK(ctx, hipMemcpyAsync(&tile_entries, d_total64, sizeof(tile_entries), hipMemcpyDeviceToHost, st));
    HIPCHK(ctx, hipStreamSynchronize(st));
    // entries 0 .. 63: the shared zero run of every empty tile (nz = 0: one entry per column)
    const uint64_t entries = (uint64_t)kTile * kTile + tile_entries;
    if (entries > 0xFFFFFFF0ull) return ELM_ERR_UNSUPPORTED;
    if (!grid_device_sizes_ok(n, entries)) return kTryHost;
    bool ok = false;
    if ((rc = tiled_budget(m, entries, n_tiles, false, grid_device_scratch_bytes(n, entries) + n_tiles * 12, &ok)) != ELM_OK) return rc;
    if (!ok) return kTryHost;
    launch_bd_scan(st, d_tcnt, (unsigned)n_tiles, d_tblk, d_ttot);
    launch_gb_tiles(st, d_zmin, d_zmax, d_tcnt, (unsigned)n_tiles, d_tiles);
    HIPCHK(ctx, hipGetLastError());
    GridSortBufs b;
    if ((rc = grid_start_table(ctx, d, entries)) != ELM_OK) return rc;
    if ((rc = grid_sort_bufs(ctx, sc, b, n, entries)) != ELM_OK) return rc;
    // entry order = (tile, column, z); the extra entry of every column (index nz) holds no point: its start = the column's end
    launch_gb_entry_tiled(st, m->d_pts, (unsigned)n, m->dm.voxel_size, box.lo, (uint64_t)tny, d_tiles, b.key[0], b.val[0], d.d_start);
    HIPCHK(ctx, hipGetLastError());
    HIPCHK(ctx, clk.mark(st));
    GridCounts c;
    if ((rc = grid_device_layout(m, clk, b, entries, (unsigned)(kTile * kTile), d, c)) != ELM_OK) return rc;
    c.on_device = true;
    rc = tiled_grid_finish(m, box, c, d, tnx, tny);
    for (int k = 0; rc == ELM_OK && k < ELM_INDEX_STAGES; ++k) m->index_stage_ms[k] = clk.ms(k);
    return rc;
}

// Dense half-voxel cell grid (see DevMap::grid_*): the map points once, counting-sorted by cell on the host (init time), the
// offsets of every cell of the bounding box (+ 2 cells of margin), and the dense voxel box of walk statistics.
// ELM_ERR_UNSUPPORTED (and grid_refused) when the grid is not affordable -- the box needs more than max_cells cells, its tables
// do not fit the host / device memory that is free right now, or an allocation fails half-way -- the caller then builds the
// neighbourhood lists instead; nothing is left allocated and the map is unchanged.
static int build_cell_grid_impl(elm_map* m, uint64_t max_cells) {
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = m->dm.n_pts;
    const double vs = m->dm.voxel_size;
    if (n == 0 || m->dm.n_vox == 0) return ELM_ERR_UNSUPPORTED;
    int rc;
    if (m->index_build == ELM_INDEX_BUILD_DEVICE) { // the same form from the device producer; kTryHost: from this one after all
        rc = build_cell_grid_device(m, max_cells);
        if (rc != kTryHost) {
            if (rc != ELM_OK) m->grid_refused = true; // as for the host's refusals below
            return rc;
        }
    }
    GridBox box;
    if ((rc = grid_box(m, box)) != ELM_OK) return rc;
    const std::vector<float4>& pts = box.pts;
    const int32_t* lo = box.lo;
    const int64_t* dim = box.dim;
    const uint64_t cells = (uint64_t)dim[0] * (uint64_t)dim[1] * (uint64_t)dim[2];
    if (dense_box_refused(dim, cells, max_cells)) {
        m->grid_refused = true;
        return ELM_ERR_UNSUPPORTED;
    }
    int32_t klo[3];
    int64_t vd[3];
    const uint64_t vcells = dense_vox_box(m, klo, vd);
    if (vcells > max_cells) {
        m->grid_refused = true;
        return ELM_ERR_UNSUPPORTED;
    }
    {
        bool ok = false;
        if ((rc = dense_budget(m, cells, vcells, true, 0, &ok)) != ELM_OK) return rc;
        if (!ok) {
            m->grid_refused = true;
            return ELM_ERR_UNSUPPORTED;
        }
    }
    // the entry of a point is its linear cell
    GridHost g;
    {
        std::vector<uint32_t> lin(n);
        for (size_t i = 0; i < n; ++i) {
            const uint64_t l = ((uint64_t)(grid_cell_of((double)pts[i].x, vs) - lo[0]) * (uint64_t)dim[1] + (uint64_t)(grid_cell_of((double)pts[i].y, vs) - lo[1])) * (uint64_t)dim[2] +
                               (uint64_t)(grid_cell_of((double)pts[i].z, vs) - lo[2]);
            lin[i] = (uint32_t)l;
        }
        // stage 1 addresses blocks by 32-bit BYTE offsets (one scalar base + a lane offset) while the array stays below 4 GB (~275 M map
        // points), by 32-bit offsets in 16-byte units beyond (template flag WIDE: one 64-bit shift-add per block); slot numbers are ints
        g.n_blk = grid_block_layout((const float*)pts.data(), n, lin, cells, kGridMaxBlocks, g.start, g.gb, g.gi);
    }
    if (g.n_blk > kGridMaxBlocks) { m->grid_refused = true; return ELM_ERR_UNSUPPORTED; }
    std::vector<float4>().swap(box.pts);
    // device side: into locals, committed to the map only when every step has succeeded
    {
        GridDev d;
        GridCounts c;
        c.n_blk = g.n_blk;
        c.n_start = g.start.size();
        if ((rc = grid_upload(ctx, g, d)) == ELM_OK) rc = dense_grid_finish(m, box, c, d, klo, vd, vcells);
    }
    if (rc != ELM_OK) m->grid_refused = true; // do not retry a multi-GB build at every registration
    return rc;
}
static int build_cell_grid(elm_map* m, uint64_t max_cells) {
    if (m->has_grid) return ELM_OK;
    try {
        return build_cell_grid_impl(m, max_cells);
    } catch (const std::bad_alloc&) { // a host table did not fit after all: same answer as the byte budget above
        m->ctx->last_error = "cell grid: host allocation failed";
        m->grid_refused = true;
        return ELM_ERR_UNSUPPORTED;
    }
}

// The two-level form of the cell grid (DevMap::grid_tiles): for maps whose bounding box is too large or too sparse for one dense
// offset table (a city-scale map at half-metre cells: billions of cells, a few hundred thousand of them occupied).  The same
// blocks, sorted (tile, column, z); offsets only inside occupied tiles and only over each tile's own z range.  Host-side build
// like the dense one; nothing is left allocated on failure.  This builder never sets grid_refused: build_search_index does, when
// neither form can be built.
static int build_tiled_grid_impl(elm_map* m) {
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = m->dm.n_pts;
    const double vs = m->dm.voxel_size;
    if (n == 0 || m->dm.n_vox == 0) return ELM_ERR_UNSUPPORTED;
    int rc;
    if (m->index_build == ELM_INDEX_BUILD_DEVICE) { // the same form from the device producer; kTryHost: from this one after all
        rc = build_tiled_grid_device(m);
        if (rc != kTryHost) return rc;
    }
    GridBox box;
    if ((rc = grid_box(m, box)) != ELM_OK) return rc;
    const std::vector<float4>& pts = box.pts;
    const int32_t* lo = box.lo;
    const int64_t* dim = box.dim;
    const int64_t tnx = (dim[0] + kTile - 1) / kTile, tny = (dim[1] + kTile - 1) / kTile;
    if (tiled_box_refused(dim, tnx, tny)) return ELM_ERR_UNSUPPORTED;
    const size_t n_tiles = (size_t)(tnx * tny);
    auto cell3 = [&](size_t i, int32_t& cx, int32_t& cy, int32_t& cz) {
        cx = grid_cell_of((double)pts[i].x, vs) - lo[0];
        cy = grid_cell_of((double)pts[i].y, vs) - lo[1];
        cz = grid_cell_of((double)pts[i].z, vs) - lo[2];
    };
    std::vector<uint16_t> zmin(n_tiles, 0xFFFFu), zmax(n_tiles, 0u);
    for (size_t i = 0; i < n; ++i) {
        int32_t cx, cy, cz;
        cell3(i, cx, cy, cz);
        const size_t t = (size_t)(cx >> kTileShift) * (size_t)tny + (size_t)(cy >> kTileShift);
        zmin[t] = std::min<uint16_t>(zmin[t], (uint16_t)cz);
        zmax[t] = std::max<uint16_t>(zmax[t], (uint16_t)cz);
    }
    std::vector<uint2> tiles(n_tiles);
    uint64_t entries = (uint64_t)kTile * kTile; // entries 0 .. 63: the shared zero run of every empty tile (nz = 0: one entry per column)
    for (size_t t = 0; t < n_tiles; ++t) {
        if (zmin[t] == 0xFFFFu) { tiles[t] = make_uint2(0u, 0u); continue; }
        const uint32_t nz = (uint32_t)zmax[t] - zmin[t] + 1;
        tiles[t] = make_uint2((uint32_t)entries, (uint32_t)zmin[t] | (nz << 16));
        entries += (uint64_t)kTile * kTile * (nz + 1);
        if (entries > 0xFFFFFFF0ull) return ELM_ERR_UNSUPPORTED;
    }
    auto entry_of = [&](int32_t cx, int32_t cy, int32_t cz) -> uint32_t {
        const uint2 te = tiles[(size_t)(cx >> kTileShift) * (size_t)tny + (size_t)(cy >> kTileShift)];
        const uint32_t z0 = te.y & 0xFFFFu, nz = te.y >> 16;
        return te.x + (uint32_t)(((cx & (kTile - 1)) << kTileShift) | (cy & (kTile - 1))) * (nz + 1) + ((uint32_t)cz - z0);
    };
    // byte budget, as for the dense grid
    {
        bool ok = false;
        if ((rc = tiled_budget(m, entries, n_tiles, true, 0, &ok)) != ELM_OK) return rc;
        if (!ok) return ELM_ERR_UNSUPPORTED;
    }
    // entry order = (tile, column, z); the extra entry of every column (index nz) holds no point: its start = the column's end
    GridHost g;
    {
        std::vector<uint32_t> ent(n);
        for (size_t i = 0; i < n; ++i) {
            int32_t cx, cy, cz;
            cell3(i, cx, cy, cz);
            ent[i] = entry_of(cx, cy, cz);
        }
        g.n_blk = grid_block_layout((const float*)pts.data(), n, ent, entries, kGridMaxBlocks, g.start, g.gb, g.gi);
    }
    if (g.n_blk > kGridMaxBlocks) return ELM_ERR_UNSUPPORTED;
    for (uint64_t e = 0; e < (uint64_t)kTile * kTile; ++e) g.start[e] = 0; // empty tiles: block 0 .. block 0 (nothing)
    std::vector<float4>().swap(box.pts);
    GridDev d;
    GridCounts c;
    c.n_blk = g.n_blk;
    c.n_start = g.start.size();
    if ((rc = grid_upload(ctx, g, d)) != ELM_OK) return rc;
    uint2* d_tiles = nullptr;
    HIPCHK_OOM(ctx, hipMalloc((void**)&d_tiles, n_tiles * sizeof(uint2)));
    d.d_side = d_tiles;
    HIPCHK_OOM(ctx, hipMemcpy(d_tiles, tiles.data(), n_tiles * sizeof(uint2), hipMemcpyHostToDevice));
    return tiled_grid_finish(m, box, c, d, tnx, tny);
}
static int build_tiled_grid(elm_map* m) {
    if (m->has_grid) return ELM_OK;
    try {
        return build_tiled_grid_impl(m);
    } catch (const std::bad_alloc&) {
        m->ctx->last_error = "tiled cell grid: host allocation failed";
        return ELM_ERR_UNSUPPORTED;
    }
}

// Neighbourhood lists (see DevMap): query voxels = every floor key within +-1 of a stored (trunc) key.
static int build_neighbourhood_lists(elm_map* m) {
    if (!m) return ELM_ERR_INVALID;
    if (m->has_nbr) return ELM_OK;
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    QueryLists ql;
    int rc;
    if ((rc = count_query_lists(m, ql, [&](uint32_t q) { return ql.counts[q]; })) != ELM_OK) return rc;
    const std::vector<uint32_t>&counts = ql.counts, &nocc = ql.nocc, &offs = ql.offs;
    const uint32_t n_q = ql.n_q;
    const uint64_t total = ql.total;
    int32_t* const d_qkeys = ql.d_qkeys;
    uint32_t *const d_counts = ql.d_counts, *const d_off = ql.d_off;
    if (total > 0xFFFFFFF0ull) {
        ctx->last_error = "neighbourhood lists exceed 2^32 entries";
        return ELM_ERR_UNSUPPORTED;
    }
    HIPCHK(ctx, hipMalloc((void**)&m->d_nbr_pts, std::max<size_t>((size_t)total * sizeof(Pt3), 256) + 64)); // + pad: blocks of 4 are read whole
    HIPCHK(ctx, hipMalloc((void**)&m->d_nbr_idx, std::max<size_t>((size_t)total * sizeof(uint32_t), 256)));
    if (n_q) {
        (void)hipGetLastError();
        launch_nbr_fill(ctx->stream, m->dm, d_qkeys, n_q, d_off, m->d_nbr_pts, m->d_nbr_idx);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    // sort every list by half-voxel cell and write the per-list offset tables (cell-indexed kernel)
    uint32_t max_count = 0;
    for (uint32_t q = 0; q < n_q; ++q) max_count = std::max(max_count, counts[q]);
    const size_t cell_bytes = std::max<size_t>((size_t)n_q * nbr_cell_stride() * sizeof(uint16_t), 256);
    HIPCHK(ctx, hipMalloc((void**)&m->d_nbr_cell_off, cell_bytes));
    HIPCHK(ctx, hipMemsetAsync(m->d_nbr_cell_off, 0, cell_bytes, ctx->stream));
    m->has_cells = max_count <= 1024;
    if (n_q && m->has_cells) {
        (void)hipGetLastError();
        launch_nbr_cellsort(ctx->stream, m->dm, d_qkeys, n_q, d_off, d_counts, m->d_nbr_pts, m->d_nbr_idx, m->d_nbr_cell_off);
        HIPCHK(ctx, hipGetLastError());
    }
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const uint32_t qcap = next_pow2((uint64_t)n_q * 2);
    if ((rc = upload_query_slots(ctx, ql, qcap, &m->d_qslots, [&](uint32_t q, HashSlot& s) { s.start = offs[q]; s.cnt = counts[q]; s.pad0 = nocc[q]; })) != ELM_OK) return rc;
    m->dm.qslots = m->d_qslots;
    m->dm.qmask = qcap - 1;
    m->dm.n_q = n_q;
    m->dm.nbr_pts = m->d_nbr_pts;
    m->dm.nbr_idx = m->d_nbr_idx;
    m->dm.nbr_cell_off = m->d_nbr_cell_off;
    m->has_nbr = true;
    m->info.device_bytes += (size_t)total * (sizeof(Pt3) + sizeof(uint32_t)) + (size_t)qcap * sizeof(HashSlot) + cell_bytes;
    m->info.n_query_voxels = n_q;
    m->info.nbr_entries = total;
    m->info.index_bytes += (size_t)total * sizeof(Pt3) + (size_t)qcap * sizeof(HashSlot) + cell_bytes;
    m->info.index_part_bytes[3] += (size_t)total * sizeof(Pt3) + (size_t)qcap * sizeof(HashSlot) + cell_bytes;
    return ELM_OK;
}

// The P2P / GICP search index of a map: the dense cell grid when its bounding box fits the cell and byte budgets, the two-level
// (tiled) grid when it does not -- large or sparse maps keep the grid kernel -- and the per-query-voxel neighbourhood lists only
// when neither can be built (or with ELM_KERNEL=lists; ELM_GRID=tiled forces the two-level form, ELM_GRID=dense forbids it).
int elm_host::build_search_index(elm_map* m, bool* use_grid) {
    *use_grid = false;
    elm_ctx* ctx = m->ctx;
    if (ctx->kernel_mode == 4 && !m->grid_refused && m->dm.n_pts) {
        const bool force_tiled = env_token("ELM_GRID", "tiled"), no_tiled = env_token("ELM_GRID", "dense");
        int rc = force_tiled ? ELM_ERR_UNSUPPORTED : build_cell_grid(m, grid_max_cells());
        if (rc == ELM_ERR_UNSUPPORTED && !no_tiled) {
            rc = build_tiled_grid(m);
            if (rc == ELM_ERR_UNSUPPORTED) m->grid_refused = true; // neither form: do not retry at every registration
            else if (rc == ELM_OK) m->grid_refused = false;
        }
        if (rc == ELM_OK) {
            *use_grid = true;
            return ELM_OK;
        }
        if (rc != ELM_ERR_UNSUPPORTED) return rc;
    }
    return build_neighbourhood_lists(m);
}
extern "C" int elm_map_build_neighbourhoods(elm_map* m) {
    if (!m) return ELM_ERR_INVALID;
    if (!m->replicas.empty() && group_call(m->ctx)) return elm_multi::map_call(m, 2, 0.0);
    bool g;
    return build_search_index(m, &g);
}

// ---- device index build: the preference, the stage times, the read-back of the grid
extern "C" int elm_map_set_index_build(elm_map* m, int where) {
    if (!m || (where != ELM_INDEX_BUILD_HOST && where != ELM_INDEX_BUILD_DEVICE)) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    if (!m->replicas.empty() || group_call(ctx) || ctx->comm || ctx->hook) {
        ctx->last_error = "elm_map_set_index_build: one rank only (not a map with replicas, a device group's lead, nor with a communicator or hook attached)";
        return ELM_ERR_UNSUPPORTED;
    }
    if (m->has_grid) return ELM_OK; // built: nothing changes
    m->index_build = where;
    return ELM_OK;
}
extern "C" int elm_map_index_build_stages(const elm_map* m, double ms[ELM_INDEX_STAGES]) {
    if (!m || !ms || !m->has_grid || !(m->info.layout_flags & 512)) return ELM_ERR_INVALID;
    for (int k = 0; k < ELM_INDEX_STAGES; ++k) ms[k] = m->index_stage_ms[k];
    return ELM_OK;
}
extern "C" int elm_map_download_cell_grid(const elm_map* m, elm_cell_grid_desc* desc, uint32_t* start, size_t start_cap, float* blocks12,
                                          size_t block_cap, uint32_t* slot_point, size_t slot_cap, uint32_t* tiles2, size_t tile_cap) {
    if (!m || !desc) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    if (!m->has_grid) {
        ctx->last_error = "elm_map_download_cell_grid: the map has no cell grid";
        return ELM_ERR_UNSUPPORTED;
    }
    const DevMap& dm = m->dm;
    elm_cell_grid_desc ds{};
    ds.gx0 = dm.gx0; ds.gy0 = dm.gy0; ds.gz0 = dm.gz0; ds.gnx = dm.gnx; ds.gny = dm.gny; ds.gnz = dm.gnz;
    ds.vx0 = dm.vx0; ds.vy0 = dm.vy0; ds.vz0 = dm.vz0; ds.vnx = dm.vnx; ds.vny = dm.vny; ds.vnz = dm.vnz;
    ds.gtny = dm.gtny; ds.grid_tiled = dm.grid_tiled; ds.grid_wide = dm.grid_wide; ds.grid_nslots = dm.grid_nslots;
    ds.n_start_words = m->grid_start_words;
    ds.n_blocks = m->grid_slots / 4;
    ds.n_tiles = dm.grid_tiled ? (uint64_t)(dm.gnx / kTile) * (uint64_t)(dm.gny / kTile) : 0;
    *desc = ds;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    const size_t ns = std::min<size_t>(start_cap, ds.n_start_words), nb = std::min<size_t>(block_cap, ds.n_blocks),
                 ni = std::min<size_t>(slot_cap, m->grid_slots), nt = std::min<size_t>(tile_cap, ds.n_tiles);
    if (start && ns) HIPCHK(ctx, hipMemcpy(start, m->d_grid_start, ns * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (blocks12 && nb) HIPCHK(ctx, hipMemcpy(blocks12, m->d_grid_blk, nb * sizeof(GridBlk), hipMemcpyDeviceToHost));
    if (slot_point && ni) HIPCHK(ctx, hipMemcpy(slot_point, m->d_grid_idx, ni * sizeof(uint32_t), hipMemcpyDeviceToHost));
    if (tiles2 && nt) HIPCHK(ctx, hipMemcpy(tiles2, m->d_grid_tiles, nt * sizeof(uint2), hipMemcpyDeviceToHost));
    return ELM_OK;
}
