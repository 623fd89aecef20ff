// elm_scan.cpp -- scans: upload (pinned staging, Hilbert ordering on the device), the handle and buffer pools, download, and the
// deskew front end (elm_deskew, elm_deskew_downsample, elm_deskew_prepare).  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "elm_host_types.hpp"

using namespace elm;
using namespace elm_host;

// ------------------------------------------------------------------------------------------------------
// scans
// ------------------------------------------------------------------------------------------------------

// index of cell (x, y) along a Hilbert curve over a 2^order x 2^order grid
static inline uint32_t hilbert_xy2d(uint32_t order, uint32_t x, uint32_t y) {
    uint32_t d = 0;
    for (uint32_t s = 1u << (order - 1); s > 0; s >>= 1) {
        const uint32_t rx = (x & s) ? 1u : 0u, ry = (y & s) ? 1u : 0u;
        d += s * s * ((3u * rx) ^ ry);
        if (ry == 0) { // rotate the quadrant
            if (rx == 1) { x = s - 1 - x; y = s - 1 - y; }
            const uint32_t t = x; x = y; y = t;
        }
    }
    return d;
}

// The ordering grid's Hilbert table (kOrderCells^2 16-bit entries), uploaded once per context.
int elm_host::ensure_hilbert(elm_ctx* ctx) {
    if (ctx->d_hilbert) return ELM_OK;
    static_assert(kOrderCells == 64, "hilbert_xy2d order below");
    std::vector<uint16_t> lut((size_t)kOrderCells * kOrderCells);
    for (int y = 0; y < kOrderCells; ++y)
        for (int x = 0; x < kOrderCells; ++x) lut[(size_t)y * kOrderCells + x] = (uint16_t)hilbert_xy2d(6, (uint32_t)x, (uint32_t)y);
    HIPCHK(ctx, hipMalloc((void**)&ctx->d_hilbert, lut.size() * sizeof(uint16_t)));
    HIPCHK(ctx, hipMemcpy(ctx->d_hilbert, lut.data(), lut.size() * sizeof(uint16_t), hipMemcpyHostToDevice));
    return ELM_OK;
}

// A scan handle + a device buffer of at least n points, both from the context's pools when possible (a scan per LiDAR message: no
// hipMalloc / hipFree on the per-scan path after warm-up).
int elm_host::scan_alloc(elm_ctx* ctx, size_t n, elm_scan** out) {
    elm_scan* s;
    if (!ctx->scan_free.empty()) {
        s = ctx->scan_free.back();
        ctx->scan_free.pop_back();
        *s = elm_scan();
    } else {
        s = new (std::nothrow) elm_scan();
        if (!s) return ELM_ERR_ALLOC;
    }
    s->ctx = ctx;
    s->ctx_id = ctx->id;
    const size_t need = std::max<size_t>(n * sizeof(Pt3), 256);
    int best = -1; // smallest pooled buffer that fits
    for (int i = 0; i < (int)ctx->scan_pool.size(); ++i)
        if (ctx->scan_pool[i].second >= need && (best < 0 || ctx->scan_pool[i].second < ctx->scan_pool[best].second)) best = i;
    if (best >= 0) {
        s->d_pts = (Pt3*)ctx->scan_pool[best].first;
        s->cap_bytes = ctx->scan_pool[best].second;
        ctx->scan_pool.erase(ctx->scan_pool.begin() + best);
    } else {
        s->cap_bytes = (need + 65535) & ~(size_t)65535;
        const hipError_t e = hipMalloc((void**)&s->d_pts, s->cap_bytes);
        if (e != hipSuccess) {
            ctx->last_error = std::string("scan buffer allocation: ") + hipGetErrorString(e);
            delete s;
            return ELM_ERR_DEVICE;
        }
    }
    *out = s;
    return ELM_OK;
}

// Uploads one scan: the caller's packed float32 xyz (12 bytes per point) goes to HBM as it is -- no repack, no host-side sort.
// order = true: the points are then ordered ON THE DEVICE along a Hilbert curve over 2 m x 2 m sensor-frame cells (k_scan_order,
// ~0.1 ms per 131 072-point scan; the host radix sort of round 2 took 1.3 ms) -- consecutive points, hence every 256-point workgroup
// and, through the XCD-aware block mapping, every XCD's L2, touch a few adjacent map cells: +11..13 % registrations/s on resident
// scans.  order = false (elm_register): the caller's order; ordering one scan costs more than it saves on ONE registration.
// No allocation after warm-up: pinned staging, scan handles and device buffers are pooled in the context.
// Copy into page-locked staging memory that the CPU will not read again: non-temporal 32-byte stores (no read-for-ownership of the
// destination lines, no cache pollution) where the CPU has AVX2, memcpy otherwise.  dst must be 32-byte aligned (staging buffers are).
#include <immintrin.h>
__attribute__((target("avx2"))) static void stage_copy_avx2(void* dst, const void* src, size_t len) {
    char* d = (char*)dst;
    const char* s = (const char*)src;
    size_t i = 0;
    for (; i + 128 <= len; i += 128) {
        const __m256i a = _mm256_loadu_si256((const __m256i*)(s + i)), b = _mm256_loadu_si256((const __m256i*)(s + i + 32));
        const __m256i c = _mm256_loadu_si256((const __m256i*)(s + i + 64)), e = _mm256_loadu_si256((const __m256i*)(s + i + 96));
        _mm256_stream_si256((__m256i*)(d + i), a);
        _mm256_stream_si256((__m256i*)(d + i + 32), b);
        _mm256_stream_si256((__m256i*)(d + i + 64), c);
        _mm256_stream_si256((__m256i*)(d + i + 96), e);
    }
    _mm_sfence();
    if (i < len) memcpy(d + i, s + i, len - i);
}
static void stage_copy(void* dst, const void* src, size_t len) {
    static const bool avx2 = __builtin_cpu_supports("avx2");
    if (avx2 && (((uintptr_t)dst) & 31u) == 0) stage_copy_avx2(dst, src, len);
    else memcpy(dst, src, len);
}

int elm_host::scan_upload_impl(elm_ctx* ctx, const float* xyz, size_t n, size_t n_total, bool order, bool sync, elm_scan** out) {
    if (!ctx || !out || (!xyz && n) || n > 0x7FFFFFFFull || n_total > 0x7FFFFFFFull || n_total < n) return ELM_ERR_INVALID;
    *out = nullptr;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t bytes = n * sizeof(Pt3);
    int rc = pinned_reserve(ctx, &ctx->h_stage, &ctx->h_stage_cap, std::max<size_t>(bytes + sizeof(OrderJob), 4096));
    if (rc != ELM_OK) return rc;
    elm_scan* s = nullptr;
    if ((rc = scan_alloc(ctx, n, &s)) != ELM_OK) return rc;
    s->n = (uint32_t)n;
    s->n_total = (uint32_t)n_total;
    const bool do_order = order && ctx->scan_order && n > 1;
    hipError_t e = hipSuccess;
    // A page-locked source (elm_host_alloc, hipHostMalloc, hipHostRegister) is read by the DMA engine where it lies.  A pageable one
    // goes through the context's pinned staging buffer in pieces, so that the copy of piece k + 1 overlaps the DMA of piece k
    // (the runtime's own staging of pageable memory is several times slower).
    bool pinned_src = false;
    if (n) {
        hipPointerAttribute_t attr;
        if (hipPointerGetAttributes(&attr, xyz) == hipSuccess && attr.type == hipMemoryTypeHost) pinned_src = true;
        else (void)hipGetLastError();
    }
    auto upload = [&](void* dst) -> hipError_t {
        if (!n) return hipSuccess;
        if (pinned_src) return hipMemcpyAsync(dst, xyz, bytes, hipMemcpyHostToDevice, ctx->stream);
        const size_t piece = (size_t)384 << 10;
        hipError_t ee = hipSuccess;
        for (size_t o = 0; o < bytes && ee == hipSuccess; o += piece) {
            const size_t len = std::min(piece, bytes - o);
            stage_copy((char*)ctx->h_stage + o, (const char*)xyz + o, len); // (pieces are multiples of 32 bytes)
            ee = hipMemcpyAsync((char*)dst + o, (const char*)ctx->h_stage + o, len, hipMemcpyHostToDevice, ctx->stream);
        }
        return ee;
    };
    if (!do_order) {
        e = upload(s->d_pts);
    } else {
        rc = ensure_hilbert(ctx);
        if (rc == ELM_OK) rc = dev_reserve(ctx, ctx->d_raw, bytes);
        const bool wide = n >= 16384; // one scan on its own: many workgroups (same bytes, ~10x sooner)
        const size_t tmp_bytes = ((n * sizeof(uint32_t) + 255) / 256) * 256;
        if (rc == ELM_OK) rc = dev_reserve(ctx, ctx->d_order_tmp, tmp_bytes + (wide ? order_wide_scratch_bytes((unsigned)n) : 0));
        if (rc == ELM_OK) rc = dev_reserve(ctx, ctx->d_order_jobs, sizeof(OrderJob));
        if (rc != ELM_OK) { elm_scan_destroy(s); return rc; }
        OrderJob* hj = (OrderJob*)((char*)ctx->h_stage + ((bytes + 15) & ~(size_t)15));
        if ((char*)(hj + 1) > (char*)ctx->h_stage + ctx->h_stage_cap) { // keep the descriptor inside the staging buffer
            rc = pinned_reserve(ctx, &ctx->h_jobs, &ctx->h_jobs_cap, 4096);
            if (rc != ELM_OK) { elm_scan_destroy(s); return rc; }
            hj = (OrderJob*)ctx->h_jobs;
        }
        hj->src = (const Pt3*)ctx->d_raw.p; hj->dst = s->d_pts; hj->tmp = (uint32_t*)ctx->d_order_tmp.p; hj->n = (uint32_t)n; hj->_pad = 0;
        e = upload(ctx->d_raw.p);
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->d_order_jobs.p, hj, sizeof(OrderJob), hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess) {
            (void)hipGetLastError();
            if (wide) launch_scan_order_wide(ctx->stream, (const OrderJob*)ctx->d_order_jobs.p, (unsigned)n, ctx->d_hilbert, (char*)ctx->d_order_tmp.p + tmp_bytes);
            else launch_scan_order(ctx->stream, (const OrderJob*)ctx->d_order_jobs.p, 1, ctx->d_hilbert);
            e = hipGetLastError();
        }
    }
    if (e == hipSuccess && sync) e = hipStreamSynchronize(ctx->stream); // the pinned staging buffer is reused by the next upload
    if (e != hipSuccess) {
        ctx->last_error = std::string("scan upload: ") + hipGetErrorString(e);
        elm_scan_destroy(s);
        return ELM_ERR_DEVICE;
    }
    *out = s;
    return ELM_OK;
}

extern "C" int elm_scan_upload(elm_ctx* ctx, const float* xyz, size_t n, size_t n_total, elm_scan** out) {
    if (group_call(ctx)) { // sharded over the group (the whole scan is handed over: a shard of a shard is not a thing)
        if (n_total != n) return ELM_ERR_INVALID;
        return elm_multi::scan_upload(ctx, xyz, n, out);
    }
    return scan_upload_impl(ctx, xyz, n, n_total, true, true, out);
}

extern "C" void elm_scan_destroy(elm_scan* s) {
    if (!s || !s->ctx) return; // a handle that is already back in the pool (double destroy)
    if (!s->shards.empty()) { // a group scan: the other ranks' shards first (each returns to its own context's pool)
        std::vector<elm_scan*> sh;
        sh.swap(s->shards);
        for (elm_scan* q : sh) elm_scan_destroy(q);
    }
    if (!ctx_alive(s->ctx, s->ctx_id)) { // the context went first (or its address was reused): release the device buffer, nothing to pool
        if (s->d_pts) (void)hipFree(s->d_pts);
        delete s;
        return;
    }
    elm_ctx* ctx = s->ctx;
    (void)hipSetDevice(ctx->device);
    if (s->d_pts) {
        if (ctx->scan_pool.size() < 64) {
            // the stream is in order: a later upload into this buffer is queued behind every kernel that still reads it
            ctx->scan_pool.emplace_back((void*)s->d_pts, s->cap_bytes);
        } else {
            (void)hipFree(s->d_pts);
        }
    }
    s->d_pts = nullptr;
    s->ctx = nullptr;
    if (ctx->scan_free.size() < 64) ctx->scan_free.push_back(s);
    else delete s;
}
extern "C" size_t elm_scan_size(const elm_scan* s) { return !s ? 0 : (s->shards.empty() ? s->n : s->n_total); }
extern "C" int elm_scan_download(const elm_scan* s, float* xyz, size_t cap) {
    if (!s || !s->ctx || (!xyz && cap)) return ELM_ERR_INVALID;
    if (!s->shards.empty() && group_call(s->ctx)) { // a group scan: rank 0's shard, then the others', each in its device order
        size_t done = std::min<size_t>(cap, s->n);
        elm_scan first = *s; // (a view without the shard list: the plain path below)
        first.shards.clear();
        int rc = elm_scan_download(&first, xyz, done);
        for (const elm_scan* q : s->shards) {
            if (rc != ELM_OK || done >= cap) break;
            const size_t k = std::min<size_t>(cap - done, q->n);
            rc = elm_scan_download(q, xyz + 3 * done, k);
            done += k;
        }
        return rc;
    }
    elm_ctx* ctx = s->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = std::min<size_t>(cap, s->n);
    if (!n) return ELM_OK;
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream)); // the kernels that fill the scan run on the context stream
    HIPCHK(ctx, hipMemcpy(xyz, s->d_pts, n * sizeof(Pt3), hipMemcpyDeviceToHost)); // packed xyz on both sides
    return ELM_OK;
}

// ------------------------------------------------------------------------------------------------------
// deskew
// ------------------------------------------------------------------------------------------------------
// the deskew kernel's arguments: the scalars of `tab`, its four tables (time, rot_x, rot_y, rot_z) of `rows` doubles each back to back at d_tab
DeskewDev elm_host::deskew_args(const elm_deskew_tables* tab, const double* d_tab, size_t rows) {
    DeskewDev d;
    d.time_scan_cur = tab->d_time_scan_cur;
    d.time_scan_end = tab->d_time_scan_end;
    d.imu_pointer_cur = tab->i_imu_pointer_cur;
    d.odom_available = tab->b_is_odom_available;
    d.incre_x = tab->f_odom_incre_x; d.incre_y = tab->f_odom_incre_y; d.incre_z = tab->f_odom_incre_z;
    d._pad = 0.f;
    d.imu_time = d_tab; d.rot_x = d_tab + rows; d.rot_y = d_tab + 2 * rows; d.rot_z = d_tab + 3 * rows;
    return d;
}
// uploads the raw points + tables and runs the deskew kernel; the undistorted points (3 floats each) stay on the device
static int deskew_enqueue(elm_ctx* ctx, const float* xyz, const float* rel_time, size_t n, const elm_deskew_tables* tab, float** d_out_p) {
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t k = (size_t)tab->i_imu_pointer_cur + 1;
    const size_t in_bytes = n * 4 * sizeof(float);
    const size_t tab_bytes = k * 4 * sizeof(double);
    int rc;
    if ((rc = dev_reserve(ctx, ctx->d_stage_pts, in_bytes + n * 3 * sizeof(float) + tab_bytes + 64)) != ELM_OK) return rc;
    if ((rc = pinned_reserve(ctx, &ctx->h_stage, &ctx->h_stage_cap, std::max<size_t>(tab_bytes, 4096))) != ELM_OK) return rc;
    char* base = (char*)ctx->d_stage_pts.p;
    double* d_tab = (double*)base;
    float* d_xyz = (float*)(base + ((tab_bytes + 63) / 64) * 64);
    float* d_time = d_xyz + 3 * n;
    float* d_out = d_time + n;
    HIPCHK(ctx, hipMemcpyAsync(d_xyz, xyz, n * 3 * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    if (!tab->b_run_deskew) { // pcm.cpp:513-525: plain copy
        *d_out_p = d_xyz;
        return ELM_OK;
    }
    double* ht = (double*)ctx->h_stage;
    memcpy(ht, tab->vec_d_imu_time, k * sizeof(double));
    memcpy(ht + k, tab->vec_d_imu_rot_x, k * sizeof(double));
    memcpy(ht + 2 * k, tab->vec_d_imu_rot_y, k * sizeof(double));
    memcpy(ht + 3 * k, tab->vec_d_imu_rot_z, k * sizeof(double));
    HIPCHK(ctx, hipMemcpyAsync(d_tab, ht, tab_bytes, hipMemcpyHostToDevice, ctx->stream));
    HIPCHK(ctx, hipMemcpyAsync(d_time, rel_time, n * sizeof(float), hipMemcpyHostToDevice, ctx->stream));
    (void)hipGetLastError();
    launch_deskew(ctx->stream, d_xyz, d_time, (uint32_t)n, deskew_args(tab, d_tab, k), d_out);
    HIPCHK(ctx, hipGetLastError());
    *d_out_p = d_out;
    return ELM_OK;
}

extern "C" int elm_deskew(elm_ctx* ctx, const float* xyz, const float* rel_time, size_t n, const elm_deskew_tables* tab,
                          float* xyz_out, int* ok) {
    if (!ctx || !tab || !ok || (n && (!xyz || !rel_time || !xyz_out)) || n > 0x7FFFFFFFull) return ELM_ERR_INVALID;
    *ok = 0;
    if (!tab->b_is_imu_available || !tab->b_is_odom_available) return ELM_OK; // pcm.cpp:494-496
    *ok = 1;
    if (!tab->b_run_deskew) { // pcm.cpp:513-525: plain copy
        memcpy(xyz_out, xyz, n * 3 * sizeof(float));
        return ELM_OK;
    }
    if (n == 0) return ELM_OK;
    float* d_out = nullptr;
    int rc = deskew_enqueue(ctx, xyz, rel_time, n, tab, &d_out);
    if (rc != ELM_OK) return rc;
    HIPCHK(ctx, hipMemcpyAsync(xyz_out, d_out, n * 3 * sizeof(float), hipMemcpyDeviceToHost, ctx->stream));
    HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    return ELM_OK;
}

// VoxelHashMap::VoxelDownsample (vhm.hpp:260-283) of `d_und` (n undistorted points in HBM) into a fresh scan, on the context
// stream, no host wait.  {kept points, "a key does not pack" flag} land in device memory right behind the state of a one-scan
// batch, so the registration's own read-back brings them to the host.  The hash table is left clean by the pass itself.
int elm_host::downsample_enqueue(elm_ctx* ctx, const float* d_und, size_t n, double voxel_size, elm_scan** sc_out, unsigned** d_total_out) {
    int rc;
    unsigned cap_log2 = 6;
    while (((size_t)1 << cap_log2) < 2 * std::max<size_t>(n, 1)) ++cap_log2;
    const size_t cap = (size_t)1 << cap_log2, nb = (n + 1023) / 1024;
    const size_t bytes = cap * 12 + std::max<size_t>(n, 1) * 4 + (nb + 1) * 4 + 64;
    if (bytes > ctx->d_ds.cap) ctx->ds_clean_ptr = nullptr; // dev_reserve reallocates: fresh memory (even at the same address) is not "all ones"
    if ((rc = dev_reserve(ctx, ctx->d_ds, bytes)) != ELM_OK) return rc;
    if ((rc = dev_reserve(ctx, ctx->d_state, sizeof(ScanState) + sizeof(StateTail))) != ELM_OK) return rc;
    char* base = (char*)ctx->d_ds.p;
    unsigned long long* d_table = (unsigned long long*)base;
    unsigned* d_first = (unsigned*)(base + cap * 8);
    unsigned* d_slot = d_first + cap;
    unsigned* d_bcount = d_slot + std::max<size_t>(n, 1);
    StateTail* tail = state_tail(ctx->d_state.p, 1);
    elm_scan* sc = nullptr;
    if ((rc = scan_alloc(ctx, n, &sc)) != ELM_OK) return rc;
    hipError_t e = hipSuccess;
    const bool clean = ctx->ds_clean_ptr == ctx->d_ds.p && ctx->ds_clean_cap_log2 == cap_log2;
    ctx->ds_clean_ptr = nullptr; // dirty until this pass has cleaned up after itself
    if (!clean) e = hipMemsetAsync(d_table, 0xFF, cap * 12, ctx->stream); // keys and first indices: all ones
    if (e == hipSuccess) e = hipMemsetAsync(&tail->ds_kept, 0, 8, ctx->stream); // kept points, overflow flag
    if (e == hipSuccess && n) {
        (void)hipGetLastError();
        launch_voxel_downsample(ctx->stream, d_und, (uint32_t)n, voxel_size, d_table, d_first, cap_log2, d_slot, d_bcount, &tail->ds_kept,
                                &tail->ds_overflow, sc->d_pts);
        e = hipGetLastError();
    }
    if (e != hipSuccess) {
        ctx->last_error = std::string("downsample: ") + hipGetErrorString(e);
        elm_scan_destroy(sc);
        return ELM_ERR_DEVICE;
    }
    ctx->ds_clean_ptr = ctx->d_ds.p;
    ctx->ds_clean_cap_log2 = cap_log2;
    sc->n = (uint32_t)n; // upper bound until the host has read the kept count
    sc->n_total = (uint32_t)n;
    *sc_out = sc;
    *d_total_out = &tail->ds_kept;
    return ELM_OK;
}

// DeskewPointCloud's per-point loop + VoxelHashMap::VoxelDownsample fused on the device: the undistorted cloud never leaves
// HBM, what comes out is a resident scan (the kept points in input order) ready for elm_register_batch.
extern "C" int elm_deskew_downsample(elm_ctx* ctx, const float* xyz, const float* rel_time, size_t n, const elm_deskew_tables* tab,
                                     double voxel_size, elm_scan** scan_out, int* ok) {
    if (!ctx || !tab || !ok || !scan_out || !(voxel_size > 0.0) || (n && (!xyz || !rel_time)) || n > 0x7FFFFFFFull) return ELM_ERR_INVALID;
    *ok = 0;
    *scan_out = nullptr;
    if (!tab->b_is_imu_available || !tab->b_is_odom_available) return ELM_OK; // pcm.cpp:494-496
    *ok = 1;
    int rc;
    float* d_und = nullptr;
    if (n) {
        if ((rc = deskew_enqueue(ctx, xyz, rel_time, n, tab, &d_und)) != ELM_OK) return rc;
    }
    elm_scan* sc = nullptr;
    unsigned* d_total = nullptr;
    if ((rc = downsample_enqueue(ctx, d_und, n, voxel_size, &sc, &d_total)) != ELM_OK) return rc;
    unsigned h_total[2] = {0, 0};
    hipError_t e = hipMemcpyAsync(h_total, d_total, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess || h_total[1]) {
        ctx->last_error = e != hipSuccess ? std::string("deskew + downsample: ") + hipGetErrorString(e)
                                          : "a voxel key does not fit the packed device table (|coordinate / voxel size| >= 2^20)";
        elm_scan_destroy(sc);
        return e != hipSuccess ? ELM_ERR_DEVICE : ELM_ERR_UNSUPPORTED;
    }
    sc->n = h_total[0];
    sc->n_total = h_total[0];
    *scan_out = sc;
    return ELM_OK;
}

namespace {
// pcl::getTransformation (float) -- rotation Rz(yaw) Ry(pitch) Rx(roll) and translation
struct Aff3f { float m[3][4]; };
static Aff3f get_transformation_f(float x, float y, float z, float roll, float pitch, float yaw) {
    const float A = cosf(yaw), B = sinf(yaw), C = cosf(pitch), D = sinf(pitch), E = cosf(roll), F = sinf(roll);
    const float DE = D * E, DF = D * F;
    Aff3f t;
    t.m[0][0] = A * C; t.m[0][1] = A * DF - B * E; t.m[0][2] = B * F + A * DE; t.m[0][3] = x;
    t.m[1][0] = B * C; t.m[1][1] = A * E + B * DF; t.m[1][2] = B * DE - A * F; t.m[1][3] = y;
    t.m[2][0] = -D;    t.m[2][1] = C * F;          t.m[2][2] = C * E;          t.m[2][3] = z;
    return t;
}
// tf::Matrix3x3(q).getRPY()
static void quat_to_rpy(const double q[4], double* roll, double* pitch, double* yaw) {
    const double x = q[0], y = q[1], z = q[2], w = q[3];
    const double s = 2.0 / (x * x + y * y + z * z + w * w);
    const double xs = x * s, ys = y * s, zs = z * s;
    const double wx = w * xs, wy = w * ys, wz = w * zs, xx = x * xs, xy = x * ys, xz = x * zs, yy = y * ys, yz = y * zs, zz = z * zs;
    const double m00 = 1.0 - (yy + zz), m10 = xy + wz, m20 = xz - wy, m21 = yz + wx, m22 = 1.0 - (xx + yy);
    if (fabs(m20) >= 1.0) {
        *yaw = 0.0;
        *roll = atan2(m21, m22);
        *pitch = (m20 < 0) ? M_PI / 2.0 : -M_PI / 2.0;
    } else {
        *pitch = -asin(m20);
        const double cp = cos(*pitch);
        *roll = atan2(m21 / cp, m22 / cp);
        *yaw = atan2(m10 / cp, m00 / cp);
    }
}
} // namespace

extern "C" int elm_deskew_prepare(const double* imu4, size_t n_imu, const double* odom14, size_t n_odom, double stamp,
                                  float front_time, float back_time, int lidar_scan_time_end, int run_deskew,
                                  double* tab_time, double* tab_rx, double* tab_ry, double* tab_rz, size_t tab_cap,
                                  elm_deskew_tables* out) {
    if (!out || !tab_time || !tab_rx || !tab_ry || !tab_rz || tab_cap < 2) return ELM_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    // DeskewPointCloud head (pcm.cpp:473-486)
    double scan_cur = stamp, scan_end = stamp + (double)back_time;
    if (lidar_scan_time_end) {
        scan_end = stamp;
        scan_cur = scan_end + (double)front_time;
    }
    out->d_time_scan_cur = scan_cur;
    out->d_time_scan_end = scan_end;
    out->b_run_deskew = run_deskew;
    out->vec_d_imu_time = tab_time; out->vec_d_imu_rot_x = tab_rx; out->vec_d_imu_rot_y = tab_ry; out->vec_d_imu_rot_z = tab_rz;
    // ImuDeskewInfo (pcm.cpp:533-585)
    {
        size_t first = 0;
        while (first < n_imu && imu4[4 * first] < scan_cur - 0.01) ++first;
        int cur = 0;
        if (first < n_imu) {
            for (size_t i = first; i < n_imu; ++i) {
                const double t = imu4[4 * i];
                if (t > scan_end + 0.01) break;
                if ((size_t)cur >= tab_cap) break;
                if (cur == 0) {
                    tab_rx[0] = tab_ry[0] = tab_rz[0] = 0.0;
                    tab_time[0] = t;
                    ++cur;
                    continue;
                }
                const double dt = t - tab_time[cur - 1];
                tab_rx[cur] = tab_rx[cur - 1] + imu4[4 * i + 1] * dt;
                tab_ry[cur] = tab_ry[cur - 1] + imu4[4 * i + 2] * dt;
                tab_rz[cur] = tab_rz[cur - 1] + imu4[4 * i + 3] * dt;
                tab_time[cur] = t;
                ++cur;
            }
            --cur;
            out->i_imu_pointer_cur = cur < 0 ? 0 : cur;
            out->b_is_imu_available = cur > 0 ? 1 : 0;
        }
    }
    // OdomDeskewInfo (pcm.cpp:587-729)
    {
        size_t first = 0;
        while (first < n_odom && odom14[14 * first] < scan_cur - 0.1) ++first;
        if (first < n_odom && !(odom14[14 * first] > scan_cur)) {
            size_t si = first;
            for (size_t i = first; i < n_odom; ++i) {
                si = i;
                if (odom14[14 * i] < scan_cur) continue;
                break;
            }
            const double* so = odom14 + 14 * si;
            double roll, pitch, yaw;
            quat_to_rpy(so + 4, &roll, &pitch, &yaw);
            const Aff3f begin = get_transformation_f((float)so[1], (float)so[2], (float)so[3], (float)roll, (float)pitch, (float)yaw);
            const double* lo = odom14 + 14 * (n_odom - 1);
            double end_stamp, ep[3], eq[4];
            if (lo[0] > scan_end) {
                size_t ei = first;
                for (size_t i = first; i < n_odom; ++i) {
                    ei = i;
                    if (odom14[14 * i] < scan_end) continue;
                    break;
                }
                const double* eo = odom14 + 14 * ei;
                end_stamp = eo[0];
                for (int k = 0; k < 3; ++k) ep[k] = eo[1 + k];
                for (int k = 0; k < 4; ++k) eq[k] = eo[4 + k];
            } else { // extrapolate with the last twist (pcm.cpp:648-708)
                const double dt = scan_end - lo[0];
                end_stamp = scan_end;
                double r2, p2, y2;
                quat_to_rpy(lo + 4, &r2, &p2, &y2);
                const double cy = cos(y2), sy = sin(y2), cp = cos(p2), sp = sin(p2), cr = cos(r2), sr = sin(r2);
                const double R[3][3] = {{cy * cp, cy * sp * sr - sy * cr, cy * sp * cr + sy * sr},
                                        {sy * cp, sy * sp * sr + cy * cr, sy * sp * cr - cy * sr},
                                        {-sp, cp * sr, cp * cr}};
                for (int k = 0; k < 3; ++k) ep[k] = lo[1 + k] + (R[k][0] * lo[8] + R[k][1] * lo[9] + R[k][2] * lo[10]) * dt;
                r2 += lo[11] * dt; p2 += lo[12] * dt; y2 += lo[13] * dt;
                const double cY = cos(y2 * 0.5), sY = sin(y2 * 0.5), cP = cos(p2 * 0.5), sP = sin(p2 * 0.5), cR = cos(r2 * 0.5), sR = sin(r2 * 0.5);
                eq[0] = sR * cP * cY - cR * sP * sY;
                eq[1] = cR * sP * cY + sR * cP * sY;
                eq[2] = cR * cP * sY - sR * sP * cY;
                eq[3] = cR * cP * cY + sR * sP * sY;
            }
            quat_to_rpy(eq, &roll, &pitch, &yaw);
            const Aff3f end = get_transformation_f((float)ep[0], (float)ep[1], (float)ep[2], (float)roll, (float)pitch, (float)yaw);
            // (begin^-1 * end).translation(), float32 (Eigen Affine3f: linear().inverse(), -linv * t)
            float L[9], Li[9];
            for (int i = 0; i < 3; ++i)
                for (int j = 0; j < 3; ++j) L[i * 3 + j] = begin.m[i][j];
            {
                const float c00 = L[4] * L[8] - L[5] * L[7], c01 = L[5] * L[6] - L[3] * L[8], c02 = L[3] * L[7] - L[4] * L[6];
                const float det = (c00 * L[0] + c01 * L[1]) + c02 * L[2];
                const float id = 1.0f / det;
                Li[0] = c00 * id; Li[3] = c01 * id; Li[6] = c02 * id;
                Li[1] = (L[2] * L[7] - L[1] * L[8]) * id; Li[4] = (L[0] * L[8] - L[2] * L[6]) * id; Li[7] = (L[1] * L[6] - L[0] * L[7]) * id;
                Li[2] = (L[1] * L[5] - L[2] * L[4]) * id; Li[5] = (L[2] * L[3] - L[0] * L[5]) * id; Li[8] = (L[0] * L[4] - L[1] * L[3]) * id;
            }
            float bt[3];
            for (int i = 0; i < 3; ++i) {
                const float ti = -((Li[i * 3] * begin.m[0][3] + Li[i * 3 + 1] * begin.m[1][3]) + Li[i * 3 + 2] * begin.m[2][3]);
                bt[i] = ((Li[i * 3] * end.m[0][3] + Li[i * 3 + 1] * end.m[1][3]) + Li[i * 3 + 2] * end.m[2][3]) + ti * 1.0f;
            }
            // InterpolateTfWithTime (lf.hpp:219-241): only the translation reaches the per-point deskew
            const double dt_scan = scan_end - scan_cur, dt_trans = end_stamp - so[0];
            if (dt_trans == 0.0) {
                out->f_odom_incre_x = out->f_odom_incre_y = out->f_odom_incre_z = 0.f;
            } else {
                const float fr = (float)(dt_scan / dt_trans);
                out->f_odom_incre_x = bt[0] * fr;
                out->f_odom_incre_y = bt[1] * fr;
                out->f_odom_incre_z = bt[2] * fr;
            }
            out->b_is_odom_available = 1;
        }
    }
    return ELM_OK;
}
