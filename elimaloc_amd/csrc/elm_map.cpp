// elm_map.cpp -- the device-resident voxel map: the host build (AddPoints) and its upload, the slot table, the covariances, info and
// downloads, the ground index and the fine-occupancy tables.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <array>
#include <chrono>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "elm_host_types.hpp"

using namespace elm;
using namespace elm_host;

// ------------------------------------------------------------------------------------------------------
// map: host-side AddPoints (vhm.cpp:270-285) + upload
// ------------------------------------------------------------------------------------------------------
namespace {

struct HostTable { // open addressing: key -> voxel id, first-seen order
    std::vector<int32_t> kx, ky, kz;
    std::vector<int32_t> vid;
    uint32_t mask = 0;
    uint32_t used = 0;
    void init(uint32_t cap) {
        kx.assign(cap, 0); ky.assign(cap, 0); kz.assign(cap, 0);
        vid.assign(cap, -1);
        mask = cap - 1;
        used = 0;
    }
    void grow() {
        HostTable n;
        n.init((mask + 1) * 2);
        for (uint32_t i = 0; i <= mask; ++i)
            if (vid[i] >= 0) n.insert_known(kx[i], ky[i], kz[i], vid[i]);
        *this = std::move(n);
    }
    void insert_known(int32_t x, int32_t y, int32_t z, int32_t v) {
        uint32_t h = hash3(x, y, z) & mask;
        while (vid[h] >= 0) h = (h + 1) & mask;
        kx[h] = x; ky[h] = y; kz[h] = z; vid[h] = v;
        ++used;
    }
    // returns the voxel id, creating next_id when absent
    int32_t find_or_add(int32_t x, int32_t y, int32_t z, int32_t next_id, bool* added) {
        uint32_t h = hash3(x, y, z) & mask;
        while (vid[h] >= 0) {
            if (kx[h] == x && ky[h] == y && kz[h] == z) {
                *added = false;
                return vid[h];
            }
            h = (h + 1) & mask;
        }
        kx[h] = x; ky[h] = y; kz[h] = z; vid[h] = next_id;
        ++used;
        *added = true;
        return next_id;
    }
};

struct HostBuild {
    std::vector<int32_t> keys; // 3 per voxel (stored / trunc keys)
    std::vector<uint2> ranges; // per voxel (start, cnt) into pts
    std::vector<float4> pts;   // retained points, bucket order
};

// AddPoints (vhm.cpp:270-285) + VoxelBlock::AddPointWithSpacing (vhm.hpp:106-113).  Insertion into one voxel never
// depends on another voxel, so the serial order only matters inside a voxel: points are grouped per voxel in input
// order (stable counting sort) and every voxel replays its own insertions sequentially.
static void build_host(const float* xyz, size_t n, double voxel_size, int max_points, HostBuild& hb) {
    const double map_resolution = sqrt(voxel_size * voxel_size / max_points);
    std::vector<uint32_t> pvid(n);
    HostTable tab;
    tab.init(next_pow2(std::max<uint64_t>(1024, n / 4)));
    int32_t n_vox = 0;
    for (size_t i = 0; i < n; ++i) {
        // Voxel((point.pose / voxel_size_).cast<int>()): truncation toward zero (vhm.cpp:275)
        const int32_t kx = (int32_t)((double)xyz[3 * i] / voxel_size);
        const int32_t ky = (int32_t)((double)xyz[3 * i + 1] / voxel_size);
        const int32_t kz = (int32_t)((double)xyz[3 * i + 2] / voxel_size);
        if (tab.used * 2 >= tab.mask) tab.grow();
        bool added;
        const int32_t v = tab.find_or_add(kx, ky, kz, n_vox, &added);
        if (added) {
            hb.keys.push_back(kx); hb.keys.push_back(ky); hb.keys.push_back(kz);
            ++n_vox;
        }
        pvid[i] = (uint32_t)v;
    }
    // stable grouping of the input indices per voxel
    std::vector<uint64_t> off((size_t)n_vox + 1, 0);
    for (size_t i = 0; i < n; ++i) off[pvid[i] + 1]++;
    for (int32_t v = 0; v < n_vox; ++v) off[v + 1] += off[v];
    std::vector<uint32_t> order(n);
    {
        std::vector<uint64_t> cur(off.begin(), off.end() - 1);
        for (size_t i = 0; i < n; ++i) order[cur[pvid[i]]++] = (uint32_t)i;
    }
    std::vector<uint32_t>().swap(pvid);
    // per-voxel replay of the insertions
    std::vector<uint32_t> kept_cnt((size_t)n_vox, 0);
    unsigned hw = std::max(1u, std::thread::hardware_concurrency());
    unsigned T = (n_vox > 4096) ? std::min(hw, 32u) : 1u;
    auto work = [&](int32_t vb, int32_t ve) {
        std::vector<uint32_t> kept;
        for (int32_t v = vb; v < ve; ++v) {
            kept.clear();
            for (uint64_t o = off[v]; o < off[v + 1]; ++o) {
                const uint32_t i = order[o];
                if (kept.empty()) { // map_.insert({voxel, VoxelBlock{{point}, ...}}): the first point is always kept
                    kept.push_back(i);
                    continue;
                }
                if (kept.size() >= (size_t)max_points) continue; // points.size() < num_points
                const double px = xyz[3 * i], py = xyz[3 * i + 1], pz = xyz[3 * i + 2];
                bool near = false;
                for (uint32_t k : kept) {
                    const double dx = (double)xyz[3 * k] - px, dy = (double)xyz[3 * k + 1] - py, dz = (double)xyz[3 * k + 2] - pz;
                    if (sqrt((dx * dx + dy * dy) + dz * dz) < map_resolution) { // (voxel_point.pose - point.pose).norm() < map_resolution
                        near = true;
                        break;
                    }
                }
                if (!near) kept.push_back(i);
            }
            kept_cnt[v] = (uint32_t)kept.size();
            for (size_t k = 0; k < kept.size(); ++k) order[off[v] + k] = kept[k]; // compact in place
        }
    };
    if (T <= 1) {
        work(0, n_vox);
    } else {
        std::vector<std::thread> pool;
        for (unsigned t = 0; t < T; ++t) {
            int32_t vb = (int32_t)((int64_t)n_vox * t / T), ve = (int32_t)((int64_t)n_vox * (t + 1) / T);
            pool.emplace_back(work, vb, ve);
        }
        for (auto& th : pool) th.join();
    }
    hb.ranges.resize(n_vox);
    uint64_t total = 0;
    for (int32_t v = 0; v < n_vox; ++v) {
        hb.ranges[v] = make_uint2((uint32_t)total, kept_cnt[v]);
        total += kept_cnt[v];
    }
    hb.pts.resize(total);
    for (int32_t v = 0; v < n_vox; ++v)
        for (uint32_t k = 0; k < kept_cnt[v]; ++k) {
            const uint32_t i = order[off[v] + k];
            hb.pts[hb.ranges[v].x + k] = make_float4(xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2], 0.f);
        }
}

} // namespace

void elm_host::map_free(elm_map* m) {
    if (!m) return;
    for (elm_map* r : m->replicas) map_free(r);
    m->replicas.clear();
    if (ctx_alive(m->ctx, m->ctx_id)) (void)hipSetDevice(m->ctx->device); // a context destroyed first: just release the device memory
    void* ptrs[] = {m->d_grid_tiles, m->d_vox_nk, m->d_bad, m->d_grid_gicp8, m->d_slots, m->d_pts, m->d_ranges, m->d_keys, m->d_vox_mean, m->d_vox_cov, m->d_vox_cinv, m->d_pt_gicp, m->d_pt_cov, m->d_qslots, m->d_nbr_pts, m->d_nbr_idx, m->d_nbr_cell_off, m->d_vqslots, m->d_vq_dense, m->d_vqf_dense, m->d_vface, m->d_vox_rec, m->d_vnbr_blk,
                    m->d_grid_blk, m->d_grid_idx, m->d_grid_start, m->d_vox_stat, m->d_grid_gicp, m->d_gpts, m->d_gstart,
                    m->d_fine_keys[0], m->d_fine_keys[1], m->d_fine_keys[2], m->d_fine_masks[0], m->d_fine_masks[1], m->d_fine_masks[2]};
    for (void* p : ptrs)
        if (p) (void)hipFree(p);
    delete m;
}

// bytes of a map array of `count` entries (never an empty allocation)
static size_t map_array_bytes(size_t count, size_t size) { return std::max<size_t>(count * size, 256); }

extern "C" int elm_map_build(elm_ctx* ctx, const float* xyz, size_t n, double voxel_size, int max_points_per_voxel,
                             elm_map** out) {
    if (!ctx || !out || (!xyz && n) || !(voxel_size > 0.0) || max_points_per_voxel <= 0 || n > 0xFFFFFFF0ull) return ELM_ERR_INVALID;
    *out = nullptr;
    if (group_call(ctx)) return elm_multi::map_build(ctx, xyz, n, voxel_size, max_points_per_voxel, out);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    HostBuild hb;
    if (n) build_host(xyz, n, voxel_size, max_points_per_voxel, hb);
    elm_map* m = new elm_map();
    m->ctx = ctx;
    m->ctx_id = ctx->id;
    const uint32_t n_vox = (uint32_t)hb.ranges.size();
    const uint32_t n_pts = (uint32_t)hb.pts.size();
    hipError_t e = hipMalloc((void**)&m->d_pts, map_array_bytes(n_pts, sizeof(float4)));
    if (e == hipSuccess) e = hipMalloc((void**)&m->d_ranges, map_array_bytes(n_vox, sizeof(uint2)));
    if (e == hipSuccess) e = hipMalloc((void**)&m->d_keys, map_array_bytes((size_t)n_vox * 3, sizeof(int32_t)));
    if (e != hipSuccess) {
        ctx->last_error = std::string("hipMalloc(map): ") + hipGetErrorString(e);
        map_free(m);
        return ELM_ERR_DEVICE;
    }
    if (n_pts) e = hipMemcpy(m->d_pts, hb.pts.data(), (size_t)n_pts * sizeof(float4), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_vox) e = hipMemcpy(m->d_ranges, hb.ranges.data(), (size_t)n_vox * sizeof(uint2), hipMemcpyHostToDevice);
    if (e == hipSuccess && n_vox) e = hipMemcpy(m->d_keys, hb.keys.data(), (size_t)n_vox * 3 * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->last_error = std::string("hipMemcpy(map): ") + hipGetErrorString(e);
        map_free(m);
        return ELM_ERR_DEVICE;
    }
    m->h_keys = std::move(hb.keys);
    m->h_ranges = std::move(hb.ranges);
    return map_finish(ctx, m, n_pts, n, voxel_size, max_points_per_voxel, out);
}

// The end of both map builds (elm_map_build above, elm_map_build_device in elm_build.cpp): m holds d_pts, d_ranges and d_keys on the
// device and h_keys and h_ranges on the host.  The slot table is filled here, on the host and in voxel-id order, and the handle gets
// its device view and its info.  m is released on failure.
int elm_host::map_finish(elm_ctx* ctx, elm_map* m, uint32_t n_pts, size_t n_input, double voxel_size, int max_points_per_voxel, elm_map** out) {
    const uint32_t n_vox = (uint32_t)m->h_ranges.size();
    const std::vector<int32_t>& keys = m->h_keys;
    // load factor <= 0.25: a probe for an absent key (most of a workgroup's box cells are empty) ends after ~1.4 slots
    const uint32_t cap = next_pow2((uint64_t)n_vox * 4);
    std::vector<HashSlot> slots;
    try {
        slots = fill_slot_table(keys.data(), n_vox, cap, [&](uint32_t v, HashSlot& s) {
            s.start = m->h_ranges[v].x;
            s.cnt = m->h_ranges[v].y;
        });
    } catch (const std::bad_alloc&) {
        map_free(m);
        throw;
    }
    hipError_t e = hipMalloc((void**)&m->d_slots, map_array_bytes(cap, sizeof(HashSlot)));
    if (e == hipSuccess) e = hipMemcpy(m->d_slots, slots.data(), (size_t)cap * sizeof(HashSlot), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        ctx->last_error = std::string("map slots: ") + hipGetErrorString(e);
        map_free(m);
        return ELM_ERR_DEVICE;
    }
    const size_t bytes = map_array_bytes(cap, sizeof(HashSlot)) + map_array_bytes(n_pts, sizeof(float4)) + map_array_bytes(n_vox, sizeof(uint2)) +
                         map_array_bytes((size_t)n_vox * 3, sizeof(int32_t));
    m->dm.slots = m->d_slots;
    m->dm.mask = cap - 1;
    m->dm.n_vox = n_vox;
    m->dm.n_pts = n_pts;
    m->dm.pts = m->d_pts;
    m->dm.voxel_size = voxel_size;
    {
        int e2 = 0;
        m->dm.inv_vs_exact = (frexp(voxel_size, &e2) == 0.5) ? 1.0 / voxel_size : 0.0;
    }
    m->info.n_input_points = n_input;
    m->info.n_points = n_pts;
    m->info.n_voxels = n_vox;
    m->info.hash_capacity = cap;
    m->info.voxel_size = voxel_size;
    m->info.max_points_per_voxel = max_points_per_voxel;
    m->info.device_bytes = bytes;
    *out = m;
    return ELM_OK;
}

extern "C" void elm_map_destroy(elm_map* m) { map_free(m); }

static bool full_records_forced() {
    return check_mode("full_records");
}
extern "C" int elm_map_cal_voxel_cov_all(elm_map* m) {
    if (!m) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    if (!m->replicas.empty() && group_call(ctx)) return elm_multi::map_call(m, 0, 0.0);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!m->d_vox_mean) {
        HIPCHK(ctx, hipMalloc((void**)&m->d_vox_mean, std::max<size_t>((size_t)m->dm.n_vox * 3 * sizeof(double), 256)));
        HIPCHK(ctx, hipMalloc((void**)&m->d_vox_cov, std::max<size_t>((size_t)m->dm.n_vox * 9 * sizeof(double), 256)));
        HIPCHK(ctx, hipMalloc((void**)&m->d_vox_cinv, std::max<size_t>((size_t)m->dm.n_vox * 9 * sizeof(double), 256)));
        HIPCHK(ctx, hipMalloc((void**)&m->d_vox_nk, std::max<size_t>((size_t)m->dm.n_vox * 4 * sizeof(double), 256)));
        m->info.device_bytes += (size_t)m->dm.n_vox * 25 * sizeof(double);
    }
    if (!m->d_bad) HIPCHK(ctx, hipMalloc((void**)&m->d_bad, 256));
    unsigned bad2[2] = {0, 0}; // [0] flagged, [1] flagged with an asymmetric stored inverse
    unsigned& bad = bad2[0];
    if (m->dm.n_vox) {
        (void)hipGetLastError(); // drop stale errors of other libraries (RCCL probes peer devices)
        HIPCHK(ctx, hipMemsetAsync(m->d_bad, 0, 2 * sizeof(unsigned), ctx->stream));
        launch_voxel_cov(ctx->stream, m->dm, m->d_ranges, m->d_vox_mean, m->d_vox_cov, m->d_vox_cinv, m->d_vox_nk, m->d_bad);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(bad2, m->d_bad, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    m->dm.vox_mean = m->d_vox_mean;
    m->dm.vox_cov = m->d_vox_cov;
    m->dm.vox_cinv = m->d_vox_cinv;
    m->dm.vox_nk = m->d_vox_nk;
    // an inverse covariance of the form I + k n n^T (to 1e-10) is rebuilt by the pairs from the 64-byte list record; the `bad` voxels
    // outside that form (rank-deficient neighbourhood, U != V in its SVD) carry k = NaN and their pairs read the stored 3x3 inverse.
    // ELM_CHECK=full_records: every pair reads the stored inverses.
    m->n_bad_vox = bad;
    m->n_asym_vox = bad2[1];
    m->info.layout_flags = (m->info.layout_flags & ~256) | (bad2[1] ? 256 : 0);
    m->dm.vox_compact = full_records_forced() ? 0 : ((bad == 0 && !check_mode("pair_nine")) ? 2 : 1); // 2: no flagged voxel at all
    m->info.has_voxel_cov = 1;
    m->info.layout_flags = (m->info.layout_flags & ~(2 | 16)) | (m->dm.vox_compact ? 2 : 0) | (m->dm.vox_compact == 2 ? 16 : 0);
    return ELM_OK;
}

extern "C" int elm_map_cal_point_cov_all(elm_map* m, double d_search_dist) {
    if (!m) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    if (!m->replicas.empty() && group_call(ctx)) return elm_multi::map_call(m, 1, d_search_dist);
    HIPCHK(ctx, hipSetDevice(ctx->device));
    if (!m->d_pt_gicp) {
        HIPCHK(ctx, hipMalloc((void**)&m->d_pt_gicp, std::max<size_t>((size_t)m->dm.n_pts * 16 * sizeof(double), 256)));
        HIPCHK(ctx, hipMalloc((void**)&m->d_pt_cov, std::max<size_t>((size_t)m->dm.n_pts * 9 * sizeof(double), 256)));
        m->info.device_bytes += (size_t)m->dm.n_pts * 25 * sizeof(double);
    }
    if (!m->d_bad) HIPCHK(ctx, hipMalloc((void**)&m->d_bad, 256));
    unsigned bad2[2] = {0, 0}; // [0] flagged, [1] flagged with an asymmetric stored inverse
    unsigned& bad = bad2[0];
    if (m->dm.n_pts) {
        (void)hipGetLastError();
        HIPCHK(ctx, hipMemsetAsync(m->d_bad, 0, 2 * sizeof(unsigned), ctx->stream));
        launch_point_cov(ctx->stream, m->dm, d_search_dist * d_search_dist, m->d_pt_gicp, m->d_pt_cov, m->d_bad);
        HIPCHK(ctx, hipGetLastError());
        HIPCHK(ctx, hipMemcpyAsync(bad2, m->d_bad, 2 * sizeof(unsigned), hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(ctx, hipStreamSynchronize(ctx->stream));
    }
    m->dm.pt_gicp = m->d_pt_gicp;
    m->dm.pt_cov = m->d_pt_cov;
    m->n_bad_pts = bad;
    m->n_asym_pts = bad2[1];
    m->info.layout_flags = (m->info.layout_flags & ~128) | (bad2[1] ? 128 : 0);
    m->want_gicp_compact = !full_records_forced(); // see elm_map_cal_voxel_cov_all: non-conforming points (k = NaN) read their full record
    m->info.has_point_cov = 1;
    return refresh_grid_gicp(m); // a grid built before the covariances (or a new search radius): regather
}

// query voxels = every floor key within +-1 of a stored (trunc) key that holds points, first-seen order
void elm_host::enumerate_query_keys(const elm_map* m, std::vector<int32_t>& qkeys) {
    const uint32_t n_vox = m->dm.n_vox;
    HostTable tab;
    tab.init(next_pow2(std::max<uint64_t>(1024, (uint64_t)n_vox * 8)));
    int32_t nq = 0;
    for (uint32_t v = 0; v < n_vox; ++v) {
        if (m->h_ranges[v].y == 0) continue;
        const int32_t kx = m->h_keys[3 * v], ky = m->h_keys[3 * v + 1], kz = m->h_keys[3 * v + 2];
        for (int dx = -1; dx <= 1; ++dx)
            for (int dy = -1; dy <= 1; ++dy)
                for (int dz = -1; dz <= 1; ++dz) {
                    if (tab.used * 2 >= tab.mask) tab.grow();
                    bool added;
                    tab.find_or_add(kx + dx, ky + dy, kz + dz, nq, &added);
                    if (added) {
                        qkeys.push_back(kx + dx); qkeys.push_back(ky + dy); qkeys.push_back(kz + dz);
                        ++nq;
                    }
                }
    }
}

extern "C" int elm_map_get_info(const elm_map* m, elm_map_info* info) {
    if (!m || !info) return ELM_ERR_INVALID;
    *info = m->info;
    return ELM_OK;
}
extern "C" int elm_map_empty(const elm_map* m) { return (!m || m->dm.n_vox == 0) ? 1 : 0; }

static void rowmajor_to_colmajor3(const double* src, double* dst) {
    for (int r = 0; r < 3; ++r)
        for (int c = 0; c < 3; ++c) dst[c * 3 + r] = src[r * 3 + c];
}

extern "C" int elm_map_download_points(const elm_map* m, double* xyz, double* cov9, double* mean3, size_t cap) {
    if (!m) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = std::min<size_t>(cap, m->dm.n_pts);
    if (xyz && n) {
        std::vector<float4> tmp(n);
        HIPCHK(ctx, hipMemcpy(tmp.data(), m->d_pts, n * sizeof(float4), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) {
            xyz[3 * i] = tmp[i].x; xyz[3 * i + 1] = tmp[i].y; xyz[3 * i + 2] = tmp[i].z;
        }
    }
    if ((cov9 || mean3) && !m->info.has_point_cov) {
        // default CovStruct of every PointStruct: (I, 0) (vhm.hpp:45)
        for (size_t i = 0; i < n; ++i) {
            if (cov9) for (int k = 0; k < 9; ++k) cov9[9 * i + k] = (k % 4 == 0) ? 1.0 : 0.0;
            if (mean3) mean3[3 * i] = mean3[3 * i + 1] = mean3[3 * i + 2] = 0.0;
        }
        return ELM_OK;
    }
    if ((cov9 || mean3) && n) {
        std::vector<double> tmp(n * 16);
        HIPCHK(ctx, hipMemcpy(tmp.data(), m->d_pt_gicp, n * 16 * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i)
            if (mean3) memcpy(&mean3[3 * i], &tmp[16 * i], 3 * sizeof(double));
        if (cov9) {
            std::vector<double>().swap(tmp);
            tmp.resize(n * 9);
            HIPCHK(ctx, hipMemcpy(tmp.data(), m->d_pt_cov, n * 9 * sizeof(double), hipMemcpyDeviceToHost));
            for (size_t i = 0; i < n; ++i) rowmajor_to_colmajor3(&tmp[9 * i], &cov9[9 * i]);
        }
    }
    return ELM_OK;
}

extern "C" int elm_map_download_voxels(const elm_map* m, int32_t* key3, int32_t* npts, double* cov9, double* mean3, size_t cap) {
    if (!m) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    const size_t n = std::min<size_t>(cap, m->dm.n_vox);
    if (key3) memcpy(key3, m->h_keys.data(), n * 3 * sizeof(int32_t));
    if (npts) for (size_t v = 0; v < n; ++v) npts[v] = (int32_t)m->h_ranges[v].y;
    if ((cov9 || mean3) && !m->info.has_voxel_cov) {
        for (size_t i = 0; i < n; ++i) {
            if (cov9) for (int k = 0; k < 9; ++k) cov9[9 * i + k] = (k % 4 == 0) ? 1.0 : 0.0;
            if (mean3) mean3[3 * i] = mean3[3 * i + 1] = mean3[3 * i + 2] = 0.0;
        }
        return ELM_OK;
    }
    if (cov9 && n) {
        std::vector<double> tmp(n * 9);
        HIPCHK(ctx, hipMemcpy(tmp.data(), m->d_vox_cov, n * 9 * sizeof(double), hipMemcpyDeviceToHost));
        for (size_t i = 0; i < n; ++i) rowmajor_to_colmajor3(&tmp[9 * i], &cov9[9 * i]);
    }
    if (mean3 && n) HIPCHK(ctx, hipMemcpy(mean3, m->d_vox_mean, n * 3 * sizeof(double), hipMemcpyDeviceToHost));
    return ELM_OK;
}

extern "C" int elm_map_find_ground_height(const elm_map* m, double x, double y, double* ground_z, int* found) {
    // vhm.hpp:285-322: mean z of the (up to) 5 lowest map points within 5 m in xy; needs more than 3 points
    if (!m || !ground_z || !found) return ELM_ERR_INVALID;
    elm_ctx* ctx = m->ctx;
    HIPCHK(ctx, hipSetDevice(ctx->device));
    *found = 0;
    const size_t n = m->dm.n_pts;
    std::vector<float4> tmp(n);
    if (n) HIPCHK(ctx, hipMemcpy(tmp.data(), m->d_pts, n * sizeof(float4), hipMemcpyDeviceToHost));
    std::vector<double> zs;
    for (size_t i = 0; i < n; ++i) {
        const double dx = (double)tmp[i].x - x, dy = (double)tmp[i].y - y;
        if (dx * dx + dy * dy <= 25.0) zs.push_back((double)tmp[i].z);
    }
    if (zs.size() <= 3) return ELM_OK;
    const size_t N = std::min<size_t>(5, zs.size());
    std::partial_sort(zs.begin(), zs.begin() + N, zs.end());
    double s = 0.0;
    for (size_t i = 0; i < N; ++i) s += zs[i];
    *ground_z = s / (double)N;
    *found = 1;
    return ELM_OK;
}

namespace elm_host {
int map_adopt(elm_ctx* ctx, void* d_pts, void* d_ranges, void* d_keys, size_t n_pts, size_t n_vox, size_t n_input, double voxel_size,
              int max_points_per_voxel, elm_map** out) {
    elm_map* m = new (std::nothrow) elm_map();
    if (!m) {
        (void)hipFree(d_pts); (void)hipFree(d_ranges); (void)hipFree(d_keys);
        throw std::bad_alloc();
    }
    m->ctx = ctx;
    m->ctx_id = ctx->id;
    m->d_pts = (float4*)d_pts;
    m->d_ranges = (uint2*)d_ranges;
    m->d_keys = (int32_t*)d_keys;
    try {
        m->h_keys.resize(n_vox * 3);
        m->h_ranges.resize(n_vox);
    } catch (const std::bad_alloc&) {
        map_free(m);
        throw;
    }
    hipError_t e = n_vox ? hipMemcpy(m->h_keys.data(), d_keys, n_vox * 3 * sizeof(int32_t), hipMemcpyDeviceToHost) : hipSuccess;
    if (e == hipSuccess && n_vox) e = hipMemcpy(m->h_ranges.data(), d_ranges, n_vox * sizeof(uint2), hipMemcpyDeviceToHost);
    if (e != hipSuccess) {
        ctx->last_error = std::string("hipMemcpy(map keys): ") + hipGetErrorString(e);
        map_free(m);
        return ELM_ERR_DEVICE;
    }
    return map_finish(ctx, m, (uint32_t)n_pts, n_input, voxel_size, max_points_per_voxel, out);
}
int map_ground_index(const elm_map* cm, const elm::GroundIndex** gi, double bounds[4]) {
    elm_map* m = const_cast<elm_map*>(cm); // the index is a cache of the (immutable) map
    elm_ctx* ctx = m->ctx;
    if (!m->has_gidx) {
        const size_t n = m->dm.n_pts;
        std::vector<float4> pts(n);
        if (n) HIPCHK(ctx, hipMemcpy(pts.data(), m->d_pts, n * sizeof(float4), hipMemcpyDeviceToHost));
        double lo[2] = {HUGE_VAL, HUGE_VAL}, hi[2] = {-HUGE_VAL, -HUGE_VAL};
        for (const float4& p : pts) {
            lo[0] = std::min(lo[0], (double)p.x); hi[0] = std::max(hi[0], (double)p.x);
            lo[1] = std::min(lo[1], (double)p.y); hi[1] = std::max(hi[1], (double)p.y);
        }
        elm::GroundIndex g{};
        g.bin = elm::kGroundBin;
        if (n) {
            g.x0 = lo[0]; g.y0 = lo[1];
            g.nbx = (int32_t)floor((hi[0] - lo[0]) / g.bin) + 1;
            g.nby = (int32_t)floor((hi[1] - lo[1]) / g.bin) + 1;
        }
        const size_t nb = (size_t)g.nbx * (size_t)g.nby;
        std::vector<uint32_t> bin(n), start(nb + 1, 0);
        for (size_t i = 0; i < n; ++i) {
            const int32_t bx = std::min((int32_t)floor(((double)pts[i].x - g.x0) / g.bin), g.nbx - 1);
            const int32_t by = std::min((int32_t)floor(((double)pts[i].y - g.y0) / g.bin), g.nby - 1);
            bin[i] = (uint32_t)bx * (uint32_t)g.nby + (uint32_t)by;
            ++start[bin[i] + 1];
        }
        for (size_t b = 0; b < nb; ++b) start[b + 1] += start[b];
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        std::vector<float4> sorted(n);
        for (size_t i = 0; i < n; ++i) sorted[fill[bin[i]]++] = pts[i];
        HIPCHK(ctx, hipMalloc((void**)&m->d_gpts, std::max<size_t>(n * sizeof(float4), 256)));
        HIPCHK(ctx, hipMalloc((void**)&m->d_gstart, (nb + 1) * sizeof(uint32_t)));
        if (n) HIPCHK(ctx, hipMemcpy(m->d_gpts, sorted.data(), n * sizeof(float4), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(m->d_gstart, start.data(), (nb + 1) * sizeof(uint32_t), hipMemcpyHostToDevice));
        g.pts = m->d_gpts;
        g.start = m->d_gstart;
        m->gidx = g;
        m->pt_bounds[0] = lo[0]; m->pt_bounds[1] = hi[0]; m->pt_bounds[2] = lo[1]; m->pt_bounds[3] = hi[1];
        m->has_gidx = true;
    }
    *gi = &m->gidx;
    memcpy(bounds, m->pt_bounds, sizeof(m->pt_bounds));
    return ELM_OK;
}
// the fine cell of every stored point for cell = voxel_size / sub: (int)floor((double)coordinate / cell)
static int fine_cells_of_points(const elm_map* m, int sub, std::vector<int32_t>& f) {
    elm_ctx* ctx = m->ctx;
    const size_t n = m->dm.n_pts;
    std::vector<float4> pts(n);
    if (n) HIPCHK(ctx, hipMemcpy(pts.data(), m->d_pts, n * sizeof(float4), hipMemcpyDeviceToHost));
    const double cell = m->dm.voxel_size / (double)sub;
    f.resize(3 * n);
    for (size_t i = 0; i < n; ++i) {
        f[3 * i] = (int32_t)floor((double)pts[i].x / cell);
        f[3 * i + 1] = (int32_t)floor((double)pts[i].y / cell);
        f[3 * i + 2] = (int32_t)floor((double)pts[i].z / cell);
    }
    return ELM_OK;
}
int map_fine_cells(const elm_map* m, int sub, std::vector<int32_t>& cells3) {
    std::vector<int32_t> f;
    int rc = fine_cells_of_points(m, sub, f);
    if (rc != ELM_OK) return rc;
    const size_t n = f.size() / 3;
    std::vector<std::array<int32_t, 3>> c(n);
    for (size_t i = 0; i < n; ++i) c[i] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
    std::sort(c.begin(), c.end());
    c.erase(std::unique(c.begin(), c.end()), c.end());
    cells3.resize(3 * c.size());
    for (size_t i = 0; i < c.size(); ++i) memcpy(&cells3[3 * i], c[i].data(), 3 * sizeof(int32_t));
    return ELM_OK;
}
int map_fine_table(const elm_map* cm, int sub, const elm::FineTable** ft, double info[2]) {
    elm_map* m = const_cast<elm_map*>(cm); // the table is a cache of the (immutable) map
    elm_ctx* ctx = m->ctx;
    const int s = sub == 1 ? 0 : (sub == 2 ? 1 : 2);
    if (!m->has_fine[s]) {
        const auto t0 = std::chrono::steady_clock::now();
        std::vector<int32_t> f;
        int rc = fine_cells_of_points(m, sub, f);
        if (rc != ELM_OK) return rc;
        const size_t n = f.size() / 3;
        // open addressing over the coarse cells (f >> 2, arithmetic), grown so that the load factor stays <= 0.5
        uint32_t cap = 1024, used = 0;
        std::vector<int4> keys(cap, int4{0, 0, 0, 0});
        std::vector<unsigned long long> masks(cap, 0ull);
        auto insert = [&](std::vector<int4>& K, std::vector<unsigned long long>& M, uint32_t c, int cx, int cy, int cz, unsigned long long bits) {
            uint32_t h = hash3(cx, cy, cz) & (c - 1);
            for (;; h = (h + 1) & (c - 1)) {
                if (K[h].w == 0) {
                    K[h] = int4{cx, cy, cz, 1};
                    M[h] = bits;
                    return true;
                }
                if (K[h].x == cx && K[h].y == cy && K[h].z == cz) {
                    M[h] |= bits;
                    return false;
                }
            }
        };
        for (size_t i = 0; i < n; ++i) {
            const int fx = f[3 * i], fy = f[3 * i + 1], fz = f[3 * i + 2];
            const unsigned long long bit = 1ull << ((((fx & 3) << 2) | (fy & 3)) << 2 | (fz & 3));
            if (insert(keys, masks, cap, fx >> 2, fy >> 2, fz >> 2, bit) && 2 * (uint64_t)++used > cap) {
                if (cap >= 0x40000000u) {
                    ctx->last_error = "fine occupancy table: too many cells";
                    return ELM_ERR_UNSUPPORTED;
                }
                const uint32_t cap2 = cap * 2;
                std::vector<int4> k2(cap2, int4{0, 0, 0, 0});
                std::vector<unsigned long long> m2(cap2, 0ull);
                for (uint32_t h = 0; h < cap; ++h)
                    if (keys[h].w) insert(k2, m2, cap2, keys[h].x, keys[h].y, keys[h].z, masks[h]);
                keys.swap(k2);
                masks.swap(m2);
                cap = cap2;
            }
        }
        HIPCHK(ctx, hipMalloc((void**)&m->d_fine_keys[s], (size_t)cap * sizeof(int4)));
        HIPCHK(ctx, hipMalloc((void**)&m->d_fine_masks[s], (size_t)cap * sizeof(unsigned long long)));
        HIPCHK(ctx, hipMemcpy(m->d_fine_keys[s], keys.data(), (size_t)cap * sizeof(int4), hipMemcpyHostToDevice));
        HIPCHK(ctx, hipMemcpy(m->d_fine_masks[s], masks.data(), (size_t)cap * sizeof(unsigned long long), hipMemcpyHostToDevice));
        elm::FineTable& t = m->fine[s];
        t.keys = m->d_fine_keys[s];
        t.masks = m->d_fine_masks[s];
        t.mask = cap - 1;
        t.n_coarse = used;
        t.cell = m->dm.voxel_size / (double)sub;
        int e = 0;
        t.inv_cell_exact = frexp(t.cell, &e) == 0.5 ? 1.0 / t.cell : 0.0; // a power of two: q * (1 / cell) is q / cell bit for bit
        m->fine_info[s][0] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        m->fine_info[s][1] = (double)cap * (sizeof(int4) + sizeof(unsigned long long));
        m->has_fine[s] = true;
    }
    *ft = &m->fine[s];
    if (info) memcpy(info, m->fine_info[s], sizeof(m->fine_info[s]));
    return ELM_OK;
}
int map_point_fine_cells(const elm_map* m, int sub, std::vector<int32_t>& cells3) { return fine_cells_of_points(m, sub, cells3); }
} // namespace elm_host
