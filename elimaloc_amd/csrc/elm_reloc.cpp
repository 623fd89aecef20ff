// elm_reloc.cpp -- relocalization from a coarse pose (include/elimaloc_hip.h, "relocalization"): the hypothesis grid,
// the occupancy scores of elm_k_reloc.hip, non-maximum suppression and the ICP refinement through elm_register_batch.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <new>
#include <string>
#include <vector>

#include "elm_hostapi.hpp"
#include "elm_internal.hpp"

using namespace elm;

extern "C" void elm_reloc_config_default(elm_reloc_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->radius_xy_m = 5.0;
    c->step_xy_m = 0.5;
    c->yaw_range_deg = 180.0;
    c->step_yaw_deg = 2.0;
    c->score_max_range_m = 50.0;
    c->max_score_points = 8192;
    c->top_k = 16;
    c->nms_xy_m = 1.0;
    c->nms_yaw_deg = 6.0;
    c->lds_budget_bytes = 64 << 10;
    c->bitmap_max_bytes = 64 << 20;
}

namespace {

constexpr size_t kMaxHypotheses = (size_t)1 << 24;
constexpr int kMaxTopK = 1024;
// the dynamic LDS of the staged form: the wave counts + the bitmap within 64 KiB
constexpr uint64_t kLdsBitmapMax = 65536 - (uint64_t)kRelocHyp * 4 * sizeof(uint32_t);

bool finite_nonneg(double v) { return isfinite(v) && v >= 0.0; }

// the fields elm_map_score_poses reads
bool score_config_ok(const elm_reloc_config* c) {
    return c && isfinite(c->score_max_range_m) && c->score_max_range_m > 0.0 && c->lds_budget_bytes >= 0 && c->bitmap_max_bytes >= 0;
}

struct HypGrid {
    long m = 0, W = 1, K = 1;
    bool full = false; // yaw_range_deg >= 180: k * step over the whole turn
};

bool grid_of(const elm_reloc_config* c, HypGrid* g) {
    if (!score_config_ok(c) || !finite_nonneg(c->radius_xy_m) || !(isfinite(c->step_xy_m) && c->step_xy_m > 0.0) ||
        !finite_nonneg(c->yaw_range_deg) || !(isfinite(c->step_yaw_deg) && c->step_yaw_deg > 0.0) || c->max_score_points <= 0 ||
        c->top_k <= 0 || c->top_k > kMaxTopK || !finite_nonneg(c->nms_xy_m) || !finite_nonneg(c->nms_yaw_deg))
        return false;
    const double mm = floor(c->radius_xy_m / c->step_xy_m + 1e-9);
    g->full = c->yaw_range_deg >= 180.0;
    const double kk = g->full ? ceil(360.0 / c->step_yaw_deg - 1e-9) : 2.0 * floor(c->yaw_range_deg / c->step_yaw_deg + 1e-9) + 1.0;
    if (!(mm <= 4096.0) || !(kk <= 1e6)) return false;
    g->m = (long)mm;
    g->W = 2 * g->m + 1;
    g->K = std::max(1L, (long)kk);
    return (double)g->K * (double)g->W * (double)g->W <= (double)kMaxHypotheses;
}

// yaw offset of hypothesis row k in degrees: full turn k * step; symmetric window 0, +step, -step, +2 step, -2 step, ...
double dyaw_deg(const HypGrid& g, const elm_reloc_config* c, long k) {
    if (g.full) return (double)k * c->step_yaw_deg;
    if (k == 0) return 0.0;
    const double a = (double)((k + 1) / 2) * c->step_yaw_deg;
    return (k & 1) ? a : -a;
}

bool finite16(const double* T) {
    for (int i = 0; i < 16; ++i)
        if (!isfinite(T[i])) return false;
    return true;
}

void make_hypotheses(const HypGrid& g, const double* Tg, const elm_reloc_config* c, double* out, size_t cap) {
    double R0[3][3], t0[3];
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) R0[r][q] = Tg[q * 4 + r];
        t0[r] = Tg[12 + r];
    }
    size_t h = 0;
    for (long k = 0; k < g.K; ++k) {
        const double a = dyaw_deg(g, c, k) * (M_PI / 180.0);
        const double ca = cos(a), sa = sin(a); // k = 0: exactly 1 and 0, so T_0 carries the guess's own rotation
        double R[3][3];
        for (int q = 0; q < 3; ++q) { // Rz(a) R0
            R[0][q] = ca * R0[0][q] - sa * R0[1][q];
            R[1][q] = sa * R0[0][q] + ca * R0[1][q];
            R[2][q] = R0[2][q];
        }
        for (long i = -g.m; i <= g.m; ++i)
            for (long j = -g.m; j <= g.m; ++j, ++h) {
                if (h >= cap) return;
                double* T = out + 16 * h;
                for (int q = 0; q < 3; ++q)
                    for (int r = 0; r < 3; ++r) T[q * 4 + r] = R[r][q];
                T[3] = T[7] = T[11] = 0.0;
                T[12] = t0[0] + (double)i * c->step_xy_m;
                T[13] = t0[1] + (double)j * c->step_xy_m;
                T[14] = t0[2];
                T[15] = 1.0;
            }
    }
}

inline double key_of(double q, const DevMap& m) { return trunc(m.inv_vs_exact != 0.0 ? q * m.inv_vs_exact : q / m.voxel_size); }

// The occupancy scores of n_poses column-major poses for the counted points S (host, float32 xyz): the key box of the hypothesis set, the
// form of the lookup (LDS bitmap / global bitmap / hash probes, from the two byte budgets), the launches, the download.
int score_impl(elm_ctx* ctx, const elm_map* map, const std::vector<float>& S, const double* poses16, uint32_t n_poses, const elm_reloc_config* c,
               uint32_t* scores) {
    const DevMap& m = elm_host::map_dev(map);
    const uint32_t nS = (uint32_t)(S.size() / 3);
    if (m.n_vox == 0 || nS == 0) {
        memset(scores, 0, (size_t)n_poses * sizeof(uint32_t));
        return ELM_OK;
    }
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    // AABB of S
    double lo[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, hi[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (uint32_t i = 0; i < nS; ++i)
        for (int a = 0; a < 3; ++a) {
            lo[a] = std::min(lo[a], (double)S[3 * i + a]);
            hi[a] = std::max(hi[a], (double)S[3 * i + a]);
        }
    // rows of every pose + the union of the key ranges: per row, the corner that minimises (maximises) every product -- the score's own
    // arithmetic is monotone in each coordinate, so the transformed AABB's keys bound every point's
    std::vector<double> rows((size_t)n_poses * 12);
    double kmin[3] = {HUGE_VAL, HUGE_VAL, HUGE_VAL}, kmax[3] = {-HUGE_VAL, -HUGE_VAL, -HUGE_VAL};
    for (uint32_t h = 0; h < n_poses; ++h) {
        const double* T = poses16 + 16 * (size_t)h;
        double* P = rows.data() + 12 * (size_t)h;
        for (int r = 0; r < 3; ++r) {
            for (int q = 0; q < 4; ++q) P[r * 4 + q] = T[q * 4 + r];
            const double a0 = P[r * 4], a1 = P[r * 4 + 1], a2 = P[r * 4 + 2], t = P[r * 4 + 3];
            const double qlo = ((a0 * (a0 >= 0.0 ? lo[0] : hi[0]) + a1 * (a1 >= 0.0 ? lo[1] : hi[1])) + a2 * (a2 >= 0.0 ? lo[2] : hi[2])) + t;
            const double qhi = ((a0 * (a0 >= 0.0 ? hi[0] : lo[0]) + a1 * (a1 >= 0.0 ? hi[1] : lo[1])) + a2 * (a2 >= 0.0 ? hi[2] : lo[2])) + t;
            kmin[r] = std::min(kmin[r], key_of(qlo, m));
            kmax[r] = std::max(kmax[r], key_of(qhi, m));
        }
    }
    // the box (one key of margin per side); a box that is not representable takes the probe form
    RelocBox box{};
    double cells = 1.0;
    bool box_ok = true;
    for (int a = 0; a < 3; ++a) {
        box_ok = box_ok && isfinite(kmin[a]) && isfinite(kmax[a]) && kmin[a] >= -1073741824.0 && kmax[a] <= 1073741824.0;
        if (box_ok) cells *= (kmax[a] - kmin[a] + 3.0);
    }
    int form = 2;
    uint64_t n_cells = 0, words64 = 0;
    if (box_ok && cells < 4294967296.0) {
        box.x0 = (int32_t)kmin[0] - 1; box.y0 = (int32_t)kmin[1] - 1; box.z0 = (int32_t)kmin[2] - 1;
        box.nx = (uint32_t)(kmax[0] - kmin[0] + 3.0); box.ny = (uint32_t)(kmax[1] - kmin[1] + 3.0); box.nz = (uint32_t)(kmax[2] - kmin[2] + 3.0);
        n_cells = (uint64_t)box.nx * box.ny * box.nz;
        words64 = (n_cells + 63) / 64;
        const uint64_t bytes = words64 * 8;
        if (bytes <= (uint64_t)c->lds_budget_bytes && bytes <= kLdsBitmapMax) form = 0;
        else if (bytes <= (uint64_t)c->bitmap_max_bytes) form = 1;
    }
    if (form == 2) box = RelocBox{0, 0, 0, 0, 0, 0};
    const uint32_t n_chunks = (nS + kRelocChunk - 1) / kRelocChunk;
    int rc = ELM_OK;
    float* d_pts = (float*)elm_host::ctx_reloc_scratch(ctx, 0, (size_t)nS * 3 * sizeof(float), &rc);
    double* d_rows = d_pts ? (double*)elm_host::ctx_reloc_scratch(ctx, 1, rows.size() * sizeof(double), &rc) : nullptr;
    unsigned long long* d_bits = d_rows ? (unsigned long long*)elm_host::ctx_reloc_scratch(ctx, 2, std::max<uint64_t>(words64, 1) * 8, &rc) : nullptr;
    uint32_t* d_part = d_bits ? (uint32_t*)elm_host::ctx_reloc_scratch(ctx, 3, (size_t)n_poses * n_chunks * sizeof(uint32_t), &rc) : nullptr;
    uint32_t* d_scores = d_part ? (uint32_t*)elm_host::ctx_reloc_scratch(ctx, 4, (size_t)n_poses * sizeof(uint32_t), &rc) : nullptr;
    if (!d_scores) return rc;
    hipError_t e = hipMemcpyAsync(d_pts, S.data(), (size_t)nS * 3 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) {
        (void)hipGetLastError();
        if (form < 2) launch_reloc_bitmap(st, m, box, n_cells, d_bits);
        launch_reloc_score(st, form, m, d_pts, nS, d_rows, n_poses, box, (const uint32_t*)d_bits, (uint32_t)(2 * words64), d_part, d_scores);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(scores, d_scores, (size_t)n_poses * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        elm_host::ctx_set_error(ctx, std::string("relocalization scores: ") + hipGetErrorString(e));
        return ELM_ERR_DEVICE;
    }
    return ELM_OK;
}

// the counted points: ((x*x + y*y) + z*z) <= r_max^2 in float64
void counted_points(const float* xyz, size_t n, size_t stride, double r_max, std::vector<float>& S) {
    const double r2 = r_max * r_max;
    S.clear();
    for (size_t i = 0; i < n; i += stride) {
        const double x = xyz[3 * i], y = xyz[3 * i + 1], z = xyz[3 * i + 2];
        if ((x * x + y * y) + z * z <= r2) S.insert(S.end(), {xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]});
    }
}

// one rank, no exchange: a device group's lead or a context with a communicator / hook attached is refused
int check_plain(elm_ctx* ctx, const char* what) {
    if ((elm_host::ctx_group(ctx) && !elm_multi::in_worker()) || elm_host::ctx_exchange_attached(ctx)) {
        elm_host::ctx_set_error(ctx, std::string(what) + ": one rank only (not on a device group, nor with a communicator or hook attached)");
        return ELM_ERR_UNSUPPORTED;
    }
    return ELM_OK;
}

double wrap_deg(double d) {
    d = fmod(d, 360.0);
    if (d > 180.0) d -= 360.0;
    if (d < -180.0) d += 360.0;
    return d;
}

int relocalize_impl(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_guess[16], const elm_reloc_config* c,
                    const elm_reg_config* reg, double T_out[16], elm_reg_result* result, elm_reloc_candidate* cands, int cap, int* n_cands) {
    HypGrid g;
    if (!ctx || !map || !scan_xyz || n == 0 || n > 0x7FFFFFFFull || !T_guess || !finite16(T_guess) || !grid_of(c, &g) || !reg ||
        reg->icp_method < ELM_P2P || reg->icp_method > ELM_AVGICP || !T_out || !result || cap < 0 || (cap > 0 && !cands))
        return ELM_ERR_INVALID;
    int rc = check_plain(ctx, "elm_relocalize");
    if (rc != ELM_OK) return rc;
    if (elm_host::map_ctx(map) != ctx || elm_host::ctx_in_flight(ctx)) return ELM_ERR_INVALID;
    if (hipSetDevice(elm_host::ctx_device(ctx)) != hipSuccess) return ELM_ERR_DEVICE;
    // 1. hypotheses and the score subsample (every ceil(n / cap)-th point of the caller's order, the counted ones)
    const size_t n_hyp = (size_t)g.K * g.W * g.W;
    std::vector<double> poses(n_hyp * 16);
    make_hypotheses(g, T_guess, c, poses.data(), n_hyp);
    const size_t stride = (n + (size_t)c->max_score_points - 1) / (size_t)c->max_score_points;
    std::vector<float> S;
    counted_points(scan_xyz, n, stride, c->score_max_range_m, S);
    // 2. scores
    std::vector<uint32_t> scores(n_hyp);
    if ((rc = score_impl(ctx, map, S, poses.data(), (uint32_t)n_hyp, c, scores.data())) != ELM_OK) return rc;
    // 3. (score desc, index asc): a counting sort over the scores
    const uint32_t smax = *std::max_element(scores.begin(), scores.end());
    std::vector<uint32_t> start((size_t)smax + 2, 0), order(n_hyp);
    for (uint32_t s : scores) ++start[smax - s + 1];
    for (size_t b = 1; b < start.size(); ++b) start[b] += start[b - 1];
    for (size_t h = 0; h < n_hyp; ++h) order[start[smax - scores[h]]++] = (uint32_t)h;
    // 4. greedy non-maximum suppression on (xy distance, |dyaw|)
    std::vector<uint32_t> kept;
    std::vector<double> kx, ky, kyaw;
    const long W2 = g.W * g.W;
    for (size_t r = 0; r < n_hyp && (int)kept.size() < c->top_k; ++r) {
        const uint32_t h = order[r];
        const double x = (double)((long)h / g.W % g.W - g.m) * c->step_xy_m, y = (double)((long)h % g.W - g.m) * c->step_xy_m;
        const double yaw = dyaw_deg(g, c, (long)h / W2);
        bool suppressed = false;
        for (size_t q = 0; q < kept.size() && !suppressed; ++q)
            suppressed = hypot(x - kx[q], y - ky[q]) <= c->nms_xy_m && fabs(wrap_deg(yaw - kyaw[q])) <= c->nms_yaw_deg;
        if (suppressed) continue;
        kept.push_back(h);
        kx.push_back(x); ky.push_back(y); kyaw.push_back(yaw);
    }
    // 5. one elm_register_batch over the kept hypotheses (the full scan, resident once, repeated)
    const int B = (int)kept.size();
    elm_scan* scan = nullptr;
    if ((rc = elm_scan_upload(ctx, scan_xyz, n, n, &scan)) != ELM_OK) return rc;
    std::vector<elm_scan*> scans((size_t)B, scan);
    std::vector<double> T0((size_t)B * 16);
    for (int b = 0; b < B; ++b) memcpy(&T0[16 * (size_t)b], &poses[16 * (size_t)kept[b]], 16 * sizeof(double));
    std::vector<elm_reg_result> res((size_t)B);
    rc = elm_register_batch(ctx, map, scans.data(), B, T0.data(), reg, res.data(), nullptr);
    elm_scan_destroy(scan);
    if (rc != ELM_OK) return rc;
    // 6. winner: success first, then the lowest fitness score, then rank
    int win = 0;
    for (int b = 1; b < B; ++b) {
        const elm_reg_result &a = res[b], &w = res[win];
        if ((a.is_success && !w.is_success) || (a.is_success && w.is_success && a.fitness_score < w.fitness_score)) win = b;
    }
    memcpy(T_out, res[win].T, 16 * sizeof(double));
    *result = res[win];
    for (int b = 0; b < B && b < cap; ++b) {
        elm_reloc_candidate& q = cands[b];
        memset(&q, 0, sizeof(q));
        memcpy(q.T0, &T0[16 * (size_t)b], sizeof(q.T0));
        memcpy(q.T, res[b].T, sizeof(q.T));
        q.score = scores[kept[b]];
        q.hyp_index = (int32_t)kept[b];
        q.is_success = res[b].is_success;
        q.iterations = res[b].iterations;
        q.fitness_score = res[b].fitness_score;
    }
    if (n_cands) *n_cands = B;
    return ELM_OK;
}

} // namespace

extern "C" int elm_reloc_make_hypotheses(const double T_guess[16], const elm_reloc_config* c, double* poses16, size_t cap, size_t* n) {
    HypGrid g;
    if (!T_guess || !finite16(T_guess) || !grid_of(c, &g) || !n || (cap && !poses16)) return ELM_ERR_INVALID;
    *n = (size_t)g.K * g.W * g.W;
    if (cap) make_hypotheses(g, T_guess, c, poses16, std::min(cap, *n));
    return ELM_OK;
}

extern "C" int elm_map_score_poses(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses,
                                   const elm_reloc_config* c, uint32_t* scores) {
    if (!ctx || !map || !scan || !poses16 || n_poses <= 0 || !score_config_ok(c) || !scores) return ELM_ERR_INVALID;
    int rc = check_plain(ctx, "elm_map_score_poses");
    if (rc != ELM_OK) return rc;
    if (elm_host::map_ctx(map) != ctx || elm_host::scan_ctx(scan) != ctx || elm_host::ctx_in_flight(ctx)) return ELM_ERR_INVALID;
    for (int h = 0; h < n_poses; ++h)
        if (!finite16(poses16 + 16 * (size_t)h)) return ELM_ERR_INVALID;
    try {
        if (hipSetDevice(elm_host::ctx_device(ctx)) != hipSuccess) return ELM_ERR_DEVICE;
        std::vector<float> xyz(3 * elm_scan_size(scan)), S;
        if ((rc = elm_scan_download(scan, xyz.data(), xyz.size() / 3)) != ELM_OK) return rc;
        counted_points(xyz.data(), xyz.size() / 3, 1, c->score_max_range_m, S);
        return score_impl(ctx, map, S, poses16, (uint32_t)n_poses, c, scores);
    } catch (const std::bad_alloc&) {
        elm_host::ctx_set_error(ctx, "elm_map_score_poses: host allocation failed");
        return ELM_ERR_ALLOC;
    }
}

extern "C" int elm_relocalize(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_guess[16],
                              const elm_reloc_config* c, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                              elm_reloc_candidate* cands, int cap, int* n_cands) {
    try {
        return relocalize_impl(ctx, map, scan_xyz, n, T_guess, c, reg, T_out, result, cands, cap, n_cands);
    } catch (const std::bad_alloc&) {
        if (ctx) elm_host::ctx_set_error(ctx, "elm_relocalize: host allocation failed");
        return ELM_ERR_ALLOC;
    }
}
