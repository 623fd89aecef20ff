// elm_reloc.cpp -- relocalization from a coarse pose (include/elimaloc_hip.h, "relocalization"): the hypothesis grid,
// the occupancy scores of elm_k_reloc.hip, non-maximum suppression and the ICP refinement through elm_register_batch.  Host-side C++17.
#include <hip/hip_runtime.h>
#include <math.h>
#include <string.h>

#include <algorithm>
#include <chrono>
#include <functional>
#include <new>
#include <string>
#include <vector>

#include "elm_query.hpp"

using namespace elm;
using namespace elm_host; // the scratch slots
using namespace elm_query;

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

// the fields elm_map_score_poses reads
bool score_config_ok(const elm_reloc_config* c) {
    return c && isfinite(c->score_max_range_m) && c->score_max_range_m > 0.0 && c->lds_budget_bytes >= 0 && c->bitmap_max_bytes >= 0;
}

struct HypGrid {
    long m = 0, W = 1, K = 1;
    bool full = false; // yaw_range_deg >= 180: k * step over the whole turn
};

bool grid_of(const elm_reloc_config* c, HypGrid* g) {
    if (!score_config_ok(c) || !fin_ge0(c->radius_xy_m) || !(isfinite(c->step_xy_m) && c->step_xy_m > 0.0) ||
        !fin_ge0(c->yaw_range_deg) || !(isfinite(c->step_yaw_deg) && c->step_yaw_deg > 0.0) || c->max_score_points <= 0 ||
        c->top_k <= 0 || c->top_k > kMaxTopK || !fin_ge0(c->nms_xy_m) || !fin_ge0(c->nms_yaw_deg))
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

// R = Rz(dyaw_deg) R0 with the host's cos / sin (dyaw 0: exactly 1 and 0, so R carries R0 itself)
void yaw_times(double dyaw_deg, const double R0[3][3], double R[3][3]) {
    const double a = dyaw_deg * (M_PI / 180.0);
    const double ca = cos(a), sa = sin(a);
    for (int q = 0; q < 3; ++q) { // Rz(a) R0
        R[0][q] = ca * R0[0][q] - sa * R0[1][q];
        R[1][q] = sa * R0[0][q] + ca * R0[1][q];
        R[2][q] = R0[2][q];
    }
}

void make_hypotheses(const HypGrid& g, const double* Tg, const elm_reloc_config* c, double* out, size_t cap) {
    double R0[3][3], t0[3];
    for (int r = 0; r < 3; ++r) {
        for (int q = 0; q < 3; ++q) R0[r][q] = Tg[q * 4 + r];
        t0[r] = Tg[12 + r];
    }
    size_t h = 0;
    for (long k = 0; k < g.K; ++k) {
        double R[3][3];
        yaw_times(dyaw_deg(g, c, k), R0, R);
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
    const DevMap& m = map->dm;
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
        double* P = rows.data() + 12 * (size_t)h;
        pose_rows12(poses16 + 16 * (size_t)h, P);
        for (int r = 0; r < 3; ++r) {
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
    QueryScratch scr{ctx};
    float* d_pts = scr.take<float>(kScrPoints, (size_t)nS * 3);
    double* d_rows = scr.take<double>(kScrRows, rows.size());
    unsigned long long* d_bits = scr.take<unsigned long long>(kScrBitmap, std::max<uint64_t>(words64, 1));
    uint32_t* d_part = scr.take<uint32_t>(kScrPartials, (size_t)n_poses * n_chunks);
    uint32_t* d_scores = scr.take<uint32_t>(kScrStats, n_poses);
    if (scr.rc != ELM_OK) return scr.rc;
    hipError_t e = hipMemcpyAsync(d_pts, S.data(), (size_t)nS * 3 * sizeof(float), hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rows, rows.data(), rows.size() * sizeof(double), hipMemcpyHostToDevice, st);
    if (e == hipSuccess)
        e = launched([&] {
            if (form < 2) launch_reloc_bitmap(st, m, box, n_cells, d_bits);
            launch_reloc_score(st, form, m, d_pts, nS, d_rows, n_poses, box, (const uint32_t*)d_bits, (uint32_t)(2 * words64), d_part, d_scores);
        });
    if (e == hipSuccess) e = hipMemcpyAsync(scores, d_scores, (size_t)n_poses * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    return e == hipSuccess ? ELM_OK : dev_error(ctx, "relocalization scores", e);
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

double wrap_deg(double d) {
    d = fmod(d, 360.0);
    if (d > 180.0) d -= 360.0;
    if (d < -180.0) d += 360.0;
    return d;
}

// Greedy non-maximum suppression over hypotheses in rank order: a hypothesis within nms_xy in xy AND nms_yaw in wrapped yaw of a kept one is
// suppressed; at most top_k are kept.  pos(h, x, y, yaw_deg) gives a hypothesis' position.  Prefix-stable: the kept ones of a prefix of the
// order are the kept ones of the whole order that lie in that prefix.
template <class Pos>
std::vector<uint32_t> greedy_nms(const std::vector<uint32_t>& order, int top_k, double nms_xy, double nms_yaw, Pos pos) {
    std::vector<uint32_t> kept;
    std::vector<double> kx, ky, kyaw;
    for (size_t r = 0; r < order.size() && (int)kept.size() < top_k; ++r) {
        const uint32_t h = order[r];
        double x, y, yaw;
        pos(h, x, y, yaw);
        bool suppressed = false;
        for (size_t q = 0; q < kept.size() && !suppressed; ++q)
            suppressed = hypot(x - kx[q], y - ky[q]) <= nms_xy && fabs(wrap_deg(yaw - kyaw[q])) <= nms_yaw;
        if (suppressed) continue;
        kept.push_back(h);
        kx.push_back(x); ky.push_back(y); kyaw.push_back(yaw);
    }
    return kept;
}

// ICP from the kept hypotheses (T0: 16 doubles each, rank order) in ONE elm_register_batch (the full scan, resident once, repeated); the
// winner is the first successful one with the lowest fitness_score (ties: rank), without success rank 0; the candidates in rank order
int refine_kept(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const std::vector<double>& T0, const std::vector<uint32_t>& kept,
                const std::vector<uint32_t>& kept_scores, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                elm_reloc_candidate* cands, int cap, int* n_cands) {
    const int B = (int)kept.size();
    elm_scan* scan = nullptr;
    int rc = elm_scan_upload(ctx, scan_xyz, n, n, &scan);
    if (rc != ELM_OK) return rc;
    std::vector<elm_scan*> scans((size_t)B, scan);
    std::vector<elm_reg_result> res((size_t)B);
    rc = elm_register_batch(ctx, map, scans.data(), B, T0.data(), reg, res.data(), nullptr);
    elm_scan_destroy(scan);
    if (rc != ELM_OK) return rc;
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
        q.score = kept_scores[b];
        q.hyp_index = (int32_t)kept[b];
        q.is_success = res[b].is_success;
        q.iterations = res[b].iterations;
        q.fitness_score = res[b].fitness_score;
    }
    if (n_cands) *n_cands = B;
    return ELM_OK;
}

int relocalize_impl(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_guess[16], const elm_reloc_config* c,
                    const elm_reg_config* reg, double T_out[16], elm_reg_result* result, elm_reloc_candidate* cands, int cap, int* n_cands) {
    HypGrid g;
    if (!ctx || !map || !scan_xyz || n == 0 || n > 0x7FFFFFFFull || !T_guess || !poses_finite(T_guess, 1) || !grid_of(c, &g) || !reg ||
        reg->icp_method < ELM_P2P || reg->icp_method > ELM_AVGICP || !T_out || !result || cap < 0 || (cap > 0 && !cands))
        return ELM_ERR_INVALID;
    int rc = check_plain(ctx, "elm_relocalize");
    if (rc != ELM_OK) return rc;
    if (map->ctx != ctx || ctx->in_flight) return ELM_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
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
    const long W2 = g.W * g.W;
    const std::vector<uint32_t> kept = greedy_nms(order, c->top_k, c->nms_xy_m, c->nms_yaw_deg, [&](uint32_t h, double& x, double& y, double& yaw) {
        x = (double)((long)h / g.W % g.W - g.m) * c->step_xy_m;
        y = (double)((long)h % g.W - g.m) * c->step_xy_m;
        yaw = dyaw_deg(g, c, (long)h / W2);
    });
    // 5. + 6. ICP from the kept hypotheses, the winner
    std::vector<double> T0(kept.size() * 16);
    std::vector<uint32_t> kept_scores(kept.size());
    for (size_t b = 0; b < kept.size(); ++b) {
        memcpy(&T0[16 * b], &poses[16 * (size_t)kept[b]], 16 * sizeof(double));
        kept_scores[b] = scores[kept[b]];
    }
    return refine_kept(ctx, map, scan_xyz, n, T0, kept, kept_scores, reg, T_out, result, cands, cap, n_cands);
}

} // namespace

extern "C" int elm_reloc_make_hypotheses(const double T_guess[16], const elm_reloc_config* c, double* poses16, size_t cap, size_t* n) {
    HypGrid g;
    if (!T_guess || !poses_finite(T_guess, 1) || !grid_of(c, &g) || !n || (cap && !poses16)) return ELM_ERR_INVALID;
    *n = (size_t)g.K * g.W * g.W;
    if (cap) make_hypotheses(g, T_guess, c, poses16, std::min(cap, *n));
    return ELM_OK;
}

extern "C" int elm_map_score_poses(elm_ctx* ctx, const elm_map* map, const elm_scan* scan, const double* poses16, int n_poses,
                                   const elm_reloc_config* c, uint32_t* scores) {
    if (n_poses <= 0) return ELM_ERR_INVALID; // no poses: refused here, where the other pose queries return at once
    int rc = check_pose_query(ctx, map, scan, poses16, n_poses, score_config_ok(c), scores, "elm_map_score_poses");
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, "elm_map_score_poses", [&] {
        if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
        std::vector<float> xyz(3 * elm_scan_size(scan)), S;
        if ((rc = elm_scan_download(scan, xyz.data(), xyz.size() / 3)) != ELM_OK) return rc;
        counted_points(xyz.data(), xyz.size() / 3, 1, c->score_max_range_m, S);
        return score_impl(ctx, map, S, poses16, (uint32_t)n_poses, c, scores);
    });
}

extern "C" int elm_relocalize(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_guess[16],
                              const elm_reloc_config* c, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                              elm_reloc_candidate* cands, int cap, int* n_cands) {
    return guard_alloc(ctx, "elm_relocalize",
                       [&] { return relocalize_impl(ctx, map, scan_xyz, n, T_guess, c, reg, T_out, result, cands, cap, n_cands); });
}

// ------------------------------------------------------------------------------------------------------
// global relocalization (include/elimaloc_hip.h, "global relocalization")
// ------------------------------------------------------------------------------------------------------

extern "C" void elm_reloc_global_config_default(elm_reloc_global_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->x_min = c->x_max = c->y_min = c->y_max = NAN;
    c->step_xy_m = 0.5;
    c->step_yaw_deg = 2.0;
    c->score_max_range_m = 50.0;
    c->score_min_height_m = 1.0;
    c->max_score_points = 8192;
    c->top_k = 16;
    c->nms_xy_m = 1.0;
    c->nms_yaw_deg = 6.0;
    c->pool_min = 64;
    c->max_kz_span = 64;
    c->bitmap_max_bytes = (int64_t)256 << 20;
}

namespace {

constexpr double kMaxSide = 8388608.0; // 2^23 lattice nodes per axis: at most 23 levels (elm_reloc_global_stats' arrays)
constexpr uint32_t kNodeBatch = 1u << 20; // nodes / leaves per launch

bool global_config_ok(const elm_reloc_global_config* c) {
    if (!c || !(isfinite(c->step_xy_m) && c->step_xy_m > 0.0) || !(isfinite(c->step_yaw_deg) && c->step_yaw_deg > 0.0) ||
        !(isfinite(c->score_max_range_m) && c->score_max_range_m > 0.0) || isnan(c->score_min_height_m) || c->score_min_height_m == HUGE_VAL ||
        c->max_score_points <= 0 || c->top_k <= 0 || c->top_k > kMaxTopK || !fin_ge0(c->nms_xy_m) || !fin_ge0(c->nms_yaw_deg) ||
        c->pool_min <= 0 || c->max_kz_span <= 0 || c->bitmap_max_bytes < 0)
        return false;
    const double r[4] = {c->x_min, c->x_max, c->y_min, c->y_max};
    const int n_nan = (int)isnan(r[0]) + (int)isnan(r[1]) + (int)isnan(r[2]) + (int)isnan(r[3]);
    if (n_nan == 4) return true;
    return n_nan == 0 && isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3]) && r[1] >= r[0] && r[3] >= r[2];
}

// T_tilt = [R0 | (0, 0, h)]: finite, no xy translation, bottom row (0 0 0 1)
bool tilt_ok(const double* T) {
    return T && poses_finite(T, 1) && T[12] == 0.0 && T[13] == 0.0 && T[3] == 0.0 && T[7] == 0.0 && T[11] == 0.0 && T[15] == 1.0;
}

struct Lattice {
    double x0, y0, step, yaw_step;
    long NX, NY, K;
    double R0[3][3], h;
    std::vector<double> rot; // [K][9] row-major Rz(yaw_k) R0
    size_t size() const { return (size_t)K * NX * NY; }
    double x(long i) const { return x0 + (double)i * step; }
    double y(long j) const { return y0 + (double)j * step; }
    // leaf h = (k NX + i) NY + j as a column-major 4 x 4 pose standing on the ground field gz
    void pose16(size_t h, const std::vector<double>& gz, double* T) const {
        const size_t k = h / ((size_t)NX * NY), i = h / NY % NX, j = h % NY;
        for (int q = 0; q < 3; ++q)
            for (int r = 0; r < 3; ++r) T[q * 4 + r] = rot[k * 9 + r * 3 + q];
        T[3] = T[7] = T[11] = 0.0;
        T[12] = x((long)i); T[13] = y((long)j); T[14] = gz[i * NY + j]; T[15] = 1.0;
    }
};

// the lattice over rect {x_min, x_max, y_min, y_max}; false: more than 2^31 - 1 poses
bool lattice_of(const elm_reloc_global_config* c, const double rect[4], const double* T_tilt, Lattice* L) {
    const double nx = floor((rect[1] - rect[0]) / c->step_xy_m + 1e-9) + 1.0, ny = floor((rect[3] - rect[2]) / c->step_xy_m + 1e-9) + 1.0;
    const double kk = std::max(1.0, ceil(360.0 / c->step_yaw_deg - 1e-9));
    if (!(nx * ny * kk <= 2147483647.0) || !(nx <= kMaxSide && ny <= kMaxSide)) return false;
    L->x0 = rect[0]; L->y0 = rect[2]; L->step = c->step_xy_m; L->yaw_step = c->step_yaw_deg;
    L->NX = (long)nx; L->NY = (long)ny; L->K = (long)kk;
    for (int r = 0; r < 3; ++r)
        for (int q = 0; q < 3; ++q) L->R0[r][q] = T_tilt[q * 4 + r];
    L->h = T_tilt[14];
    L->rot.resize((size_t)L->K * 9);
    for (long k = 0; k < L->K; ++k) {
        double R[3][3];
        yaw_times((double)k * c->step_yaw_deg, L->R0, R);
        for (int r = 0; r < 3; ++r)
            for (int q = 0; q < 3; ++q) L->rot[(size_t)k * 9 + r * 3 + q] = R[r][q];
    }
    return true;
}

int ground_impl(elm_ctx* ctx, const elm_map* map, const double* xy, size_t n, double* z, int32_t* found) {
    const GroundIndex* gi = nullptr;
    double bounds[4];
    int rc = elm_host::map_ground_index(map, &gi, bounds);
    if (rc != ELM_OK || n == 0) return rc;
    hipStream_t st = (hipStream_t)elm_ctx_stream(ctx);
    const size_t batch = (size_t)1 << 22;
    QueryScratch scr{ctx};
    double* d_xy = scr.take<double>(kScrGroundXY, std::min(n, batch) * 2);
    double* d_z = scr.take<double>(kScrGroundZ, std::min(n, batch));
    int32_t* d_f = scr.take<int32_t>(kScrGroundFound, std::min(n, batch));
    if (scr.rc != ELM_OK) return scr.rc;
    for (size_t o = 0; o < n; o += batch) {
        const size_t m = std::min(batch, n - o);
        hipError_t e = hipMemcpyAsync(d_xy, xy + 2 * o, m * 2 * sizeof(double), hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = launched([&] { launch_ground_heights(st, *gi, d_xy, (uint32_t)m, d_z, d_f); });
        if (e == hipSuccess) e = hipMemcpyAsync(z + o, d_z, m * sizeof(double), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipMemcpyAsync(found + o, d_f, m * sizeof(int32_t), hipMemcpyDeviceToHost, st);
        if (e == hipSuccess) e = hipStreamSynchronize(st);
        if (e != hipSuccess) return dev_error(ctx, "ground heights", e);
    }
    return ELM_OK;
}

// the rectangle (the config's, or the map's point bounds), the lattice, its ground field gz = fl(g + h) and validity per (i, j)
int lattice_field(elm_ctx* ctx, const elm_map* map, const double* T_tilt, const elm_reloc_global_config* c, Lattice* L, std::vector<double>& gz,
                  std::vector<int32_t>& valid) {
    double rect[4] = {c->x_min, c->x_max, c->y_min, c->y_max};
    if (isnan(rect[0])) {
        const GroundIndex* gi = nullptr;
        int rc = elm_host::map_ground_index(map, &gi, rect);
        if (rc != ELM_OK) return rc;
        if (map->dm.n_pts == 0) rect[0] = rect[1] = rect[2] = rect[3] = 0.0;
    }
    if (!lattice_of(c, rect, T_tilt, L)) return ELM_ERR_INVALID;
    const size_t nxy = (size_t)L->NX * L->NY;
    std::vector<double> xy(2 * nxy);
    for (long i = 0; i < L->NX; ++i)
        for (long j = 0; j < L->NY; ++j) {
            xy[2 * ((size_t)i * L->NY + j)] = L->x(i);
            xy[2 * ((size_t)i * L->NY + j) + 1] = L->y(j);
        }
    gz.assign(nxy, 0.0);
    valid.assign(nxy, 0);
    if (map->dm.n_pts == 0) {
        for (double& v : gz) v = L->h;
        return ELM_OK;
    }
    int rc = ground_impl(ctx, map, xy.data(), nxy, gz.data(), valid.data());
    if (rc != ELM_OK) return rc;
    for (size_t q = 0; q < nxy; ++q) gz[q] = valid[q] ? gz[q] + L->h : L->h;
    return ELM_OK;
}

// Branch-and-bound over the lattice.  Level l node (k, I, J) covers leaves i in [I 2^l, (I + 1) 2^l), j likewise, of
// yaw k; its bound is the k_reloc_bound count over the level's window bitmap D_l.  Output: every valid leaf whose exact score is >= the
// final pass's threshold, with its score, in (score desc, hyp asc) order -- a prefix of the exhaustive order -- and the kept ones after NMS.
struct Search {
    elm_ctx* ctx;
    const elm_map* map;
    const DevMap* m;
    hipStream_t st;
    const Lattice* L;
    const std::vector<double>* gz;
    const std::vector<int32_t>* valid;
    uint32_t nS = 0;
    float* d_pts = nullptr;
    double* d_rot = nullptr;
    double* d_gz = nullptr;
    RelocBox box{};
    unsigned long long* d_b0 = nullptr; // the level-0 bitmap
    uint32_t* d_lv = nullptr;           // levels 1 .. top, words_per_level each
    uint64_t words = 0;                 // 32-bit words per level
    int top = 0;
    std::vector<uint32_t> w;            // window width per level
    std::vector<std::vector<double>> zmin, zmax; // per level, [ceil(NX / 2^l)][ceil(NY / 2^l)]
    elm_reloc_global_stats* stats;

    long nI(int l) const { return (L->NX + (1L << l) - 1) >> l; }
    long nJ(int l) const { return (L->NY + (1L << l) - 1) >> l; }

    // One batched call: per slice of kNodeBatch of the n items, stage(scr, o, b, d_part, d_out) takes the slots of the slice's input,
    // uploads it and queues the launches on the partials and the output (nothing once scr has failed); the b output words come down
    // into out + o, and the stream is joined.
    template <class Stage>
    int batched(size_t n, uint32_t* out, const char* what, Stage stage) {
        const uint32_t n_chunks = (nS + kRelocChunk - 1) / kRelocChunk;
        for (size_t o = 0; o < n; o += kNodeBatch) {
            const uint32_t b = (uint32_t)std::min<size_t>(kNodeBatch, n - o);
            QueryScratch scr{ctx};
            uint32_t* d_part = scr.take<uint32_t>(kScrNodePartials, (size_t)b * n_chunks);
            uint32_t* d_out = scr.take<uint32_t>(kScrNodeOut, b);
            hipError_t e = stage(scr, o, b, d_part, d_out);
            if (scr.rc != ELM_OK) return scr.rc;
            if (e == hipSuccess) e = hipMemcpyAsync(out + o, d_out, (size_t)b * sizeof(uint32_t), hipMemcpyDeviceToHost, st);
            if (e == hipSuccess) e = hipStreamSynchronize(st);
            if (e != hipSuccess) return dev_error(ctx, what, e);
        }
        return ELM_OK;
    }

    int bound(int l, const std::vector<uint32_t>& nodes, std::vector<uint32_t>& out) { // nodes: (k, I, J) triples
        const size_t n = nodes.size() / 3;
        out.resize(n);
        if (stats) { stats->nodes_bounded[l] += (int64_t)n; stats->point_evals += (int64_t)n * nS; }
        if (nS == 0) { std::fill(out.begin(), out.end(), 0u); return ELM_OK; }
        std::vector<RelocNode> rec;
        return batched(n, out.data(), "global relocalization bounds", [&](QueryScratch& scr, size_t o, uint32_t b, uint32_t* d_part, uint32_t* d_out) {
            rec.resize(b);
            for (uint32_t q = 0; q < b; ++q) {
                const uint32_t k = nodes[3 * (o + q)], I = nodes[3 * (o + q) + 1], J = nodes[3 * (o + q) + 2];
                const long i1 = std::min(((long)I + 1) << l, L->NX) - 1, j1 = std::min(((long)J + 1) << l, L->NY) - 1;
                RelocNode& r = rec[q];
                r.xlo = L->x((long)I << l); r.xhi = L->x(i1);
                r.ylo = L->y((long)J << l); r.yhi = L->y(j1);
                r.zlo = zmin[l][(size_t)I * nJ(l) + J]; r.zhi = zmax[l][(size_t)I * nJ(l) + J];
                r.k = (int32_t)k; r._pad = 0;
            }
            RelocNode* d_nodes = scr.take<RelocNode>(kScrNodes, b);
            if (scr.rc != ELM_OK) return hipSuccess;
            hipError_t e = hipMemcpyAsync(d_nodes, rec.data(), (size_t)b * sizeof(RelocNode), hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = launched([&] {
                    launch_reloc_bound(st, *m, d_pts, nS, d_nodes, b, d_rot, box, d_lv + (size_t)(l - 1) * words, w[l],
                                       (uint32_t)std::max(stats_kz_cap, 1), d_part, d_out);
                });
            return e;
        });
    }
    int stats_kz_cap = 64;

    int score_leaves(const std::vector<uint32_t>& hyps, std::vector<uint32_t>& out) {
        const size_t n = hyps.size();
        out.resize(n);
        if (stats) { stats->leaves_scored += (int64_t)n; stats->point_evals += (int64_t)n * nS; }
        if (nS == 0) { std::fill(out.begin(), out.end(), 0u); return ELM_OK; }
        return batched(n, out.data(), "global relocalization leaf scores", [&](QueryScratch& scr, size_t o, uint32_t b, uint32_t* d_part, uint32_t* d_out) {
            uint32_t* d_h = scr.take<uint32_t>(kScrLeafIds, b);
            double* d_rows = scr.take<double>(kScrLeafRows, (size_t)b * 12);
            if (scr.rc != ELM_OK) return hipSuccess;
            hipError_t e = hipMemcpyAsync(d_h, hyps.data() + o, (size_t)b * sizeof(uint32_t), hipMemcpyHostToDevice, st);
            if (e == hipSuccess)
                e = launched([&] {
                    launch_reloc_leaf_rows(st, d_h, b, d_rot, L->x0, L->y0, L->step, (uint32_t)L->NX, (uint32_t)L->NY, d_gz, d_rows);
                    launch_reloc_score(st, 1, *m, d_pts, nS, d_rows, b, box, (const uint32_t*)d_b0, 0, d_part, d_out);
                });
            return e;
        });
    }

    // the valid children at level l - 1 of a level-l node
    void children(int l, uint32_t k, uint32_t I, uint32_t J, std::vector<uint32_t>& out) const {
        for (uint32_t a = 0; a < 2; ++a)
            for (uint32_t c = 0; c < 2; ++c) {
                const long ci = 2L * I + a, cj = 2L * J + c;
                if (ci >= nI(l - 1) || cj >= nJ(l - 1)) continue;
                if (l - 1 == 0) {
                    if ((*valid)[(size_t)ci * L->NY + cj]) out.push_back((uint32_t)(((long)k * L->NX + ci) * L->NY + cj));
                } else if (zmin[l - 1][(size_t)ci * nJ(l - 1) + cj] <= zmax[l - 1][(size_t)ci * nJ(l - 1) + cj]) {
                    out.insert(out.end(), {k, (uint32_t)ci, (uint32_t)cj});
                }
            }
    }

    // the starting frontier: every valid node of the top level (leaves when top = 0)
    void top_nodes(std::vector<uint32_t>& out) const {
        out.clear();
        for (long k = 0; k < L->K; ++k)
            for (long I = 0; I < nI(top); ++I)
                for (long J = 0; J < nJ(top); ++J) {
                    if (top == 0) {
                        if ((*valid)[(size_t)I * L->NY + J]) out.push_back((uint32_t)((k * L->NX + I) * L->NY + J));
                    } else if (zmin[top][(size_t)I * nJ(top) + J] <= zmax[top][(size_t)I * nJ(top) + J]) {
                        out.insert(out.end(), {(uint32_t)k, (uint32_t)I, (uint32_t)J});
                    }
                }
    }

    // one pass at threshold tau: every valid leaf with score >= tau and its score
    int pass(uint32_t tau, std::vector<uint32_t>& leaves, std::vector<uint32_t>& scores) {
        std::vector<uint32_t> front, b, next;
        top_nodes(front);
        for (int l = top; l >= 1; --l) {
            int rc = bound(l, front, b);
            if (rc != ELM_OK) return rc;
            next.clear();
            int64_t kept = 0;
            for (size_t q = 0; q < b.size(); ++q)
                if (b[q] >= tau) {
                    ++kept;
                    children(l, front[3 * q], front[3 * q + 1], front[3 * q + 2], next);
                }
            if (stats) stats->nodes_kept[l] += kept;
            front.swap(next);
        }
        std::vector<uint32_t> s;
        int rc = score_leaves(front, s);
        if (rc != ELM_OK) return rc;
        leaves.clear();
        scores.clear();
        for (size_t q = 0; q < front.size(); ++q)
            if (s[q] >= tau) { leaves.push_back(front[q]); scores.push_back(s[q]); }
        return ELM_OK;
    }

    // the first threshold: greedy descents under the pool_min best top-level nodes, the pool_min-th best of their leaves' scores
    int initial_tau(int pool_min, uint32_t* tau) {
        *tau = 0;
        std::vector<uint32_t> front, b;
        top_nodes(front);
        if (top == 0 || front.empty()) return ELM_OK;
        int rc = bound(top, front, b);
        if (rc != ELM_OK) return rc;
        const size_t n = front.size() / 3;
        std::vector<uint32_t> idx(n);
        for (size_t q = 0; q < n; ++q) idx[q] = (uint32_t)q;
        const size_t D = std::min<size_t>((size_t)pool_min, n);
        std::partial_sort(idx.begin(), idx.begin() + D, idx.end(), [&](uint32_t a, uint32_t c) { return b[a] != b[c] ? b[a] > b[c] : a < c; });
        std::vector<uint32_t> path;
        for (size_t q = 0; q < D; ++q) path.insert(path.end(), {front[3 * idx[q]], front[3 * idx[q] + 1], front[3 * idx[q] + 2]});
        for (int l = top; l >= 1; --l) {
            // the children of every path; the best one continues
            std::vector<uint32_t> ch, owner, nb;
            for (size_t p = 0; p < path.size() / 3; ++p) {
                const size_t before = ch.size();
                children(l, path[3 * p], path[3 * p + 1], path[3 * p + 2], ch);
                owner.insert(owner.end(), (ch.size() - before) / (l - 1 == 0 ? 1 : 3), (uint32_t)p);
            }
            if (l - 1 == 0) { path.swap(ch); break; }
            if ((rc = bound(l - 1, ch, nb)) != ELM_OK) return rc;
            std::vector<uint32_t> np;
            for (size_t q = 0; q < owner.size();) {
                size_t best = q, e = q;
                while (e < owner.size() && owner[e] == owner[q]) {
                    if (nb[e] > nb[best]) best = e;
                    ++e;
                }
                np.insert(np.end(), {ch[3 * best], ch[3 * best + 1], ch[3 * best + 2]});
                q = e;
            }
            path.swap(np);
        }
        // path: leaves (each path's children at level 0); score them all
        std::vector<uint32_t> s;
        if ((rc = score_leaves(path, s)) != ELM_OK) return rc;
        if (s.empty()) return ELM_OK;
        std::sort(s.begin(), s.end(), std::greater<uint32_t>());
        *tau = s[std::min<size_t>((size_t)pool_min, s.size()) - 1];
        return ELM_OK;
    }
};

// the search's device state: counted points, rotations, ground field, the level-0 bitmap of the map's key box and the level windows
int search_setup(Search& S, const std::vector<float>& pts, const elm_reloc_global_config* c) {
    const Lattice& L = *S.L;
    S.nS = (uint32_t)(pts.size() / 3);
    S.stats_kz_cap = c->max_kz_span;
    // ground-height pyramids over the valid leaves (invalid: +inf / -inf, so a node without a valid leaf has zmin > zmax)
    int top = 0;
    while ((1L << top) < std::max(L.NX, L.NY)) ++top;
    // the frontier starts where it has some thousands of nodes (coarser levels prune little)
    while (top > 1 && (double)L.K * (double)((L.NX + (1L << (top - 1)) - 1) >> (top - 1)) * (double)((L.NY + (1L << (top - 1)) - 1) >> (top - 1)) <= 4096.0)
        --top;
    S.top = top;
    S.zmin.assign(top + 1, {});
    S.zmax.assign(top + 1, {});
    S.zmin[0].resize((size_t)L.NX * L.NY);
    S.zmax[0].resize((size_t)L.NX * L.NY);
    for (size_t q = 0; q < S.zmin[0].size(); ++q) {
        S.zmin[0][q] = (*S.valid)[q] ? (*S.gz)[q] : HUGE_VAL;
        S.zmax[0][q] = (*S.valid)[q] ? (*S.gz)[q] : -HUGE_VAL;
    }
    for (int l = 1; l <= top; ++l) {
        const long ni = S.nI(l), nj = S.nJ(l), pj = S.nJ(l - 1), pi = S.nI(l - 1);
        S.zmin[l].assign((size_t)ni * nj, HUGE_VAL);
        S.zmax[l].assign((size_t)ni * nj, -HUGE_VAL);
        for (long i = 0; i < pi; ++i)
            for (long j = 0; j < pj; ++j) {
                const size_t d = (size_t)(i / 2) * nj + j / 2, s = (size_t)i * pj + j;
                S.zmin[l][d] = std::min(S.zmin[l][d], S.zmin[l - 1][s]);
                S.zmax[l][d] = std::max(S.zmax[l][d], S.zmax[l - 1][s]);
            }
    }
    S.w.assign(top + 1, 1);
    for (int l = 1; l <= top; ++l) S.w[l] = (uint32_t)(floor((double)((1L << l) - 1) * L.step / S.m->voxel_size) + 2.0);
    if (S.nS == 0) return ELM_OK;
    // the map's key box, z padded to whole 64-bit words per column
    const std::vector<int32_t>& keys = S.map->h_keys;
    int32_t lo[3] = {INT32_MAX, INT32_MAX, INT32_MAX}, hi[3] = {INT32_MIN, INT32_MIN, INT32_MIN};
    for (size_t v = 0; v < keys.size() / 3; ++v)
        for (int a = 0; a < 3; ++a) { lo[a] = std::min(lo[a], keys[3 * v + a]); hi[a] = std::max(hi[a], keys[3 * v + a]); }
    const uint64_t nx = (uint64_t)((int64_t)hi[0] - lo[0] + 1), ny = (uint64_t)((int64_t)hi[1] - lo[1] + 1);
    const uint64_t nz = ((uint64_t)((int64_t)hi[2] - lo[2] + 1) + 63) / 64 * 64;
    const uint64_t cells = nx * ny * nz;
    S.words = cells / 32;
    if (cells >= ((uint64_t)1 << 32) || (double)S.words * 4.0 * (double)(top + 2) > (double)c->bitmap_max_bytes) {
        elm_host::ctx_set_error(S.ctx, "elm_relocalize_global: the occupancy bitmap and its level windows exceed bitmap_max_bytes");
        return ELM_ERR_UNSUPPORTED;
    }
    S.box = RelocBox{lo[0], lo[1], lo[2], (uint32_t)nx, (uint32_t)ny, (uint32_t)nz};
    QueryScratch scr{S.ctx}; // the first five are held to the end of the search (elm_hostapi.hpp)
    S.d_pts = scr.take<float>(kScrPoints, pts.size());
    S.d_rot = scr.take<double>(kScrRows, L.rot.size());
    S.d_b0 = scr.take<unsigned long long>(kScrBitmap, S.words / 2); // nz is whole 64-bit words
    S.d_gz = scr.take<double>(kScrGroundField, S.gz->size());
    S.d_lv = scr.take<uint32_t>(kScrLevelWindows, std::max<uint64_t>(S.words * (uint64_t)top, 1));
    uint32_t* d_tmp = scr.take<uint32_t>(kScrWindowTmp, S.words);
    if (scr.rc != ELM_OK) return scr.rc;
    hipError_t e = hipMemcpyAsync(S.d_pts, pts.data(), pts.size() * sizeof(float), hipMemcpyHostToDevice, S.st);
    if (e == hipSuccess) e = hipMemcpyAsync(S.d_rot, L.rot.data(), L.rot.size() * sizeof(double), hipMemcpyHostToDevice, S.st);
    if (e == hipSuccess) e = hipMemcpyAsync(S.d_gz, S.gz->data(), S.gz->size() * sizeof(double), hipMemcpyHostToDevice, S.st);
    if (e == hipSuccess)
        e = launched([&] {
            launch_reloc_bitmap(S.st, *S.m, S.box, cells, S.d_b0);
            const uint32_t nzw = (uint32_t)(nz / 32);
            for (int l = 1; l <= top; ++l) {
                const uint32_t* in = l == 1 ? (const uint32_t*)S.d_b0 : S.d_lv + (size_t)(l - 2) * S.words;
                const uint32_t wp = S.w[l - 1];
                launch_reloc_window_or(S.st, in, d_tmp, (uint32_t)nx, (uint32_t)ny, nzw, 0, wp, S.w[l]);
                launch_reloc_window_or(S.st, d_tmp, S.d_lv + (size_t)(l - 1) * S.words, (uint32_t)nx, (uint32_t)ny, nzw, 1, wp, S.w[l]);
            }
        });
    if (e == hipSuccess) e = hipStreamSynchronize(S.st);
    return e == hipSuccess ? ELM_OK : dev_error(S.ctx, "global relocalization bitmaps", e);
}

double ms_since(const std::chrono::steady_clock::time_point& t) {
    return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
}

int common_checks(elm_ctx* ctx, const elm_map* map, const char* what) {
    int rc = check_plain(ctx, what);
    if (rc != ELM_OK) return rc;
    if (map->ctx != ctx || ctx->in_flight) return ELM_ERR_INVALID;
    if (hipSetDevice(ctx->device) != hipSuccess) return ELM_ERR_DEVICE;
    return ELM_OK;
}

int relocalize_global_impl(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_tilt[16],
                           const elm_reloc_global_config* c, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                           elm_reloc_candidate* cands, int cap, int* n_cands, elm_reloc_global_stats* stats) {
    if (!global_config_ok(c) || !tilt_ok(T_tilt) || !ctx || !map || !scan_xyz || n == 0 || n > 0x7FFFFFFFull || !reg ||
        reg->icp_method < ELM_P2P || reg->icp_method > ELM_AVGICP || !T_out || !result || cap < 0 || (cap > 0 && !cands))
        return ELM_ERR_INVALID;
    if (!isnan(c->x_min)) {
        const double rect[4] = {c->x_min, c->x_max, c->y_min, c->y_max};
        Lattice probe;
        if (!lattice_of(c, rect, T_tilt, &probe)) return ELM_ERR_INVALID;
    }
    int rc = common_checks(ctx, map, "elm_relocalize_global");
    if (rc != ELM_OK) return rc;
    elm_reloc_global_stats st{};
    auto t0 = std::chrono::steady_clock::now();
    // 1. the lattice and its ground field
    Lattice L;
    std::vector<double> gz;
    std::vector<int32_t> valid;
    if ((rc = lattice_field(ctx, map, T_tilt, c, &L, gz, valid)) != ELM_OK) return rc;
    st.lattice_poses = (int64_t)L.size();
    st.nx = (int32_t)L.NX; st.ny = (int32_t)L.NY; st.n_yaw = (int32_t)L.K;
    for (int32_t v : valid) st.valid_leaves += v ? L.K : 0;
    st.ms_ground = ms_since(t0);
    if (n_cands) *n_cands = 0;
    if (st.valid_leaves == 0) { // no pose stands on ground (an empty map, a rectangle off the map)
        memset(result, 0, sizeof(*result));
        result->gate = 1;
        memcpy(T_out, T_tilt, 16 * sizeof(double));
        memcpy(result->T, T_tilt, 16 * sizeof(double));
        if (stats) *stats = st;
        return ELM_OK;
    }
    // 2. counted points: r_max, then the height filter (R0 p)_z + h >= score_min_height_m
    t0 = std::chrono::steady_clock::now();
    const size_t stride = (n + (size_t)c->max_score_points - 1) / (size_t)c->max_score_points;
    std::vector<float> P, pts;
    counted_points(scan_xyz, n, stride, c->score_max_range_m, P);
    for (size_t i = 0; i < P.size() / 3; ++i) {
        const double x = P[3 * i], y = P[3 * i + 1], z = P[3 * i + 2];
        if (((L.R0[2][0] * x + L.R0[2][1] * y) + L.R0[2][2] * z) + L.h >= c->score_min_height_m) pts.insert(pts.end(), {P[3 * i], P[3 * i + 1], P[3 * i + 2]});
    }
    st.n_counted = (int32_t)(pts.size() / 3);
    // 3. branch-and-bound passes: all leaves >= tau, NMS over them; fewer than top_k kept (and tau > 0): a lower tau
    Search S{ctx, map, &map->dm, (hipStream_t)elm_ctx_stream(ctx), &L, &gz, &valid};
    S.stats = &st;
    if ((rc = search_setup(S, pts, c)) != ELM_OK) return rc;
    st.levels = S.top;
    uint32_t tau = 0;
    if ((rc = S.initial_tau(c->pool_min, &tau)) != ELM_OK) return rc;
    std::vector<uint32_t> leaves, scores, kept;
    std::vector<uint32_t> order;
    const long NXY = L.NX * L.NY;
    for (;;) {
        ++st.passes;
        st.tau = tau;
        if ((rc = S.pass(tau, leaves, scores)) != ELM_OK) return rc;
        order.resize(leaves.size());
        for (size_t q = 0; q < order.size(); ++q) order[q] = (uint32_t)q;
        std::sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return scores[a] != scores[b] ? scores[a] > scores[b] : leaves[a] < leaves[b]; });
        for (uint32_t& q : order) q = leaves[q];
        kept = greedy_nms(order, c->top_k, c->nms_xy_m, c->nms_yaw_deg, [&](uint32_t h, double& x, double& y, double& yaw) {
            x = L.x((long)h / L.NY % L.NX);
            y = L.y((long)h % L.NY);
            yaw = (double)((long)h / NXY) * L.yaw_step;
        });
        if ((int)kept.size() >= c->top_k || tau == 0) break;
        tau = tau * 3 / 4;
    }
    st.ms_search = ms_since(t0);
    // 4. ICP from the kept poses
    t0 = std::chrono::steady_clock::now();
    std::vector<double> T0(kept.size() * 16);
    std::vector<uint32_t> kept_scores(kept.size());
    for (size_t b = 0; b < kept.size(); ++b) {
        L.pose16(kept[b], gz, &T0[16 * b]);
        for (size_t q = 0; q < leaves.size(); ++q)
            if (leaves[q] == kept[b]) { kept_scores[b] = scores[q]; break; }
    }
    rc = refine_kept(ctx, map, scan_xyz, n, T0, kept, kept_scores, reg, T_out, result, cands, cap, n_cands);
    st.ms_refine = ms_since(t0);
    if (stats) *stats = st;
    return rc;
}

} // namespace

extern "C" int elm_map_ground_heights(elm_ctx* ctx, const elm_map* map, const double* xy, size_t n, double* z, int32_t* found) {
    if (!ctx || !map || (n && (!xy || !z || !found)) || n > 0xFFFFFFFFull) return ELM_ERR_INVALID;
    return guard_alloc(ctx, "elm_map_ground_heights", [&] {
        int rc = common_checks(ctx, map, "elm_map_ground_heights");
        return rc != ELM_OK ? rc : ground_impl(ctx, map, xy, n, z, found);
    });
}

extern "C" int elm_reloc_global_hypotheses(elm_ctx* ctx, const elm_map* map, const double T_tilt[16], const elm_reloc_global_config* c,
                                           double* poses16, int32_t* valid, size_t cap, size_t* n) {
    if (!global_config_ok(c) || !tilt_ok(T_tilt) || !n || (cap && (!poses16 || !valid))) return ELM_ERR_INVALID;
    if (cap == 0 && !isnan(c->x_min)) { // the size of an explicit rectangle's lattice: no map, no device
        const double rect[4] = {c->x_min, c->x_max, c->y_min, c->y_max};
        Lattice L;
        if (!lattice_of(c, rect, T_tilt, &L)) return ELM_ERR_INVALID;
        *n = L.size();
        return ELM_OK;
    }
    if (!ctx || !map) return ELM_ERR_INVALID;
    return guard_alloc(ctx, "elm_reloc_global_hypotheses", [&] {
        int rc = common_checks(ctx, map, "elm_reloc_global_hypotheses");
        if (rc != ELM_OK) return rc;
        Lattice L;
        std::vector<double> gz;
        std::vector<int32_t> ok;
        if ((rc = lattice_field(ctx, map, T_tilt, c, &L, gz, ok)) != ELM_OK) return rc;
        *n = L.size();
        const size_t m = std::min(cap, *n);
        for (size_t h = 0; h < m; ++h) {
            L.pose16(h, gz, poses16 + 16 * h);
            valid[h] = ok[h % ((size_t)L.NX * L.NY)];
        }
        return ELM_OK;
    });
}

extern "C" int elm_relocalize_global(elm_ctx* ctx, const elm_map* map, const float* scan_xyz, size_t n, const double T_tilt[16],
                                     const elm_reloc_global_config* c, const elm_reg_config* reg, double T_out[16], elm_reg_result* result,
                                     elm_reloc_candidate* cands, int cap, int* n_cands, elm_reloc_global_stats* stats) {
    return guard_alloc(ctx, "elm_relocalize_global",
                       [&] { return relocalize_global_impl(ctx, map, scan_xyz, n, T_tilt, c, reg, T_out, result, cands, cap, n_cands, stats); });
}
