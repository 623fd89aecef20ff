// elm_odom.cpp -- LiDAR odometry on a rolling local map (include/elimaloc_hip.h, "LiDAR odometry on a rolling local map"; DESIGN.md
// section 20): the object (one owned local map, the pose history, the last inserted pose), the keyframe test and the constant-velocity
// prediction in float64 on the host, and the step -- one elm_register_batch against the local map, one elm_map_build_device_from that
// forgets what lies behind and inserts the scan, the covariances the method reads.  Everything on the device goes through the public
// entry points; nothing here launches a kernel (who may call is elm_call.hpp's check_call).  Host-side C++17.
#include <math.h>
#include <string.h>

#include "elm_query.hpp"

using namespace elm_query;

struct elm_odometry {
    elm_ctx* ctx = nullptr;
    uint64_t ctx_id = 0; // the owning context's unique id (as maps and scans keep it)
    elm_odometry_config cfg{};
    elm_map* map = nullptr;
    int n_poses = 0;                 // poses in the history, counted up to 2
    double T_last[16], T_prev[16];   // T_{k-1}, T_{k-2}
    double T_key[16];                // the last inserted pose (valid while map != nullptr)
};

extern "C" void elm_odometry_config_default(elm_odometry_config* c) {
    if (!c) return;
    memset(c, 0, sizeof(*c));
    c->voxel_size = 1.0;
    c->max_points_per_voxel = 30;
    c->max_range_m = 100.0;
    elm_reg_config_default(&c->reg);
}

namespace {

void identity16(double T[16]) {
    for (int k = 0; k < 16; ++k) T[k] = (k % 5 == 0) ? 1.0 : 0.0;
}

// column-major: entry (r, c) of T
inline double at(const double T[16], int r, int c) { return T[4 * c + r]; }

// T_{k-1} (T_{k-2}^-1 T_{k-1}), the rigid inverse [R^T, -R^T t]; every 3-term sum as (a + b) + c
void predict_cv(const double T1[16], const double T0[16], double out[16]) {
    double D[3][4]; // T0^-1 T1
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) D[r][c] = (at(T0, 0, r) * at(T1, 0, c) + at(T0, 1, r) * at(T1, 1, c)) + at(T0, 2, r) * at(T1, 2, c);
        const double d0 = at(T1, 0, 3) - at(T0, 0, 3), d1 = at(T1, 1, 3) - at(T0, 1, 3), d2 = at(T1, 2, 3) - at(T0, 2, 3);
        D[r][3] = (at(T0, 0, r) * d0 + at(T0, 1, r) * d1) + at(T0, 2, r) * d2; // R0^T (t1 - t0)
    }
    identity16(out);
    for (int r = 0; r < 3; ++r) {
        for (int c = 0; c < 3; ++c) out[4 * c + r] = (at(T1, r, 0) * D[0][c] + at(T1, r, 1) * D[1][c]) + at(T1, r, 2) * D[2][c];
        out[12 + r] = ((at(T1, r, 0) * D[0][3] + at(T1, r, 1) * D[1][3]) + at(T1, r, 2) * D[2][3]) + at(T1, r, 3);
    }
}

// the keyframe test of T against the last inserted pose K
bool is_keyframe(const elm_odometry_config& c, const double K[16], const double T[16]) {
    const double dx = at(T, 0, 3) - at(K, 0, 3), dy = at(T, 1, 3) - at(K, 1, 3), dz = at(T, 2, 3) - at(K, 2, 3);
    if (sqrt((dx * dx + dy * dy) + dz * dz) >= c.key_min_trans_m) return true;
    double R[3];
    for (int i = 0; i < 3; ++i) R[i] = (at(K, 0, i) * at(T, 0, i) + at(K, 1, i) * at(T, 1, i)) + at(K, 2, i) * at(T, 2, i);
    return (((R[0] + R[1]) + R[2]) - 1.0) / 2.0 <= cos(c.key_min_rot_rad);
}

int check_odom(const elm_odometry* o, const char* what) {
    if (!o || !elm_host::ctx_is_alive(o->ctx, o->ctx_id)) return ELM_ERR_INVALID;
    return check_call(o->ctx, what);
}

void push_pose(elm_odometry* o, const double T[16]) {
    memcpy(o->T_prev, o->T_last, sizeof(o->T_prev));
    memcpy(o->T_last, T, sizeof(o->T_last));
    if (o->n_poses < 2) ++o->n_poses;
}

// The insert: a new map from the current one without what is farther than max_range_m from T's translation, followed by the scan at T,
// with the device index build and the covariances the method reads.  The old map goes only when all of it worked.
int insert_scan(elm_odometry* o, const elm_scan* scan, const double T[16], elm_build_sources_stats* stats) {
    elm_build_sources src;
    memset(&src, 0, sizeof(src));
    src.base = o->map;
    src.keep_within = o->map ? 1 : 0;
    for (int r = 0; r < 3; ++r) src.keep_center[r] = T[12 + r];
    src.keep_radius_m = o->cfg.max_range_m;
    src.scans = &scan;
    src.poses16 = T;
    src.n_jobs = 1;
    elm_map* m = nullptr;
    int rc = elm_map_build_device_from(o->ctx, &src, o->cfg.voxel_size, o->cfg.max_points_per_voxel, &m, stats);
    if (rc != ELM_OK) return rc;
    rc = elm_map_set_index_build(m, ELM_INDEX_BUILD_DEVICE);
    const int method = o->cfg.reg.icp_method;
    if (rc == ELM_OK && method == ELM_GICP) rc = elm_map_cal_point_cov_all(m, o->cfg.reg.gicp_cov_search_dist);
    if (rc == ELM_OK && (method == ELM_VGICP || method == ELM_AVGICP)) rc = elm_map_cal_voxel_cov_all(m);
    if (rc != ELM_OK) {
        elm_map_destroy(m);
        return rc;
    }
    if (o->map) elm_map_destroy(o->map);
    o->map = m;
    memcpy(o->T_key, T, sizeof(o->T_key));
    return ELM_OK;
}

} // namespace

extern "C" int elm_odometry_create(elm_ctx* ctx, const elm_odometry_config* c, elm_odometry** out) {
    if (out) *out = nullptr;
    if (!ctx || !c || !out) return ELM_ERR_INVALID;
    if (!(c->voxel_size > 0.0) || c->max_points_per_voxel <= 0 || !fin_ge0(c->max_range_m) || !fin_ge0(c->key_min_trans_m) ||
        !fin_ge0(c->key_min_rot_rad))
        return ELM_ERR_INVALID;
    if (c->reg.icp_method < ELM_P2P || c->reg.icp_method > ELM_AVGICP) return ELM_ERR_INVALID;
    const int rc = check_plain(ctx, "elm_odometry_create");
    if (rc != ELM_OK) return rc;
    return guard_alloc(ctx, "elm_odometry_create", [&] {
        elm_odometry* o = new elm_odometry();
        o->ctx = ctx;
        o->ctx_id = ctx->id;
        o->cfg = *c;
        *out = o;
        return (int)ELM_OK;
    });
}

extern "C" void elm_odometry_destroy(elm_odometry* o) {
    if (!o) return;
    if (o->map && elm_host::ctx_is_alive(o->ctx, o->ctx_id)) elm_map_destroy(o->map);
    delete o;
}

extern "C" int elm_odometry_reset(elm_odometry* o) {
    const int rc = check_odom(o, "elm_odometry_reset");
    if (rc != ELM_OK) return rc;
    if (o->map) elm_map_destroy(o->map);
    o->map = nullptr;
    o->n_poses = 0;
    return ELM_OK;
}

extern "C" int elm_odometry_predict(const elm_odometry* o, double T_guess[16]) {
    if (!o || !T_guess) return ELM_ERR_INVALID;
    if (o->n_poses == 0) identity16(T_guess);
    else if (o->n_poses == 1) memcpy(T_guess, o->T_last, 16 * sizeof(double));
    else predict_cv(o->T_last, o->T_prev, T_guess);
    return ELM_OK;
}

extern "C" const elm_map* elm_odometry_map(const elm_odometry* o) { return o ? o->map : nullptr; }

extern "C" int elm_odometry_step_scan(elm_odometry* o, const elm_scan* scan, const double T_guess[16], elm_odometry_step* out) {
    if (!o || !scan || !out) return ELM_ERR_INVALID;
    int rc = check_odom(o, "elm_odometry_step_scan");
    if (rc != ELM_OK) return rc;
    if (scan->ctx != o->ctx || (T_guess && !poses_finite(T_guess, 1))) return ELM_ERR_INVALID;
    memset(out, 0, sizeof(*out));
    double T0[16];
    if (T_guess) memcpy(T0, T_guess, sizeof(T0));
    else (void)elm_odometry_predict(o, T0);
    if (!o->map) { // the first scan
        memcpy(out->T, T0, sizeof(T0));
        out->is_success = 1;
        rc = insert_scan(o, scan, T0, &out->build);
        if (rc != ELM_OK) return rc;
        out->inserted = 1;
        push_pose(o, T0);
        return ELM_OK;
    }
    elm_scan* one = const_cast<elm_scan*>(scan); // (the batch does not modify its scans)
    rc = elm_register_batch(o->ctx, o->map, &one, 1, T0, &o->cfg.reg, &out->reg, nullptr);
    if (rc != ELM_OK) return rc;
    out->registered = 1;
    out->is_success = out->reg.is_success;
    memcpy(out->T, out->reg.T, sizeof(out->T));
    if (!out->is_success) return ELM_OK;
    if (is_keyframe(o->cfg, o->T_key, out->T)) {
        rc = insert_scan(o, scan, out->T, &out->build);
        if (rc != ELM_OK) return rc;
        out->inserted = 1;
    }
    push_pose(o, out->T);
    return ELM_OK;
}
