// elm_dev_pgraph.hpp -- the pose graph's relative-pose edge (include/elimaloc_hip.h, "pose graph"): SO(3) Log through the
// unit quaternion, the inverse right Jacobian, the residual and its two 6 x 6 Jacobians, the Huber weight and cost, and the retraction.
// Host and device run this same code (elm_posegraph_edge_terms is the host's call of it).  Float64, row-major, no contraction.
// Below the edge math: the 6 x 6 block primitives of the solver's kernels, the edge-group launch geometry, and (device only) the
// fixed-order workgroup reductions and the load of an edge's three poses.  Every sum here is the first product, then the other five
// added left to right; no helper indexes an array by a value that varies by lane.
#pragma once
#include "elm_internal.hpp"
#include "elm_la.hpp"

namespace elm {

constexpr double kPgLogSmallN = 1e-8;    // |vec| of the unit quaternion below which Log is 2 vec (the next term is n^2 / 3 relative)
constexpr double kPgSeriesTheta = 1e-2;  // below it c(theta) is its series 1/12 + theta^2/720 + theta^4/30240

// Log of a rotation matrix: the unit quaternion as matrix_to_angle forms it, signed to w >= 0; phi = vec * (theta / n),
// theta = 2 atan2(n, w); below kPgLogSmallN phi = 2 vec.  Also returns theta and the quaternion's (w, n) = (cos, sin)(theta / 2).
// Log(I) is exactly 0.
ELM_HD void pg_log(const double R[9], double phi[3], double& theta, double& qw_out, double& n_out) {
    const double tr = R[0] + R[4] + R[8];
    double qw, qx, qy, qz;
    if (tr > 0.0) {
        double t = sqrt(tr + 1.0);
        qw = 0.5 * t;
        t = 0.5 / t;
        qx = (R[7] - R[5]) * t;
        qy = (R[2] - R[6]) * t;
        qz = (R[3] - R[1]) * t;
    } else if (R[0] >= R[4] && R[0] >= R[8]) { // the largest diagonal entry leads (the three cases written out: no indexed registers)
        double t = sqrt(R[0] - R[4] - R[8] + 1.0);
        qx = 0.5 * t;
        t = 0.5 / t;
        qw = (R[7] - R[5]) * t;
        qy = (R[3] + R[1]) * t;
        qz = (R[6] + R[2]) * t;
    } else if (R[4] >= R[8]) {
        double t = sqrt(R[4] - R[8] - R[0] + 1.0);
        qy = 0.5 * t;
        t = 0.5 / t;
        qw = (R[2] - R[6]) * t;
        qz = (R[7] + R[5]) * t;
        qx = (R[1] + R[3]) * t;
    } else {
        double t = sqrt(R[8] - R[0] - R[4] + 1.0);
        qz = 0.5 * t;
        t = 0.5 / t;
        qw = (R[3] - R[1]) * t;
        qx = (R[2] + R[6]) * t;
        qy = (R[5] + R[7]) * t;
    }
    if (qw < 0.0) { qw = -qw; qx = -qx; qy = -qy; qz = -qz; }
    const double n = sqrt((qx * qx + qy * qy) + qz * qz);
    double k;
    if (n < kPgLogSmallN) {
        k = 2.0;
        theta = 2.0 * n;
    } else {
        theta = 2.0 * atan2(n, qw);
        k = theta / n;
    }
    phi[0] = qx * k;
    phi[1] = qy * k;
    phi[2] = qz * k;
    qw_out = qw;
    n_out = n;
}

// c(theta) of J^-1 = I + [phi]x / 2 + c [phi]x^2: 1/theta^2 - (1 + cos theta) / (2 theta sin theta), whose second term is
// cot(theta / 2) / (2 theta) = w / (2 theta n) with the quaternion's w = cos(theta / 2), n = sin(theta / 2) -- the same number without
// the cancellation of 1 + cos theta near pi.  Below kPgSeriesTheta the series.
ELM_HD double pg_jinv_c(double theta, double qw, double n) {
    if (theta < kPgSeriesTheta) {
        const double t2 = theta * theta;
        return (1.0 / 12.0 + t2 / 720.0) + (t2 * t2) / 30240.0;
    }
    return 1.0 / (theta * theta) - qw / ((2.0 * theta) * n);
}

ELM_HD void pg_jinv(const double phi[3], double c, double J[9]) {
    const double x = phi[0], y = phi[1], z = phi[2];
    // [phi]x^2 = phi phi^T - |phi|^2 I
    const double xx = x * x, yy = y * y, zz = z * z;
    J[0] = 1.0 - c * (yy + zz);
    J[4] = 1.0 - c * (xx + zz);
    J[8] = 1.0 - c * (xx + yy);
    const double cxy = c * (x * y), cxz = c * (x * z), cyz = c * (y * z);
    J[1] = cxy - 0.5 * z;
    J[3] = cxy + 0.5 * z;
    J[2] = cxz + 0.5 * y;
    J[6] = cxz - 0.5 * y;
    J[5] = cyz - 0.5 * x;
    J[7] = cyz + 0.5 * x;
}

// r = a^T b (3 x 3, row-major)
ELM_HD void pg_mul3_at(const double a[9], const double b[9], double r[9]) {
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) r[i * 3 + j] = (a[i] * b[j] + a[3 + i] * b[3 + j]) + a[6 + i] * b[6 + j];
}
ELM_HD void pg_mul3_atv(const double a[9], const double v[3], double r[3]) {
#pragma unroll
    for (int i = 0; i < 3; ++i) r[i] = (a[i] * v[0] + a[3 + i] * v[1]) + a[6 + i] * v[2];
}

// One pose as the twelve rows of pose_rows12: P[r * 4 + q] = (R_r0, R_r1, R_r2, t_r).
ELM_HD void pg_split(const double P[12], double R[9], double t[3]) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        R[r * 3] = P[r * 4];
        R[r * 3 + 1] = P[r * 4 + 1];
        R[r * 3 + 2] = P[r * 4 + 2];
        t[r] = P[r * 4 + 3];
    }
}

// The residual alone (the cost kernel): r = [R_Z^T (d - t_Z); Log(R_Z^T R_i^T R_j)], d = R_i^T (t_j - t_i).
ELM_HD void pg_residual(const double Pi[12], const double Pj[12], const double PZ[12], double r[6]) {
    double Ri[9], ti[3], Rj[9], tj[3], RZ[9], tZ[3];
    pg_split(Pi, Ri, ti);
    pg_split(Pj, Rj, tj);
    pg_split(PZ, RZ, tZ);
    const double dt[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
    double d[3], Rij[9], RE[9];
    pg_mul3_atv(Ri, dt, d);
    pg_mul3_at(Ri, Rj, Rij);
    pg_mul3_at(RZ, Rij, RE);
    const double e[3] = {d[0] - tZ[0], d[1] - tZ[1], d[2] - tZ[2]};
    pg_mul3_atv(RZ, e, r);
    double theta, qw, n, phi[3];
    pg_log(RE, phi, theta, qw, n);
    r[3] = phi[0];
    r[4] = phi[1];
    r[5] = phi[2];
}

// The residual and the non-zero 3 x 3 blocks of the Jacobians A = dr/dx_i, B = dr/dx_j (rows in the order of r, columns of x):
//   A = [ Att  Atr ;  0  Arr ] = [ -R_Z^T   R_Z^T [d]x ;  0  -J^-1 R_j^T R_i ],   B = [ Btt  0 ;  0  Brr ] = [ R_E  0 ;  0  J^-1 ].
struct PgBlocks {
    double Att[9], Atr[9], Arr[9], Btt[9], Brr[9];
};
ELM_HD void pg_edge_blocks(const double Pi[12], const double Pj[12], const double PZ[12], double r[6], PgBlocks& K) {
    double Ri[9], ti[3], Rj[9], tj[3], RZ[9], tZ[3];
    pg_split(Pi, Ri, ti);
    pg_split(Pj, Rj, tj);
    pg_split(PZ, RZ, tZ);
    const double dt[3] = {tj[0] - ti[0], tj[1] - ti[1], tj[2] - ti[2]};
    double d[3], Rij[9];
    pg_mul3_atv(Ri, dt, d);
    pg_mul3_at(Ri, Rj, Rij);
    pg_mul3_at(RZ, Rij, K.Btt);
    const double e[3] = {d[0] - tZ[0], d[1] - tZ[1], d[2] - tZ[2]};
    pg_mul3_atv(RZ, e, r);
    double theta, qw, n, phi[3];
    pg_log(K.Btt, phi, theta, qw, n);
    r[3] = phi[0];
    r[4] = phi[1];
    r[5] = phi[2];
    pg_jinv(phi, pg_jinv_c(theta, qw, n), K.Brr);
    const double dx[9] = {0.0, -d[2], d[1], d[2], 0.0, -d[0], -d[1], d[0], 0.0};
    pg_mul3_at(RZ, dx, K.Atr);
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            K.Att[a * 3 + b] = -RZ[b * 3 + a];
            // -(J Rij^T)[a][b]
            K.Arr[a * 3 + b] = -((K.Brr[a * 3] * Rij[b * 3] + K.Brr[a * 3 + 1] * Rij[b * 3 + 1]) + K.Brr[a * 3 + 2] * Rij[b * 3 + 2]);
        }
}
// the blocks as full row-major 6 x 6 matrices (registers, LDS or the host's arrays)
ELM_HD void pg_blocks_full(const PgBlocks& K, double* A, double* B) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            A[a * 6 + b] = K.Att[a * 3 + b];
            A[a * 6 + 3 + b] = K.Atr[a * 3 + b];
            A[(3 + a) * 6 + b] = 0.0;
            A[(3 + a) * 6 + 3 + b] = K.Arr[a * 3 + b];
            B[a * 6 + b] = K.Btt[a * 3 + b];
            B[a * 6 + 3 + b] = 0.0;
            B[(3 + a) * 6 + b] = 0.0;
            B[(3 + a) * 6 + 3 + b] = K.Brr[a * 3 + b];
        }
}
ELM_HD void pg_edge_terms(const double Pi[12], const double Pj[12], const double PZ[12], double r[6], double A[36], double B[36]) {
    PgBlocks K;
    pg_edge_blocks(Pi, Pj, PZ, r, K);
    pg_blocks_full(K, A, B);
}

// ---- the prior (include/elimaloc_hip_posegraph_prior.h): a measured pose Z of node v's point l ----
// The residual alone (the cost kernel): r = [R_Z^T ((t_v + R_v l) - t_Z); Log(R_Z^T R_v)].  With l = 0 every operation is the one
// pg_residual performs on (I, T_v, Z), so the numbers are the same.
ELM_HD void pg_prior_point(const double Rv[9], const double tv[3], const double l[3], const double tZ[3], double e[3]) {
#pragma unroll
    for (int a = 0; a < 3; ++a) e[a] = (tv[a] + ((Rv[a * 3] * l[0] + Rv[a * 3 + 1] * l[1]) + Rv[a * 3 + 2] * l[2])) - tZ[a];
}
ELM_HD void pg_prior_residual(const double Pv[12], const double PZ[12], const double l[3], double r[6]) {
    double Rv[9], tv[3], RZ[9], tZ[3], e[3], RE[9];
    pg_split(Pv, Rv, tv);
    pg_split(PZ, RZ, tZ);
    pg_prior_point(Rv, tv, l, tZ, e);
    pg_mul3_atv(RZ, e, r);
    pg_mul3_at(RZ, Rv, RE);
    double theta, qw, n, phi[3];
    pg_log(RE, phi, theta, qw, n);
    r[3] = phi[0];
    r[4] = phi[1];
    r[5] = phi[2];
}
// The residual and the non-zero 3 x 3 blocks of J = dr/dx_v = [ Jtt  Jtr ;  0  Jrr ] = [ R_E  -R_E [l]x ;  0  J^-1 ].
struct PgPriorBlocks {
    double Jtt[9], Jtr[9], Jrr[9];
};
ELM_HD void pg_prior_blocks(const double Pv[12], const double PZ[12], const double l[3], double r[6], PgPriorBlocks& K) {
    double Rv[9], tv[3], RZ[9], tZ[3], e[3];
    pg_split(Pv, Rv, tv);
    pg_split(PZ, RZ, tZ);
    pg_prior_point(Rv, tv, l, tZ, e);
    pg_mul3_atv(RZ, e, r);
    pg_mul3_at(RZ, Rv, K.Jtt);
    double theta, qw, n, phi[3];
    pg_log(K.Jtt, phi, theta, qw, n);
    r[3] = phi[0];
    r[4] = phi[1];
    r[5] = phi[2];
    pg_jinv(phi, pg_jinv_c(theta, qw, n), K.Jrr);
    const double lx[9] = {0.0, -l[2], l[1], l[2], 0.0, -l[0], -l[1], l[0], 0.0};
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) K.Jtr[a * 3 + b] = -((K.Jtt[a * 3] * lx[b] + K.Jtt[a * 3 + 1] * lx[3 + b]) + K.Jtt[a * 3 + 2] * lx[6 + b]);
}
// the blocks as a full row-major 6 x 6 matrix
ELM_HD void pg_prior_full(const PgPriorBlocks& K, double* J) {
#pragma unroll
    for (int a = 0; a < 3; ++a)
#pragma unroll
        for (int b = 0; b < 3; ++b) {
            J[a * 6 + b] = K.Jtt[a * 3 + b];
            J[a * 6 + 3 + b] = K.Jtr[a * 3 + b];
            J[(3 + a) * 6 + b] = 0.0;
            J[(3 + a) * 6 + 3 + b] = K.Jrr[a * 3 + b];
        }
}
ELM_HD void pg_prior_terms(const double Pv[12], const double PZ[12], const double l[3], double r[6], double J[36]) {
    PgPriorBlocks K;
    pg_prior_blocks(Pv, PZ, l, r, K);
    pg_prior_full(K, J);
}

// Huber on s = r^T Omega r: the weight, and the cost rho.  k = 0: off.  s == k^2 is an inlier.
ELM_HD double pg_huber_weight(double s, double k) { return (k > 0.0 && s > k * k) ? k / sqrt(s) : 1.0; }
ELM_HD double pg_huber_cost(double s, double k) { return (k > 0.0 && s > k * k) ? (2.0 * k) * sqrt(s) - k * k : s; }

// The retraction of x = [v; w]: R <- R Exp(w), t <- t + R v, on pose rows.
ELM_HD void pg_retract(const double P[12], const double x[6], double out[12]) {
    double R[9], t[3], E[9], Rn[9];
    pg_split(P, R, t);
    rotvec_to_matrix(x + 3, E);
    mul3(R, E, Rn);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        out[r * 4] = Rn[r * 3];
        out[r * 4 + 1] = Rn[r * 3 + 1];
        out[r * 4 + 2] = Rn[r * 3 + 2];
        out[r * 4 + 3] = t[r] + ((R[r * 3] * x[0] + R[r * 3 + 1] * x[1]) + R[r * 3 + 2] * x[2]);
    }
}

// ---- 6 x 6 blocks (row-major) ----
// row . v
ELM_HD double pg_dot6(const double* row, const double* v) {
    double t = row[0] * v[0];
#pragma unroll
    for (int b = 1; b < 6; ++b) t += row[b] * v[b];
    return t;
}
// out = M v
ELM_HD void pg_mv6(const double* M, const double* v, double out[6]) {
#pragma unroll
    for (int a = 0; a < 6; ++a) out[a] = pg_dot6(M + a * 6, v);
}
// column . v, the column's entries 6 apart: entry a of M^T v is pg_dot6_col(M + a, v)
ELM_HD double pg_dot6_col(const double* col, const double* v) {
    double t = col[0] * v[0];
#pragma unroll
    for (int b = 1; b < 6; ++b) t += col[b * 6] * v[b];
    return t;
}
// entry (a, c) of X Y, of X Y^T and of X^T Y
ELM_HD double pg_mm6(const double* X, const double* Y, int a, int c) {
    double t = X[a * 6] * Y[c];
#pragma unroll
    for (int b = 1; b < 6; ++b) t += X[a * 6 + b] * Y[b * 6 + c];
    return t;
}
ELM_HD double pg_mmt6(const double* X, const double* Y, int a, int c) { return pg_dot6(X + a * 6, Y + c * 6); }
ELM_HD double pg_mtm6(const double* X, const double* Y, int a, int c) {
    double t = X[a] * Y[c];
#pragma unroll
    for (int b = 1; b < 6; ++b) t += X[b * 6 + a] * Y[b * 6 + c];
    return t;
}

// the workgroups of a kernel that gives every edge a lane group of kPgLanesPerEdge; the most hubs a graph of Ec edges can have
constexpr uint32_t pg_edge_group_blocks(uint32_t E) { return (uint32_t)(((size_t)E * kPgLanesPerEdge + 255) / 256); }
constexpr size_t pg_max_hubs(size_t Ec) { return 2 * Ec / (kPgHubDegree + 1) + 1; }

#if defined(__HIPCC__) && defined(__forceinline__) // ---- device only ----
// The sum of one value per lane of a 256-lane workgroup, as a fixed tree in LDS (buf: 256 doubles); every lane returns it.
__device__ __forceinline__ double pg_block_sum(double v, double* buf) {
    const uint32_t tid = threadIdx.x;
    __syncthreads(); // (an earlier use of buf has been read)
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t h = kPgBlock / 2; h > 0; h >>= 1) {
        if (tid < h) buf[tid] = buf[tid] + buf[tid + h];
        __syncthreads();
    }
    return buf[0];
}
__device__ __forceinline__ double pg_block_max(double v, double* buf) {
    const uint32_t tid = threadIdx.x;
    __syncthreads();
    buf[tid] = v;
    __syncthreads();
#pragma unroll
    for (uint32_t h = kPgBlock / 2; h > 0; h >>= 1) {
        if (tid < h) buf[tid] = fmax(buf[tid], buf[tid + h]);
        __syncthreads();
    }
    return buf[0];
}
// The sum of n partial slots: lane t adds slots t, t + 256, ... in ascending order, then the tree.  The same n gives the same tree.
__device__ __forceinline__ double pg_sum_slots(const double* __restrict__ slots, uint32_t n, double* buf) {
    double v = 0.0;
    for (uint32_t k = threadIdx.x; k < n; k += kPgBlock) v += slots[k];
    return pg_block_sum(v, buf);
}

// the pose rows of edge e's two nodes at `poses`, and of its measurement
__device__ __forceinline__ void pg_load_edge_poses(const PgDev& d, const double* __restrict__ poses, uint32_t e, double Pi[12], double Pj[12],
                                                   double PZ[12]) {
    const double* __restrict__ pi = poses + 12 * (size_t)d.ei[e];
    const double* __restrict__ pj = poses + 12 * (size_t)d.ej[e];
    const double* __restrict__ pz = d.Z + 12 * (size_t)e;
#pragma unroll
    for (int k = 0; k < 12; ++k) {
        Pi[k] = pi[k];
        Pj[k] = pj[k];
        PZ[k] = pz[k];
    }
}
#endif

} // namespace elm
