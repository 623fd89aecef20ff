// elm_dev_reginfo.hpp -- registration information (include/elimaloc_hip_reginfo.h): one pair's terms, the cyclic
// Jacobi of a symmetric 6 x 6 and the finish of a job from its sums.  Host and device run this same code (elm_reginfo_pair_terms is the
// host's call of the pair terms).  Float64, row-major, no contraction.
#pragma once
#include <math.h>
#include <stdint.h>

#include "../../include/elimaloc_hip.h"
#include "elm_la.hpp"

namespace elm {

// a job's sums, and a chunk's partial: the upper triangle of H, g, chi2, sum w, sum w |p|^2, the pairs, the default-target pairs
constexpr int kRiH = 0, kRiG = 21, kRiChi2 = 27, kRiSw = 28, kRiSwr2 = 29, kRiPairs = 30, kRiDefault = 31, kRiWords = 32;
// upper-triangle packing of the symmetric 6 x 6: index of (i, j), i <= j
ELM_HD constexpr int ri_tri(int i, int j) { return i * 6 - (i * (i - 1)) / 2 + (j - i); }

// One pair, unweighted: M6 = {M00, M01, M02, M11, M12, M22} of the local metric, Ht the upper triangle of J^T M J, gt = J^T M e,
// chi = e^T M e, with J = [I, B], B = -[p]x.
struct RegInfoPair {
    double w;
    double Ht[21];
    double gt[6];
    double chi;
};

// rows: (R_r0, R_r1, R_r2, t_r) per row r of the pose.  S: the stored inverse covariance, row-major, or null for the identity; nrm: the
// plane normal in the map frame (METRIC == ELM_REGINFO_METRIC_PLANE only).  false: the pair contributes nothing.
template <int METHOD, int METRIC>
ELM_HD bool reginfo_pair(const double* rows, double px, double py, double pz, double mx, double my, double mz, const double* S, const double* nrm,
                         double th, RegInfoPair& o) {
    const double d0 = mx - rows[3], d1 = my - rows[7], d2 = mz - rows[11];
    const double e0 = ((rows[0] * d0 + rows[4] * d1) + rows[8] * d2) - px;
    const double e1 = ((rows[1] * d0 + rows[5] * d1) + rows[9] * d2) - py;
    const double e2 = ((rows[2] * d0 + rows[6] * d1) + rows[10] * d2) - pz;
    const double en2 = (e0 * e0 + e1 * e1) + e2 * e2;
    const double w0 = (th * th) / ((th + en2) * (th + en2));
    if ((METHOD == ELM_VGICP || METHOD == ELM_AVGICP) && w0 < 0.01) return false;
    o.w = (METHOD == ELM_GICP) ? w0 * 0.8 + 0.2 : w0;
    double m00 = 1.0, m01 = 0.0, m02 = 0.0, m11 = 1.0, m12 = 0.0, m22 = 1.0;
    if (METRIC == ELM_REGINFO_METRIC_PLANE) {
        const double n0 = (rows[0] * nrm[0] + rows[4] * nrm[1]) + rows[8] * nrm[2];
        const double n1 = (rows[1] * nrm[0] + rows[5] * nrm[1]) + rows[9] * nrm[2];
        const double n2 = (rows[2] * nrm[0] + rows[6] * nrm[1]) + rows[10] * nrm[2];
        m00 = n0 * n0; m01 = n0 * n1; m02 = n0 * n2; m11 = n1 * n1; m12 = n1 * n2; m22 = n2 * n2;
    } else if (METHOD != ELM_P2P && S) {
        const double s00 = S[0], s11 = S[4], s22 = S[8];
        const double s01 = 0.5 * (S[1] + S[3]), s02 = 0.5 * (S[2] + S[6]), s12 = 0.5 * (S[5] + S[7]);
        // A = Sbar R, M = R^T A
        const double a00 = (s00 * rows[0] + s01 * rows[4]) + s02 * rows[8], a01 = (s00 * rows[1] + s01 * rows[5]) + s02 * rows[9],
                     a02 = (s00 * rows[2] + s01 * rows[6]) + s02 * rows[10];
        const double a10 = (s01 * rows[0] + s11 * rows[4]) + s12 * rows[8], a11 = (s01 * rows[1] + s11 * rows[5]) + s12 * rows[9],
                     a12 = (s01 * rows[2] + s11 * rows[6]) + s12 * rows[10];
        const double a20 = (s02 * rows[0] + s12 * rows[4]) + s22 * rows[8], a21 = (s02 * rows[1] + s12 * rows[5]) + s22 * rows[9],
                     a22 = (s02 * rows[2] + s12 * rows[6]) + s22 * rows[10];
        m00 = (rows[0] * a00 + rows[4] * a10) + rows[8] * a20;
        m01 = (rows[0] * a01 + rows[4] * a11) + rows[8] * a21;
        m02 = (rows[0] * a02 + rows[4] * a12) + rows[8] * a22;
        m11 = (rows[1] * a01 + rows[5] * a11) + rows[9] * a21;
        m12 = (rows[1] * a02 + rows[5] * a12) + rows[9] * a22;
        m22 = (rows[2] * a02 + rows[6] * a12) + rows[10] * a22;
    }
    const double v0 = (m00 * e0 + m01 * e1) + m02 * e2, v1 = (m01 * e0 + m11 * e1) + m12 * e2, v2 = (m02 * e0 + m12 * e1) + m22 * e2;
    o.chi = (e0 * v0 + e1 * v1) + e2 * v2;
    // M B, row i: (M_i2 py - M_i1 pz, M_i0 pz - M_i2 px, M_i1 px - M_i0 py)
    const double b00 = m02 * py - m01 * pz, b01 = m00 * pz - m02 * px, b02 = m01 * px - m00 * py;
    const double b10 = m12 * py - m11 * pz, b11 = m01 * pz - m12 * px, b12 = m11 * px - m01 * py;
    const double b20 = m22 * py - m12 * pz, b21 = m02 * pz - m22 * px, b22 = m12 * px - m02 * py;
    o.Ht[ri_tri(0, 0)] = m00; o.Ht[ri_tri(0, 1)] = m01; o.Ht[ri_tri(0, 2)] = m02; o.Ht[ri_tri(1, 1)] = m11; o.Ht[ri_tri(1, 2)] = m12;
    o.Ht[ri_tri(2, 2)] = m22;
    o.Ht[ri_tri(0, 3)] = b00; o.Ht[ri_tri(0, 4)] = b01; o.Ht[ri_tri(0, 5)] = b02;
    o.Ht[ri_tri(1, 3)] = b10; o.Ht[ri_tri(1, 4)] = b11; o.Ht[ri_tri(1, 5)] = b12;
    o.Ht[ri_tri(2, 3)] = b20; o.Ht[ri_tri(2, 4)] = b21; o.Ht[ri_tri(2, 5)] = b22;
    // B^T (M B), upper triangle; B^T x = (py x2 - pz x1, pz x0 - px x2, px x1 - py x0)
    o.Ht[ri_tri(3, 3)] = py * b20 - pz * b10; o.Ht[ri_tri(3, 4)] = py * b21 - pz * b11; o.Ht[ri_tri(3, 5)] = py * b22 - pz * b12;
    o.Ht[ri_tri(4, 4)] = pz * b01 - px * b21; o.Ht[ri_tri(4, 5)] = pz * b02 - px * b22;
    o.Ht[ri_tri(5, 5)] = px * b12 - py * b02;
    o.gt[0] = v0; o.gt[1] = v1; o.gt[2] = v2;
    o.gt[3] = py * v2 - pz * v1; o.gt[4] = pz * v0 - px * v2; o.gt[5] = px * v1 - py * v0;
    return true;
}

// Cyclic Jacobi eigen-decomposition of a symmetric 6 x 6 (row-major), on the pattern of eig3_sym_desc (elm_la.hpp): eigenvalues w[6]
// ASCENDING, eigenvector k in column k of v (row-major), signed so that its largest-magnitude component, the first of equals, is positive.
ELM_HD void eig6_sym_asc(const double* ain, double* w, double* v) {
    double a[36];
    for (int i = 0; i < 36; ++i) { a[i] = ain[i]; v[i] = (i % 7 == 0) ? 1.0 : 0.0; }
    for (int sweep = 0; sweep < 48; ++sweep) {
        double off = 0.0, dia = 0.0;
        for (int i = 0; i < 6; ++i) {
            dia += fabs(a[i * 7]);
            for (int j = i + 1; j < 6; ++j) off += fabs(a[i * 6 + j]);
        }
        if (off <= 1e-300 || off <= 1e-22 * dia) break;
        for (int p = 0; p < 5; ++p)
            for (int q = p + 1; q < 6; ++q) {
                const double apq = a[p * 6 + q];
                if (apq == 0.0) continue;
                const double th = (a[q * 7] - a[p * 7]) / (2.0 * apq);
                const double t = (th >= 0.0 ? 1.0 : -1.0) / (fabs(th) + sqrt(th * th + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                a[p * 7] = a[p * 7] - t * apq;
                a[q * 7] = a[q * 7] + t * apq;
                a[p * 6 + q] = 0.0; a[q * 6 + p] = 0.0;
                for (int k = 0; k < 6; ++k) {
                    if (k != p && k != q) {
                        const double akp = a[k * 6 + p], akq = a[k * 6 + q];
                        const double np = c * akp - s * akq, nq = s * akp + c * akq;
                        a[k * 6 + p] = np; a[p * 6 + k] = np;
                        a[k * 6 + q] = nq; a[q * 6 + k] = nq;
                    }
                    const double vkp = v[k * 6 + p], vkq = v[k * 6 + q];
                    v[k * 6 + p] = c * vkp - s * vkq;
                    v[k * 6 + q] = s * vkp + c * vkq;
                }
            }
    }
    for (int i = 0; i < 6; ++i) w[i] = a[i * 7];
    for (int i = 0; i < 5; ++i) { // selection sort, ascending, the first of equals stays first; the columns of v follow
        int pos = i;
        for (int k = i + 1; k < 6; ++k)
            if (w[k] < w[pos]) pos = k;
        if (pos != i) {
            double q = w[i]; w[i] = w[pos]; w[pos] = q;
            for (int r = 0; r < 6; ++r) { q = v[r * 6 + i]; v[r * 6 + i] = v[r * 6 + pos]; v[r * 6 + pos] = q; }
        }
    }
    for (int k = 0; k < 6; ++k) {
        int big = 0;
        for (int r = 1; r < 6; ++r)
            if (fabs(v[r * 6 + k]) > fabs(v[big * 6 + k])) big = r;
        if (v[big * 6 + k] < 0.0)
            for (int r = 0; r < 6; ++r) v[r * 6 + k] = -v[r * 6 + k];
    }
}

// A job's result from its sums s[kRiWords] (step 6 of the contract); m = 3 (method metric) or 1 (plane metric).
ELM_HD void reginfo_finish(const double* s, const elm_reginfo_config& cfg, int m, int32_t n_points, elm_reginfo_result& r) {
    for (int k = 0; k < 36; ++k) { r.information[k] = 0.0; r.H[k] = 0.0; r.eigenvectors[k] = 0.0; }
    for (int k = 0; k < 6; ++k) { r.g[k] = 0.0; r.eigenvalues[k] = 0.0; }
    r.chi2 = 0.0; r.sigma2 = 0.0; r.length_scale = 0.0;
    r.n_points = n_points; r.n_pairs = (int32_t)s[kRiPairs]; r.n_default = (int32_t)s[kRiDefault];
    r.dof = 0; r.rank = 0; r.status = 0;
    if (r.n_pairs == 0) {
        r.n_default = 0;
        r.status = ELM_REGINFO_NO_PAIRS | ELM_REGINFO_DEGENERATE;
        return;
    }
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { r.H[i * 6 + j] = s[kRiH + ri_tri(i, j)]; r.H[j * 6 + i] = r.H[i * 6 + j]; }
    for (int k = 0; k < 6; ++k) r.g[k] = s[kRiG + k];
    r.chi2 = s[kRiChi2];
    double l = cfg.length_scale_m > 0.0 ? cfg.length_scale_m : sqrt(s[kRiSwr2] / s[kRiSw]);
    if (!(l > 0.0)) l = 1.0;
    r.length_scale = l;
    double dinv[6], S6[36];
    for (int k = 0; k < 6; ++k) dinv[k] = k < 3 ? 1.0 : 1.0 / l;
    for (int i = 0; i < 6; ++i)
        for (int j = i; j < 6; ++j) { S6[i * 6 + j] = (dinv[i] * r.H[i * 6 + j]) * dinv[j]; S6[j * 6 + i] = S6[i * 6 + j]; }
    eig6_sym_asc(S6, r.eigenvalues, r.eigenvectors);
    const double cut = cfg.min_eigen_ratio * r.eigenvalues[5];
    int rank = 0;
    for (int k = 0; k < 6; ++k)
        if (r.eigenvalues[k] > cut && r.eigenvalues[k] > 0.0) ++rank;
    r.rank = rank;
    r.dof = m * r.n_pairs - rank;
    if (rank < 6) r.status |= ELM_REGINFO_DEGENERATE;
    if (cfg.sigma2 > 0.0) r.sigma2 = cfg.sigma2;
    else if (r.dof > 0) r.sigma2 = r.chi2 / (double)r.dof;
    else r.status |= ELM_REGINFO_NO_DOF;
    if (!(r.status & ELM_REGINFO_NO_DOF)) {
        if (cfg.min_eigen_ratio > 0.0 && rank < 6) {
            for (int i = 0; i < 6; ++i)
                for (int j = i; j < 6; ++j) {
                    double acc = 0.0;
                    for (int k = 0; k < 6; ++k)
                        if (r.eigenvalues[k] > cut && r.eigenvalues[k] > 0.0) acc += (r.eigenvectors[i * 6 + k] * r.eigenvalues[k]) * r.eigenvectors[j * 6 + k];
                    const double val = ((acc / dinv[i]) / dinv[j]) / r.sigma2;
                    r.information[i * 6 + j] = val;
                    r.information[j * 6 + i] = val;
                }
        } else {
            for (int k = 0; k < 36; ++k) r.information[k] = r.H[k] / r.sigma2;
        }
    }
    bool fin = isfinite(r.chi2) && isfinite(r.sigma2) && isfinite(r.length_scale);
    for (int k = 0; k < 36; ++k) fin = fin && isfinite(r.information[k]) && isfinite(r.H[k]) && isfinite(r.eigenvectors[k]);
    for (int k = 0; k < 6; ++k) fin = fin && isfinite(r.g[k]) && isfinite(r.eigenvalues[k]);
    if (!fin) r.status |= ELM_REGINFO_NON_FINITE;
}

} // namespace elm
