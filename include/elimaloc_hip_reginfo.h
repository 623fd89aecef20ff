/* elimaloc_hip_reginfo.h -- registration information: the 6 x 6 Gauss-Newton information of a scan registered against a map at a pose,
 * an a-posteriori variance factor and the directions the scan does not constrain.  Part of elimaloc_hip.h, which includes it; include
 * that header, not this one.
 *
 * WHY.  Every measurement of the graph back end (elm_posegraph_add_edges, elm_posegraph_add_priors, the loop consistency) takes a 6 x 6
 * information matrix, and the registration did not produce one: elm_reg_result.local_cov is the identity for P2P, VGICP and AVGICP and an
 * arbitrarily scaled inverse of the damped normal matrix for GICP.  This call computes, for many (scan, pose) jobs in one call on the
 * GPU, the matrix a caller hands to the graph as it is.
 *
 * CONVENTIONS are the pose graph's: the tangent is x = [v; w] with t <- t + R v and R <- R Exp(w), which is also
 * the local-frame Jacobian of the registration itself (registration.cpp:36-41).  The matrix is therefore an edge information for
 * Z = T_a^-1 T and a prior information for Z = T with a zero lever; no adjoint is needed.  Float64 without contraction.  All 6 x 6
 * blocks are row-major.
 *
 * PER JOB (scan s, pose T = [R | t]), with reg->icp_method and th = reg->max_search_dist:
 *   1. every resident scan point p (float32 widened) gives g = T p = ((T0 px + T4 py) + T8 pz) + T12, ...;
 *   2. the pairs are exactly those of elm_map_get_correspondences at g (what = 0 for P2P and GICP, 1 for VGICP, 2 for AVGICP), the
 *      reference's default target at the origin included, found by the search that call itself would choose;
 *   3. the target mu is the map point (P2P), the point's neighbourhood mean (GICP) or the voxel mean (VGICP, AVGICP); the residual is
 *      e = R^T (mu - t) - p and J = [I, -[p]x];
 *      ELM_REGINFO_METRIC_METHOD: M = I for P2P, else M = R^T Sbar R with Sbar = (S + S^T) / 2 of the stored inverse covariance the
 *      registration uses; the default-target pair has M = I;
 *      ELM_REGINFO_METRIC_PLANE (P2P and GICP on a map with point covariances): M = n n^T, n = R^T (the point's plane normal), the
 *      point-to-plane information; the default-target pair is dropped;
 *   4. weights, with w0 = th^2 / (th + |e|^2)^2: P2P w0; GICP 0.8 w0 + 0.2; VGICP / AVGICP w0, and a pair with w0 < 0.01 contributes
 *      nothing and is not counted;
 *   5. H = sum w J^T M J (upper triangle, mirrored: exactly symmetric), g = sum w J^T M e, chi2 = sum w e^T M e, sw = sum w,
 *      swr2 = sum w |p|^2, n_pairs, n_default.
 *      ORDER OF THE SUMS (no float atomics): a partial per 256-point chunk of the job -- per wavefront the lanes' sum, then
 *      ((w0 + w1) + w2) + w3 over the four wavefronts -- and then the job's chunks one by one in ascending order, each added onto the
 *      running sum that starts at 0.  A job's bytes are the same on every run and do not depend on which jobs share the call;
 *   6. finish, on the GPU: l = cfg->length_scale_m if > 0, else sqrt(swr2 / sw) (1 if that is not positive); D = diag(1, 1, 1, 1/l, 1/l,
 *      1/l); S6 = D H D; cyclic Jacobi on S6: eigenvalues ascending, eigenvector k in column k of `eigenvectors`, signed so that its
 *      largest-magnitude component (the first of equals) is positive.  rank = the number of lambda_k > min_eigen_ratio lambda_max (at
 *      ratio 0: lambda_k > 0, decided by rounding where H is exactly singular -- give a ratio to ask a robust question).
 *      dof = m n_pairs - rank, m = 3 (method metric) or 1 (plane metric).  sigma2 = cfg->sigma2 if > 0, else chi2 / dof.
 *      information = H / sigma2 when nothing is dropped (min_eigen_ratio == 0, or rank == 6), else D^-1 V_o Lambda_o V_o^T D^-1 / sigma2
 *      over the kept eigenpairs (upper triangle, mirrored).  Exactly symmetric either way.
 *
 * STATUS, a bit set:
 *   NO_PAIRS    n_pairs == 0: every number is zero (n_points is the scan's size; rank = 0, so DEGENERATE is set too);
 *   NO_DOF      dof <= 0 and no cfg->sigma2: sigma2 = 0 and information = 0; H and the rest are delivered;
 *   DEGENERATE  rank < 6;
 *   NON_FINITE  some delivered number is not finite (e.g. chi2 == 0 with dof > 0 and no cfg->sigma2).
 *
 * REFUSED.  ELM_ERR_UNSUPPORTED on a device group or with a communicator or hook attached, and for reg->use_radar_cov != 0 (source
 * covariances are not part of this call).  ELM_ERR_INVALID for a null argument, a batch in flight, a map or scan of another context,
 * non-finite poses, n_jobs outside 1 .. ELM_REGINFO_MAX_JOBS, an unknown method or metric, th not finite or <= 0, sigma2 or
 * length_scale_m negative or not finite, min_eigen_ratio outside [0, 1), the plane metric with VGICP / AVGICP, and more than 0x7FFFFF00
 * points in all.  Missing covariances: the code and text of the registration itself.  An empty map: ELM_OK, every job NO_PAIRS. */
#ifndef ELIMALOC_HIP_REGINFO_H
#define ELIMALOC_HIP_REGINFO_H
#ifdef __cplusplus
extern "C" {
#endif

#define ELM_REGINFO_MAX_JOBS 4096
#define ELM_REGINFO_METRIC_METHOD 0
#define ELM_REGINFO_METRIC_PLANE 1
#define ELM_REGINFO_NO_PAIRS 1
#define ELM_REGINFO_NO_DOF 2
#define ELM_REGINFO_DEGENERATE 4
#define ELM_REGINFO_NON_FINITE 8

typedef struct elm_reginfo_config {
    int32_t metric;         /* ELM_REGINFO_METRIC_METHOD (default) or _PLANE */
    int32_t _pad;
    double sigma2;          /* > 0: the variance factor; 0 (default): chi2 / dof */
    double length_scale_m;  /* > 0: l; 0 (default): sqrt(swr2 / sw) */
    double min_eigen_ratio; /* 0 <= . < 1; default 0: nothing is dropped */
} elm_reginfo_config;
typedef struct elm_reginfo_result {
    double information[36];
    double H[36];
    double g[6];
    double chi2, sigma2, length_scale;
    double eigenvalues[6];   /* of S6 = D H D, ascending */
    double eigenvectors[36]; /* of S6: entry [i * 6 + k] is component i of eigenvector k */
    int32_t n_points, n_pairs, n_default, dof, rank, status;
} elm_reginfo_result;
void elm_reginfo_config_default(elm_reginfo_config* c);
/* scans [n_jobs], poses16 [n_jobs][16] column-major, results [n_jobs] */
int elm_register_information(elm_ctx* ctx, const elm_map* map, const elm_scan* const* scans, const double* poses16, int n_jobs,
                             const elm_reg_config* reg, const elm_reginfo_config* cfg, elm_reginfo_result* results);
/* Host only: one pair's terms by the code the kernel runs, compiled for the host.  T16 column-major, p the scan point, mu the target,
 * S9 the stored inverse covariance row-major (NULL: the identity, as for the default target), normal3 the plane normal in the map frame
 * (read by the plane metric only, where it must not be NULL), th, method, metric.  w (0 for a pair that contributes nothing), JtMJ36
 * row-major, JtMe6 and eMe -- not yet multiplied by w -- each when not NULL. */
int elm_reginfo_pair_terms(const double T16[16], const double p[3], const double mu[3], const double* S9, const double* normal3, double th,
                           int method, int metric, double* w, double* JtMJ36, double* JtMe6, double* eMe);

#ifdef __cplusplus
}
#endif
#endif
