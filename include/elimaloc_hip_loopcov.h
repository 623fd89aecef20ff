/* elimaloc_hip_loopcov.h -- loop closing with a propagated covariance: the pairwise consistency check of elimaloc_hip_loops.h with the
 * 6 x 6 covariance of the odometry carried along the chain and a Mahalanobis distance on the cycle's residual, so that gamma = 16.81 is
 * the 99 % point of chi^2 with 6 degrees of freedom.  Part of elimaloc_hip.h, which includes it; include that header, not this one.
 *
 * WHY.  The scalar model of elimaloc_hip_loops.h is a random walk in the number of steps: rotation drift times lever arm is not in it,
 * and a caller had to inflate q_t by hand until the true loops agreed.  Here the caller states the covariance of one odometry step and
 * of every loop measurement, and the arithmetic does the rest.
 *
 * CONVENTIONS, those of the pose graph.  A tangent is x = [v; w] and T (+) x = [R Exp(w) | t + R v]; a covariance is a 6 x 6 in that
 * order, row-major (symmetric, so the order of the two indices does not matter).  For X = [R | t], Ad(X) = [[R, [t]x R], [0, R]].  A
 * loop's covariance Sigma_k is that of xi in Z_k = X_true (+) xi; to first order it is the inverse of the information that the pose
 * graph puts on that edge's residual (r ~ -xi).
 *
 * INPUTS.  n poses (a chain in index order) and L loops (a_k, b_k, Z_k), exactly as elm_loops_consistency takes them.  Sigma36 [L][36],
 * one covariance per loop.  Q36 [q_count][36], the covariance of the odometry step v -> v + 1, of xi in X_{v,v+1} = X_true (+) xi;
 * q_count is 1 (one Q for every step) or n - 1.
 *
 * CHAIN COVARIANCE.  Y_v = T_0^-1 T_v (re-basing on pose 0 keeps map coordinates of 1e5 m out of the lever arms).
 *   P_v = Ad(Y_{v+1}) Q_v Ad(Y_{v+1})^T,   W_0 = 0,   W_v = sum_{u < v} P_u
 * a plain additive prefix sum of symmetric 6 x 6 matrices in the frame of pose 0.  The covariance of the odometry between u and v, in
 * either direction, expressed in that frame, is C(u, v) = W_max(u,v) - W_min(u,v).  The sum's tree is fixed (a shift-and-add scan
 * over the 64 lanes of a wavefront, the 16 wavefronts of a block of 1 024 terms added in sequence, the same once more over the block
 * totals): the same inputs give the same bytes on every run, and there are no atomics.  21 entries are computed and
 * mirrored, so W is exactly symmetric.  S_v = Ad(Y_v^-1) W_v Ad(Y_v^-1)^T is the covariance of T_v relative to T_0 in v's own tangent.
 *
 * PAIR TERM.  For k < l, on the re-based poses Y (X_uv = Y_u^-1 Y_v): e is the e of elimaloc_hip_loops.h by the same code,
 * B = X_{b_l b_k}, C_a = C(a_k, a_l), C_b = C(b_k, b_l),
 *   Sigma_Zhat = (G_A C_a G_A^T + G_l Sigma_l G_l^T) + G_B C_b G_B^T
 *                G_B = Ad(Y_{b_k}^-1),  G_l = Ad(B^-1),  G_A = Ad((Y_{a_l} Z_l B)^-1)
 *   Sigma_e    = Sigma_k + Sigma_Zhat
 *   s          = e^T Sigma_e^-1 e
 * Sigma_e^-1 comes from an L D L^T without pivoting in index order 0 .. 5 (s = sum_j y_j^2 / d_j with L y = e); a pivot that is not
 * finite or not > 0 gives s = NaN, which is not adjacent.  adj[k][l] = adj[l][k] = (s <= gamma), the lower index always k, the
 * diagonal 0.  Float64 without contraction throughout.
 *
 * MODEL LIMITS.  The model is first order.  The residual's Jacobians are taken at e = 0, where they are +-I.  The two odometry ranges
 * of a cycle are treated as independent even where they overlap (the scalar model's m has the same limit).  Odometry and loops are
 * treated as independent.
 *
 * CLIQUE.  That of elimaloc_hip_loops.h, by the same kernels.
 *
 * LIMITS AND PRECONDITIONS: those of elm_loops_consistency (without its variances), checked on the host before anything is launched;
 * each is ELM_ERR_INVALID with a text in elm_last_error and leaves the outputs untouched.  In addition: q_count not 1 and not n - 1
 * (with n = 1, q_count = 1 is accepted and nothing is read); a NULL Q36 where one is read, or with L > 0 a NULL Sigma36; a Q or Sigma
 * that is non-finite or not exactly symmetric; a Sigma_k whose L D L^T (the routine of the pair term) has a pivot that is not > 0; a
 * config whose q_t or q_r is not 0 (the two models do not add up).  Q need not be definite: an indefinite sum makes pairs non-adjacent.
 * L = 0 is ELM_OK and launches nothing.  A device group's lead, a communicator or hook, and a batch in flight are refused as there.
 * The calls keep nothing on the device between calls. */
#ifndef ELIMALOC_HIP_LOOPCOV_H
#define ELIMALOC_HIP_LOOPCOV_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct elm_loopcov_result {
    int32_t size;                              /* members of the clique */
    int32_t steps;                             /* greedy picks */
    int64_t adjacent_pairs;                    /* pairs k < l with adj[k][l] */
    int64_t non_finite_pairs;                  /* pairs k < l whose s is NaN */
    double chain_ms, adjacency_ms, greedy_ms;  /* device time of the chain covariance, the pair kernels and the greedy loop (stream events) */
} elm_loopcov_result;
/* W_out [n][36]; S_out [n][36] or NULL.  Refused as above: a NULL ctx, poses16 or W_out, n outside 1 .. 2^20, a non-finite pose, q_count,
 * Q.  Column-major 4 x 4 poses as everywhere. */
int elm_loopcov_chain(elm_ctx* ctx, const double* poses16, size_t n, const double* Q36, size_t q_count, double* W_out, double* S_out);
/* Host only: one pair by the code the kernel runs.  T0: pose 0 of the chain; Ta, Tb, Zk, Sigma_k: loop k's ends, measurement and
 * covariance; Tc, Td, Zl, Sigma_l: loop l's; Ca = C(a_k, a_l), Cb = C(b_k, b_l) [36] as elm_loopcov_chain's W gives them.  Writes
 * e_out [6], cov_out [36] (Sigma_e) and s_out [1] (NaN on a bad pivot).  ELM_ERR_INVALID for a NULL or non-finite argument. */
int elm_loopcov_pair_terms(const double* T0, const double* Ta, const double* Tb, const double* Zk, const double* Sigma_k, const double* Tc,
                           const double* Td, const double* Zl, const double* Sigma_l, const double* Ca, const double* Cb, double* e_out,
                           double* cov_out, double* s_out);
/* The arguments of elm_loops_consistency with Sigma36 [L][36] in place of the two variances, and Q36 [q_count][36].  cfg gives gamma and
 * steps_per_batch; its q_t and q_r must be 0.  L <= ELM_LOOPS_MAX, and ELM_LOOPS_MAX_S with s_out (NaN where a pivot failed). */
int elm_loopcov_consistency(elm_ctx* ctx, const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16,
                            const double* Sigma36, size_t L, const double* Q36, size_t q_count, const elm_loops_config* cfg,
                            elm_loopcov_result* result, uint8_t* member_out, int32_t* degree_out, uint64_t* adj_out, double* s_out);

#ifdef __cplusplus
}
#endif
#endif
