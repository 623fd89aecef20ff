/* elimaloc_hip_posegraph_cov.h -- the pose graph's marginal and relative covariances: blocks of the inverse of the normal equations of the
 * current linearization, by conjugate gradients on many unit right-hand sides at once.  Part of elimaloc_hip.h, which includes it;
 * include that header, not this one.
 *
 * WHY.  After elm_posegraph_optimize the graph is far better known than the open-loop chain covariance of elimaloc_hip_loopcov.h says.
 * These calls report how well: the covariance of a node, of a pair of nodes, and of a relative pose T_a^-1 T_b -- what a Mahalanobis
 * gate on a new loop candidate, an EKF update and a map-quality display need.
 *
 * WHAT.  With H the Hessian of the current linearization (elm_posegraph_linearize with its Huber weights, or the last one of
 * elm_posegraph_optimize; ELM_ERR_INVALID without a valid one, exactly as elm_posegraph_solve), column (k, c) is the solution x of
 *   (H + lambda diag H) x = e_(k,c)
 * over the active nodes; Sigma(row, col) is the 6 x 6 block [x_row of column (col, 0) | ... | x_row of column (col, 5)].  lambda = 0 gives
 * the covariance of the linearized problem, lambda > 0 that of the damped system.  The tangent is the pose graph's own: x = [v; w],
 * R <- R Exp(w), t <- t + R v; a block is row-major in that order.  An inactive node (fixed, or free without an edge) has a zero column
 * and zero rows; it is no error, and its columns report converged = 1 with 0 iterations.
 *
 * HOW.  The requested columns, column 6 i + c being component c of col_nodes[i], are cut into groups of 64, and the conjugate gradients
 * of elm_posegraph_solve run on a whole group with the lane as the column.  Each column has its own alpha, beta,
 * stop test (sqrt(r^T z) <= pcg_rel_tol sqrt(r0^T z0), the test of elm_posegraph_solve) and iteration count, and is frozen once it has
 * stopped.  The object's preconditioner is honoured: block Jacobi, or the chain of elimaloc_hip_posegraph_precond.h (the same factor; its
 * apply runs on whole column groups).
 *
 * DETERMINISM.  The bytes of a column depend on the graph, the linearization, lambda, the tolerance, the iteration limit and the
 * preconditioner, and on nothing else: not on which other columns were requested, not on the column's position in col_nodes, not on the
 * pass it fell into, not on the run.  There are no float atomics; every sum has a fixed order that depends only on the graph.
 *
 * NON-CONVERGENCE.  A column that has not met the stop test after pcg_max_iterations is returned as it is, with converged = 0; the other
 * columns of the call are not affected.  The typical case is lambda = 0 on a graph with a connected component that holds no fixed node:
 * H is singular on that component, the columns of its nodes do not converge and are meaningless, those of the other components are
 * right.  (A graph with no fixed node at all is refused, as below.)
 *
 * MEMORY.  The column vectors x, r, z, p, q of a group are 5 x 6 x 64 doubles per node: 15 360 N bytes, 16 GB at 2^20 nodes (with the
 * chain preconditioner a sixth of the same size, padded to whole segments of 256 nodes per level).  They live
 * in a scratch allocation of the call, freed before it returns.  As many groups as fit under scratch_bytes are solved together, the
 * others in further passes; one group is always allowed, whatever scratch_bytes says. */
#ifndef ELIMALOC_HIP_POSEGRAPH_COV_H
#define ELIMALOC_HIP_POSEGRAPH_COV_H
#ifdef __cplusplus
extern "C" {
#endif

typedef struct elm_posegraph_cov_config {
    double lambda;              /* 0: the covariance of the linearized problem; > 0: of the damped system */
    double pcg_rel_tol;         /* default 1e-10: the stop test of elm_posegraph_solve, per column */
    int32_t pcg_max_iterations; /* default 20000 */
    int32_t pcg_check_every;    /* default 32: iterations queued between two reads of the stop word */
    uint64_t scratch_bytes;     /* 0: the default cap of 2 GiB; one column group is always allowed */
} elm_posegraph_cov_config;

typedef struct elm_posegraph_cov_stats {
    int32_t n_columns;        /* 6 m */
    int32_t n_converged;      /* columns that met the stop test (those of inactive nodes included) */
    int32_t passes;
    int32_t iterations_max;   /* the largest iteration count of a column */
    double rel_residual_max;  /* the largest sqrt(r^T z) / sqrt(r0^T z0) of a column, from the recurrence */
    double ms_device;         /* stream events around the device work of all passes */
    uint64_t scratch_bytes;   /* what the call allocated */
} elm_posegraph_cov_stats;

void elm_posegraph_cov_config_default(elm_posegraph_cov_config* cfg);

/* Blocks of the inverse for the m nodes col_nodes (duplicates are legal and are solved again).  row_nodes [n_rows], or NULL and 0 for
 * the diagonal blocks only.  Every output may be NULL:
 *   diag36     [m][36]          Sigma(col_i, col_i), symmetrised once on the host as 0.5 (S + S^T)
 *   cross36    [m][n_rows][36]  Sigma(row_k, col_i) as solved
 *   iterations [m][6], converged [m][6]   per column
 * ELM_ERR_INVALID: a NULL ctx, pg or cfg; col_nodes NULL with m > 0, row_nodes NULL with n_rows > 0, cross36 without rows; a node out of
 * range; m above ELM_POSEGRAPH_MAX_NODES; a config with a negative or non-finite lambda or tolerance or a count below 1; no valid
 * linearization; lambda == 0 on a graph without a fixed node ("no fixed node (the gauge is free)", as elm_posegraph_optimize).
 * ELM_ERR_UNSUPPORTED: a device group's lead, a communicator or hook (as every pose-graph call); more than 2^25 requested blocks.  Each with a text in elm_last_error.  m = 0 is ELM_OK and launches nothing. */
int elm_posegraph_covariance(elm_ctx* ctx, elm_posegraph* pg, const int32_t* col_nodes, size_t m, const int32_t* row_nodes, size_t n_rows,
                             const elm_posegraph_cov_config* cfg, double* diag36, double* cross36, int32_t* iterations, uint8_t* converged,
                             elm_posegraph_cov_stats* stats);

/* cov36 [L][36]: the covariance of the residual coordinates of T_a^-1 T_b at Z = T_a^-1 T_b of the current poses,
 *   A Sigma_aa A^T + A Sigma_ab B^T + B Sigma_ba A^T + B Sigma_bb B^T,
 * A and B the edge Jacobians of elm_posegraph_edge_terms (the same host code) at (T_a, T_b, Z).  The columns solved are those of the
 * unique nodes of a and b in ascending order; the four products of a pair are formed and added on the host in the order written, and the
 * result is symmetrised as 0.5 (C + C^T).  a[k] == b[k] is ELM_ERR_INVALID; the other refusals are those of elm_posegraph_covariance.
 * stats may be NULL. */
int elm_posegraph_relative_covariance(elm_ctx* ctx, elm_posegraph* pg, const int32_t* a, const int32_t* b, size_t L,
                                      const elm_posegraph_cov_config* cfg, double* cov36, elm_posegraph_cov_stats* stats);

#ifdef __cplusplus
}
#endif
#endif
