/* elimaloc_hip_posegraph_init.h -- the pose graph's linear initialization: rotations first, then translations.  Part of elimaloc_hip.h
 * ("pose graph"), which includes it; include that header, not this one.  The calls live here so that the list of pose-graph calls in
 * elimaloc_hip.h itself, which is pinned, stays as it is.
 *
 * WHY.  A Gauss-Newton step from a start far outside the linear regime is not a good step however exactly it is solved: a long ring
 * whose odometry has drifted by hundreds of metres does not close under elm_posegraph_optimize alone.  The
 * remedy is an initial guess from two LINEAR least-squares problems with the graph's own sparsity, each written with 6 unknowns per
 * node so that the per-node assembly, both preconditioners and the deterministic conjugate gradients of elimaloc_hip.h solve them as
 * they are.  Everything is float64 without contraction; the conventions are those of elimaloc_hip.h: T_v = [R_v | t_v], an edge
 * (i, j, Z, Omega) with Z ~ T_i^-1 T_j, Omega in the order [translation; rotation], the retraction t <- t + R v.
 *
 * WEIGHTS.  Per edge w_r = trace(Omega_ww) / 3 (the rotation block) and w_t = trace(Omega_vv) / 3 (the translation block).  The cross
 * block and the anisotropy of Omega are ignored and Huber is not used: this is an initial guess, elm_posegraph_optimize afterwards
 * uses Omega whole.  A false loop therefore pulls the initialization as hard as a true one.
 *
 * ROTATION STAGE (ELM_PG_INIT_ROT).  The unknown of node v is y_v = [rho1_v; rho2_v], the first two ROWS of R_v as columns.  An edge
 * asks rho^k_j = R_Z^T rho^k_i (k = 1, 2), which is R_j = R_i R_Z row by row.  Its residual is
 *   e = [R_Z^T rho1_i - rho1_j; R_Z^T rho2_i - rho2_j],   A = de/dy_i = blockdiag(R_Z^T, R_Z^T),   B = de/dy_j = -I_6,
 * and its contributions, evaluated at the current rows, are
 *   H_ii = H_jj = w_r I_6,   H_ij = w_r A^T B = -w_r blockdiag(R_Z, R_Z),   g_i = w_r A^T e,   g_j = w_r B^T e = -w_r e
 * (A^T A = I_6 because R_Z is a rotation; the identity is written, not computed).  H Delta = -g is solved at lambda = 0 from Delta = 0
 * over the active nodes with the object's preconditioner, then y <- y + Delta.  Fixed nodes keep their rows, and their rows stand in
 * the gradients of their neighbours.  The problem is quadratic, so this one step is its minimum from any start: the result does not
 * depend on the free nodes' starting poses.
 * Two rows and not three: two rows are exactly six unknowns, so the 6 x 6 blocks of the solver serve them in ONE solve, and the third
 * row of a rotation is the cross product of the other two.  A second solve for the third row would add a third of the information to
 * a guess that elm_posegraph_optimize refines anyway.
 *
 * PROJECTION, in closed form (no SVD).  u = rho1 / |rho1|, v = rho2 / |rho2|, s = (u + v) / |u + v|, d = (u - v) / |u - v|; then
 *   r1 = (s + d) / sqrt(2),   r2 = (s - d) / sqrt(2),   r3 = r1 x r2
 * are the rows of the node's new rotation.  s and d are orthogonal whenever u and v are unit vectors, so r1 and r2 are orthonormal:
 * this is the symmetric orthogonalization of the two rows, neither is preferred.  A node is DEGENERATE if any of |rho1|, |rho2|,
 * |u + v|, |u - v| is below 1e-6 (the rows of a rotation have length 1 and are orthogonal; values that small mean that the incident
 * edges contradict one another).  A degenerate node keeps its rotation and is counted in degenerate_nodes.  Only active nodes are
 * projected; every other node keeps its pose bit for bit.  rows_out receives y before the projection (the current rows for nodes the
 * solve does not move).
 *
 * TRANSLATION STAGE (ELM_PG_INIT_TRANS).  At the rotations just projected, or at the current ones if the rotation stage was not
 * requested, the unknown of node v is [v_v; 0_3] with the retraction t_v <- t_v + R_v v_v.  The residual and the top-left 3 x 3 of the
 * Jacobians are those of elimaloc_hip.h with the rotation columns dropped:
 *   e = R_Z^T (R_i^T (t_j - t_i) - t_Z),   A_v = -R_Z^T,   B_v = R_Z^T R_i^T R_j,   weight w_t.
 * With rotations held e is exactly linear in v.  The contributions are H_ii = H_jj = w_t I_6 (A_v^T A_v = B_v^T B_v = I_3; the lower
 * three unknowns are padding with the diagonal w_t I_3 per side, zero coupling and zero gradient, so their solution is exactly 0),
 * H_ij = w_t A_v^T B_v in the top-left block and g_i = w_t A_v^T e, g_j = w_t B_v^T e in the top three entries.  Because the weight
 * is isotropic R_Z R_Z^T = I drops out of every product; with u = R_i^T (t_j - t_i) - t_Z the library evaluates the same terms as
 *   H_ij = -w_t R_i^T R_j,   g_i = -w_t u,   g_j = w_t (R_i^T R_j)^T u.
 * Solved at lambda = 0 from 0, then t <- t + R v.  v_out receives v.
 *
 * Both solves are the conjugate gradients of elimaloc_hip.h (and of elimaloc_hip_posegraph_precond.h for the chain kind), the sums in
 * the same fixed orders: two calls from the same state give the same bytes.
 *
 * PRECONDITIONS, all checked on the host before anything is launched; each is ELM_ERR_INVALID (the last five with a text in
 * elm_last_error) and leaves the graph untouched:
 *   a NULL ctx, graph, config or result; stages outside 1 .. 3; pcg_rel_tol not finite and > 0; pcg_max_iterations or
 *   pcg_check_every < 1; no node in the graph; an edge with w_r <= 0 (rotation stage) or w_t <= 0 (translation stage); a connected
 *   component of nodes that has edges but contains no fixed node.
 * At lambda = 0 such a component is singular and the chain factor would invert a zero pivot.  That is also why the call has no damping
 * parameter: lambda diag(H) on a 65 536-node chain biases the solution by roughly lambda N^2.  A node without edges is inactive and
 * keeps its pose, as in every solve.
 *
 * ATOMICITY.  The stages work on the object's trial poses.  The poses are replaced (by the pointer exchange of
 * elm_posegraph_optimize) only if EVERY requested stage met its tolerance; `applied` says so.  Otherwise the call returns ELM_OK with
 * the poses unchanged byte for byte and a linearization that was valid still valid, and the result, rows_out and v_out are filled all
 * the same.  An applied call invalidates the linearization, as elm_posegraph_set_poses does.  cost_before and cost_after are the full
 * SE(3) cost sum r^T Omega r (Huber off) at the poses before and at the trial poses, applied or not. */
#ifndef ELIMALOC_HIP_POSEGRAPH_INIT_H
#define ELIMALOC_HIP_POSEGRAPH_INIT_H
#ifdef __cplusplus
extern "C" {
#endif

#define ELM_PG_INIT_ROT 1
#define ELM_PG_INIT_TRANS 2
typedef struct elm_posegraph_init_config {
    double pcg_rel_tol;         /* > 0: both solves stop at sqrt(r^T M^-1 r) <= pcg_rel_tol sqrt(r0^T M^-1 r0) */
    int32_t pcg_max_iterations; /* >= 1, per stage */
    int32_t pcg_check_every;    /* >= 1 */
    int32_t stages;             /* ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS */
    int32_t reserved;
} elm_posegraph_init_config;
typedef struct elm_posegraph_init_result {
    double cost_before, cost_after;
    double rot_rel_residual, trans_rel_residual; /* of the recurrence, as elm_posegraph_solve_stats; 0 for a stage not requested */
    int32_t rot_iterations, trans_iterations;
    int32_t rot_converged, trans_converged;      /* 0 for a stage not requested */
    int32_t degenerate_nodes;
    int32_t applied;
} elm_posegraph_init_result;
/* pcg_rel_tol 1e-8, at most 50 000 iterations per stage checked every 32, stages = ELM_PG_INIT_ROT | ELM_PG_INIT_TRANS */
void elm_posegraph_init_config_default(elm_posegraph_init_config* c);
/* rows_out [N][6] and v_out [N][3], each when not NULL.  Refused as every pose-graph call that takes ctx: ELM_ERR_UNSUPPORTED on a
 * device group's lead or with a communicator / hook attached, ELM_ERR_INVALID while a batch is in flight or for an object of another
 * context. */
int elm_posegraph_initialize(elm_ctx* ctx, elm_posegraph* pg, const elm_posegraph_init_config* cfg, elm_posegraph_init_result* result,
                             double* rows_out, double* v_out);

#ifdef __cplusplus
}
#endif
#endif
