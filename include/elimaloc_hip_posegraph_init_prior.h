/* elimaloc_hip_posegraph_init_prior.h -- the pose graph's linear initialization with the priors in it.  Part of elimaloc_hip.h ("pose
 * graph"), which includes it; include that header, not this one.
 *
 * WHY.  elm_posegraph_initialize (elimaloc_hip_posegraph_init.h) brings a start hundreds of metres off into Gauss-Newton's reach, but it
 * refuses every connected component without a fixed node and it ignores priors.  Priors (elimaloc_hip_posegraph_prior.h) make a graph
 * without a fixed node legal: a trajectory held by GNSS positions or map matches alone.  That graph had no linear initialization, and
 * elm_posegraph_optimize alone leaves a long ring with a position on every 8th node metres off.  This call is the
 * initialization of such a graph.  elm_posegraph_initialize itself is unchanged.
 *
 * Conventions, edge weights, the two linear problems, the projection and the degenerate rule are those of elimaloc_hip_posegraph_init.h;
 * a prior q = (v, Z, l, Omega) is that of elimaloc_hip_posegraph_prior.h.  Float64 without contraction, no Huber.
 *
 * WEIGHTS PER PRIOR.  w_r^q = trace(Omega_ww) / 3 and w_t^q = trace(Omega_vv) / 3.  Both may be 0 (a position prior has w_r^q = 0); a
 * prior whose weight in a stage is 0 does not enter that stage.
 * ROTATION STAGE TERM.  The prior asks R_v = R_Z: e_q = y_v - [rho1_Z; rho2_Z], H_q = w_r^q I_6, g_q = w_r^q e_q.
 * TRANSLATION STAGE TERM, at the stage's rotations: u_q = (t_v - t_Z) + R_v l, H_q = w_t^q I_6 (the upper block is J^T J = I_3, the
 * lower block the padding diagonal, so a node that has only priors is non-singular), g_q = [w_t^q R_v^T u_q; 0_3].  The padding
 * solution stays exactly 0.
 * ORDER OF THE SUMS.  A node's sums take its edges first in ascending edge index, then its priors in ascending prior index, one addition
 * each (the order of elimaloc_hip_posegraph_prior.h).
 *
 * COMPONENTS, from a union-find over the edges, classed on the host:
 *   fixed           it has a fixed node.  Every prior enters with its weights.
 *   prior-anchored  no fixed node, some prior with w_r^q > 0.  With ELM_PG_INIT_TRANS requested it also needs a prior with w_t^q > 0,
 *                   else the call is refused.
 *   aligned         no fixed node, no w_r^q > 0, some w_t^q > 0.  With stages == ROT | TRANS it takes the aligned path below; with TRANS
 *                   alone its priors anchor the translations directly and nothing is aligned; with ROT alone the call is refused.
 * A component with edges, no fixed node and no prior of positive weight is refused.  A component without edges (a single node) is never
 * aligned and never refused: the active rule (max |H_vv| > 0, not fixed) decides per stage whether it moves.  A prior on a fixed node
 * enters the costs only.
 *
 * SEQUENCE.
 *   S1, rotations: edge terms plus prior terms.  The smallest-index node of every aligned component is its GAUGE NODE, held as if fixed
 *       during S1 and S2 only.  One solve at lambda = 0, the projection and the degenerate rule.  rows_out as elm_posegraph_initialize.
 *   S2, translations at the projected rotations: the gauge nodes still held, the priors of aligned components masked out (weight 0), all
 *       other priors in.  t <- t + R v.  With an aligned component v_pre_out receives v (else zeros).
 *   ALIGNMENT, per aligned component over its priors with w = w_t^q > 0 in ascending prior index: the points a_q = t_v + R_v l_q at
 *       the S2 poses and b_q = t_Z; W = sum w, c_a = sum w a / W, c_b = sum w b / W; in a second pass S = sum w (b - c_b)(a - c_a)^T;
 *       S = U Sigma V^T; G = U diag(1, 1, det(U V^T)) V^T.  Every node of the component gets R_v <- G R_v, t_v <- c_b + G (t_v - c_a).
 *       The component is RANK-DEFICIENT if sigma_2 <= align_min_ratio sigma_1: fewer than three points, or collinear points (coplanar
 *       points are fine).  S is a second moment, so the default 1e-4 asks for a lateral spread of about 1 % of the length; it is a
 *       condition chosen here, not a measurement.  A rank-deficient component is still moved in the trial poses, and the call is then not
 *       applied.
 *       align_out row, 28 doubles, components in ascending order of their smallest node: c_a[3], c_b[3], S[9] row-major, W, G[9]
 *       row-major, sigma[3] descending.  At most align_capacity rows are written.
 *   S3, translations again, only if some component was aligned: the gauge nodes released, every prior in.  v_out and trans_* are this
 *       solve's; pre_* are S2's.  Without an aligned component S2 is the translation solve: it fills v_out and trans_*, pre_* are 0.
 *
 * PRECONDITIONS, checked on the host before any launch, each ELM_ERR_INVALID (the ones that read the graph with a text in
 * elm_last_error) and the object untouched: those of elm_posegraph_initialize on ctx, graph, config (`base`), result, node count and
 * edge weights; align_min_ratio not finite or <= 0; align_capacity < 0; a component refused above.
 *
 * ATOMICITY is elm_posegraph_initialize's: the poses are exchanged only if every solve that ran converged AND no component is
 * rank-deficient (`base.applied`); otherwise they are unchanged in bytes and a linearization that was valid is queued again.  On every
 * exit path, errors included, the fixed flags on host and device, the priors and the priors' Huber threshold are as before.
 * cost_before / cost_after are edges + priors with both Huber thresholds off.
 * NO PRIOR.  With no prior in the object `base`, rows_out, v_out and the poses are byte for byte those of elm_posegraph_initialize. */
#ifndef ELIMALOC_HIP_POSEGRAPH_INIT_PRIOR_H
#define ELIMALOC_HIP_POSEGRAPH_INIT_PRIOR_H
#ifdef __cplusplus
extern "C" {
#endif

#define ELM_PG_INIT_ALIGN_ROW 28

typedef struct elm_posegraph_init_prior_config {
    elm_posegraph_init_config base; /* as elm_posegraph_initialize */
    double align_min_ratio;         /* > 0, finite; default 1e-4 */
} elm_posegraph_init_prior_config;
typedef struct elm_posegraph_init_prior_result {
    elm_posegraph_init_result base; /* rot_*: the rotation solve; trans_*: the LAST translation solve (all priors in);
                                       cost_before / cost_after: edges + priors, both Huber thresholds off */
    double pre_rel_residual;        /* the gauge-fixed translation solve S2; 0 when no component is aligned */
    int32_t pre_iterations, pre_converged;
    int32_t aligned_components, rank_deficient_components;
    double min_align_ratio;         /* smallest sigma_2 / sigma_1 over aligned components (0 for sigma_1 == 0); 0 when none */
} elm_posegraph_init_prior_result;
/* base: elm_posegraph_init_config_default; align_min_ratio 1e-4 */
void elm_posegraph_init_prior_config_default(elm_posegraph_init_prior_config* c);
/* rows_out [N][6], v_pre_out [N][3], v_out [N][3], align_out [align_capacity][28], each when not NULL.  Refused as every pose-graph call
 * that takes ctx. */
int elm_posegraph_initialize_priors(elm_ctx* ctx, elm_posegraph* pg, const elm_posegraph_init_prior_config* cfg,
                                    elm_posegraph_init_prior_result* result, double* rows_out, double* v_pre_out, double* v_out,
                                    double* align_out, int align_capacity);

#ifdef __cplusplus
}
#endif
#endif
