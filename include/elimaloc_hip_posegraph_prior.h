/* elimaloc_hip_posegraph_prior.h -- the pose graph's absolute factors: a measured pose, or a measured position, of ONE node in the world
 * frame (GNSS, a match against an existing map).  Part of elimaloc_hip.h, which includes it; include that header, not this one.
 *
 * WHY.  Every edge of the pose graph is a relative pose between two nodes, and the only tie to the world is a node's `fixed` flag: an
 * infinite information on a whole pose.  A GNSS fix (a full pose, or a position only, at the antenna) and a registration against a
 * georeferenced map could not enter the graph.  A prior is that measurement: it anchors a trajectory that never revisits a place,
 * georeferences a map built from a log, and stitches a new session onto an existing map.
 *
 * WHAT.  A PRIOR q is (v, Z, l, Omega):
 *   v      the node
 *   Z      [R_Z | t_Z], world <- measured frame, column-major 4 x 4, finite
 *   l      the lever arm: the measured point in the node's frame (the antenna), finite
 *   Omega  6 x 6, row-major, in the order [translation; rotation], finite and exactly symmetric.  It may be singular: a position
 *          measurement is R_Z = I with the rotation rows and columns of Omega zero.
 * v past the node count, a non-finite entry or an Omega that is not exactly symmetric is ELM_ERR_INVALID.  Several priors on one node,
 * and a prior on a fixed node, are legal.
 * RESIDUAL.  R_E = R_Z^T R_v, r = [R_Z^T (t_v + R_v l - t_Z); Log(R_E)], Log the pose graph's (elimaloc_hip.h, "pose graph").
 * JACOBIAN with respect to x_v = [v; w] under the pose graph's retraction, rows in the order of r:
 *   J = [ R_E   -R_E [l]x ;  0   J^-1(phi) ],   J^-1 and c(theta) exactly as for an edge.
 * With l = 0, r and J are, as numbers, the r and B of elm_posegraph_edge_terms(I, T_v, Z).
 * ROBUST WEIGHT.  Huber on s_q = r^T Omega r as for an edge, with a threshold of the object's own, prior_huber_k (a GNSS outlier and a
 * loop outlier do not live on one scale): elm_posegraph_set_prior_huber; 0, the default, is off; it is kept across elm_posegraph_reset,
 * as the preconditioner kind is.  s_q == k^2 is an inlier.
 * NORMAL EQUATIONS.  H_vv += w_q J^T Omega J, g_v += w_q J^T Omega r; no off-diagonal block.  In a node's sums all its edges come first,
 * in ascending edge index as ever, then its priors in ascending prior index, one addition per prior.  The active rule is unchanged -- not
 * fixed, and the block not all zero -- so a free node that has only priors is now active.  A prior on a fixed node counts in the cost
 * and the stats and not in the solve.  A free node whose rotation only position priors could determine is the caller's business, as a
 * component without a fixed node is.
 * COST AND STATS.  F = (sum rho_e) + (sum rho_q): the edges' total formed exactly as without priors, the priors' total by a fixed tree of
 * its own, then one addition; chi2 likewise; n_outliers counts edges and priors.  grad and diag of
 * elm_posegraph_download_linearization include the priors ("as summed").
 * GAUGE.  elm_posegraph_optimize, and elm_posegraph_covariance / elm_posegraph_relative_covariance at lambda == 0, refuse with "no fixed
 * node (the gauge is free)" only when the graph has no fixed node AND no prior.
 * INITIALIZATION.  elm_posegraph_initialize ignores priors: its conditions, its two linear problems, its costs and its results are what
 * they are without them.
 * NO PRIOR.  With no prior in the object every result of every pose-graph call is byte for byte what it was before priors existed: the
 * added launches are skipped, not run on empty input, and elm_posegraph_create allocates nothing more.
 *
 * HOW.  DESIGN.md section 27: a lane group of 8 per prior linearizes it (the lane is the column), one wavefront per node that has priors
 * adds them onto the node's sums of the edges, and a cost kernel with partial slots of its own adds the priors' totals to the record.
 * Float64 without contraction, no atomics: the bytes of every result depend on the graph and the priors alone. */
#ifndef ELIMALOC_HIP_POSEGRAPH_PRIOR_H
#define ELIMALOC_HIP_POSEGRAPH_PRIOR_H
#ifdef __cplusplus
extern "C" {
#endif

#define ELM_POSEGRAPH_MAX_PRIORS (1 << 22)

/* Room for `capacity` priors (1 .. ELM_POSEGRAPH_MAX_PRIORS), fixed for the object's life: a second device allocation, made here.  Once
 * per object: a second call is ELM_ERR_INVALID.  ELM_ERR_UNSUPPORTED on a device group's lead or with a communicator / hook attached,
 * here and in every call below that takes ctx. */
int elm_posegraph_reserve_priors(elm_ctx* ctx, elm_posegraph* pg, int capacity);
/* n priors appended: node[n], Z16[n][16] column-major, lever3[n][3] (NULL: all zero), info36[n][36] row-major.  A call that would
 * overfill, or a call without a reserve, is ELM_ERR_UNSUPPORTED and changes nothing.  Invalidates the linearization, as adding edges
 * does. */
int elm_posegraph_add_priors(elm_ctx* ctx, elm_posegraph* pg, const int32_t* node, const double* Z16, const double* lever3, const double* info36,
                             size_t n);
int elm_posegraph_prior_count(elm_ctx* ctx, const elm_posegraph* pg, size_t* n_priors);
/* Priors first .. first + count - 1 as they were added, each output when not NULL: node[count], Z16[count][16], lever3[count][3],
 * info36[count][36].  ELM_ERR_INVALID beyond the count. */
int elm_posegraph_get_priors(elm_ctx* ctx, const elm_posegraph* pg, size_t first, size_t count, int32_t* node, double* Z16, double* lever3,
                             double* info36);
/* No priors; the capacity and prior_huber_k stay.  (elm_posegraph_reset does the same to the priors.)  Invalidates the linearization. */
int elm_posegraph_clear_priors(elm_ctx* ctx, elm_posegraph* pg);
/* The priors' Huber threshold, finite and >= 0; 0: off.  Setting it invalidates the linearization. */
int elm_posegraph_set_prior_huber(elm_ctx* ctx, elm_posegraph* pg, double k);
int elm_posegraph_get_prior_huber(elm_ctx* ctx, const elm_posegraph* pg, double* k);
/* The priors' part of the current linearization, each output when not NULL: r[P][6], J[P][36] row-major, s[P], w[P].  ELM_ERR_INVALID
 * without a valid linearization. */
int elm_posegraph_download_prior_linearization(elm_ctx* ctx, const elm_posegraph* pg, double* r, double* J, double* s, double* w);
/* The residual and Jacobian of one prior, each output when not NULL: r[6], J[36] row-major; lever3 NULL: zero.  Host only: the same code
 * the kernel runs, compiled for the host. */
int elm_posegraph_prior_terms(const double T16[16], const double Z16[16], const double* lever3, double* r, double* J);

#ifdef __cplusplus
}
#endif
#endif
