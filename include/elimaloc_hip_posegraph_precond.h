/* elimaloc_hip_posegraph_precond.h -- the pose graph's choice of preconditioner.  Part of elimaloc_hip.h ("pose graph"), which includes
 * it; include that header, not this one.  The calls live here so that the list of pose-graph calls in elimaloc_hip.h itself, which is
 * pinned, stays as it is.
 *
 * The conjugate gradients of elm_posegraph_solve and elm_posegraph_optimize are preconditioned by one of two matrices M, chosen per
 * object.  The kind is not part of elm_posegraph_config (whose layout is fixed).
 *
 * BLOCK JACOBI (ELM_PG_PRECOND_BLOCK_JACOBI, the default).  M is the damped diagonal blocks H_vv + lambda diag(H_vv) alone, as
 * elimaloc_hip.h describes.
 *
 * CHAIN (ELM_PG_PRECOND_CHAIN).
 * The CHAIN EDGE of v is the lowest-index edge e with {i_e, j_e} = {v, v + 1}, in either direction, if there is one.  It counts only
 * if both nodes are active in the solve (active: not fixed and not an all-zero diagonal block, the rule of elimaloc_hip.h).  Where
 * there is none the chain breaks between v and v + 1.
 * M is block tridiagonal over the active nodes:
 *   M_vv = H_vv + lambda diag(H_vv), the same damped diagonal block as block Jacobi forms, all incident edges included;
 *   M_{i_e, j_e} = H_ij of the chain edge e, and its transpose below the diagonal;
 *   every other block is zero; inactive nodes are left out, as in H.
 * M is symmetric positive semi-definite by construction: it is the sum of the chain edges' w J^T Omega J, the other edges' diagonal
 * blocks and the damping.  It is positive definite exactly where H + lambda diag(H) restricted to a chain segment is.  A segment with
 * no edge to a fixed or otherwise anchored node and lambda = 0 may be singular: as for a component without a fixed node, that is the
 * caller's business.
 * The conjugate gradients are those of elimaloc_hip.h but for z = M^-1 r: the stop test is sqrt(r^T M^-1 r) <= pcg_rel_tol
 * sqrt(r0^T M^-1 r0) with this M, and rel_residual of the stats is in this norm.  H + lambda diag(H) - M holds only the off-diagonal
 * blocks of the L edges that are not chain edges, a matrix of rank at most 12 L, so in exact arithmetic the iteration ends within
 * 12 L + 1 iterations.  A graph without chain edges (a star) has the block-Jacobi M.
 * M^-1 r is computed on the GPU by block cyclic reduction (Gaussian elimination in odd-even order, every pivot a Schur complement of
 * M, inverted without a search over blocks): a factor once per linearization and lambda, an apply of one, three or five launches per
 * iteration for up to 256, 65 536 and 2^20 nodes.  No atomics; every sum in a fixed order that depends on the node count and the edge
 * set alone, so results are the same bytes from run to run.  A direct elimination loses digits in proportion to the condition of M:
 * the measured backward error is in DESIGN.md section 22.
 *
 * The kind applies to elm_posegraph_solve and elm_posegraph_optimize alike.  Setting it does not invalidate the linearization.  It
 * SURVIVES elm_posegraph_reset: it is a property of the object, not of the graph in it. */
#ifndef ELIMALOC_HIP_POSEGRAPH_PRECOND_H
#define ELIMALOC_HIP_POSEGRAPH_PRECOND_H
#ifdef __cplusplus
extern "C" {
#endif

#define ELM_PG_PRECOND_BLOCK_JACOBI 0 /* default */
#define ELM_PG_PRECOND_CHAIN 1
/* An unknown kind is ELM_ERR_INVALID.  Refused as every pose-graph call that takes ctx: ELM_ERR_UNSUPPORTED on a device group's lead or
 * with a communicator / hook attached, ELM_ERR_INVALID while a batch is in flight or for an object of another context. */
int elm_posegraph_set_preconditioner(elm_ctx* ctx, elm_posegraph* pg, int kind);
int elm_posegraph_get_preconditioner(elm_ctx* ctx, const elm_posegraph* pg, int* kind);

#ifdef __cplusplus
}
#endif
#endif
