/* elimaloc_hip_loops.h -- loop closing: the largest set of mutually consistent loop measurements, found before the solver sees any of
 * them (pairwise consistent measurement set maximization; Mangelson et al., ICRA 2018).  Part of elimaloc_hip.h, which includes it;
 * include that header, not this one.  The calls live here so that the pinned declaration lists of elimaloc_hip.h and of the two
 * pose-graph headers stay as they are.
 *
 * WHY.  A false loop that passed its registration (two similar corridors) is used by elm_posegraph_optimize like a true one: Huber
 * bounds its pull and does not remove it, and elm_posegraph_initialize does not even bound it (DESIGN.md sections 22 and 23).  Two
 * loop measurements and the odometry between their ends form a cycle that must compose to the identity; every pair of loops is tested
 * against that, and the largest set whose members all agree with one another is kept.  Nothing of the solver is touched.
 *
 * INPUTS.  n poses T_v, column-major 4 x 4 as every pose-graph call takes them: a chain in index order, the odometry estimate.  L
 * loops (a_k, b_k, Z_k) with Z_k ~ T_a^-1 T_b, and per loop two variances var_t[k] > 0 (m^2) and var_r[k] > 0 (rad^2).
 *
 * PAIR TERM.  For k < l, with X_uv = T_u^-1 T_v = [R_u^T R_v | R_u^T (t_v - t_u)], loop k is predicted from loop l through the odometry:
 *   Zhat = (X_{a_k a_l} Z_l) X_{b_l b_k}      (a product A B is [R_A R_B | R_A t_B + t_A])
 *   e    = the pose graph's residual of the edge (I, Zhat, Z_k) = [R_Z^T (t_Zhat - t_Z); Log(R_Z^T R_Zhat)], Z = Z_k, with the Log of
 *          elimaloc_hip.h ("pose graph"), by the same code
 *   m    = |a_k - a_l| + |b_k - b_l|          (the odometry steps the cycle runs over)
 *   s_kl = ((e0^2 + e1^2) + e2^2) / ((var_t[k] + var_t[l]) + q_t m) + ((e3^2 + e4^2) + e5^2) / ((var_r[k] + var_r[l]) + q_r m)
 * Everything is float64 without contraction, in exactly that order; every sum of three products is the first two, then the third.
 *
 * ADJACENCY.  adj[k][l] = adj[l][k] = (s_kl <= gamma), always evaluated with the lower index as k, so the matrix is symmetric by
 * construction.  A non-finite s is not adjacent.  The diagonal is 0.
 *
 * MODEL LIMITS.  The model is deliberately scalar: a random walk in the NUMBER of odometry steps with one translation and one rotation
 * variance per step, not a 6 x 6 covariance propagated along the chain.  In particular rotation drift times lever arm (a heading
 * error of the chain moves the far end sideways) is not modelled: the caller folds it into q_t.
 *
 * CLIQUE.  A deterministic greedy clique over adj: cand = all loops; while cand is not empty, pick the candidate with the most
 * neighbours inside cand (ties go to the lowest index), make it a member, cand <- cand & adj[v].  The result is a clique and it is
 * maximal by construction; it is a HEURISTIC for the maximum clique, not the maximum clique.  `steps` counts the picks.
 *
 * LIMITS AND PRECONDITIONS, all checked on the host before anything is launched; each is ELM_ERR_INVALID (with a text in
 * elm_last_error) and leaves the outputs untouched: a NULL ctx, poses, config, result, member_out or degree_out, or with L > 0 a NULL
 * a, b, Z, var_t or var_r; n outside 1 .. 2^20; L above ELM_LOOPS_MAX; s_out with L above ELM_LOOPS_MAX_S; an index outside
 * 0 .. n - 1; a == b; a non-finite pose, Z or variance; a variance <= 0; a negative or non-finite q; a gamma that is not finite and
 * > 0; steps_per_batch < 1.  L = 0 is ELM_OK with size 0 and launches nothing.  Refused as every pose-graph call that takes ctx:
 * ELM_ERR_UNSUPPORTED on a device group's lead or with a communicator / hook attached, ELM_ERR_INVALID while a batch is in flight.
 * The call keeps nothing on the device between calls.  Everything after the pair terms is integer work in fixed orders: two calls
 * with the same inputs give the same bytes. */
#ifndef ELIMALOC_HIP_LOOPS_H
#define ELIMALOC_HIP_LOOPS_H
#ifdef __cplusplus
extern "C" {
#endif

#define ELM_LOOPS_MAX 16384
#define ELM_LOOPS_MAX_S 2048
typedef struct elm_loops_config {
    double q_t, q_r;         /* >= 0: the odometry's translation (m^2) and rotation (rad^2) variance per chain step */
    double gamma;            /* > 0: a pair is consistent when s <= gamma */
    int32_t steps_per_batch; /* >= 1: greedy steps queued between two reads of the device's state */
    int32_t reserved;
} elm_loops_config;
typedef struct elm_loops_result {
    int32_t size;                     /* members of the clique */
    int32_t steps;                    /* greedy picks */
    int64_t adjacent_pairs;           /* pairs k < l with adj[k][l] */
    double adjacency_ms, greedy_ms;   /* device time of the pair kernel and of the greedy loop (stream events; not part of the result's bytes contract) */
} elm_loops_result;
/* q_t = q_r = 0, gamma = 16.81 (the 99 % point of chi^2 with 6 degrees of freedom), steps_per_batch = 32 */
void elm_loops_config_default(elm_loops_config* c);
/* Host only: e_out[6] of one pair, by the code the kernel runs.  Ta, Tb, Zk: the poses of loop k's ends and its measurement; Tc, Td,
 * Zl: those of loop l (all column-major 4 x 4).  ELM_ERR_INVALID for a NULL or non-finite argument. */
int elm_loops_pair_terms(const double* Ta, const double* Tb, const double* Zk, const double* Tc, const double* Td, const double* Zl, double* e_out);
/* poses16 [n][16], a, b [L], Z16 [L][16], var_t, var_r [L]; member_out [L] (1: in the clique), degree_out [L] (the neighbours of each
 * loop in adj).  Optional, each when not NULL: adj_out [L][(L + 63) / 64], bit l & 63 of word l >> 6 of row k is adj[k][l] and the
 * padding bits are zero; s_out [L][L], symmetric with a zero diagonal (L <= ELM_LOOPS_MAX_S). */
int elm_loops_consistency(elm_ctx* ctx, const double* poses16, size_t n, const int32_t* a, const int32_t* b, const double* Z16, const double* var_t,
                          const double* var_r, size_t L, const elm_loops_config* cfg, elm_loops_result* result, uint8_t* member_out,
                          int32_t* degree_out, uint64_t* adj_out, double* s_out);

#ifdef __cplusplus
}
#endif
#endif
