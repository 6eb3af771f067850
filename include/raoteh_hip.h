/*
 * raoteh_hip.h -- C ABI of libraoteh_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary for the tree-CTMC likelihood hot path of
 * argriffing/raoteh.  Plain pointers and sizes only; the caller owns every
 * host buffer; the library never keeps a host pointer after a call returns;
 * device memory is owned by the opaque handles.  No exception crosses the
 * ABI: every function returns 0 (RT_OK) or a negative RT_ERR_* code and
 * rt_last_error() returns a human-readable message for the calling thread.
 *
 * Ownership and destruction order.  A site batch (rt_sites) refers to its model, a model and
 * a chain batch (rt_chains) refer to their context, until they are destroyed.  Children go
 * first: rt_model_destroy returns RT_ERR_INVALID (and destroys nothing) while a batch created
 * from the model is alive, rt_ctx_destroy while a model or a chain batch of the context is
 * alive; rt_last_error() names what is left.  Destroying NULL is a no-op.  Using a handle
 * after its destroy call returned RT_OK is undefined.
 *
 * "Reference" citations are file:line under the reference repository root
 * (argriffing/raoteh).  The reference's only native boundary on this path is
 * the third-party Cython module `pyfelscore` (absent from the reference
 * tree, version unpinned, README.md:8-9); section 1 below replaces exactly
 * the pyfelscore entry points the path calls plus the scipy expm call.
 * Section 2 is the batched, device-resident form of the same path.
 *
 * All floating point data is IEEE binary64; all index data int64 (as the
 * reference passes, _density.py:138-139, _mcy_dense.py:49); row-major,
 * C-contiguous.
 */
#ifndef RAOTEH_HIP_H
#define RAOTEH_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define RT_OK                0
#define RT_ERR_INVALID      -1   /* bad argument (shape, null, range)        */
#define RT_ERR_HIP          -2   /* a HIP runtime call failed                */
#define RT_ERR_UNSUPPORTED  -3   /* valid input outside implemented limits   */
#define RT_ERR_NOMEM        -4   /* host or device allocation failed         */
#define RT_ERR_RCCL         -5   /* RCCL missing or a collective failed      */
#define RT_ERR_SINGULAR     -6   /* expm: non-finite Q t / singular Pade den. */
#define RT_ERR_ZERO_PROB    -7   /* a chain's observations have likelihood 0 */

#define RT_MAX_STATES      128   /* pruning kernels and the reference-format passes
                                    (pset / set / pmap / distn / joint): n <= 128 --
                                    examples/p53/liwen.py:599-621 runs _mcy_dense on
                                    2 x 61 = 122 compound states                */
#define RT_MAX_EXPECT_STATES 64  /* reference-shaped expectation passes on host
                                    arrays (rt_mjp_*_expectation_*), spectral
                                    reconstruction: n <= 64 (the Rao-Teh forest
                                    passes and chains of sections 4 and 5 take
                                    n <= 128)                                    */
#define RT_MAX_EXPECT_STEP_STATES 128 /* rt_expect_step on a resident batch and
                                    rt_mjp_frechet_statistics: n <= 128 (above 64 the
                                    Frechet derivative is carried as a pair (X, L)
                                    through the scaling and squaring, no order-2n
                                    block)                                       */
#define RT_MAX_EXPM_STATES 128   /* expm: n <= 64 LDS-resident, <= 128 through
                                    L2-resident scratch (the Frechet blocks of the
                                    61-state codon model have order 122)        */

/* per-site status written by rt_prune (reference: StructuralZeroProb raised
 * by _mc0_dense.py:190-203 when the root likelihood is zero)                */
#define RT_SITE_OK           0
#define RT_SITE_ZERO_PROB    1
#define RT_SITE_NEGATIVE     4   /* bit: a negative root pmap entry was
                                    clamped (reference warns + clamps,
                                    _mc0_dense.py:184-189)                   */

/* observation encodings for rt_sites_create                                 */
#define RT_OBS_DENSE         0   /* f64 [nsites][nobs][n] likelihood vectors
                                    (type z, _mcz.py:159-160; 0/1 masks and
                                    one-hot vectors are special cases)       */
#define RT_OBS_STATE         1   /* uint8 [nsites][nobs] observed state,
                                    255 = unobserved (type x, _mcx.py:12-23) */
#define RT_OBS_MASK          2   /* uint64 [nsites][nobs][ceil(n/64)]: bit s % 64
                                    of word s / 64 = state s allowed (type y,
                                    _mcy.py:12-16); one word per node for n <= 64 */

/* kernel ids for rt_ctx_kernel_time                                         */
#define RT_K_EXPM            0
#define RT_K_PRUNE           1
#define RT_K_REDUCE          2
#define RT_K_COMBINE         3   /* second kernel of a root-halves pruning launch */
#define RT_K_COUNT           4

typedef struct rt_ctx   rt_ctx;     /* one per GPU / process                 */
typedef struct rt_model rt_model;   /* tree + transition matrices on device  */
typedef struct rt_sites rt_sites;   /* one resident batch of site data       */

/* ---- 0. library / context ------------------------------------------------ */

int         rt_version(void);                 /* 100*major + minor            */
const char *rt_last_error(void);              /* thread-local, never NULL     */
int         rt_device_count(int *count);
int         rt_ctx_create(int device, rt_ctx **ctx);
int         rt_ctx_destroy(rt_ctx *ctx);
int         rt_ctx_sync(rt_ctx *ctx);         /* wait for the ctx stream      */
/* Optional per-kernel HIP-event timing (events are recorded on the stream
 * the kernels are launched on).  rt_ctx_kernel_time drains finished events
 * and returns the accumulated device time and launch count since the last
 * reset; `name` receives a static string with the kernel variant used.      */
int         rt_ctx_set_timing(rt_ctx *ctx, int enabled); /* N > 1: every N-th launch */
int         rt_ctx_reset_timing(rt_ctx *ctx);
int         rt_ctx_kernel_time(rt_ctx *ctx, int kernel, double *total_ms,
                               int64_t *launches, const char **name);

/* ---- 1. reference-shaped entry points (host pointers in and out) --------- */

/* P[b] = expm(Q[q_index[b]] * t[b]) for b in [0,count).  Replaces
 * scipy.linalg.expm(Q * weight) at _mjp_dense.py:24-25 (called once per edge
 * at _mjp_dense.py:352-358) and pyfelscore.get_tolerance_rate_matrix(t,Q,P)
 * (_tmjp_dense.py:239, tests/test_expm.py:38).  q_index may be NULL
 * (then matrix b uses Q[b] if nq == count, or Q[0] if nq == 1).
 * info (optional, int32[count][2]) receives the Pade degree and the number
 * of squarings used.  n <= RT_MAX_EXPM_STATES.                              */
int rt_expm(rt_ctx *ctx, int64_t n, int64_t count,
            const double *Q, int64_t nq, const int64_t *q_index,
            const double *t, double *P, int32_t *info);
/* getp_spectral_v2 (examples/p53/qtop.py:76-88) at `count` branch lengths in one launch:
 * P[b] = A diag(exp(lam t[b])) B, diagonal 1 where D == 0 (D may be NULL).  n <= 64.    */
int rt_expm_spectral(rt_ctx *ctx, int64_t n, int64_t count, const double *A,
            const double *lam, const double *B, const double *D, const double *t, double *P);

/* pyfelscore.get_lb_transition_matrix(t, Q, P) (examples/p53/liwen.py:45; pure-Python twin
 * getp_lb, liwen.py:47-82) at `count` interval lengths in one launch: the lower bound of
 * expm(Q t) that keeps the histories with no change (diagonal: exp(t Q[a][a])) or exactly one
 * change a -> b (rab (exp(-ra t) - exp(-rb t)) / (rb - ra), or rab t exp(-rb t) when ra == rb;
 * ra = -Q[a][a]).  Q f64[n][n] with diagonal = minus the row sum, t f64[count],
 * P f64[count][n][n] out.  Any n.                                                       */
int rt_lb_transition_matrix(rt_ctx *ctx, int64_t n, int64_t count, const double *Q,
            const double *t, double *P);
/* pyfelscore.tmjp_get_inhomogeneous_mjp (_tmjp_dense.py:1039-1054; sparse twin
 * _tmjp.get_inhomogeneous_mjp, _tmjp.py:863-900), same argument order: the tree CSR, the
 * primary state of the edge above every node (int64[nnodes], entry 0 ignored),
 * primary_to_part int64[nprimary], Q_primary f64[nprimary][nprimary], the two tolerance
 * rates and the class under consideration; node_to_allowed_tolerances int64[nnodes][2]
 * (ones on entry; column 0 cleared where the class of an adjacent edge's state is the class
 * under consideration) and tol_rate_matrices f64[nnodes][3][3] (keyed by the child index,
 * diagonal = minus the row sum; the root's slot zero) are filled.  Host only: no context. */
int rt_tmjp_get_inhomogeneous_mjp(int64_t nnodes, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const int64_t *edge_to_primary_state,
            int64_t nprimary, const int64_t *primary_to_part, const double *Q_primary,
            double rate_on, double rate_off, int64_t tolerance_class,
            int64_t *node_to_allowed_tolerances, double *tol_rate_matrices);

/* The three pyfelscore passes of _mcy_dense.py:261-291, batched over
 * `nsites` independent sites that share the tree and the transitions:
 *   tree_csr_indices int64[nnodes-1], tree_csr_indptr int64[nnodes+1]:
 *       children CSR in DFS-preorder index space (_density.py:104-140)
 *   esd_transitions  f64[nnodes][n][n], slot = CHILD preorder index, root
 *       slot ignored (_density.py:143-180)
 *   state_mask       int64[nsites][nnodes][n], 0/1
 *   subtree_probability f64[nsites][nnodes][n], every entry written.
 * nsites == 1 is the exact single-call shape of the reference.              */

/* pyfelscore.mcy_esd_get_node_to_pset (call sites _mcy_dense.py:168,270,
 * _mcx_dense.py:145, _mcy.py:219,309,508): backward boolean pass, in place. */
int rt_mcy_esd_get_node_to_pset(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            int64_t *state_mask);

/* pyfelscore.esd_get_node_to_set (_mcy_dense.py:175,277, _mcx_dense.py:152,
 * _mcy.py:226,515): forward boolean pass, in place.                         */
int rt_esd_get_node_to_set(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            int64_t *state_mask);

/* pyfelscore.mcy_esd_get_node_to_pmap (_mcy_dense.py:184,286,
 * _mcx_dense.py:161, _mcy.py:533): Felsenstein upward pass
 *   L[v,s] = mask[v,s] * obs_lik[v,s] * prod_c sum_s' P_c[s,s'] L[c,s'].
 * obs_likelihood (optional, f64[nsites][nnodes][n]) is the type-z factor of
 * _mcz.py:159-160; pass NULL for the plain type-x/y pass.                   */
int rt_mcy_esd_get_node_to_pmap(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            const int64_t *state_mask, const double *obs_likelihood,
            double *subtree_probability);
/* The three passes above in one call (the sequence _mcy_dense.py:261-291 runs:
 * pset, set, pmap; with obs_likelihood the type-z upward pass, _mcz.py:128-163):
 * state_mask is updated in place by the two boolean passes, subtree_probability
 * is filled; one upload of the tree and the matrices instead of three.        */
int rt_mcy_esd_passes(rt_ctx *ctx, int64_t nnodes, int64_t n, int64_t nsites,
            const int64_t *tree_csr_indices, const int64_t *tree_csr_indptr,
            const double *esd_transitions, int64_t *state_mask,
            const double *obs_likelihood, double *subtree_probability);

/* pyfelscore.mc0_esd_get_node_to_distn (_mc0_dense.py:381, _mcy_dense.py:195;
 * pure-Python twin _mc0_dense.py:446-486): downward pass, posterior marginal
 * state distribution of every node given the upward messages.  root_distn
 * f64[n] or NULL (= ones).  node_to_distn_array f64[nsites][nnodes][n] out.
 * status (optional) int32[nsites]: 2 where a normalising denominator is zero
 * (the reference raises NumericalZeroProb, _util.py:164-165).                */
int rt_mc0_esd_get_node_to_distn(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            const double *root_distn, const double *subtree_probability,
            double *node_to_distn_array, int32_t *status);

/* pyfelscore.mc0_esd_get_joint_endpoint_distn (_mcy_dense.py:205; twin
 * _mc0_dense.py:246-267): joint (parent state, child state) posterior of every
 * edge, f64[nsites][nnodes][n][n] keyed by the child index (root slot zero). */
int rt_mc0_esd_get_joint_endpoint_distn(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            const double *subtree_probability, const double *node_to_distn_array,
            double *joint_distns);

/* Site sums for _mjp_dense.get_expected_history_statistics (_mjp_dense.py:458-475,
 * 497-533): the upward passes (:261-291 of _mcy_dense.py), the downward pass
 * (mc0_esd_get_node_to_distn) and, per edge, the site sum of J / P over the nonzero
 * entries of the joint endpoint posterior J (what the reference contracts with its
 * Frechet derivatives, one site at a time) in one call; only n*n numbers per edge
 * leave the device.  state_mask int64[nsites][nnodes][n] as for the passes (input
 * only), site_weights f64[nsites] or NULL (= ones), root_distn f64[n] or NULL.
 * edge_weights f64[nnodes][n][n] out, keyed by the child index; slot 0 carries the
 * weighted sum of the root posteriors in its column 0.  status as above.        */
int rt_mjp_esd_expectation_weights(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            const double *root_distn, const int64_t *state_mask,
            const double *site_weights, double *edge_weights, int32_t *status);

/* The same with the observations in the compact encodings of rt_sites_create instead
 * of the reference's int64 mask array (8 n bytes per site and NODE): kind RT_OBS_STATE,
 * data uint8[nsites][nobs] (a value >= n = unobserved), or RT_OBS_MASK, data
 * uint64[nsites][nobs]; obs_nodes int64[nobs] are preorder indices, every other node
 * is unrestricted.  The mask array is built on the device.                      */
int rt_mjp_esd_expectation_weights_obs(rt_ctx *ctx, int64_t nnodes, int64_t n,
            int64_t nsites, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *esd_transitions,
            const double *root_distn, int64_t nobs, const int64_t *obs_nodes, int kind,
            const void *data, const double *site_weights, double *edge_weights,
            int32_t *status);

/* The rest of _mjp_dense.get_expected_history_statistics (:476-533) on the device: from
 * the per-edge weights W_e (edge_weights above, one slice per edge: f64[nedges][n][n]),
 * the rate matrix Q[q_index[e]] and branch length t[e] of every edge,
 *   M_e = L(t_e Q_e^T, W_e)  (Frechet derivative of expm: the corner of the exponential
 *   of the 2n x 2n block [[t Q^T, W], [0, t Q^T]], all edges in one expm launch),
 *   dwell[c] = sum_e t_e M_e[c][c],   trans[c][d] = sum_e t_e Q_e[c][d] M_e[c][d]
 * -- what the reference gets from n + nnz(Q) scipy.linalg.expm_frechet calls per edge
 * and site.  n <= RT_MAX_EXPECT_STEP_STATES: for n <= 64 the block exponential above (order
 * 2n <= RT_MAX_EXPM_STATES), for 64 < n <= 128 the pair recurrence (X1, L1)(X2, L2) =
 * (X1 X2, X1 L2 + L1 X2) with the same degree and squarings rule, taken from |t Q| alone.  */
int rt_mjp_frechet_statistics(rt_ctx *ctx, int64_t n, int64_t nedges, const double *Q,
            int64_t nq, const int64_t *q_index, const double *t, const double *W,
            double *dwell, double *trans);

/* ---- 2. batched, device-resident hot path --------------------------------
 * _mjp_dense.get_likelihood (_mjp_dense.py:362-407) for many sites:
 *   rt_model_create        tree (same CSR as above) -> device, schedule built
 *   rt_model_set_rates     per-edge expm(Q*t) on the device, P stays resident
 *                          (get_expm_augmented_tree, _mjp_dense.py:328-359)
 *   rt_sites_create        per-site observations -> kernel-native HBM layout
 *   rt_prune               upward pass + root reduce + log + batch sum
 *                          (_mcy_dense.py:286 + _mc0_dense.py:147-212)
 * rt_model_set_rates, rt_prune and rt_allreduce_totals are asynchronous on the
 * context's stream; the rt_*_get_* functions synchronise.                    */

int rt_model_create(rt_ctx *ctx, int64_t nnodes, int64_t n,
            const int64_t *tree_csr_indices, const int64_t *tree_csr_indptr,
            rt_model **model);
int rt_model_destroy(rt_model *model);

/* Q f64[nq][n][n]; node_q int64[nnodes] = which Q the edge above node v uses
 * (entry 0, the root, is ignored; NULL = all edges use Q[0]); t f64[nnodes]
 * branch length of the edge above node v (t[0] ignored).                    */
int rt_model_set_rates(rt_model *model, const double *Q, int64_t nq,
            const int64_t *node_q, const double *t);
/* ONE time-reversible rate matrix given by its spectral decomposition, the reference's
 * optional fast path (examples/p53/qtop.py:128-152 decompose_spectral_v2, :76-88
 * getp_spectral_v2): Q = S diag(D), eigh(diag(sqrt D) S diag(sqrt D)) = U diag(lam) U^T,
 * A = diag(1/sqrt D) U (rows of states with D == 0 zero), B = U^T diag(sqrt D).  Every edge
 * gets P_e = A diag(exp(lam t_e)) B, and P_e[i][i] = 1 where D[i] == 0 (D may be NULL: no
 * such state).  The decomposition is the caller's (once per Q); this call and every later
 * rt_model_recompute_transitions / rt_step rebuild all edges from it in one launch, until
 * rt_model_set_rates is called again.  A, B f64[n][n]; lam, D f64[n]; t as above.  n <= 64. */
int rt_model_set_rates_spectral(rt_model *model, const double *A, const double *lam,
            const double *B, const double *D, const double *t);
/* Re-run the per-edge expm from the Q / node_q / t already resident on the
 * device (what an optimiser or MCMC loop does after changing rates in place;
 * also one benchmark step).                                                 */
int rt_model_recompute_transitions(rt_model *model);
/* Set / read back esd_transitions f64[nnodes][n][n] directly.               */
int rt_model_set_transitions(rt_model *model, const double *esd_transitions);
int rt_model_get_transitions(rt_model *model, double *esd_transitions);
/* Pade degree / squarings per node from the last rt_model_set_rates.        */
int rt_model_get_expm_info(rt_model *model, int32_t *info /*[nnodes][2]*/);
/* root_distn f64[n] or NULL (= weights of one, NOT uniform:
 * _mjp_dense.py:389-393).                                                   */
int rt_model_set_root_distn(rt_model *model, const double *root_distn);

/* Number of accumulator slots the post-order schedule needs (the fast
 * kernels hold 8 in registers; deeper trees use the generic kernel).        */
int rt_model_schedule_depth(const rt_model *model);
/* Copy the schedule out: int32[nops][4] = {node, obs, pop, dst} (see
 * csrc/common.h rt_op).  ops may be NULL to query nops only.                */
int rt_model_get_schedule(const rt_model *model, int32_t *ops, int64_t capacity,
            int64_t *nops);
/* The same schedule computed on the host only (no device needed; tests).    */
int rt_build_schedule(int64_t nnodes, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, int32_t *ops /*[nnodes][4]*/,
            int32_t *depth);
/* Process-wide options: "force_generic" (0/1) routes every later
 * rt_sites_create to the generic fallback kernel.  "jit" (-1 automatic, 0
 * never, 1 always): rt_sites_create compiles (hiprtc, once per distinct tree
 * and set of observed nodes) a pruning kernel specialised for the tree (n <=
 * 64); automatic = batches of at least 65 536 / n sites.  Results are
 * bit-identical with and without it.  "jit_block_sites" (0 automatic, 1..64):
 * sites per wave of those kernels (automatic balances the waves over the CUs). */
/* "jit_async" (1 default / 0): rt_sites_create does not wait for hiprtc -- a host
 * thread of this process compiles the kernel (or loads its code object from the persistent
 * cache directory: RAOTEH_JIT_CACHE_DIR, default ~/.cache/raoteh_amd/jit; RAOTEH_JIT_CACHE=0
 * disables it) while the batch runs the interpreter kernel; a later rt_prune / rt_step swaps
 * the kernel in once it is there and has passed the probe verification.  rt_sites_jit_wait
 * blocks until that has happened (or failed: the batch then stays on the interpreter).
 * At most RAOTEH_JIT_MAX_JOBS (default 2) such threads run at a time in a process: a batch
 * created while they are busy keeps the interpreter kernel (a search over topologies does
 * not pile up compiles; set "jit" to 0 there to skip the source generation as well).     */
/* "rescale" (0 default / 1): batches created while it is set rescale their messages on the
 * way up -- whenever the largest entry of a site's message falls below 2^-256 the message is
 * multiplied by the exact power of two that brings it back to [1, 2) and the exponent is kept
 * per site; log-likelihood = log(scaled likelihood) + exponent ln 2.  The reference never
 * rescales (_mc0_dense.py:184-209 works on plain f64): a tree of a thousand leaves is "zero
 * probability" there and, by default, here.  With the option such a batch keeps the
 * interpreter kernels (no tree-specialised kernel); a batch that never comes near the
 * threshold gets the default kernels' numbers bit for bit (powers of two are exact).
 * Likelihood evaluation only (rt_prune / rt_step): rt_expect_step and rt_sites_posteriors
 * return RT_ERR_UNSUPPORTED for such a batch (their passes do not rescale).                 */
/* "leaf_state_kernels" (1 default / 0): a batch uploaded as observed states at the leaves
 * (RT_OBS_STATE, every leaf observed, 5..128 states) may run a tree-specialised kernel whose
 * leaf steps gather a column of P instead of multiplying P by the one-hot vector -- the same
 * numbers bit for bit, about half the products; likewise RT_OBS_MASK batches whose leaves all
 * have one or two allowed states (two columns added); 0 keeps the products (what a dense upload
 * runs).                                                                                      */
int rt_set_option(const char *key, int64_t value);
/* The same options for ONE context (they take precedence over the process-wide
 * defaults above; value -2 = back to the default): two contexts on two threads can
 * then run with different settings without sharing mutable state.              */
int rt_ctx_set_option(rt_ctx *ctx, const char *key, int64_t value);
/* Diagnostics, host only: the HIP source rt_sites_create would compile for this
 * tree (n <= 32; MFMA family for n > 4), observation stream and prefetch distance. */
int rt_jit_source(int64_t nnodes, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, int64_t n, int64_t nobs,
            const int64_t *obs_nodes, int64_t prefetch, char *buf, int64_t capacity);

/* obs_nodes int64[nobs]: preorder indices of the nodes that carry per-site
 * data (all other nodes are unrestricted).  data layout per `kind` above.   */
int rt_sites_create(rt_model *model, int64_t nsites, int kind, int64_t nobs,
            const int64_t *obs_nodes, const void *data, rt_sites **sites);
/* A second batch with the same values at different HBM addresses (used by
 * the benchmark to rotate batches so the 256 MiB Infinity Cache cannot hold
 * the working set): the same observations, pruning kernel, per-site
 * log-likelihoods, statuses and totals (a pending batch sum is reduced first),
 * so that both read the same until either is pruned again.  A clone of a batch
 * that was never pruned is never pruned either.  (Site weights are not copied, and neither are
 * the results of rt_step_multi: its getters return RT_ERR_INVALID on the clone until the clone
 * has been stepped.)                                                            */
int rt_sites_clone(rt_sites *sites, rt_sites **clone);
/* Wait for the background compile of this batch's tree-specialised kernel, if one is
 * pending, and switch the batch to it (see "jit_async").                              */
int rt_sites_jit_wait(rt_sites *sites);
/* Join every background compile of the process.  Call it before the process exits if batches
 * may still be compiling (rt_ctx_destroy does it for its own context): a compile thread must
 * not be running while exit handlers tear the compiler down.                            */
int rt_jit_wait_all(void);
int rt_sites_destroy(rt_sites *sites);
int64_t rt_sites_device_bytes(const rt_sites *sites);
/* Seconds rt_sites_create spent in hiprtc for this batch's tree-specialised kernel
 * (0: none, or the kernel came from the cache), and the name of the pruning kernel
 * variant the batch last ran (owned by the batch; "" before the first rt_prune). */
double rt_sites_jit_compile_seconds(const rt_sites *sites);
/* Diagnostics: copy a __device__ variable of the batch's compiled kernel to the host
 * (the per-step clock stamps of RAOTEH_JIT_TRACE, tools/trace_c3.py).              */
int rt_debug_jit_global(rt_sites *sites, const char *name, void *dst, int64_t bytes);
const char *rt_sites_kernel_name(const rt_sites *sites);

int rt_prune(rt_model *model, rt_sites *sites);
/* One evaluation of the repeated-evaluation loop (optimiser / MCMC iteration) in
 * one call: rt_model_recompute_transitions (if recompute_transitions != 0) +
 * rt_prune.                                                                   */
int rt_step(rt_model *model, rt_sites *sites, int recompute_transitions);
/* When the results of rt_step exist.  rt_step queues work and returns; two pieces of a step
 * may still be pending after it: the batch sum (it rides in the next expm launch of the
 * context) and, for a 49..64-state batch that runs its tree as two root halves, the root
 * combine that writes the per-site log-likelihoods, the status and the partial sums (it runs
 * in the idle waves of the next expm launch, the batch sum one launch later).  Nothing changes
 * for callers: every call that reads or replaces a batch's results, its observations or the
 * model's root distribution -- the getters, rt_sites_clone, rt_prune, the multi and
 * partitioned steps, the resident reads, the all-reduce entries, rt_ctx_sync, the destroy
 * calls -- runs what is pending first, with the stand-alone kernels, and the numbers are the
 * same bit for bit.  RAOTEH_CARRY_COMBINE=0 (read per call) keeps the combine a launch of
 * its own right after the pruning kernel; RAOTEH_NO_DEFER_REDUCE keeps both.              */
/* The rule of the carried combine on the host (no device needed; tests): may an expm launch
 * of G matrix workgroups carry the root combine of a batch of nt row tiles per site tile and
 * nblocks16 site tiles?  1 / 0.  With tile_of (int64[4 G]) non-NULL and the answer 1,
 * tile_of[4 g + k] = the tile that idle wave k of workgroup g finishes, or -1.            */
int rt_carry_combine_deal(int64_t nt, int64_t nblocks16, int64_t G, int root_halves,
            int rescale, int partitioned, int multi, int64_t *tile_of);
/* _mjp_dense.get_expected_history_statistics (_mjp_dense.py:410-539) summed over a RESIDENT
 * batch: (optionally) the per-edge expm from the resident rates, the upward pass, the downward
 * pass (mc0_esd_get_node_to_distn), the per-edge site sums of J / P and one Frechet block
 * exponential per edge, all on the device; 2 n + n^2 numbers come back:
 *   dwell[c]       expected time spent in state c, summed over edges and sites
 *   root_posterior[c]  sum over sites of the posterior probability of state c at the root
 *   trans[c][d]    expected number of c -> d transitions (0 where no rate matrix has c -> d)
 * each site weighted by rt_sites_set_weights (multiplicities of site patterns; default 1).
 * status (optional, int32[nsites]): 2 where a normalising denominator is zero (the reference
 * raises NumericalZeroProb).  n <= RT_MAX_EXPECT_STEP_STATES (every n rt_sites_create takes in
 * the matrix-pipe layout: the 122-state switching model included), batches created by
 * rt_sites_create (n > 4: any observation kind; n <= 4: the fused lane kernel works on allowed sets, so a
 * dense batch counts a state as allowed where its likelihood is not zero), rates set by
 * rt_model_set_rates.  RT_ERR_INVALID for a model with spectral rates or with transitions set
 * directly: on a model that never had rates, or after them with recompute_transitions == 0 (the
 * resident rate matrices would no longer describe the transition matrices).
 * RT_ERR_UNSUPPORTED for a "rescale" batch (the passes work on unscaled f64 messages), at every
 * n.  Synchronous.                                                                       */
int rt_expect_step(rt_model *model, rt_sites *sites, int recompute_transitions,
            double *dwell, double *root_posterior, double *trans, int32_t *status);
/* _mcy_dense.kitchen_sink (_mcy_dense.py:57-230) for every site of a RESIDENT batch: the
 * posterior node marginals D_v (mc0_esd_get_node_to_distn with the model's root distribution)
 * and the joint endpoint posteriors J_v[a][b] = D_p[a] P_v[a][b] L_v[b] / (P_v L_v)[a] of every
 * edge p -> v (mc0_esd_get_joint_endpoint_distn), reduced on the device to sums over state sets.
 * A set is a state bit mask of two 64-bit words (bit s % 64 of word s / 64, as RT_OBS_MASK).
 *   node_sets  uint64[n_node_sets][2]; edge_sets uint64[n_edge_sets][2][2] = (A, B)
 *   node_values[i][v][k] = sum_{s in S_k} D_v[s]                  f64[nsites][nnodes][n_node_sets]
 *   edge_values[i][v][k] = sum_{a in A_k, b in B_k} J_v[a][b]     f64[nsites][nnodes][n_edge_sets]
 *                          (keyed by the child's preorder index; the root's slot is 0)
 *   marginals[i][j] = D_{marginal_nodes[j]}                       f64[nsites][n_marginal_nodes][n]
 *                          (marginal_nodes preorder indices, distinct; NULL with
 *                          n_marginal_nodes = nnodes: every node in preorder)
 *   status[i]: 0, RT_SITE_ZERO_PROB (the site's likelihood is 0: every output of the site is
 *              0), or 2 (a normalising denominator is zero under a non-zero parent probability)
 * Any output may be NULL; only the ones given cross PCIe.  Every batch rt_sites_create makes for
 * 2 <= n <= 128 (dense observations are used as values at every n), models whose transitions came
 * from any of the rt_model_set_* calls (recompute_transitions != 0 needs rates).  RT_ERR_UNSUPPORTED:
 * a "rescale" batch, a tree deeper than the fast kernels take, nnodes < 2, more than
 * RT_MAX_POSTERIOR_SETS sets of a kind, more than 96 GB of scratch.  Synchronous; the batch keeps
 * its kernel, log-likelihoods, status and totals; sums in a fixed order (bit-identical calls).  */
#define RT_MAX_POSTERIOR_SETS 8
int rt_sites_posteriors(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t n_node_sets, const uint64_t *node_sets,
            int64_t n_edge_sets, const uint64_t *edge_sets,
            int64_t n_marginal_nodes, const int64_t *marginal_nodes,
            double *node_values, double *edge_values, double *marginals, int32_t *status);
/* The reference's branch-site map, examples/code2x3/extras.get_expected_ntransitions
 * (extras.py:19-132), for every site of a RESIDENT batch and up to RT_MAX_BRANCH_COEFS coefficient
 * matrices in one call: per site, per branch, the conditional expectation of a linear statistic
 * of the history on that branch.  One coefficient matrix E (f64[n][n]) means
 *   E[c][d], c != d   the weight of one c -> d transition
 *   E[c][c]           the weight of a unit of time spent in c
 * so on the edge above node v, with that edge's rate matrix Q_v and length t_v, the direction is
 * C_v[c][d] = E[c][d] Q_v[c][d] off the diagonal, C_v[c][c] = E[c][c], and with
 * G_v = L(t_v Q_v, t_v C_v) (the Frechet derivative of the matrix exponential) and J_v, P_v the
 * joint endpoint posterior and the transition matrix of the edge
 *   values[i][v][k] = sum_{a,b} J_v[a][b] G_v[a][b] / P_v[a][b]     f64[nsites][nnodes][n_coefs]
 *                     (keyed by the child's preorder index; the root's slot is 0)
 *   edge_sums[v][k] = sum_i w_i values[i][v][k]                     f64[nnodes][n_coefs]
 *                     (w: rt_sites_set_weights, default 1; reduced on the device, fixed order)
 * With a zero diagonal E is exactly the reference's E (an indicator of the synonymous changes,
 * say: the expected number of them on every branch).  E = identity gives the branch length;
 * E = ones off the diagonal and diag(Q) on it gives C = Q and values = t_v d log L_i / d t_v, the
 * analytic branch-length gradient.  Coefficients may be negative; an all-zero matrix gives zeros;
 * they must be finite.
 *   status[i]: as rt_sites_posteriors (a site of zero likelihood: RT_SITE_ZERO_PROB, its values
 *              are 0 and it adds nothing to edge_sums)
 * values, edge_sums and status may each be NULL; only what is given crosses PCIe (the per-site
 * array is large: nsites * nnodes * n_coefs doubles).  Every batch rt_sites_create makes for
 * 2 <= n <= 128 (dense observations are used as values at every n), per-edge rate matrices, any
 * tree rt_sites_posteriors takes.  The rates must come from rt_model_set_rates (the derivative
 * needs Q): RT_ERR_INVALID for a model with spectral rates or with transitions set directly (on
 * a model that never had rates, or after them with recompute_transitions == 0).
 * RT_ERR_UNSUPPORTED: a "rescale" batch, a tree deeper than the fast kernels take, nnodes < 2,
 * more than RT_MAX_BRANCH_COEFS matrices, more than 96 GB of scratch.  Synchronous; the batch
 * keeps its kernel, log-likelihoods, status and totals; two calls return the same bits.      */
#define RT_MAX_BRANCH_COEFS 8
int rt_sites_branch_expectations(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t n_coefs, const double *coefs, double *values, double *edge_sums,
            int32_t *status);
/* Per-branch likelihood profiles of a RESIDENT batch: what a line search, Brent or Newton per
 * branch, a test for a zero-length branch or a likelihood-ratio interval of one branch asks of the
 * likelihood, for every branch at once and without one rt_model_set_rates + rt_step per branch and
 * trial length.  lengths f64[nnodes][npoints], rows in preorder (row 0, the root's, is ignored):
 * 1..RT_MAX_PROFILE_POINTS trial lengths per branch, finite and >= 0.
 *   values[i][v][g] = log L_i(t_v -> lengths[v][g]) - log L_i       f64[nsites][nnodes][npoints]
 *                     the change of site i's log-likelihood when the branch above preorder node v
 *                     alone takes the length lengths[v][g], every other branch staying at its
 *                     resident length; the root's row is 0; -inf where the site has likelihood 0
 *                     at that length
 *   sums[v][g]      = sum_i w_i values[i][v][g]                     f64[nnodes][npoints]
 *                     (w: rt_sites_set_weights, default 1; reduced on the device, fixed order;
 *                     a site of weight 0 adds nothing, even where its value is -inf)
 *   status[i]       : as rt_sites_branch_expectations (a site of zero likelihood:
 *                     RT_SITE_ZERO_PROB, its values are 0 and it adds nothing to sums; 2: a live
 *                     parent state over a non-positive denominator)
 * One upward and one downward pass serve all branches and lengths: with J_v the joint endpoint
 * posterior and P_v the resident transition matrix of the edge, L_i(tau) / L_i =
 * sum_{a,b} J_v[a][b] expm(tau Q_v)[a][b] / P_v[a][b]; the (nnodes - 1) npoints exponentials are
 * one launch.  The identity is exact while the resident t_v > 0 (where J_v / P_v has lost a state
 * pair because P_v[a][b] = 0, Q_v cannot reach b from a at any length).  CAVEAT: at a resident
 * t_v = 0, P_v is the identity and that argument fails -- the row of such an edge is NaN in values
 * (at every site but those of zero likelihood, which stay 0) and in sums; give the edge a
 * positive length to profile it.
 * values, sums and status may each be NULL; only what is given crosses PCIe.  Every batch
 * rt_sites_posteriors takes; rates from rt_model_set_rates (per-edge rate matrices included) or
 * from rt_model_set_rates_spectral (n <= 64).  RT_ERR_INVALID: no rates (transitions set
 * directly: on a model that never had rates, or after them with recompute_transitions == 0 --
 * the resident rates would no longer describe P_v), npoints outside 1..RT_MAX_PROFILE_POINTS, a
 * negative or non-finite length, lengths NULL, a batch of another model.  RT_ERR_SINGULAR: an
 * exponential failed (tau Q_v not finite: a huge length); nothing returned is usable then.
 * RT_ERR_UNSUPPORTED: a "rescale" batch, a batch of the generic
 * kernel, a tree deeper than the fast kernels take, nnodes < 2, more than 96 GB of scratch.
 * Synchronous; the model keeps its transitions and the batch its kernel, log-likelihoods, status
 * and totals; two calls return the same bits.                                                  */
#define RT_MAX_PROFILE_POINTS 64
int rt_sites_branch_profiles(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t npoints, const double *lengths, double *values, double *sums,
            int32_t *status);
/* The branch lengths of the last rt_model_set_rates / rt_model_set_rates_spectral, f64[nnodes] in
 * preorder (0 at the root).  RT_ERR_INVALID before either call.                               */
int rt_model_get_branch_lengths(rt_model *model, double *t);
/* The nearest-neighbour interchanges (NNI) of the model's tree.  Nodes are preorder indices.  A
 * move is a triple (v, c, s): v a non-root node with at least one child, c a child of v, s a
 * sibling of v (another child of p = parent(v)).  The move exchanges the subtrees of c and s: the
 * edges v->c, p->s become v->s, p->c, and every moved subtree keeps its own edge -- the length,
 * rate matrix and transition matrix of c and of s go with the node below the edge.  The list is
 * ordered by v ascending, then c in the CSR child order of v, then s in the CSR child order of p:
 * a pure function of the topology, nmoves = sum_v #children(v) #siblings(v) (0 for a star or a
 * path).
 * The definition is ROOTED, because rate matrices need not be reversible.  One case to know:
 * where p is a root with exactly the two children v and s, the moved tree has the same UNROOTED
 * topology as before: the edges p->v and p->s are one edge of the unrooted tree, of length
 * t_v + t_s, and the move only redistributes lengths along it (c now hangs t_c + t_v from v, and
 * v is t_s from s).  Under a stationary reversible model the moved tree's likelihood is that of
 * the unmoved tree at those lengths -- the same as before where t_v = 0 -- so a caller with such
 * a model learns nothing about the topology from those moves and can skip them.
 * Host only.  moves int32[capacity][3]; moves == NULL asks for the count alone; RT_ERR_INVALID
 * when capacity < *nmoves (the count is still returned).                                       */
int rt_model_nni_moves(const rt_model *model, int32_t *moves, int64_t capacity, int64_t *nmoves);
/* The same list from the tree alone, children CSR in preorder indices as for rt_model_create:
 * for a caller that has no model (and no device) yet.                                          */
int rt_tree_nni_moves(int64_t nnodes, const int64_t *tree_csr_indices, const int64_t *tree_csr_indptr,
            int32_t *moves, int64_t capacity, int64_t *nmoves);
/* Every NNI neighbour of the tree scored on a RESIDENT batch, without one model build, upload and
 * rt_step per candidate.  For site i, move mv of rt_model_nni_moves and trial length g of the edge
 * above v:
 *   values[i][mv][g] = log L_i(tree after mv, t_v -> lengths[v][g]) - log L_i
 *                                                                  f64[nsites][nmoves][npoints]
 *                      -inf where a live site has likelihood 0 on the moved tree
 *   sums[mv][g]      = sum_i w_i values[i][mv][g]                  f64[nmoves][npoints]
 *                      (w: rt_sites_set_weights, default 1; reduced on the device, fixed order;
 *                      a site of weight 0 adds nothing, even where its value is -inf)
 *   status[i]        : a site of zero likelihood has RT_SITE_ZERO_PROB, its values are 0 and it
 *                      adds nothing to sums
 * lengths == NULL: npoints must be 1 and the edge above v keeps its resident matrix (the plain
 * swap); no exponential runs, so a model whose transitions were set directly is taken too.
 * Otherwise lengths f64[nnodes][npoints] as for rt_sites_branch_profiles: 1..RT_MAX_PROFILE_POINTS
 * trial lengths per node, finite and >= 0, shared by all moves about v; the rows of nodes that
 * have no move (the root's among them) are ignored.  The (nnodes - 1) npoints exponentials are the
 * one launch of rt_sites_branch_profiles, from rt_model_set_rates (per-edge rate matrices
 * included) or rt_model_set_rates_spectral (n <= 64).
 * With L_w, M_w = P_w L_w of the stored upward pass, up_p the message into p from above (the root
 * weights at the root), W[a] = up_p[a] obs_p[a] prod_{w child of p, not v, s} M_w[a] and
 * L'_v[b] = obs_v[b] prod_{w child of v, not c} M_w[b] M_s[b]:
 *   L_i(mv, tau) = sum_b L'_v[b] (P_v(tau)^T (W o M_c))[b].
 * Nothing is divided: the `up` vectors come from a downward pass of their own, normalised once at
 * the root by 1 / L_i, so the result is exact where transition matrices or observations have
 * zeros, and a resident t_v = 0 is nothing special (no NaN rows, unlike rt_sites_branch_profiles).
 * values, sums and status may each be NULL; only what is given crosses PCIe.  Every batch
 * rt_sites_posteriors takes.  nmoves == 0: RT_OK, and no output but status is touched.  Where
 * the result of all moves would not fit the scratch the moves go through the device in chunks.
 * RT_ERR_INVALID: npoints out of range (or not 1 without lengths), a negative or non-finite
 * length in a row that counts, lengths on a model without rates (or whose transitions were set
 * directly after them, with recompute_transitions == 0), a batch of another model.
 * RT_ERR_SINGULAR: an exponential failed; nothing returned is usable then.  RT_ERR_UNSUPPORTED:
 * a partitioned batch, a "rescale" batch, a batch of the generic kernel, a tree deeper than the
 * fast kernels take, nnodes < 2, more than 96 GB of scratch.  Synchronous; the model keeps its
 * transitions and the batch its kernel, log-likelihoods, status and totals; two calls return the
 * same bits.                                                                                   */
int rt_sites_nni_scores(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t npoints, const double *lengths, double *values, double *sums,
            int32_t *status);
/* Query sequences placed on every branch of the tree of a RESIDENT batch (evolutionary placement),
 * without one model build, upload and rt_step per candidate.  Nodes are preorder indices.  v is a
 * non-root node, p = parent(v), Q_v and t_v the rate matrix and the length of the edge above v.  A
 * placement of query q is (v, rho, tau): a new unobserved node x cuts the edge p -> v into p -> x
 * of length rho t_v and x -> v of length (1 - rho) t_v, and a new leaf that carries the query's
 * observation o_q hangs below x on an edge of length tau; all three edges under Q_v.  The
 * definition is ROOTED, as for NNI, because rate matrices need not be reversible; the root has no
 * row.  For site i:
 *   values[i][q][v][r][k] = log L_i(tree with q placed at (v, fractions[r], pendant[k])) - log L_i
 *                           f64[nsites][nqueries][nnodes][nfractions][npendant]: the log of the
 *                           conditional probability of the query's column given the reference
 *                           column; -inf where it is 0; the root's row is 0
 *   sums[q][v][r][k]      = sum_i w_i values[i][q][v][r][k]
 *                           f64[nqueries][nnodes][nfractions][npendant]
 *                           (w: rt_sites_set_weights, default 1; reduced on the device, fixed order;
 *                           a site of weight 0 adds nothing, even where its value is -inf)
 *   status[i]             : a site of zero likelihood has RT_SITE_ZERO_PROB, its values are 0 and it
 *                           adds nothing to sums
 * queries: query_kind RT_OBS_DENSE, f64[nqueries][nsites][n] likelihood vectors, or RT_OBS_STATE,
 * uint8[nqueries][nsites] (a value >= n = unobserved, as for an upload); RT_OBS_MASK queries are
 * not taken.  fractions f64[nfractions], each in [0, 1], 1..RT_MAX_PLACE_FRACTIONS of them;
 * pendant f64[npendant], finite and >= 0, shared by all edges, 1..RT_MAX_PLACE_PENDANT of them;
 * 2 nfractions + npendant <= 32: per node the lengths rho_r t_v, (1 - rho_r) t_v and tau_k are the
 * grid of ONE launch of the model's exponential (fractions 0 and 1 go through it like any other
 * length), from rt_model_set_rates (per-edge rate matrices included) or
 * rt_model_set_rates_spectral (n <= 64).
 * With L_w, M_w = P_w L_w of the stored upward pass and up_p the message into p from above,
 * normalised once at the root by 1 / L_i:
 *   A_v[a]       = up_p[a] obs_p[a] prod_{w child of p, w != v} M_w[a]
 *   F_{v,r}[b]   = (P_v(rho_r t_v)^T A_v)[b] (P_v((1 - rho_r) t_v) L_v)[b]
 *   h_{d,k,q}[b] = sum_c expm(Q_d tau_k)[b][c] o_q[c]         (d: a distinct rate-matrix index)
 *   ratio        = sum_b F_{v,r}[b] h_{qidx(v),k,q}[b]
 * Nothing is divided, so the result is exact where transition matrices or observations have
 * zeros and at a resident t_v = 0.  h is made once per distinct rate matrix in use, never once
 * per edge.  values, sums and status may each be NULL; only what is given crosses PCIe.  Every
 * batch rt_sites_posteriors takes.  Where the per-site result of all queries would not fit the
 * scratch the queries go through the device in chunks (RAOTEH_PLACE_CHUNK_BYTES of result per
 * chunk, default 4 GB, or what the 96 GB cap leaves); the field F is made once, and chunked and
 * unchunked calls give the same bits.
 * RT_ERR_INVALID: nqueries < 1, counts out of range, a fraction outside [0, 1] or not finite, a
 * negative or non-finite pendant length, NULL queries, fractions or pendant, a model without
 * rates (or whose transitions were set directly after them, with recompute_transitions == 0), a
 * batch of another model.  RT_ERR_SINGULAR: an exponential failed; nothing returned is usable
 * then.  RT_ERR_UNSUPPORTED: RT_OBS_MASK queries, a partitioned batch, a "rescale" batch, a batch
 * of the generic kernel, a tree deeper than the fast kernels take, nnodes < 2, more than 96 GB of
 * scratch.  Synchronous; the model keeps its transitions and the batch its kernel,
 * log-likelihoods, status and totals; two calls return the same bits.                          */
#define RT_MAX_PLACE_FRACTIONS 8
#define RT_MAX_PLACE_PENDANT   16
int rt_sites_placements(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t nqueries, int query_kind, const void *queries,
            int64_t nfractions, const double *fractions,
            int64_t npendant, const double *pendant,
            double *values, double *sums, int32_t *status);
/* Subtree pruning and regrafting (SPR): every move of the tree within a radius scored on a
 * RESIDENT batch, without one model build, upload and rt_step per candidate.  Nodes are preorder
 * indices.  A move is (c, y) with a fraction rho: c is a non-root node, v = parent(c); y is a
 * non-root node outside the subtree of c, q = parent(y).  The subtree of c leaves v and keeps its
 * own edge (length, rate matrix and transition matrix go with the node below the edge, as in an
 * NNI); a new unobserved node x cuts q -> y into q -> x of length rho t_y and x -> y of length
 * (1 - rho) t_y, both under Q_y as in a placement, and c hangs below x.  v stays with one child
 * fewer -- a single-child or childless node where that leaves one or none (an unobserved
 * childless node contributes ones); no edges are merged: with per-edge rate matrices merging is
 * not defined, and a single-child node has the same likelihood.  The definition is ROOTED, as
 * for NNI and placements, because rate matrices need not be reversible.
 * The radius of a move is d(c, y) = min(dist(v, y), dist(v, parent(y))) in edges of the tree:
 * d = 0 for the edge above v and the edges above the siblings of c, d = 1 for the edge above
 * parent(v), those above the siblings of v and those above the children of the siblings of c,
 * and so on outward.  radius >= 0 lists every (c, y) with d <= radius; radius < 0 means no limit:
 * nmoves = sum_{c != root} (nnodes - 1 - |subtree(c)|).  The list goes by c ascending, then by y
 * ascending: a pure function of topology and radius.  Two families of moves leave the tree
 * unchanged and stay in the list: y = v at rho = 1, and y a sibling of c at rho = 0 (x coincides
 * with v across an identity matrix; their values are 0 to rounding).  Other moves onto those
 * edges only slide c along an edge where v has two children; they are scored like any other.
 * rt_model_spr_moves / rt_tree_spr_moves (from a CSR alone) are host only: moves
 * int32[capacity][2] receives the pairs (c, y) and *nmoves their number; moves == NULL asks for
 * the number alone; RT_ERR_INVALID, with *nmoves set, where capacity is short; RT_ERR_INVALID
 * for a CSR that is no tree (a child before its parent, a child listed twice).                */
int rt_model_spr_moves(const rt_model *model, int64_t radius, int32_t *moves, int64_t capacity,
            int64_t *nmoves);
int rt_tree_spr_moves(int64_t nnodes, const int64_t *tree_csr_indices, const int64_t *tree_csr_indptr,
            int64_t radius, int32_t *moves, int64_t capacity, int64_t *nmoves);
/* The moves of rt_model_spr_moves(model, radius) scored.  For site i:
 *   values[i][mv][r] = log L_i(tree after move mv at fractions[r]) - log L_i
 *                      f64[nsites][nmoves][nfractions]; -inf where a live site has likelihood 0
 *                      after the move
 *   sums[mv][r]      = sum_i w_i values[i][mv][r]          f64[nmoves][nfractions]
 *                      (w: rt_sites_set_weights, default 1; reduced on the device, fixed order;
 *                      sites of weight 0 and of zero likelihood add nothing)
 *   status[i]        : as for rt_sites_nni_scores: a site of zero likelihood has
 *                      RT_SITE_ZERO_PROB, its values are 0
 * fractions f64[nfractions], each in [0, 1], 1..RT_MAX_PLACE_FRACTIONS of them.  Per node the
 * lengths rho_r t and (1 - rho_r) t are the grid of ONE launch of the model's exponential
 * (fractions 0 and 1 go through it like any other length), from rt_model_set_rates (per-edge rate
 * matrices included) or rt_model_set_rates_spectral (n <= 64).
 * With L_w, M_w = P_w L_w, obs_w of the stored upward pass, up_w the message into w from above,
 * normalised once at the root by 1 / L_i, and a_0 = v, a_1 = parent(v), ... the path to the root:
 *   L-_{a_0}[b]  = obs_v[b] prod_{w child of v, w != c} M_w[b]
 *   M-_{a_j}     = P_{a_j} L-_{a_j}
 *   L-_{a_j}[b]  = obs_{a_j}[b] M-_{a_{j-1}}[b] prod_{w child of a_j, w != a_{j-1}} M_w[b]
 *   up-_{a_j}    = up_{a_j}             (an ancestor's message from above holds no c)
 *   off the path: L-_x = L_x, M-_x = M_x,
 *   A-_x[a]      = up-_q[a] obs_q[a] prod_{w child of q, w not in {x, c}} M-_w[a]   (q = parent(x))
 *   up-_x        = P_x^T A-_x
 *   F_{c,y,r}[b] = (P_y(rho_r t_y)^T A-_y)[b] (P_y((1 - rho_r) t_y) L-_y)[b]
 *   ratio        = sum_b F_{c,y,r}[b] M_c[b]
 * Nothing is divided, so the result is exact where transition matrices or observations have
 * zeros and at resident lengths of 0.  Work per pruned node is bounded by the radius: only path
 * nodes and off-path nodes within it are touched.  values, sums and status may each be NULL;
 * only what is given crosses PCIe.  Every batch rt_sites_placements takes.  nmoves == 0 (two
 * nodes) returns RT_OK with the status alone.  Where the per-site result of all moves would not
 * fit the scratch the pruned nodes go through the device in chunks (RAOTEH_SPR_CHUNK_BYTES of
 * result per chunk, default 4 GB, or what the 96 GB cap leaves); a chunk never splits the moves
 * of one pruned node, and chunked and unchunked calls give the same bits.
 * RT_ERR_INVALID: nfractions out of range, a fraction outside [0, 1] or not finite, NULL
 * fractions, a model without rates (or whose transitions were set directly after them, with
 * recompute_transitions == 0), a batch of another model, 2^31 or more (move, fraction) pairs.
 * RT_ERR_SINGULAR: an exponential failed; nothing returned is usable then.  RT_ERR_UNSUPPORTED:
 * a partitioned batch, a "rescale" batch, a batch of the generic kernel, a tree deeper than the
 * fast kernels take, nnodes < 2, more than 96 GB of scratch.  Synchronous; the model keeps its
 * transitions and the batch its kernel, log-likelihoods, status and totals; two calls return
 * the same bits.  Not done here: trial lengths for the pruned edge or lengths optimised after
 * the move (rt_sites_branch_profiles on the adopted tree), partitioned and mixture batches,
 * unrooted de-duplication of moves.                                                           */
int rt_sites_spr_scores(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t radius, int64_t nfractions, const double *fractions,
            double *values, double *sums, int32_t *status);
/* _sample_mcy_dense.resample_states (_sample_mcy_dense.py:23-69, through
 * _sample_mc0_dense.resample_states, _sample_mc0_dense.py:20-98) for every site of a RESIDENT
 * batch: ndraws joint draws of a state for every node from the posterior given the observations.
 *   states[d][i][v]  uint8[ndraws][nsites][nnodes], v the preorder index; 255 = no state (the code
 *                    an RT_OBS_STATE upload reads as "unobserved": a draw can be uploaded back)
 * With L_v the subtree likelihood of node v including its own observation (dense observations are
 * used as values, as in rt_sites_posteriors), the weights of the root are
 *   w[s] = root_w[s] * L_root[s]       (root_w: rt_model_set_root_distn, ones if unset)
 * and those of a node v whose parent drew state a
 *   w[b] = P_v[a][b] * L_v[b];
 * a negative product counts as 0.  With total = sum_s w[s] and
 *   u = philox_uniform(seed, first_draw + d, i * nnodes + v)
 * (Philox4x32-10: counter words {index low, index high, draw low, draw high}, key {seed low, seed
 * high}; u = (((c0 << 21) ^ (c1 >> 11)) mod 2^53) * 2^-53 of the output words c0, c1 -- the
 * generator of rt_forest_resample_states with the draw number as its sweep) the pick is the first
 * state in index order with w > 0 whose cumulative weight exceeds u * total; if rounding leaves
 * none, the last state with w > 0.  (The kernels accumulate in chunks of four states: the
 * cumulative weights agree with a sequential sum to rounding.)  So a draw depends on (seed,
 * first_draw + d, site, node) and the numbers alone: not on ndraws, not on the batch's pruning
 * kernel, and draws [f, f + k) of one call equal draws [0, k) of a call with first_draw = f.
 *   status[i] (optional), OR-ed over the draws: RT_SITE_ZERO_PROB when the root's total is not
 *              positive and finite (every node of every draw of the site is 255); 2 when a
 *              non-root node has no state of positive weight (that node and its descendants are
 *              255; impossible with a consistent L)
 * Every batch rt_sites_create makes for 2 <= n <= 128 (all observation kinds), transitions from
 * any of the rt_model_set_* calls (recompute_transitions != 0 needs rates).  RT_ERR_INVALID:
 * ndraws < 1, states NULL, a batch of another model, no transitions yet.  RT_ERR_UNSUPPORTED: what
 * rt_sites_posteriors refuses (a "rescale" batch, a generic-kernel batch, a tree deeper than the
 * fast kernels take, nnodes < 2), more than 96 GB of scratch, and for n > 4 a tree of more than
 * RT_MAX_SAMPLE_NODES nodes (the sampled states of one wave's sites live in LDS, 16 bytes per node
 * and draw of a block).  Synchronous; only states and status cross PCIe; the batch keeps its
 * kernel, log-likelihoods, status and totals.                                                  */
#define RT_MAX_SAMPLE_NODES 8192
int rt_sites_sample_states(rt_model *model, rt_sites *sites, int recompute_transitions,
            uint64_t seed, uint64_t first_draw, int64_t ndraws,
            uint8_t *states /* [ndraws][nsites][nnodes], preorder index */,
            int32_t *status /* [nsites] or NULL */);
/* draws that share one read of L in rt_sites_sample_states for a tree of nnodes nodes (n > 4):
 * 16 at most, fewer as the tree grows, 1 from 1025 nodes on; 0 beyond RT_MAX_SAMPLE_NODES       */
int rt_sample_states_draw_block(int64_t nnodes);
/* The joint maximum-likelihood reconstruction (Pupko, Pe'er, Shamir & Graur 2000) of every site of
 * a RESIDENT batch: the single most probable assignment of a state to every node, with its
 * probability.  The quantities for site i:
 *   o_v  the observation vector of node v, all ones where unobserved (dense observations are used
 *        as values);
 *   w    the root weights (rt_model_set_root_distn), or ones if none was set;
 *   P_v  the model's transition matrix of edge parent(v) -> v.
 * The probability of an assignment x of a state to every node is
 *   J(x) = w[x_root] * prod_v o_v[x_v] * prod_{v != root} P_v[x_parent(v)][x_v];
 * negative or NaN factors count as 0, as in rt_sites_sample_states.  The recursion:
 *   L_v(b) = o_v(b) * prod_{c child of v} M_c(b)
 *   M_c(a) = max_b P_c(a, b) * L_c(b)
 * The reconstruction, ties ALWAYS to the lowest state index: x_root is the lowest a that maximises
 * w(a) * L_root(a); then, walking in preorder, x_v is the lowest b that maximises
 * P_v(x_parent, b) * L_v(b).
 *   states[i][v]  uint8[nsites][nnodes], v the preorder index
 *   log_joint[i]  (optional) log J(x*)
 *   status[i]     (optional) 0; RT_SITE_ZERO_PROB for a site whose maximum is not positive and
 *                 finite: every state of the site is 255 and log_joint is -inf.  (2: a live parent
 *                 state without a child state of positive weight, that node and its descendants
 *                 are 255; impossible with a consistent L.)
 * Scaling: every node's L_v is multiplied per site by a power of two (the one that brings its
 * largest entry into [0.5, 1)); the multiplication is exact, so it never changes an arg-max.  The
 * exponents are summed per site over all nodes and log_joint = log(root maximum) + E ln 2: the
 * result is what f64 arithmetic with an unbounded exponent would give, with one deviation: entries
 * more than about 2^1000 below the largest entry of their node's vector (before the scale: the
 * products of the children's scaled messages) may flush to zero.  Posterior probability of the
 * reconstruction: exp(log_joint[i] - log-likelihood of site i).
 * A site's result depends on the site alone: not on the other sites of its tile or batch, not on
 * the launch shape.  Batches and trees: those of rt_sites_sample_states (2..128 states; dense, state
 * and mask uploads; observed internal nodes; per-edge P).  RT_ERR_INVALID: states NULL, a batch of
 * another model, no transitions yet.  RT_ERR_UNSUPPORTED: what rt_sites_sample_states refuses (a
 * partitioned batch, a "rescale" batch, a generic-kernel batch, a tree deeper than the fast kernels
 * take, nnodes < 2), more than 96 GB of scratch, and for n > 4 a tree of more than
 * RT_MAX_SAMPLE_NODES nodes (the states of a tile live in LDS).  Synchronous; only states,
 * log_joint and status cross PCIe; nothing of the batch is written: it keeps its kernel,
 * log-likelihoods, status, totals and multi results.                                            */
int rt_sites_map_states(rt_model *model, rt_sites *sites, int recompute_transitions,
            uint8_t *states      /* [nsites][nnodes], preorder index */,
            double  *log_joint   /* [nsites] or NULL */,
            int32_t *status      /* [nsites] or NULL */);
/* Stochastic mappings (Nielsen 2002; the uniformization sampler of Hobolth & Stone 2009) of every
 * branch for every site of a RESIDENT batch: ndraws independent, exact draws of a substitution
 * history given the observations, each reduced on the device to the linear statistics of
 * rt_sites_branch_expectations.  coefs f64[n_coefs][n][n], 1..RT_MAX_BRANCH_COEFS matrices E with
 * the meaning they have there (E[c][d], c != d: the weight of one c -> d change; E[c][c]: the
 * weight of a unit of time in c).  Arrays are keyed by the child's preorder index v of the edge,
 * the root's slot is 0:
 *   states[d][i][v]     uint8   the node states of draw d: exactly those of rt_sites_sample_states
 *                               for the same (seed, first_draw, ndraws), bit for bit
 *   values[d][i][v][c]  f64     the statistic c of the sampled path on the edge above v
 *   counts[d][i][v][2]  int32   {uniformized events k, real changes} of that path
 *   means[i][v][c]      f64     (sum_d values[d][i][v][c]) / ndraws, summed on the device in draw
 *                               order: the same bits whether or not values is asked for
 *   status[i]           int32   OR-ed over the draws: RT_SITE_ZERO_PROB and 2 as
 *                               rt_sites_sample_states; 4: an edge whose event-count weights have
 *                               no positive finite total
 * Each output may be NULL; only those given cross PCIe.  The rule, per draw d, site i and edge
 * above v with rate matrix Q_v and length t_v, the parent having drawn state a and v state b:
 *   constants  mu = max_c(-Q_v[c][c]), R = I + Q_v / mu (R = I if mu = 0), lam = mu t_v (a lam
 *              that is not positive counts as 0), K_v = ceil(lam + 10 sqrt(lam) + 20),
 *              pois[0] = exp(-lam) (1 if lam = 0), pois[k] = pois[k-1] * lam / k.
 *   uniforms   ub(j) = philox_uniform(seed, first_draw + d, 2^63 + (i * nnodes + v) * 2048 + j)
 *              (the generator of rt_sites_sample_states; its node-state draws use indices below
 *              2^63, so nsites * nnodes < 2^52 is required).
 *   1. k among 0..K_v with weights pois[k] * (R^k)[a][b] and ub(0), by the pick rule of
 *      rt_sites_sample_states: the first index with a positive weight whose cumulative weight
 *      exceeds u * total, the last positive one if rounding leaves none.  lam = 0 gives k = 0.
 *   2. x_0 = a, x_k = b and for i = 1 .. k-1 in turn x_i among the states c with weights
 *      R[x_{i-1}][c] * (R^{k-i})[c][b] and ub(i), by the same rule (x_i = b if no weight is
 *      positive, which only underflow can cause).
 *   3. e_l = -log1p(-ub(1024 + l)), l = 0..k; the time spent in x_l is dt_l = t_v e_l / sum(e)
 *      (normalised exponentials are the spacings of k sorted uniforms; if every e_l is 0 the
 *      whole length is spent in x_0).
 *   4. values[c] = sum_l E_c[x_l][x_l] dt_l + sum_{i : x_i != x_{i-1}} E_c[x_{i-1}][x_i],
 *      counts = {k, the number of i with x_i != x_{i-1}}.
 * (The kernels sum weights in chunks of four and scale the dwell sum once by t_v / sum(e): sums
 * agree with sequential ones to rounding.)  A node without a state (255) has values and counts 0
 * on the edge above it and on those below; so has an edge of status 4.  A draw depends on (seed,
 * first_draw + d, site, node) and the numbers alone: draws [f, f + k) of one call equal a call
 * with first_draw = f.  The mean over the draws converges to rt_sites_branch_expectations.
 * Batches and trees: those of rt_sites_sample_states (2..128 states, every observation kind,
 * per-edge rate matrices).  The rates must come from rt_model_set_rates: RT_ERR_INVALID for
 * spectral rates or transitions set directly (on a model that never had rates, or after them with
 * recompute_transitions == 0), as for ndraws < 1, no coefficient matrix, a batch of another model.  RT_ERR_UNSUPPORTED: what rt_sites_sample_states refuses, more than
 * RT_MAX_BRANCH_COEFS matrices, more than 96 GB of scratch, an edge with K_v >
 * RT_MAX_MAPPING_EVENTS (checked before anything is launched).  The per-draw outputs pass through
 * the device in chunks: scratch grows with ndraws by the node states only.  Synchronous; the
 * batch keeps its kernel, log-likelihoods, status and totals.                                  */
#define RT_MAX_MAPPING_EVENTS 512
int rt_sites_sample_mappings(rt_model *model, rt_sites *sites, int recompute_transitions,
            uint64_t seed, uint64_t first_draw, int64_t ndraws,
            int64_t n_coefs, const double *coefs /* f64[n_coefs][n][n] */,
            uint8_t *states  /* [ndraws][nsites][nnodes] or NULL */,
            double *values   /* [ndraws][nsites][nnodes][n_coefs] or NULL */,
            int32_t *counts  /* [ndraws][nsites][nnodes][2] or NULL */,
            double *means    /* [nsites][nnodes][n_coefs] or NULL */,
            int32_t *status  /* [nsites] or NULL */);
/* weights f64[nsites] (copied to the device) or NULL = every site counts once           */
int rt_sites_set_weights(rt_sites *sites, const double *weights);
/* loglik f64[nsites] (-inf where status has RT_SITE_ZERO_PROB),
 * status int32[nsites]; either may be NULL.  What the last rt_prune / rt_step
 * of the batch wrote (or its clone source's); RT_ERR_INVALID for a batch that
 * no pruning kernel has written yet.                                        */
int rt_sites_get_logliks(rt_sites *sites, double *loglik, int32_t *status);
/* totals[0] = sum of log-likelihoods over sites with non-zero likelihood,
 * totals[1] = number of zero-probability sites, totals[2] = number of sites;
 * all three are 0 for a batch that was never pruned.                        */
int rt_sites_get_totals(rt_sites *sites, double totals[3]);

/* ---- 2b. K rate sets against one resident batch in a single step ----------
 *
 * A finite-difference gradient, a line search, a multi-start or a site-class mixture evaluates
 * the same tree and alignment under K parameter vectors.  The rate sets are a SECOND state of
 * the model, independent of the one rt_model_set_rates owns: their own rate matrices, branch
 * lengths and K transition tables in every layout the pruning kernels read.  Nothing below
 * changes the model's own transitions or a batch's own kernel, log-likelihoods, status or totals.
 *
 * rt_model_set_rate_sets: Q f64[K][nq][n][n], node_q int64[nnodes] shared by all sets (NULL: every
 *   edge uses matrix 0 of its set), t f64[K][nnodes].  Argument checks as rt_model_set_rates, and
 *   1 <= K <= RT_MAX_RATE_SETS.  The exponentials of all K (nnodes - 1) edges are computed in ONE
 *   launch; set k's matrices are bit for bit those of rt_model_set_rates(Q[k], nq, node_q, t[k]).
 *   Buffers are allocated on first use and grow with K.
 * rt_step_multi: (recompute_transitions != 0: those exponentials again from the resident rate
 *   sets,) then the batch is pruned once per set and K batch sums are reduced.  Asynchronous on the
 *   context's stream; a pending deferred reduction of the context is flushed first and nothing is
 *   deferred by this call.  Every batch rt_sites_create makes.  RT_ERR_INVALID without rate sets.
 * rt_sites_get_multi_logliks: loglik f64[K][nsites], status int32[K][nsites] of the last
 *   rt_step_multi (either may be NULL); set k's slice has the bits a separate rt_model_set_rates +
 *   rt_step with set k leaves in rt_sites_get_logliks.
 * rt_sites_get_multi_totals: totals f64[K][3], totals[k] with the meaning and the bits of
 *   rt_sites_get_totals after a separate step with set k; weighted_sums f64[K] (or NULL),
 *   weighted_sums[k] = sum_i w_i loglik[k][i] over the sites of non-zero likelihood, w from
 *   rt_sites_set_weights at the time of the step (default 1), reduced on the device in a fixed
 *   order (what a pattern-compressed alignment needs).
 * rt_sites_multi_mixture: per site log sum_k c_k exp(loglik[k][i]) with the maximum taken out;
 *   sets with c_k = 0 or zero likelihood are skipped, a site where none remains gets -inf and
 *   RT_SITE_ZERO_PROB.  totals as rt_sites_get_totals, with the site weights applied to
 *   totals[0] (the weights of the time of this call, not of the step).  class_weights f64[K] finite, >= 0, not all zero.  loglik, status and totals may
 *   each be NULL.  Synchronous; two calls return the same bits.
 * The getters and the mixture synchronise; they return RT_ERR_INVALID before any rt_step_multi
 * of the batch and after the number of rate sets changed (until the next rt_step_multi).
 * rt_sites_multi_kernel_name: the batch's kernel plus ",loop" (one launch per set) or ",multi"
 *   (one launch for all sets); "" before the first rt_step_multi.  RAOTEH_MULTI=loop forces the
 *   loop form.                                                                            */
#define RT_MAX_RATE_SETS 64
int rt_model_set_rate_sets(rt_model *model, int64_t K, const double *Q, int64_t nq,
            const int64_t *node_q, const double *t);
int rt_step_multi(rt_model *model, rt_sites *sites, int recompute_transitions);
int rt_sites_get_multi_logliks(rt_sites *sites, double *loglik, int32_t *status);
int rt_sites_get_multi_totals(rt_sites *sites, double *totals, double *weighted_sums);
int rt_sites_multi_mixture(rt_sites *sites, const double *class_weights, double *loglik,
            int32_t *status, double totals[3]);
const char *rt_sites_multi_kernel_name(const rt_sites *sites);

/* ---- 2c. partitioned likelihood: each site under its own rate set, one pruning launch ------
 *
 * Codon positions, genes, rate categories fixed per column, or one compound process per
 * alignment column (examples/p53/liwen.py:599-650): site i is evaluated under rate set
 * site_set[i] of rt_model_set_rate_sets (section 2b: the K transition tables of one exponential
 * launch).  Neither K sub-batches with K x (rt_model_set_rates + rt_step) nor rt_step_multi on
 * everything (K times the arithmetic) is needed.
 *
 * rt_partition_plan: the resident order of such a batch, host only (no context).  A granule is
 *   `granule` consecutive resident sites that share one copy of the tables in the kernel that
 *   runs: 16 in the matrix-pipe layout (n > 4), the workgroup's span of sites in the lane layout.
 *   The sites are sorted by set (stable counting sort: a set's sites keep the caller's order),
 *   every set's run is padded up to a multiple of the granule by repeating the run's last real
 *   site (valid data, no spurious zero-probability status); an empty set has an empty run.
 *   site_set int32[nsites]; *padded receives the number of slots; with every array NULL that is
 *   all.  Otherwise `capacity` >= *padded slots (nsites + nsets * (granule - 1) always holds
 *   them) and each array given is filled: order int64[padded] (source site of every slot),
 *   slot_of_site int64[nsites] (the slot holding site i itself), is_pad uint8[padded],
 *   granule_set int32[padded / granule], run_begin int64[nsets + 1] (set k's run is the slots
 *   [run_begin[k], run_begin[k + 1])).  RT_ERR_INVALID: a set index outside 0..nsets-1, sizes
 *   below 1, a capacity too small.
 * rt_sites_create_partitioned: rt_sites_create (same nsites, kind, nobs, obs_nodes, data: all
 *   three observation kinds; the host data is site-major, so the permutation is a row gather
 *   before the packing) plus site_set int32[nsites] and nsets.  The batch is resident in the
 *   planner's order and runs the interpreter kernels only (no tree-specialised kernel is
 *   compiled): in the lane family the register-ring form, above 4 states the one-wave and the
 *   split-M forms a "jit" = 0 batch runs -- leaf states and root halves included -- with the
 *   tables of granule g taken from set granule_set[g] (one scalar load and add per wave; tiles
 *   of different sets share workgroups).  RT_ERR_UNSUPPORTED with a message: the "rescale" or
 *   "force_generic" option set, a tree the fast kernels do not take, nsets outside
 *   1..RT_MAX_RATE_SETS.  RT_ERR_INVALID: a set index outside 0..nsets-1, and what
 *   rt_sites_create refuses.
 * rt_step_partitioned: (recompute_transitions != 0: the K (nnodes - 1) exponentials again from
 *   the resident rate sets, as rt_step_multi,) ONE pruning launch, then per set a fixed-order
 *   two-stage sum over the resident results with the pads masked, the batch totals and the
 *   gather into caller order.  Asynchronous on the context's stream; a pending deferred reduction
 *   of the context is flushed first and nothing is deferred.  RT_ERR_INVALID: an ordinary batch;
 *   fewer rate sets resident in the model than the batch's nsets (none at all included; sets
 *   beyond nsets are simply not used).
 * On a partitioned batch
 *   rt_sites_get_logliks   returns caller order, never a pad;
 *   rt_sites_set_weights   takes caller order (f64[nsites]);
 *   rt_sites_get_totals    gives the totals over the real sites;
 *   rt_sites_get_partition_totals: totals f64[nsets][3], totals[k] with the meaning of
 *     rt_sites_get_totals over set k's sites ({0, 0, 0} for an empty set); weighted_sums
 *     f64[nsets] (or NULL), weighted_sums[k] = sum_i w_i loglik[i] over set k's sites of non-zero
 *     likelihood, w from rt_sites_set_weights at the time of the step (default 1).  Two steps
 *     give the same bits (the shape of the sums depends on the plan alone);
 *   rt_sites_kernel_name   ends in ",partitioned" after a step.
 *   The getters synchronise; they return RT_ERR_INVALID before the first rt_step_partitioned
 *   (rt_sites_get_totals: zeros) and after the model's number of rate sets changed, until the
 *   next rt_step_partitioned (the epoch of section 2b).
 * rt_sites_branch_expectations_partitioned: rt_sites_branch_expectations (above) for a
 *   partitioned batch, with one change: on the edge above node v, site i uses Q, t, P and the
 *   derivative G of its own set k = site_set[i] of rt_model_set_rate_sets, Q[k][node_q[v]] and
 *   t[k][v].  The per-branch map of expected changes when the columns do not share one rate set
 *   (the per-column compound process above), and with C = Q[k] the analytic gradient in the
 *   branch lengths of every set, t[k][v] d log L_i / d t[k][v], for a tree shared by partitions.
 *     coefs           f64[n_coefs][n][n] shared by all sets (coefs_per_set == 0), or
 *                     f64[nsets][n_coefs][n][n], set k's matrices at [k] (coefs_per_set != 0: the
 *                     gradient needs diag(Q[k]) on the diagonal); 1 <= n_coefs <=
 *                     RT_MAX_BRANCH_COEFS, every entry finite
 *     values          f64[nsites][nnodes][n_coefs] in CALLER order, real sites only, never a
 *                     pad; the root's slot is 0; a site of zero likelihood under its set: zeros
 *     edge_sums       f64[nnodes][n_coefs]: the sum over all real sites, weighted by
 *                     rt_sites_set_weights (caller order); the per-set rows added in set order
 *     set_edge_sums   f64[nsets][nnodes][n_coefs]: the same over set k's sites; zeros for an
 *                     empty set
 *     status          int32[nsites] in caller order, as rt_sites_branch_expectations:
 *                     RT_SITE_ZERO_PROB, or 2 (a zero denominator)
 *   Each output may be NULL; only what is given crosses PCIe.  The sums are reduced on the device
 *   per (set, node, matrix) over the set's run in two stages whose shape depends on the plan
 *   alone, with the pad slots skipped (a pad repeats a real site: weighting it out would not do).
 *   recompute_transitions != 0: the K (nnodes - 1) exponentials again from the resident rate
 *   sets, as rt_step_partitioned; no earlier rt_step_partitioned is needed.  The derivatives of
 *   all K (nnodes - 1) edges come from one launch of the derivative route per coefficient matrix;
 *   every edge's derivative and every site's arithmetic are those of rt_sites_branch_expectations
 *   under that site's set, bit for bit (per-set scratch grows with K; no chunking over the sets:
 *   a call whose scratch passes 96 GB is refused).  Synchronous; two calls return the same bits.
 *   The batch's log-likelihoods, status, totals, per-set totals and kernel name, the model's own
 *   transitions and its rate sets keep what they had.  RT_ERR_INVALID: an ordinary batch; fewer
 *   rate sets resident in the model than the batch's nsets; a batch of another model; n_coefs < 1
 *   or coefs NULL; a coefficient that is not finite.  RT_ERR_UNSUPPORTED: more than
 *   RT_MAX_BRANCH_COEFS matrices; more than 96 GB of scratch.
 * rt_sites_branch_profiles_partitioned, rt_sites_nni_scores_partitioned: rt_sites_branch_profiles
 *   and rt_sites_nni_scores (above) for a partitioned batch.  Site i with k = site_set[i] uses
 *   Q[k][node_q[v]], t[k][v] and P of its own set on every edge; under set k the moved tree of an
 *   NNI keeps every moved subtree's own edge of set k.  Trial lengths are FACTORS, as in section 2d:
 *   at point g the edge above v has length factors[v][g] * t[k][v] under set k -- the same meaning
 *   whether the sets differ in Q or in t, and what a shared tree with one multiplier per partition
 *   needs.
 *     factors         f64[nnodes][npoints], 1 <= npoints <= RT_MAX_PROFILE_POINTS, finite, >= 0
 *                     (row 0, and for the NNI scores the rows of nodes without a move, are ignored);
 *                     rt_sites_nni_scores_partitioned: NULL with npoints == 1 is the plain swap
 *     values          f64[nsites][nnodes][npoints] / f64[nsites][nmoves][npoints] in CALLER order,
 *                     real sites only: log L_i(trial) - log L_i.  -inf where a live site has
 *                     likelihood 0 at the trial; a site of zero likelihood under its set: zeros
 *                     (RT_SITE_ZERO_PROB).  Profiles: the root's row is 0, and where the resident
 *                     t[k][v] == 0 (v != root) row v is NaN for the live sites of set k.  NNI: the
 *                     moves of rt_model_nni_moves, division-free and exact as
 *                     rt_sites_nni_scores, no NaN rows
 *     set_sums        f64[nsets][rows][npoints]: the sum of w_i values over the real sites of set k
 *                     (rt_sites_set_weights, caller order; pads skipped; a site of weight 0 adds
 *                     nothing even at -inf); zeros for an empty set; profiles: NaN in row v where
 *                     t[k][v] == 0 and set k has a site
 *     sums            f64[rows][npoints]: the per-set rows added in set order
 *     status          int32[nsites] in caller order, as the single-set calls
 *   Each output may be NULL; only what is given crosses PCIe.  The trial matrices of all sets with
 *   a site come from ONE launch of the sets' exponential (its variant chosen by one set's count: a
 *   matrix does not depend on K), the pass runs once with every 16-site tile (n <= 4: every wave)
 *   under the tables of its granule's set, and the sums are reduced on the device in two stages
 *   whose shape depends on the plan alone: two calls return the same bits.  The NNI scores are
 *   made in chunks of moves as rt_sites_nni_scores makes them.  nmoves == 0: RT_OK, only status is
 *   written.  Synchronous; the batch's log-likelihoods, status and totals, the model's transitions
 *   and rate sets keep what they had.  RT_ERR_INVALID: fewer rate sets resident in the model than
 *   the batch's nsets; a batch of another model; npoints outside 1..RT_MAX_PROFILE_POINTS; factors
 *   NULL (NNI: with npoints != 1); a factor that is negative or not finite.
 *   RT_ERR_UNSUPPORTED: an ordinary batch, a "rescale" or generic-kernel batch, a tree deeper than the
 *   fast kernels take, more than 96 GB of scratch.  RT_ERR_SINGULAR: a failed exponential.
 * rt_sites_spr_scores_partitioned, rt_sites_placements_partitioned: rt_sites_spr_scores and
 *   rt_sites_placements (above) for a partitioned batch, every site under its own set as for the
 *   two reads before.  SPR: the moves of rt_model_spr_moves(model, radius); under set k the edge
 *   above y is cut at fractions[r] of the set's own resident length t[k][y] and the pruned subtree
 *   keeps its own edge of set k.  Placements: the cut edge likewise; the pendant edge has length
 *   pendant_scale[k] * pendant[j] under Q[k][node_q[v]].
 *     fractions       f64[nfractions], 1 <= nfractions <= RT_MAX_PLACE_FRACTIONS, in [0, 1]
 *     pendant         f64[npendant], 1 <= npendant <= RT_MAX_PLACE_PENDANT, finite, >= 0;
 *                     2 nfractions + npendant <= 32
 *     pendant_scale   f64[the model's sets], finite, >= 0; NULL: ones (as
 *                     rt_sites_placements_mixture)
 *     queries         RT_OBS_DENSE f64[nqueries][nsites][n] or RT_OBS_STATE uint8[nqueries][nsites]
 *                     in CALLER order over the real sites (the caller never sees slots or pads:
 *                     the library brings a chunk's queries to slot order on the device)
 *     values          f64[nsites][nmoves][nfractions] /
 *                     f64[nsites][nqueries][nnodes][nfractions][npendant] in CALLER order, real
 *                     sites only (the root's rows are 0): -inf where a live site has likelihood 0
 *                     after the change; a site of zero likelihood under its set: zeros
 *                     (RT_SITE_ZERO_PROB).  Division-free and exact at t[k][v] == 0: no NaN rule
 *     set_sums        f64[nsets][rows]: as above (a site of weight 0 adds nothing even at -inf;
 *                     zeros for an empty set);  sums f64[rows]: the per-set rows added in set order
 *     status          int32[nsites] in caller order
 *   Each output may be NULL; only what is given crosses PCIe.  The matrices of all sets with a
 *   site (both halves of every cut edge, the pendant edges) come from ONE launch of the sets'
 *   exponential, their fragments are packed once, and per chunk ONE launch of every kernel runs with
 *   every 16-site tile (n <= 4: every wave) under the tables of its granule's set.  Grid limits,
 *   chunks (RAOTEH_SPR_CHUNK_BYTES over pruned nodes, RAOTEH_PLACE_CHUNK_BYTES over queries), the
 *   96 GB cap and nmoves == 0 (RT_OK, only status is written) are those of the single-set calls.
 *   Synchronous; two calls return the same bits, chunked or not; the batch's log-likelihoods, status
 *   and totals, the model's transitions and rate sets keep what they had.  RT_ERR_INVALID: fewer
 *   rate sets resident in the model than the batch's nsets; a batch of another model; counts,
 *   fractions, pendant lengths or scales out of range; NULL fractions, pendant or queries; a
 *   query_kind that is no observation kind.  RT_ERR_UNSUPPORTED: an ordinary batch, a "rescale" or
 *   generic-kernel batch, RT_OBS_MASK queries, more than 96 GB of scratch.  RT_ERR_SINGULAR: a
 *   failed exponential.
 * Everything else refuses a partitioned batch with RT_ERR_UNSUPPORTED and leaves it untouched:
 *   rt_prune, rt_step, rt_step_multi, rt_sites_clone, rt_expect_step, rt_sites_posteriors,
 *   rt_sites_branch_expectations, rt_sites_branch_profiles, rt_sites_sample_states,
 *   rt_sites_map_states, rt_sites_sample_mappings, rt_sites_branch_expectations_mixture,
 *   rt_sites_branch_profiles_mixture, rt_sites_nni_scores_mixture, rt_sites_nni_scores,
 *   rt_sites_spr_scores, rt_sites_placements and their _mixture forms, rt_allreduce_totals,
 *   rt_allreduce_totals_group.
 *                                                               */
int rt_partition_plan(const int32_t *site_set, int64_t nsites, int64_t nsets, int64_t granule,
            int64_t capacity, int64_t *order, int64_t *slot_of_site, uint8_t *is_pad,
            int32_t *granule_set, int64_t *run_begin, int64_t *padded);
int rt_sites_create_partitioned(rt_model *model, int64_t nsites, int kind, int64_t nobs,
            const int64_t *obs_nodes, const void *data, const int32_t *site_set, int64_t nsets,
            rt_sites **sites);
int rt_step_partitioned(rt_model *model, rt_sites *sites, int recompute_transitions);
int rt_sites_get_partition_totals(rt_sites *sites, double *totals, double *weighted_sums);
int rt_sites_branch_expectations_partitioned(rt_model *model, rt_sites *sites,
            int recompute_transitions, int64_t n_coefs, int coefs_per_set, const double *coefs,
            double *values, double *edge_sums, double *set_edge_sums, int32_t *status);
int rt_sites_branch_profiles_partitioned(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t npoints, const double *factors, double *values, double *sums,
            double *set_sums, int32_t *status);
int rt_sites_nni_scores_partitioned(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t npoints, const double *factors, double *values, double *sums,
            double *set_sums, int32_t *status);
int rt_sites_spr_scores_partitioned(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t radius, int64_t nfractions, const double *fractions,
            double *values, double *sums, double *set_sums, int32_t *status);
int rt_sites_placements_partitioned(rt_model *model, rt_sites *sites, int recompute_transitions,
            int64_t nqueries, int query_kind, const void *queries,
            int64_t nfractions, const double *fractions, int64_t npendant, const double *pendant,
            const double *pendant_scale, double *values, double *sums, double *set_sums,
            int32_t *status);
/* what the batch was laid out with: any pointer may be NULL; an ordinary batch gives zeros */
int rt_sites_partition_info(const rt_sites *sites, int64_t *nsets, int64_t *granule,
            int64_t *padded);

/* ---- 2d. site-class mixtures: posterior-weighted branch expectations, gradient ------------
 *
 * A site-class mixture (discrete-gamma rate categories, codon omega classes, a +I class) has the
 * site likelihood L_i = sum_k c_k L_ik over the K rate sets of rt_model_set_rate_sets (section
 * 2b gives its value).  rt_sites_branch_expectations_mixture gives what an optimiser or an EM
 * step needs beyond the value, for an ORDINARY resident batch, every site under every set:
 *     class_weights   f64[K], finite, >= 0, not all zero (the rule of rt_sites_multi_mixture)
 *     coefs           f64[n_coefs][n][n] shared by all sets (coefs_per_set == 0), or
 *                     f64[K][n_coefs][n][n], set k's matrices at [k]: layouts and meaning of
 *                     rt_sites_branch_expectations_partitioned
 *   L_ik is the site's likelihood under set k; set k is LIVE at site i when c_k > 0 and
 *   L_ik > 0.  A set that is not live is skipped entirely: nothing of it is multiplied in.  All
 *   sums over k run in set order.
 *     loglik          f64[nsites]: log sum_k c_k L_ik; -inf where no set is live
 *     class_post      f64[nsites][K]: c_k L_ik / sum_j c_j L_ij, the class posteriors (the
 *                     empirical-Bayes site classification); a site with no live set: zeros
 *     values          f64[nsites][nnodes][n_coefs]: sum_k class_post[i][k] x_k[i][v][c], x_k
 *                     exactly what rt_sites_branch_expectations computes for the site with Q, t,
 *                     P and the derivative G of set k (product and sum rounded separately: a
 *                     posterior of 1 returns x_k bit for bit); the root's slot is 0; a site
 *                     with no live set: zeros
 *     set_edge_sums   f64[K][nnodes][n_coefs]: sum_i w_i class_post[i][k] x_k[i][v][c], w from
 *                     rt_sites_set_weights (default 1)
 *     edge_sums       f64[nnodes][n_coefs]: the per-set rows added in set order
 *     class_sums      f64[K]: sum_i w_i class_post[i][k]
 *     status          int32[nsites]: RT_SITE_ZERO_PROB where no set is live; else the OR over the
 *                     LIVE sets of the 2 (a zero denominator) their passes report -- a set under
 *                     which the site has zero likelihood leaks no bit
 *   With C = Q_k (coefficients: ones off the diagonal, diag(Q_k) on it) set_edge_sums[k][v] is
 *   t[k][v] d/d t[k][v] of sum_i w_i loglik[i]; with C = dQ_k/d theta, values is d loglik[i] / d
 *   theta on each branch; class_sums[k] / c_k is the derivative in c_k.
 *   Each output may be NULL; only what is given crosses PCIe.  The sums are reduced on the device in
 *   a fixed order whose shape depends on (nsites, K, nnodes, n_coefs) alone: two calls return the
 *   same bits.  The per-set sums go over the whole batch in pieces of 4096 sites: with K = 1 and
 *   one piece edge_sums has the bits of rt_sites_branch_expectations.  Synchronous.
 *   recompute_transitions != 0: rt_model_set_rate_sets's exponentials again from the resident rate
 *   sets; no earlier rt_step_multi is needed.  The passes run set after set over one scratch for
 *   L, M and D; the unweighted x_k of all sets stay in scratch (no chunking over the sets: a call
 *   whose scratch passes 96 GB is refused).  Nothing resident changes: the batch's kernel,
 *   log-likelihoods, status and totals, its rt_step_multi results, the model's own transitions
 *   and the rate sets keep what they had.
 *   RT_ERR_INVALID: no rate sets; a batch of another model; class_weights NULL or with a negative
 *   or non-finite entry or all zero; n_coefs < 1 or coefs NULL; a coefficient that is not finite.
 *   RT_ERR_UNSUPPORTED: a partitioned batch; what rt_sites_branch_expectations refuses ("rescale",
 *   a generic-kernel batch, deep trees, nnodes < 2); more than RT_MAX_BRANCH_COEFS matrices; more
 *   than 96 GB of scratch.                                                  */
int rt_sites_branch_expectations_mixture(rt_model *model, rt_sites *sites,
            int recompute_transitions, const double *class_weights, int64_t n_coefs,
            int coefs_per_set, const double *coefs, double *values, double *edge_sums,
            double *set_edge_sums, double *class_post, double *class_sums, double *loglik,
            int32_t *status);
/* The tree-search reads under the same mixture: rt_sites_branch_profiles and rt_sites_nni_scores
 * of an ORDINARY resident batch with every site under every one of the model's K rate sets.
 *     class_weights   f64[K], as above; a set with c_k = 0 is never run and never read
 *     factors         f64[nnodes][npoints], 1 <= npoints <= RT_MAX_PROFILE_POINTS, finite, >= 0;
 *                     row 0 is ignored.  Trial lengths are FACTORS of the resident ones: at point
 *                     g, set k's edge above v takes the length factors[v][g] * t[k][v] -- the one
 *                     parametrisation that means the same for every class, whether the classes
 *                     differ in Q (Q_k = r_k Q, shared t) or in t (shared Q, t_k = r_k t)
 *   L_ik is the likelihood of site i under set k, Lambda_i = sum_k c_k L_ik the mixture
 *   likelihood, summed in set order.  A site whose Lambda_i is not positive gets
 *   RT_SITE_ZERO_PROB; its values are 0 and it adds nothing to the sums.
 * rt_sites_branch_profiles_mixture:
 *     values          f64[nsites][nnodes][npoints]:
 *                     log sum_k c_k L_ik(t[k][v] -> factors[v][g] t[k][v]) - log Lambda_i;
 *                     the root's row is 0; -inf where the mixture likelihood is 0 at the point
 *     sums            f64[nnodes][npoints]: sum_i w_i values[i][v][g], w from rt_sites_set_weights,
 *                     in a fixed order; sites of weight 0 and of zero likelihood are skipped
 *     loglik          f64[nsites]: log Lambda_i, -inf where dead (the loglik of
 *                     rt_sites_branch_expectations_mixture)
 *   As in rt_sites_branch_profiles, the row of edge v is NaN -- in values at live sites and in
 *   sums -- when a set with c_k > 0 has resident t[k][v] == 0.
 * rt_sites_nni_scores_mixture: moves and their order are those of rt_model_nni_moves;
 *     values          f64[nsites][nmoves][npoints]: log sum_k c_k L_ik(tree after the move,
 *                     t[k][v] -> factors[v][g] t[k][v]) - log Lambda_i
 *     sums            f64[nmoves][npoints], loglik f64[nsites]: as above
 *   factors == NULL: npoints must be 1, every set keeps its resident matrix on the edge above v
 *   and no exponential runs; only the rows of nodes v with a move count.  The call is exact in
 *   every term: a set with L_ik == 0 on the resident tree and L_ik > 0 on the moved one adds its
 *   term (nothing is divided by L_ik), and a resident t[k][v] == 0 gives no NaN row.  Where the
 *   result of all moves does not fit, the moves go in chunks as in rt_sites_nni_scores
 *   (RAOTEH_NNI_CHUNK_BYTES), the sets' passes again per chunk.
 * Both: each output may be NULL, only what is given crosses PCIe.  Synchronous; two calls return the
 *   same bits.  Nothing resident changes: the batch's kernel, log-likelihoods, status and totals,
 *   its rt_step_multi results, the model's own transitions and the rate sets keep what they had.
 *   recompute_transitions != 0: the sets' exponentials again from the resident rate sets; no
 *   earlier rt_step_multi is needed.  status: RT_SITE_ZERO_PROB where Lambda_i is not positive,
 *   else the OR over the sets LIVE at the site of the 2 their passes report.
 *   RT_ERR_INVALID: no rate sets; a batch of another model; bad class weights; npoints out of
 *   range, or not 1 without factors; a negative or non-finite factor in a row that counts.
 *   RT_ERR_SINGULAR: an exponential failed.  RT_ERR_UNSUPPORTED: a partitioned batch; what
 *   rt_sites_branch_profiles / rt_sites_nni_scores refuse ("rescale", a generic-kernel batch, deep
 *   trees, nnodes < 2); more than 96 GB of scratch.                          */
int rt_sites_branch_profiles_mixture(rt_model *model, rt_sites *sites, int recompute_transitions,
            const double *class_weights, int64_t npoints, const double *factors, double *values,
            double *sums, double *loglik, int32_t *status);
int rt_sites_nni_scores_mixture(rt_model *model, rt_sites *sites, int recompute_transitions,
            const double *class_weights, int64_t npoints, const double *factors, double *values,
            double *sums, double *loglik, int32_t *status);
/* rt_sites_spr_scores_mixture: rt_sites_spr_scores of an ORDINARY resident batch under the same
 * mixture.  Moves, their order, radius, fractions and the output shapes are those of
 * rt_sites_spr_scores and rt_model_spr_moves; class_weights as above (a set with c_k = 0 is never
 * run and never read).
 *     values          f64[nsites][nmoves][nfractions]:
 *                     log sum_k c_k L_ik(tree after the move at fractions[r]) - log Lambda_i, the
 *                     sum in set order; 0 at a site whose Lambda_i is not positive
 *                     (RT_SITE_ZERO_PROB; it adds nothing to the sums); -inf where the mixture
 *                     likelihood after the move is 0 at a live site
 *     sums            f64[nmoves][nfractions], loglik f64[nsites], status: exactly those of
 *                     rt_sites_nni_scores_mixture
 *   Under set k the cut edge above y has the lengths fractions[r] t[k][y] and
 *   (1 - fractions[r]) t[k][y] under Q[k][node_q[y]]: the fractions are factors of the resident
 *   length already, nothing new is parametrised.  The pruned subtree keeps set k's resident
 *   matrix on its own edge.  The call is exact in every term and nothing is divided by L_ik: a set
 *   dead on the resident tree and alive after a move adds its term; a resident t[k][y] == 0 gives
 *   no NaN row, as in rt_sites_spr_scores.
 *   Each output may be NULL.  Synchronous; two calls return the same bits, chunked or not, whatever
 *   the number of groups of pruned nodes.  Nothing resident changes.  recompute_transitions as in
 *   the other mixture reads.  Where the result of all moves does not fit, the pruned nodes go in
 *   chunks as in rt_sites_spr_scores (RAOTEH_SPR_CHUNK_BYTES), the sets' passes again per chunk.
 *   RT_ERR_INVALID: no rate sets; a batch of another model; bad class weights; fractions NULL,
 *   nfractions outside 1..RT_MAX_PLACE_FRACTIONS, a fraction outside [0, 1] or not finite; too
 *   many moves.  RT_ERR_SINGULAR: an exponential failed.  RT_ERR_UNSUPPORTED: a partitioned batch;
 *   what rt_sites_spr_scores refuses ("rescale", a generic-kernel batch, deep trees, nnodes < 2);
 *   more than 96 GB of scratch.                                              */
int rt_sites_spr_scores_mixture(rt_model *model, rt_sites *sites, int recompute_transitions,
            const double *class_weights, int64_t radius, int64_t nfractions,
            const double *fractions, double *values, double *sums, double *loglik,
            int32_t *status);
/* rt_sites_placements_mixture: rt_sites_placements of an ORDINARY resident batch under the same
 * mixture.  Queries, their kinds (RT_OBS_DENSE, RT_OBS_STATE; RT_OBS_MASK is not taken), the grid
 * limits (RT_MAX_PLACE_FRACTIONS, RT_MAX_PLACE_PENDANT, 2 nfractions + npendant <= 32) and the
 * output shapes are those of rt_sites_placements; class_weights as above.
 *     pendant_scale   f64[K], finite and >= 0, or NULL for ones: under set k the query at pendant
 *                     point tau_j hangs on an edge of length pendant_scale[k] * tau_j under the
 *                     cut edge's rate matrix of set k, Q[k][node_q[v]].  Where the classes differ
 *                     in Q (Q_k = r_k Q over a shared t) ones is right; where they share Q and
 *                     differ in t (t_k = r_k t) pass r_k, so that the new edge is stretched as
 *                     the resident ones are.  The entry of a set with c_k = 0 is not read.
 *     values          f64[nsites][nqueries][nnodes][nfractions][npendant]:
 *                     log sum_k c_k L_ik(tree with the query placed) - log Lambda_i, the sum in set
 *                     order; the root's rows are 0; 0 at a site whose Lambda_i is not positive;
 *                     -inf where the mixture likelihood with the query placed is 0 at a live site
 *     sums            f64[nqueries][nnodes][nfractions][npendant], loglik f64[nsites], status:
 *                     exactly those of rt_sites_nni_scores_mixture
 *   Under set k the cut edge above v has the lengths fractions[r] t[k][v] and
 *   (1 - fractions[r]) t[k][v] under Q[k][node_q[v]].  Exact in every term, nothing is divided by
 *   L_ik; a resident t[k][v] == 0 gives no NaN row.  Each output may be NULL.  Synchronous; two
 *   calls return the same bits, chunked or not.  Nothing resident changes.  recompute_transitions
 *   as in the other mixture reads.  Where the result of all queries does not fit, the queries go
 *   in chunks as in rt_sites_placements (RAOTEH_PLACE_CHUNK_BYTES); every chunk runs the sets'
 *   passes and fields again (the scratch holds one set's field at a time).
 *   RT_ERR_INVALID: no rate sets; a batch of another model; bad class weights; nqueries < 1; a
 *   query_kind that is none of the three; queries, fractions or pendant NULL; a count out of
 *   range; a fraction outside [0, 1], a pendant length or a pendant_scale entry that is negative
 *   or not finite.  RT_ERR_SINGULAR: an exponential failed.  RT_ERR_UNSUPPORTED: RT_OBS_MASK
 *   queries; a partitioned batch; what rt_sites_placements refuses ("rescale", a generic-kernel
 *   batch, deep trees, nnodes < 2); more than 96 GB of scratch.               */
int rt_sites_placements_mixture(rt_model *model, rt_sites *sites, int recompute_transitions,
            const double *class_weights, int64_t nqueries, int query_kind, const void *queries,
            int64_t nfractions, const double *fractions, int64_t npendant, const double *pendant,
            const double *pendant_scale, double *values, double *sums, double *loglik,
            int32_t *status);

/* ---- 3. multi-GPU: one process per GPU, RCCL over xGMI ------------------- */

/* rank 0 calls rt_comm_unique_id and ships the 128 bytes to the other ranks
 * by any host channel; then every rank calls rt_comm_init.                  */
/* rt_comm_available: RT_OK iff librccl loads (dlopen + symbols only, no GPU, no
 * network) -- the ranks agree on it over their host channel BEFORE any rank enters
 * rt_comm_init, where a missing peer would be a hang.                        */
int rt_comm_available(void);
int rt_comm_unique_id(unsigned char id[128]);
int rt_comm_init(rt_ctx *ctx, int nranks, int rank, const unsigned char id[128]);
int rt_comm_destroy(rt_ctx *ctx);
/* ncclAllReduce(sum, f64, 3) of the totals of `sites`, in place on the
 * device, asynchronously on the context's communication stream (the next
 * rt_prune of the batch and rt_sites_get_totals wait for it).               */
int rt_allreduce_totals(rt_ctx *ctx, rt_sites *sites);
/* The totals of `count` batches in one collective (3 * count doubles) when the
 * batches were created one after the other (their totals are then neighbours in
 * device memory), else one collective each.                                  */
int rt_allreduce_totals_group(rt_ctx *ctx, rt_sites **sites, int64_t count);

/* ---- 4. Rao-Teh sweep core: ragged batches of trees, one shared matrix --------
 * One sweep of the Rao-Teh sampler (_sampler.py:366-390) re-samples the states of a
 * chunk tree (_graph_transform.py:298-375) per chain, all with the SAME uniformized
 * transition matrix P = I + Q / omega (_sample_mjp_dense.py:72-114); the topologies
 * differ from chain to chain and from sweep to sweep.  A forest is the concatenation
 * of `ntrees` such trees:
 *   tree_node_offset int64[ntrees + 1]   tree k owns nodes [off[k], off[k+1]), numbered
 *       in ITS OWN DFS preorder (local index 0 = its root)
 *   tree_csr_indptr  int64[total + ntrees]  tree k's indptr (nnodes_k + 1 entries, as
 *       _density.digraph_to_bool_csr returns it) starts at off[k] + k
 *   tree_csr_indices int64[total - ntrees]  tree k's child indices (nnodes_k - 1 local
 *       preorder indices) start at off[k] - k
 *   P f64[n][n]: an entry that is exactly zero is a structural zero; n <= 128
 *   allowed_sets (in / out): for n <= 64 uint64[total], bit s = state s allowed at the
 *       node; for 64 < n <= 128 uint64[total][2], state s = bit s % 64 of word s / 64 (the
 *       layout of RT_OBS_MASK).  Bits at or above n are ignored on input and, for
 *       n > 64, zero on output.
 *
 * rt_forest_passes: pyfelscore.mcy_get_node_to_pset then pyfelscore.get_node_to_set
 * with a boolean CSR of P (_mcy.py:139-181; un-accelerated twins _mcy.py:396-470,
 * _mc0.py:89-138), in place on allowed_sets, then (subtree_probability != NULL) the
 * upward pass with that matrix on every edge (_mcy.py:611-682): f64[total][n], every
 * entry written.                                                                  */
int rt_forest_passes(rt_ctx *ctx, int64_t n, int64_t ntrees,
            const int64_t *tree_node_offset, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *P,
            uint64_t *allowed_sets, double *subtree_probability);
/* pyfelscore.mcy_get_node_to_pset (_mcy.py:158,259; un-accelerated twin _mcy.py:396-470)
 * and pyfelscore.get_node_to_set (_mcy.py:168; twin _mc0.py:89-138) with the reference's own
 * arguments: ONE tree (children CSR in preorder index space), the transition matrix as a
 * boolean CSR shared by every edge (trans_csr_indptr int64[n + 1], trans_csr_indices the
 * column indices of the nonzero entries of each row, _mcy.py:148-149), state_mask
 * int64[nnodes][n] 0/1 updated in place.  tmp_state_mask int64[n] is the scratch row
 * pyfelscore asks for (may be NULL).  n <= 128 (the mask stays one int64 per state;
 * above 64 states the two-word set kernels of rt_forest_passes run underneath).      */
int rt_mcy_get_node_to_pset(rt_ctx *ctx, int64_t nnodes, int64_t n,
            const int64_t *tree_csr_indices, const int64_t *tree_csr_indptr,
            const int64_t *trans_csr_indices, const int64_t *trans_csr_indptr,
            int64_t *state_mask);
int rt_get_node_to_set(rt_ctx *ctx, int64_t nnodes, int64_t n,
            const int64_t *tree_csr_indices, const int64_t *tree_csr_indptr,
            const int64_t *trans_csr_indices, const int64_t *trans_csr_indptr,
            int64_t *state_mask, int64_t *tmp_state_mask);
/* The same passes followed by _sample_mc0_dense.resample_states (:53-98) for every
 * tree: root ~ root_distn * L[root] (root_distn NULL = weights of one), child ~
 * P[parent's state] * L[child].  Draws come from Philox-4x32-10 keyed by `seed` with
 * counter (sweep, global node index): the same (seed, sweep, forest) gives the same
 * states whatever the launch shape.  states int32[total] out (-1 where status != 0),
 * status int32[ntrees] out: 1 = the tree has zero likelihood (the reference raises
 * StructuralZeroProb / NumericalZeroProb, _sample_mc0_dense.py:57-62), 2 = a
 * non-root node had no state of positive weight.  subtree_probability (optional,
 * f64[total][n]) receives the upward messages the draws were made from.           */
int rt_forest_resample_states(rt_ctx *ctx, int64_t n, int64_t ntrees,
            const int64_t *tree_node_offset, const int64_t *tree_csr_indices,
            const int64_t *tree_csr_indptr, const double *P, const double *root_distn,
            uint64_t *allowed_sets, uint64_t seed, uint64_t sweep, int32_t *states,
            int32_t *status, double *subtree_probability);
/* The same with the topologies as ONE local parent index per node instead of the CSR
 * (tree_parent int32[total]: -1 at each tree's node 0, else an index below the node's
 * own) -- what a batched sweep has at hand after cutting its histories into chunks
 * (raoteh_amd/_sampler.py; the chunk trees of _graph_transform.py:298-375 come out in
 * that order), without a pass over the forest to build child lists.              */
int rt_forest_resample_states_parents(rt_ctx *ctx, int64_t n, int64_t ntrees,
            const int64_t *tree_node_offset, const int32_t *tree_parent, const double *P,
            const double *root_distn, uint64_t *allowed_sets, uint64_t seed, uint64_t sweep,
            int32_t *states, int32_t *status);

/* ---- 5. Rao-Teh sweeps with the histories resident on the device ---------------
 * A batch of `nchains` independent chains on ONE base tree (nnodes <= 1024 nodes in an
 * order with parent[v] < v, parent[0] = -1; branch_lengths[v] = length of the edge above
 * v) under ONE rate matrix, given as the caller computes it for the reference's sampler
 * (_sampler.py:344-357): P = I + Q / omega (f64[n][n]), poisson_rates[s] = omega - q_s,
 * root_distn (f64[n] or NULL = weights of one), node_masks uint64[nchains][nnodes]
 * allowed-state sets of the base nodes -- for 64 < n <= 128 uint64[nchains][nnodes][2],
 * state s = bit s % 64 of word s / 64 as in section 4; bits at or above n are ignored;
 * n <= 128.  A history is a run of rows (edge = index of the
 * edge's lower node, length, state) sorted by (edge, position); rt_chains_create finds a
 * first feasible one by bisecting the edges (_sampler.py:563-648; RT_ERR_ZERO_PROB when
 * some chain has none), rt_chains_sweep runs whole sweeps (_sampler.py:366-390: Poisson
 * events, chunk trees, posterior draw of the chunk states, removal of self transitions)
 * without the rows leaving the device.  Draws are counter-based: (seed, batch) fixes
 * every history.  rt_chains_get_statistics: per chain the time spent in each state
 * (f64[nchains][n]), the transition counts (int64[nchains][n][n]) and the states of the
 * base nodes (int32[nchains][nnodes]) of the CURRENT histories; any pointer may be NULL.
 * rt_chains_get_rows: the histories themselves (chain_offset int64[nchains + 1], then
 * `capacity` >= total rows entries of edge / length / state; rt_chains_get_sizes tells
 * the total).                                                                        */
typedef struct rt_chains rt_chains;
int rt_chains_create(rt_ctx *ctx, int64_t nnodes, const int32_t *parent,
            const double *branch_lengths, int64_t n, const double *P,
            const double *poisson_rates, const double *root_distn, int64_t nchains,
            const uint64_t *node_masks, uint64_t seed, rt_chains **out);
int rt_chains_sweep(rt_chains *chains, int64_t nsweeps);
int rt_chains_get_sizes(const rt_chains *chains, int64_t *rows, int64_t *chunks,
            int64_t *sweeps);
int rt_chains_get_statistics(rt_chains *chains, double *dwell, int64_t *transitions,
            int32_t *node_states);
int rt_chains_get_rows(rt_chains *chains, int64_t capacity, int64_t *chain_offset,
            int32_t *edge, double *length, int32_t *state);
/* Metropolis-Hastings on top of the sweeps (_sampler.py:393-551): rt_chains_snapshot keeps
 * a copy of the current histories; after further sweeps rt_chains_restore gives the chains
 * with reject[c] != 0 (uint8[nchains]) their snapshot back, the others keep what they have. */
int rt_chains_snapshot(rt_chains *chains);
int rt_chains_restore(rt_chains *chains, const uint8_t *reject);
int rt_chains_destroy(rt_chains *chains);

#ifdef __cplusplus
}
#endif
#endif /* RAOTEH_HIP_H */
