// What the reads of a RESIDENT batch share.  Host:
//   post_pass (post_open .. post_up), one description of such a call -- its checks, the common
//       pieces of its scratch, the upward pass with L (and M) of every step stored (the plan of the
//       scratch and the dispatch over the kernels' template arguments: common.h): posterior.hip,
//       branch_expect.hip, sample.hip, mapping.hip, map_states.hip and the tree-search reads
//       branch_profile.hip, nni.hip, place.hip, spr.hip; post_internal_nodes, the mark post_up's
//       table carries (branch_expect.hip and the four tree-search reads);
//   post_grid, the trial lengths of the edges through the model's own exponential (the four
//       tree-search reads), and post_fraction_*, the grid of an edge cut at fractions of its length
//       (place.hip, spr.hip);
//   post_set_pt, post_set_grid, post_mix and the mix_* kernels: the reads under a site-class mixture
//       over the rate sets (branch_expect.hip; branch_profile.hip, nni.hip, place.hip, spr.hip), and
//       post_set_fractions, the fraction grid of every set (place.hip, spr.hip);
//   post_chunk_units and post_result: the chunks a result that does not fit the scratch is made
//       in, the weighted site sums (post_sums_kernel) and the way of the result to the caller (the
//       four tree-search reads); post_part and post_part_result: the same for a PARTITIONED batch
//       (the four tree-search reads) -- the sets' fragments and which of them have a site, the
//       per-set sums over the runs of the plan (post_part_sums_*) and the gather to caller order;
//       post_part_arg, what the PART forms of spr.hip's and place.hip's kernels take;
//   post_csr_parents: the parents of a caller's CSR tree (nni.hip, spr.hip).
// Device: the steps the downward kernels have in common; the division-free `up` pass (nni.hip,
// place.hip, spr.hip).
#pragma once

#include "common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>

constexpr double POST_SCRATCH_CAP = 96e9;        // bytes of scratch one call may plan

// One read of a resident batch.  post_open .. post_layout make the checks every such call makes
// and take the common pieces from `plan`; the caller takes its own from the same plan, then
// post_begin reserves the scratch and post_up leaves L (and M) of every node in it.  `table` and
// `step_node` feed asynchronous copies: the pass lives until the stream is synchronised.
struct post_pass {
    const char *who = nullptr;                  // the entry point, for the messages
    rt_model *m = nullptr;
    rt_sites *s = nullptr, *x = nullptr;        // x: the split-M interpreter twin (n > 4)
    rt_ctx *ctx = nullptr;
    hipStream_t st = nullptr;
    int64_t n = 0, N = 0, nsites = 0;
    bool lane = false, with_D = false;
    bool per_set = false;                       // an ordinary batch read under the model's rate sets:
                                                // the caller runs the upward pass set by set (post_up_set)
    const double *d_cw = nullptr;               // (post_mix: the class weights [K] on the device)
    int NT = 0, KS = 0, KP = 0, nops = 0;       // row tiles, k-steps, k-step pairs; schedule steps
    post_plan plan;
    size_t o_L = 0, o_M = 0, o_D = 0, o_status = 0, o_steps = 0, o_ptab = 0, o_PT = 0;
    unsigned char *base = nullptr;
    double *d_L = nullptr, *d_M = nullptr, *d_D = nullptr, *d_PT = nullptr;
    int *d_status = nullptr, *d_ptab = nullptr; // ptab: the lane table, or step -> node
    int4 *d_steps = nullptr;
    std::vector<int32_t> table, step_node;
};

// sample.hip: the device part of rt_sites_sample_states for a caller that goes on with the draws
// on the device (mapping.hip).  rt_sample_states_plan is post_layout, the checks of the draws and
// their piece of the scratch (*o_states: [ndraws][nsites][nnodes]); after post_begin,
// rt_sample_states_enqueue runs the upward pass and the draws on the context's stream and leaves
// the states at d_states and the status (OR-ed over the draws) at p->d_status.
int rt_sample_states_plan(post_pass *p, int64_t ndraws, size_t *o_states);
int rt_sample_states_enqueue(post_pass *p, uint64_t seed, uint64_t first_draw, int64_t ndraws,
                             unsigned char *d_states);

// branch_profile.hip: the arguments of the rate sets' trial exponentials, [set][point][node] -- set
// k's edge above v at fac[v][point] times its resident length under the set's own rate matrix; the
// root and the sets of weight zero: no matrix (-1: a zero matrix, no exponential runs).  The last
// nabs of the np points are ABSOLUTE: set k's argument at point np - nabs + j is
// abs_scale[k] * abs_tau[j] at every node, not a multiple of the resident length
// (rt_sites_placements_mixture: the pendant edge); nabs = 0: the two tables are not read.
int rt_launch_set_grid_args(rt_ctx *ctx, int K, int np, int nnodes, const int32_t *d_set_qidx,
                            const double *d_set_t, const double *d_fac, const double *d_cw,
                            int nabs, const double *d_abs_tau, const double *d_abs_scale,
                            int32_t *d_qidx, double *d_tau);

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

// n > 4: steps[i] = {node, step of the parent, stream position of an observed leaf or -1,
// w_of_node[node]} in the schedule order of the split-M twin `x` (the root is the last step), and
// step -> node for rt_launch_pack_pt
inline int post_step_table(const rt_model *m, const rt_sites *x, const int *w_of_node,
                           std::vector<int32_t> *table, std::vector<int32_t> *step_node)
{
    const int64_t N = m->nnodes;
    const int nops = (int)x->ops.size();
    std::vector<int> step_of((size_t)N, -1);
    for (int i = 0; i < nops; ++i) step_of[(size_t)x->ops[(size_t)i].node] = i;
    RT_REQUIRE(nops == N && x->ops[(size_t)nops - 1].dst < 0, "unexpected schedule");
    table->assign((size_t)nops * 4, -1);
    step_node->assign((size_t)nops, 0);
    for (int i = 0; i < nops; ++i) {
        const rt_op &op = x->ops[(size_t)i];
        (*table)[(size_t)i * 4] = op.node;
        (*table)[(size_t)i * 4 + 1] = i + 1 < nops ? step_of[(size_t)m->parent[(size_t)op.node]] : 0;
        (*table)[(size_t)i * 4 + 2] = (op.pop < 0 && op.obs >= 0) ? op.obs : -1;
        (*table)[(size_t)i * 4 + 3] = w_of_node[(size_t)op.node];
        (*step_node)[(size_t)i] = op.node;
    }
    return RT_OK;
}

// n <= 4: [parent][stream position or -1][w_of_node] per node, in preorder
inline void post_lane_table(const rt_model *m, const rt_sites *s, const int *w_of_node,
                            std::vector<int32_t> *table)
{
    const int64_t N = m->nnodes;
    table->assign((size_t)3 * N, -1);
    for (int64_t v = 0; v < N; ++v) {
        (*table)[(size_t)v] = v ? m->parent[(size_t)v] : 0;
        (*table)[(size_t)2 * N + v] = w_of_node[(size_t)v];
    }
    for (const rt_op &op : s->ops)               // (the stream is in schedule order)
        if (op.obs >= 0) (*table)[(size_t)N + op.node] = op.obs;
}

// [nnodes]: 1 for a node with children, what the downward passes take as post_up's w_of_node
inline std::vector<int32_t> post_internal_nodes(const post_pass *p)
{
    std::vector<int32_t> internal((size_t)p->N, 0);
    for (int64_t v = 1; v < p->N; ++v) internal[(size_t)p->m->parent[(size_t)v]] = 1;
    return internal;
}

// the handles and the sizes every later check and layout goes by
// (partitioned: the call is one of those that take a partitioned batch, and nothing else --
// nsites counts its slots, the tables are those of the model's rate sets)
inline int post_open(post_pass *p, const char *who, rt_model *m, rt_sites *s, bool partitioned = false)
{
    RT_REQUIRE(m && s, "null pointer");
    if (s->part && !partitioned) {
        rt_set_error("%s: a partitioned batch is evaluated by rt_step_partitioned and read by "
                     "rt_sites_branch_expectations_partitioned, rt_sites_branch_profiles_partitioned, "
                     "rt_sites_nni_scores_partitioned, rt_sites_spr_scores_partitioned and "
                     "rt_sites_placements_partitioned only", who);
        return RT_ERR_UNSUPPORTED;
    }
    RT_REQUIRE(!partitioned || s->part, "%s: an ordinary batch (rt_sites_create_partitioned makes "
               "the batches this call takes)", who);
    RT_REQUIRE(s->model == m, "the site batch belongs to another model");
    RT_REQUIRE(!partitioned || m->multi.K >= s->part->nsets, "%s: the batch uses %lld rate sets, the "
               "model holds %lld (rt_model_set_rate_sets)", who,
               (long long)(s->part ? s->part->nsets : 0), (long long)m->multi.K);
    p->who = who; p->m = m; p->s = s; p->ctx = m->ctx; p->st = m->ctx->stream;
    p->n = m->n; p->N = m->nnodes; p->nsites = s->nsites; p->nops = (int)s->ops.size();
    p->lane = s->layout == RT_LAYOUT_LANE;
    p->NT = (int)((p->n + 15) / 16); p->KS = (int)((p->n + 3) / 4); p->KP = (p->KS + 1) / 2;
    return RT_OK;
}

// the tree-search reads of a partitioned batch refuse an ordinary one as every other read refuses
// a batch it does not take (before post_open, whose own check stays that of
// rt_sites_branch_expectations_partitioned)
inline int post_partitioned_only(const char *who, const rt_sites *s)
{
    if (s && !s->part) {
        rt_set_error("%s: an ordinary batch (rt_sites_create_partitioned makes the batches this "
                     "call takes)", who);
        return RT_ERR_UNSUPPORTED;
    }
    return RT_OK;
}

// the batches these passes take, and the common pieces of the scratch.  with_D: M, D and the P^T
// fragments (8 bytes in the lane layout) as well; else L alone -- and a buffer for M where the
// upward kernel's store variant writes it unconditionally (n > 4).  with_M = false: a call that
// makes its upward pass itself and stores no M (map_states.hip) reserves none.
inline int post_layout(post_pass *p, bool with_D, bool with_M = true)
{
    const rt_model *m = p->m;
    const rt_sites *s = p->s;
    const int64_t n = p->n, N = p->N;
    if (s->rescale || N < 2 || n < 2 || n > RT_MAX_STATES || s->d_scratch ||
        m->max_depth > RT_FAST_MAX_DEPTH || p->lane != (n <= 4)) {
        rt_set_error("%s: batches of 2..%d states without \"rescale\" on trees of at least two "
                     "nodes that the fast kernels take (n=%lld, nnodes=%lld, depth %d%s)", p->who,
                     RT_MAX_STATES, (long long)n, (long long)N, m->max_depth,
                     s->rescale ? ", rescale" : "");
        return RT_ERR_UNSUPPORTED;
    }
    // L, M, D of every node and site
    const size_t arr = p->lane ? (size_t)N * n * p->nsites * 8
                               : (size_t)p->nops * s->nblocks * p->NT * 256 * 8;
    p->with_D = with_D;
    p->o_L = p->plan.take(arr);
    if (with_M) p->o_M = p->plan.take(with_D || !p->lane ? arr : 8);
    if (with_D) p->o_D = p->plan.take(arr);
    p->o_status = p->plan.take((size_t)p->nsites * 4);
    p->o_steps = p->plan.take((size_t)std::max<int64_t>(p->nops, N) * 16);
    p->o_ptab = p->plan.take((size_t)3 * N * 4);
    if (with_D) p->o_PT = p->plan.take(p->lane ? 8 : (size_t)p->nops * p->NT * p->KP * 128 * 8);
    return RT_OK;
}

// once the caller has taken its pieces: the cap, the transition matrices, the twin, the scratch
// (status cleared).  `draws`: the call's scratch grows with a number of draws too.
inline int post_begin(post_pass *p, int recompute_transitions, bool draws = false)
{
    if ((double)p->plan.total > POST_SCRATCH_CAP) {
        rt_set_error("%s: this %s needs %.0f GB of scratch; split the batch%s", p->who,
                     draws ? "call" : "batch", (double)p->plan.total / 1e9,
                     draws ? " or the draws" : "");
        return RT_ERR_UNSUPPORTED;
    }
    RT_HIP(hipSetDevice(p->ctx->device));
    if (p->s->part || p->per_set) {              // (the sets' tables exist since set_rate_sets)
        if (recompute_transitions) RT_TRY(rt_rate_sets_recompute(p->m));
    } else {
        if (recompute_transitions) RT_TRY(rt_model_recompute_transitions(p->m));
        RT_REQUIRE(p->m->have_P, "the model has no transition matrices yet");
    }
    if (!p->lane) {
        if (!p->s->expect_twin) RT_TRY(rt_sites_twin_interpreter(p->s, &p->s->expect_twin));
        p->x = p->s->expect_twin;
    }
    RT_TRY(rt_scratch_reserve(p->ctx, p->plan.total));
    unsigned char *base = p->base = p->ctx->d_scratch;
    p->d_L = (double *)(base + p->o_L);
    p->d_M = (double *)(base + p->o_M);
    p->d_D = p->with_D ? (double *)(base + p->o_D) : nullptr;
    p->d_PT = p->with_D ? (double *)(base + p->o_PT) : nullptr;
    p->d_status = (int *)(base + p->o_status);
    p->d_steps = (int4 *)(base + p->o_steps);
    p->d_ptab = (int *)(base + p->o_ptab);
    RT_HIP(hipMemsetAsync(p->d_status, 0, (size_t)p->nsites * 4, p->st));
    return RT_OK;
}

// n > 4: the upward pass of the twin under the tables of rate set k of the model, L and M of every
// step stored (the outputs are the twin's).  granule_set (a partitioned batch, k = 0): every tile
// under the set of its granule instead.
inline int post_up_set(post_pass *p, int64_t k, const int32_t *granule_set)
{
    rt_sites *x = p->x;
    const rt_rate_sets &r = p->m->multi;
    rt_prune_view v;
    v.P = r.d_P + k * r.P_stride;
    v.Pfrag = r.d_Pfrag + k * r.frag_stride;
    v.Pquad = r.d_Pquad ? r.d_Pquad + k * r.quad_stride : nullptr;
    v.Pcol = r.d_Pcol ? r.d_Pcol + k * r.pcol_stride : nullptr;
    v.loglik = x->d_loglik; v.status = x->d_status; v.partial = x->d_partial;
    v.granule_set = granule_set;
    v.frag_stride = r.frag_stride; v.pcol_stride = r.pcol_stride;
    x->d_Lout = p->d_L;
    x->d_Mout = p->d_M;
    const int rc = rt_launch_prune(p->m, x, false, false, &v);
    x->d_Lout = x->d_Mout = nullptr;
    return rc;
}

// the table of the downward pass with `w_of_node` as its last column and, for n > 4, the upward
// pass: the split-M interpreter kernel with L and M of every step stored (its own log-likelihoods
// and totals are the twin's, not the batch's), then with pack_pt the model's P^T as A fragments.
// (n <= 4: the lane kernels make the upward pass themselves, lane_up.)
inline int post_up(post_pass *p, const int *w_of_node, bool pack_pt)
{
    if (p->lane) {
        post_lane_table(p->m, p->s, w_of_node, &p->table);
        RT_HIP(hipMemcpyAsync(p->d_ptab, p->table.data(), p->table.size() * 4, hipMemcpyHostToDevice,
                              p->st));
        return RT_OK;
    }
    rt_sites *x = p->x;
    RT_TRY(post_step_table(p->m, x, w_of_node, &p->table, &p->step_node));
    RT_HIP(hipMemcpyAsync(p->d_steps, p->table.data(), p->table.size() * 4, hipMemcpyHostToDevice,
                          p->st));
    if (pack_pt)
        RT_HIP(hipMemcpyAsync(p->d_ptab, p->step_node.data(), (size_t)p->nops * 4,
                              hipMemcpyHostToDevice, p->st));
    if (p->per_set) return RT_OK;                // (post_up_set per rate set; the caller packs per set)
    if (p->s->part) {
        // every tile under the tables of its own set, as rt_step_partitioned launches the batch
        if (x->nblocks * 16 != p->s->part->padded) {         // (one granule_set entry per tile)
            rt_set_error("%s: the twin's tiles do not match the batch's plan", p->who);
            return RT_ERR_INVALID;
        }
        return post_up_set(p, 0, p->s->part->d_granule_set);
    }
    x->d_Lout = p->d_L;
    x->d_Mout = p->d_M;
    const int rc = rt_launch_prune(p->m, x, false);
    x->d_Lout = x->d_Mout = nullptr;
    RT_TRY(rc);
    if (pack_pt)
        RT_TRY(rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, p->nops, p->d_ptab, p->m->d_P,
                                 p->d_PT));
    return RT_OK;
}

// ---- trial lengths of the edges (rt_sites_branch_profiles, rt_sites_nni_scores): P_v(tau) of
// every node and grid point from the model's own exponential, [point][node][n][n] like the model's
// transition matrices, and for n > 4 their transposes as A fragments [point][step] ----

// the model keeps the branch lengths of the last rt_model_set_rates / _spectral on the host
inline bool post_model_has_rates(const rt_model *m)
{
    return (m->d_Q || m->spectral) && (int64_t)m->h_t.size() == m->nnodes &&
           (int64_t)m->h_qidx.size() == m->nnodes;
}

// (the host vectors feed asynchronous copies: alive until the stream is synchronised)
struct post_grid {
    int np = 0;
    size_t cnt = 0;                              // np * nnodes exponentials (the root's: zero matrices)
    size_t o_G = 0, o_tau = 0, o_qidx = 0, o_info = 0, o_GT = 0;
    double *d_G = nullptr, *d_GT = nullptr;
    std::vector<double> tau;
    std::vector<int32_t> qidx, info;

    // what such a call asks of the model and of lengths[nnodes][npoints] (row 0 is ignored; with
    // use_row [nnodes], every row v with use_row[v] == 0 too)
    static int check(const post_pass *p, int recompute_transitions, int64_t npoints,
                     const double *lengths, const unsigned char *use_row = nullptr)
    {
        const rt_model *m = p->m;
        RT_REQUIRE(post_model_has_rates(m),
                   "%s: no rates have been set (rt_model_set_rates or "
                   "rt_model_set_rates_spectral; a model with transitions set directly has no rate "
                   "matrix to exponentiate at another length)", p->who);
        RT_REQUIRE(m->rates_current || recompute_transitions,
                   "%s: the transitions were set directly after the rates "
                   "(rt_model_set_transitions): the resident rates and lengths no longer describe them; "
                   "set the rates again or pass recompute_transitions", p->who);
        RT_REQUIRE(lengths, "%s: lengths is NULL", p->who);
        RT_REQUIRE(npoints >= 1 && npoints <= RT_MAX_PROFILE_POINTS,
                   "%s: 1..%d grid points per branch (%lld here)", p->who,
                   RT_MAX_PROFILE_POINTS, (long long)npoints);
        for (int64_t v = 1; v < p->N; ++v)
            for (int64_t g = 0; g < npoints && (!use_row || use_row[v]); ++g) {
                const double x = lengths[v * npoints + g];
                RT_REQUIRE(std::isfinite(x) && x >= 0.0,
                           "%s: length %d of node %lld is negative or not finite", p->who, (int)g,
                           (long long)v);
            }
        return RT_OK;
    }

    // after post_layout: the orders the model's exponential takes, the grid's pieces of the scratch
    int take(post_pass *p, int npoints)
    {
        const rt_model *m = p->m;
        if (m->spectral ? p->n > 64 : p->n > RT_MAX_EXPM_STATES) {
            rt_set_error("%s: n=%lld is beyond what the model's exponential takes", p->who,
                         (long long)p->n);
            return RT_ERR_UNSUPPORTED;
        }
        np = npoints;
        cnt = (size_t)np * p->N;
        const size_t nn = (size_t)p->n * p->n;
        o_G = p->plan.take(cnt * nn * 8);
        o_tau = p->plan.take(cnt * 8);
        o_qidx = p->plan.take(cnt * 4);
        o_info = p->plan.take(cnt * 8);
        o_GT = p->lane ? p->plan.take(8) : p->plan.take((size_t)np * p->nops * p->NT * p->KP * 128 * 8);
        return RT_OK;
    }

    // after post_begin: the tiled qidx / tau arrays and ONE launch of the route the model's own
    // transitions take (an ignored row: the resident length at every point)
    int launch(post_pass *p, const double *lengths, const unsigned char *use_row = nullptr)
    {
        const rt_model *m = p->m;
        const int64_t n = p->n, N = p->N;
        const size_t nn = (size_t)n * n;
        hipStream_t st = p->st;
        d_G = (double *)(p->base + o_G);
        d_GT = (double *)(p->base + o_GT);
        double *d_tau = (double *)(p->base + o_tau);
        int32_t *d_qidx = (int32_t *)(p->base + o_qidx), *d_info = (int32_t *)(p->base + o_info);
        tau.assign(cnt, 0.0);
        qidx.assign(cnt, 0);
        info.assign(2 * cnt, 0);
        for (int k = 0; k < np; ++k)
            for (int64_t v = 0; v < N; ++v) {
                qidx[(size_t)k * N + v] = m->h_qidx[(size_t)v];  // (the root's: -1, a zero matrix)
                if (v)
                    tau[(size_t)k * N + v] = !use_row || use_row[v] ? lengths[v * np + k] : m->h_t[(size_t)v];
            }
        RT_HIP(hipMemcpyAsync(d_tau, tau.data(), cnt * 8, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(d_qidx, qidx.data(), cnt * 4, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemsetAsync(d_info, 0, cnt * 8, st));
        if (m->spectral)
            RT_TRY(rt_launch_spectral(p->ctx, n, (int64_t)cnt, m->d_spec, m->d_spec + 2 * nn,
                                      m->d_spec + nn, m->spectral_has_D ? m->d_spec + 2 * nn + n : nullptr,
                                      d_qidx, d_tau, d_G, d_info, nullptr, 0, nullptr));
        else
            RT_TRY(rt_launch_expm(p->ctx, n, (int64_t)cnt, m->d_Q, d_qidx, d_tau, d_G, d_info, nullptr,
                                  0, nullptr));
        RT_HIP(hipMemcpyAsync(info.data(), d_info, cnt * 8, hipMemcpyDeviceToHost, st));
        return RT_OK;
    }

    // n > 4, after post_up: P(tau)^T of every point as A fragments in step order
    int pack(post_pass *p)
    {
        const size_t nn = (size_t)p->n * p->n, tab = (size_t)p->nops * p->NT * p->KP * 128;
        for (int k = 0; k < np; ++k)
            RT_TRY(rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, p->nops, p->d_ptab,
                                     d_G + (size_t)k * p->N * nn, d_GT + (size_t)k * tab));
        return RT_OK;
    }

    // after the synchronisation: an exponential the kernel gave up on (tau Q not finite) -- its
    // rows hold nothing usable
    int result(const post_pass *p) const
    {
        for (size_t j = 0; j < cnt; ++j)
            if (info[2 * j] < 0) {
                rt_set_error("%s: expm failed for node %lld at length %g (a non-finite entry or norm "
                             "of tau Q)", p->who, (long long)(j % (size_t)p->N), tau[j]);
                return RT_ERR_SINGULAR;
            }
        return RT_OK;
    }
};

// ---- an edge cut at fractions of its length (rt_sites_placements, rt_sites_spr_scores): the grid
// of every node v is rho_r t_v at the points 0 .. R - 1 and (1 - rho_r) t_v at R .. 2 R - 1 ----

// (two checks: rt_sites_placements checks its other counts between them)
inline int post_fraction_count(const char *who, int64_t nfractions)
{
    RT_REQUIRE(nfractions >= 1 && nfractions <= RT_MAX_PLACE_FRACTIONS,
               "%s: 1..%d fractions (%lld here)", who, RT_MAX_PLACE_FRACTIONS, (long long)nfractions);
    return RT_OK;
}

inline int post_fraction_values(const char *who, int64_t nfractions, const double *fractions)
{
    for (int64_t r = 0; r < nfractions; ++r)
        RT_REQUIRE(std::isfinite(fractions[r]) && fractions[r] >= 0.0 && fractions[r] <= 1.0,
                   "%s: fraction %d is outside [0, 1] or not finite", who, (int)r);
    return RT_OK;
}

// lengths [nnodes][2 R + nmore] for post_grid, the further points `more` the same at every node
// (zeros while the model has no rates: post_grid::check refuses it)
inline std::vector<double> post_fraction_lengths(const post_pass *p, int R, const double *fractions,
                                                 int nmore = 0, const double *more = nullptr)
{
    const rt_model *m = p->m;
    const int np = 2 * R + nmore;
    std::vector<double> lengths((size_t)p->N * np, 0.0);
    if (post_model_has_rates(m))
        for (int64_t v = 1; v < p->N; ++v) {
            double *row = lengths.data() + (size_t)v * np;
            const double t = m->h_t[(size_t)v];
            for (int r = 0; r < R; ++r) {
                row[r] = fractions[r] * t;
                row[R + r] = (1.0 - fractions[r]) * t;
            }
            for (int k = 0; k < nmore; ++k) row[2 * R + k] = more[k];
        }
    return lengths;
}

// n > 4, after post_up(.., true): in the grid's own fragment piece, [point][step], P(rho t)^T at
// the points 0 .. R - 1 and P((1 - rho) t) itself at R .. 2 R - 1
inline int post_fraction_pack(post_pass *p, post_grid *g, int R)
{
    const size_t nn = (size_t)p->n * p->n, tab = (size_t)p->nops * p->NT * p->KP * 128;
    for (int r = 0; r < R; ++r) {
        RT_TRY(rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, p->nops, p->d_ptab,
                                 g->d_G + (size_t)r * p->N * nn, g->d_GT + (size_t)r * tab));
        RT_TRY(rt_launch_pack_p(p->ctx, (int)p->n, p->NT, p->KP, p->nops, p->d_ptab,
                                g->d_G + (size_t)(R + r) * p->N * nn, g->d_GT + (size_t)(R + r) * tab));
    }
    return RT_OK;
}

// ---- an ORDINARY batch read under a site-class mixture over the model's rate sets
// (rt_sites_branch_expectations_mixture, rt_sites_branch_profiles_mixture,
// rt_sites_nni_scores_mixture) ----

// the model holds rate sets; class_weights [K] finite, >= 0, not all zero
inline int post_class_weights(const char *who, const rt_model *m, const double *class_weights)
{
    const int64_t K = m->multi.K;
    RT_REQUIRE(K >= 1, "%s: the model holds no rate sets (rt_model_set_rate_sets)", who);
    RT_REQUIRE(class_weights, "%s: class_weights is NULL", who);
    bool any = false;
    for (int64_t k = 0; k < K; ++k) {
        const double c = class_weights[k];
        RT_REQUIRE(std::isfinite(c) && c >= 0.0, "class_weights[%lld] is not finite and >= 0",
                   (long long)k);
        any = any || c > 0.0;
    }
    RT_REQUIRE(any, "class_weights are all zero");
    return RT_OK;
}

// n > 4: P^T of every node of the model's first K rate sets as A fragments [set][step], by ONE
// rt_launch_pack_pt over a step table that spans the sets (step -> matrix of r.d_P [set][node]; the
// root's step is never read: any matrix of the set).  The table feeds an asynchronous copy: alive
// until the stream is synchronised.
struct post_set_pt {
    int64_t K = 0;
    size_t tab = 0;                              // bytes of one set's table
    size_t o_PT = 0, o_tab = 0;
    double *d_PT = nullptr;
    std::vector<int32_t> steps;

    void take(post_pass *p, int64_t sets)
    {
        K = sets;
        tab = (size_t)p->nops * p->NT * p->KP * 128 * 8;
        o_PT = p->lane ? p->plan.take(8) : p->plan.take((size_t)K * tab);
        o_tab = p->plan.take((size_t)K * p->nops * 4);
    }
    // after post_begin
    void place(post_pass *p) { d_PT = (double *)(p->base + o_PT); }
    // after post_up (the step -> node table)
    int pack(post_pass *p)
    {
        const rt_rate_sets &r = p->m->multi;
        int *d_tab = (int *)(p->base + o_tab);
        steps.resize((size_t)K * p->nops);
        for (int64_t k = 0; k < K; ++k)
            for (int i = 0; i < p->nops; ++i)
                steps[(size_t)(k * p->nops + i)] = (int32_t)(k * p->N + p->step_node[(size_t)i]);
        RT_HIP(hipMemcpyAsync(d_tab, steps.data(), steps.size() * 4, hipMemcpyHostToDevice, p->st));
        return rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, (int)(K * p->nops), d_tab, r.d_P, d_PT);
    }
    const double *of_set(int64_t k) const { return d_PT + (size_t)k * (tab / 8); }
};

// trial lengths under the rate sets, given as factors[nnodes][npoints] of every set's own resident
// lengths: post_grid over the sets' d_Q / d_qidx / d_t -- P_kv(factor t_kv) of every set, point and
// node [set][point][node][n][n] in ONE launch of the sets' exponential, and for n > 4 their
// transposes as A fragments [set][point][step].  With nabs > 0 the last nabs points are absolute
// lengths abs_scale[k] * abs_tau[j], the same at every node (rt_launch_set_grid_args).  (The host
// vectors feed asynchronous copies: alive until the stream is synchronised.)
struct post_set_grid {
    int64_t K = 0;
    int np = 0, nabs = 0;
    size_t o_abs = 0;
    std::vector<double> abs;                     // abs_tau [nabs], then abs_scale [K]
    size_t cnt = 0, tab = 0;                     // K np nnodes matrices; doubles of one step table
    size_t o_G = 0, o_tau = 0, o_qidx = 0, o_info = 0, o_fac = 0, o_GT = 0, o_tab = 0;
    double *d_G = nullptr, *d_GT = nullptr;
    std::vector<double> fac;
    std::vector<int32_t> info, steps;

    // factors [nnodes][npoints] finite and >= 0 (row 0 is ignored; with use_row [nnodes], every row
    // v with use_row[v] == 0 too).  (The arguments of post_grid::check: the sets' tables follow
    // rt_model_set_rate_sets, there is nothing to ask of recompute_transitions.)
    static int check(const post_pass *p, int /*recompute_transitions*/, int64_t npoints,
                     const double *factors, const unsigned char *use_row = nullptr)
    {
        RT_REQUIRE(factors, "%s: factors is NULL", p->who);
        RT_REQUIRE(npoints >= 1 && npoints <= RT_MAX_PROFILE_POINTS,
                   "%s: 1..%d grid points per branch (%lld here)", p->who, RT_MAX_PROFILE_POINTS,
                   (long long)npoints);
        for (int64_t v = 1; v < p->N; ++v)
            for (int64_t g = 0; g < npoints && (!use_row || use_row[v]); ++g) {
                const double x = factors[v * npoints + g];
                RT_REQUIRE(std::isfinite(x) && x >= 0.0,
                           "%s: factor %d of node %lld is negative or not finite", p->who, (int)g,
                           (long long)v);
            }
        return RT_OK;
    }

    // after post_layout: every rate set the model holds (npoints counts the absolute points)
    int take(post_pass *p, int npoints, int nabsolute = 0)
    {
        if (p->n > RT_MAX_EXPM_STATES) {
            rt_set_error("%s: n=%lld is beyond what the sets' exponential takes", p->who,
                         (long long)p->n);
            return RT_ERR_UNSUPPORTED;
        }
        K = p->m->multi.K; np = npoints; nabs = nabsolute;
        cnt = (size_t)K * np * p->N;
        tab = (size_t)p->nops * p->NT * p->KP * 128;
        const size_t nn = (size_t)p->n * p->n;
        post_plan &plan = p->plan;
        o_G = plan.take(cnt * nn * 8);
        o_tau = plan.take(cnt * 8);
        o_qidx = plan.take(cnt * 4);
        o_info = plan.take(cnt * 8);
        o_fac = plan.take((size_t)p->N * np * 8);
        o_GT = p->lane ? plan.take(8) : plan.take((size_t)K * np * tab * 8);
        o_tab = plan.take((size_t)K * np * p->nops * 4);
        if (nabs) o_abs = plan.take((size_t)(nabs + K) * 8);
        return RT_OK;
    }

    // after post_begin and post_mix::begin (p->d_cw: the class weights on the device).  An ignored
    // row: factor 1, the resident length at every point.  What the choice of the exponential's
    // variant goes by is one set's count, whatever the number of sets that run.
    int launch(post_pass *p, const double *factors, const unsigned char *use_row = nullptr,
               const double *abs_tau = nullptr, const double *abs_scale = nullptr)
    {
        RT_REQUIRE(p->d_cw, "%s: the class weights are not on the device yet (post_mix::begin)", p->who);
        const rt_rate_sets &r = p->m->multi;
        const int64_t N = p->N;
        hipStream_t st = p->st;
        d_G = (double *)(p->base + o_G);
        d_GT = (double *)(p->base + o_GT);
        double *d_tau = (double *)(p->base + o_tau), *d_fac = (double *)(p->base + o_fac);
        int32_t *d_qidx = (int32_t *)(p->base + o_qidx), *d_info = (int32_t *)(p->base + o_info);
        fac.assign((size_t)N * np, 1.0);
        for (int64_t v = 1; v < N; ++v)
            for (int g = 0; g < np && (!use_row || use_row[v]); ++g)
                fac[(size_t)(v * np + g)] = factors[v * np + g];
        info.assign(2 * cnt, 0);
        RT_HIP(hipMemcpyAsync(d_fac, fac.data(), fac.size() * 8, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemsetAsync(d_info, 0, cnt * 8, st));
        const double *d_abs = nullptr;
        if (nabs) {                              // (abs_scale null: ones)
            abs.assign(abs_tau, abs_tau + nabs);
            for (int64_t k = 0; k < K; ++k) abs.push_back(abs_scale ? abs_scale[k] : 1.0);
            d_abs = (const double *)(p->base + o_abs);
            RT_HIP(hipMemcpyAsync(p->base + o_abs, abs.data(), abs.size() * 8, hipMemcpyHostToDevice, st));
        }
        RT_TRY(rt_launch_set_grid_args(p->ctx, (int)K, np, (int)N, r.d_qidx, r.d_t, d_fac, p->d_cw,
                                       nabs, d_abs, d_abs ? d_abs + nabs : nullptr, d_qidx, d_tau));
        RT_TRY(rt_launch_expm(p->ctx, p->n, (int64_t)cnt, r.d_Q, d_qidx, d_tau, d_G, d_info, nullptr, 0,
                              nullptr, nullptr, nullptr, (int64_t)np * N));
        RT_HIP(hipMemcpyAsync(info.data(), d_info, cnt * 8, hipMemcpyDeviceToHost, st));
        return RT_OK;
    }

    // n > 4, after post_up: P(tau)^T of every set and point as A fragments in step order, one
    // rt_launch_pack_pt over a step table that spans them
    int pack(post_pass *p)
    {
        int *d_tab = (int *)(p->base + o_tab);
        const int64_t tables = K * np;
        steps.resize((size_t)tables * p->nops);
        for (int64_t j = 0; j < tables; ++j)
            for (int i = 0; i < p->nops; ++i)
                steps[(size_t)(j * p->nops + i)] = (int32_t)(j * p->N + p->step_node[(size_t)i]);
        RT_HIP(hipMemcpyAsync(d_tab, steps.data(), steps.size() * 4, hipMemcpyHostToDevice, p->st));
        return rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, (int)(tables * p->nops), d_tab, d_G, d_GT);
    }

    // set k's tables: [point][node][n][n], [point][step] fragments
    const double *G_of_set(const post_pass *p, int64_t k) const
    {
        return d_G + (size_t)k * np * p->N * p->n * p->n;
    }
    const double *GT_of_set(int64_t k) const { return d_GT + (size_t)k * np * tab; }

    // after the synchronisation: an exponential the kernel gave up on
    int result(const post_pass *p) const
    {
        for (size_t j = 0; j < cnt; ++j)
            if (info[2 * j] < 0) {
                rt_set_error("%s: expm failed for node %lld of rate set %lld at point %lld (a "
                             "non-finite entry or norm of tau Q)", p->who,
                             (long long)(j % (size_t)p->N), (long long)(j / ((size_t)np * p->N)),
                             (long long)(j / (size_t)p->N % (size_t)np));
                return RT_ERR_SINGULAR;
            }
        return RT_OK;
    }
};

// An edge cut at fractions under the rate sets (rt_sites_spr_scores_mixture,
// rt_sites_placements_mixture): the set grid of 2 R + nmore points per node, the factors rho_r at
// 0 .. R - 1 and 1 - rho_r at R .. 2 R - 1 of every set's own resident length; the nmore further
// points are the grid's absolute ones (factor 1, not read).  factors: [nnodes][2 R + nmore] for
// post_set_grid::launch.
inline std::vector<double> post_set_fraction_factors(const post_pass *p, int R, const double *fractions,
                                                     int nmore = 0)
{
    const int np = 2 * R + nmore;
    std::vector<double> fac((size_t)p->N * np, 1.0);
    for (int64_t v = 0; v < p->N; ++v)
        for (int r = 0; r < R; ++r) {
            fac[(size_t)(v * np + r)] = v ? fractions[r] : 0.0;
            fac[(size_t)(v * np + R + r)] = v ? 1.0 - fractions[r] : 0.0;
        }
    return fac;
}

// n > 4, after post_up: the fraction fragment tables of EVERY set in the set grid's own fragment
// piece by one rt_launch_pack_pt and one rt_launch_pack_p over step tables that span the sets
// (post_fraction_pack is the single-set form): [half][set][fraction][step], P(rho t)^T in the first
// half, P((1 - rho) t) itself in the second.
struct post_set_fractions {
    int R = 0;
    const post_set_grid *g = nullptr;

    int pack(post_pass *p, post_set_grid *grid, int nfractions)
    {
        g = grid; R = nfractions;
        RT_REQUIRE(g->np >= 2 * R, "%s: the set grid holds %d points, fewer than 2 x %d", p->who, g->np, R);
        int *d_tab = (int *)(p->base + g->o_tab);
        const int64_t K = g->K, half = K * R * p->nops;
        std::vector<int32_t> &steps = grid->steps;
        steps.resize((size_t)(2 * half));
        for (int h = 0; h < 2; ++h)
            for (int64_t k = 0; k < K; ++k)
                for (int r = 0; r < R; ++r)
                    for (int i = 0; i < p->nops; ++i)
                        steps[(size_t)(h * half + (k * R + r) * p->nops + i)] =
                            (int32_t)((k * g->np + h * R + r) * p->N + p->step_node[(size_t)i]);
        RT_HIP(hipMemcpyAsync(d_tab, steps.data(), steps.size() * 4, hipMemcpyHostToDevice, p->st));
        RT_TRY(rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, (int)half, d_tab, g->d_G, g->d_GT));
        return rt_launch_pack_p(p->ctx, (int)p->n, p->NT, p->KP, (int)half, d_tab + half, g->d_G,
                                g->d_GT + (size_t)K * R * g->tab);
    }
    // set k's [fraction][step] tables of P(rho t)^T and of P((1 - rho) t)
    const double *T_of_set(int64_t k) const { return g->d_GT + (size_t)k * R * g->tab; }
    const double *A_of_set(int64_t k) const { return g->d_GT + (size_t)(g->K + k) * R * g->tab; }
};

// per site, over the K root totals tot [K][nsites] (L_ik; set k live: c_k > 0 and L_ik > 0): the
// plain sum of c_k L_ik in set order, post [site][K] = c_k L_ik / sum (0 for a set that is not
// live), loglik, and the status words of the LIVE sets OR-ed (set_status [K][nsites]); no live
// set: a row of zeros, -inf, RT_SITE_ZERO_PROB.  (Templates, BS = 256 threads: only the translation
// units that launch them hold a copy.)
template <int BS>
__global__ void __launch_bounds__(BS)
mix_post_kernel(int K, long nsites, const double *__restrict__ cw, const double *__restrict__ tot,
                const int *__restrict__ set_status, double *__restrict__ post,
                double *__restrict__ loglik, int *__restrict__ status)
{
    const long i = (long)blockIdx.x * BS + threadIdx.x;
    if (i >= nsites) return;
    double sum = 0.0;
    for (int k = 0; k < K; ++k) {
        const double c = cw[k];
        if (!(c > 0.0)) continue;
        const double L = tot[(size_t)k * nsites + i];
        if (L > 0.0) sum = __dadd_rn(sum, __dmul_rn(c, L));
    }
    const bool none = !(sum > 0.0);
    int st = none ? RT_SITE_ZERO_PROB : 0;
    for (int k = 0; k < K; ++k) {
        const double c = cw[k];
        double pk = 0.0;
        if (!none && c > 0.0) {
            const double L = tot[(size_t)k * nsites + i];
            if (L > 0.0) {
                pk = __dmul_rn(c, L) / sum;
                st |= set_status[(size_t)k * nsites + i];
            }
        }
        post[(size_t)i * K + k] = pk;
    }
    loglik[i] = none ? -HUGE_VAL : log(sum);
    status[i] = st;
}

// the mixture values from the accumulated terms: x [row][site] holds sum_k c_k L_ik(row) in set
// order; -> log x - log Lambda_i (loglik), -inf where x is not positive, 0 at a site of zero
// mixture likelihood.  row_node (or null) [rows / np]: the node of a row's edge, and dead_edge
// [node] != 0: a NaN row (an edge of resident length 0 under a set of the mixture); the root's
// row (node 0) is 0.
template <int BS>
__global__ void __launch_bounds__(BS)
mix_log_ratio_kernel(long rows, int np, long nsites, const double *__restrict__ loglik,
                     const int *__restrict__ status, const int *__restrict__ dead_edge,
                     double *__restrict__ x)
{
    const long i = (long)blockIdx.x * BS + threadIdx.x;
    if (i >= nsites) return;
    const bool zero = status[i] & RT_SITE_ZERO_PROB;
    const double ll = loglik[i];
    for (long r = blockIdx.y; r < rows; r += gridDim.y) {
        double *at = x + (size_t)r * nsites + i;
        const double a = *at;
        double v = a > 0.0 ? log(a) - ll : -HUGE_VAL;
        if (dead_edge) {
            const long node = r / np;
            if (node == 0) v = 0.0;
            else if (dead_edge[node]) v = __builtin_nan("");
        }
        *at = zero ? 0.0 : v;
    }
}

// dead_edge[v] = 1 where a set with c_k > 0 has resident t[k][v] == 0 (v > 0)
template <int BS>
__global__ void __launch_bounds__(BS)
mix_dead_edge_kernel(int K, int nnodes, const double *__restrict__ cw, const double *__restrict__ set_t,
                     int *__restrict__ dead_edge, double *__restrict__ tlen)
{
    const int v = blockIdx.x * BS + threadIdx.x;
    if (v >= nnodes) return;
    int dead = 0;
    for (int k = 0; k < K; ++k)
        if (v > 0 && cw[k] > 0.0 && set_t[(size_t)k * nnodes + v] == 0.0) dead = 1;
    dead_edge[v] = dead;
    tlen[v] = dead ? 0.0 : 1.0;                  // (what post_sums_kernel goes by)
}

// What a tree-search read under the mixture (rt_sites_branch_profiles_mixture,
// rt_sites_nni_scores_mixture) holds beside the single-set one: the class weights on the device,
// the sets' P^T fragments, per set the root totals L_ik and a status word (tot_of / status_of: what
// the MIX kernel instance of set k writes), the class posteriors and log Lambda_i.
struct post_mix {
    int64_t K = 0;
    const double *cw = nullptr;                  // the caller's class weights
    post_set_pt PT;
    size_t o_tot = 0, o_stat = 0, o_post = 0, o_ll = 0, o_cw = 0;
    double *d_tot = nullptr, *d_post = nullptr, *d_ll = nullptr;
    int *d_stat = nullptr;

    // after post_layout
    int take(post_pass *p, const double *class_weights)
    {
        const rt_rate_sets &r = p->m->multi;
        RT_REQUIRE(r.P_stride == p->N * p->n * p->n, "unexpected stride of the sets' transition matrices");
        K = r.K; cw = class_weights;
        PT.take(p, K);
        o_tot = p->plan.take((size_t)K * p->nsites * 8);
        o_stat = p->plan.take((size_t)K * p->nsites * 4);
        o_post = p->plan.take((size_t)p->nsites * K * 8);
        o_ll = p->plan.take((size_t)p->nsites * 8);
        o_cw = p->plan.take((size_t)K * 8);
        return RT_OK;
    }
    // after post_begin: the weights go up, the sets' totals and status words are cleared
    int begin(post_pass *p)
    {
        PT.place(p);
        d_tot = (double *)(p->base + o_tot); d_post = (double *)(p->base + o_post);
        d_ll = (double *)(p->base + o_ll); d_stat = (int *)(p->base + o_stat);
        p->d_cw = (double *)(p->base + o_cw);
        RT_HIP(hipMemcpyAsync(p->base + o_cw, cw, (size_t)K * 8, hipMemcpyHostToDevice, p->st));
        RT_HIP(hipMemsetAsync(d_stat, 0, (size_t)K * p->nsites * 4, p->st));
        RT_HIP(hipMemsetAsync(d_tot, 0, (size_t)K * p->nsites * 8, p->st));
        return RT_OK;
    }
    const double *P_of(const post_pass *p, int64_t k) const { return p->m->multi.d_P + k * p->m->multi.P_stride; }
    double *tot_of(const post_pass *p, int64_t k) const { return d_tot + (size_t)k * p->nsites; }
    int *status_of(const post_pass *p, int64_t k) const { return d_stat + (size_t)k * p->nsites; }
    // once every set's launch is in: log Lambda_i and the status of the live sets.  (Templates,
    // as the kernels: only a translation unit that calls them holds a copy.)
    template <int BS = 256>
    int post(post_pass *p)
    {
        hipLaunchKernelGGL(mix_post_kernel<BS>, dim3((unsigned)((p->nsites + BS - 1) / BS)), dim3(BS), 0,
                           p->st, (int)K, (long)p->nsites, p->d_cw, (const double *)d_tot,
                           (const int *)d_stat, d_post, d_ll, p->d_status);
        RT_HIP(hipGetLastError());
        return RT_OK;
    }
    // after post: the accumulator x [rows][site] -> values
    template <int BS = 256>
    int log_ratio(post_pass *p, size_t rows, int np, const int *d_dead_edge, double *x)
    {
        hipLaunchKernelGGL(mix_log_ratio_kernel<BS>,
                           dim3((unsigned)((p->nsites + BS - 1) / BS), (unsigned)std::min<size_t>(rows, 1024)),
                           dim3(BS), 0, p->st, (long)rows, np, (long)p->nsites, (const double *)d_ll,
                           (const int *)p->d_status, d_dead_edge, x);
        RT_HIP(hipGetLastError());
        return RT_OK;
    }
};

// n <= 4: one lane per site.  The observation of stream position k from the batch's lane-family
// image (dense pairs, or one byte per leaf: a state or an allowed-set mask; passes.hip
// sets_from_lane_batch_kernel reads the same layouts).
template <int N>
__device__ inline void lane_obs(const void *obs, int compact, int K, int block_sites, long site, int k,
                                double (&x)[N])
{
    const long blk = site / block_sites;
    const int ln = (int)(site - blk * block_sites);
    if (compact) {
        const int KQ = (K + 3) / 4;
        const unsigned w = ((const unsigned *)obs)[((size_t)blk * KQ + (k >> 2)) * block_sites + ln];
        const unsigned b = (w >> (8 * (k & 3))) & 255u;
#pragma unroll
        for (int s = 0; s < N; ++s)
            x[s] = compact == 2 ? (double)((b >> s) & 1u) : (b >= (unsigned)N || b == (unsigned)s) ? 1.0 : 0.0;
    } else {
        constexpr int hp = ((N + 1) & ~1) / 2;
        const double *o = (const double *)obs + (((size_t)blk * K + k) * hp * block_sites + ln) * 2;
#pragma unroll
        for (int s = 0; s < N; ++s) x[s] = o[(size_t)(s >> 1) * block_sites * 2 + (s & 1)];
    }
}

// ---- n <= 4: one lane per site; arrays [node][state][site], nodes in preorder (a parent before
// its children) ----

// up: L_v = observation, times the messages M_v = P_v L_v of the children (descending preorder
// index); M stored too where the downward pass divides by it
template <int N, bool STORE_M>
__device__ __forceinline__ void lane_up(int nnodes, long nsites, long site, const double *P,
                               const int *parent, const int *node_k,
                               const void *obs, int compact, int K, int block_sites,
                               double *Larr, double *Marr)
{
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    for (int v = 0; v < nnodes; ++v) {
        double x[N];
        const int k = node_k[v];
        if (k >= 0) lane_obs<N>(obs, compact, K, block_sites, site, k, x);
        else
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] = 1.0;
#pragma unroll
        for (int s = 0; s < N; ++s) Larr[idx(v, s)] = x[s];
    }
    for (int v = nnodes - 1; v >= 1; --v) {
        double x[N];
#pragma unroll
        for (int s = 0; s < N; ++s) x[s] = Larr[idx(v, s)];
        const double *Pv = P + (size_t)v * N * N;
        const int p = parent[v];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) t += Pv[a * N + b] * x[b];
            if (STORE_M) Marr[idx(v, a)] = t;
            Larr[idx(p, a)] *= t;
        }
    }
}

// the root: D = w L / sum_states(w L), stored and in d; true where the sum is not positive (D = 0);
// tot (or null): the sum itself, the site's likelihood
template <int N>
__device__ __forceinline__ bool lane_root(long nsites, long site, const double *root_w,
                                 const double *Larr, double *Darr,
                                 double (&d)[N], double *tot_out = nullptr)
{
    double wl[N], tot = 0.0;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        wl[s] = (root_w ? root_w[s] : 1.0) * Larr[(size_t)s * nsites + site];
        tot += wl[s];
    }
    const bool zero = !(tot > 0.0);
    if (tot_out) *tot_out = tot;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        d[s] = zero ? 0.0 : wl[s] / tot;
        Darr[(size_t)s * nsites + site] = d[s];
    }
    return zero;
}

// u = D_p / M_v of node v below p; bad is set where a live parent state meets a denominator <= 0
template <int N>
__device__ __forceinline__ void lane_u(long nsites, long site, int p, int v, const double *Darr,
                                       const double *Marr, double (&u)[N], bool &bad)
{
#pragma unroll
    for (int a = 0; a < N; ++a) {
        const double dp = Darr[((size_t)p * N + a) * nsites + site];
        const double den = Marr[((size_t)v * N + a) * nsites + site];
        u[a] = 0.0;
        if (dp != 0.0) {
            if (den > 0.0) u[a] = dp / den;
            else bad = true;
        }
    }
}

// ---- n > 4: one workgroup of NT row-tile waves per 16-site tile; wave m, lane l holds rows
// 16 m + 4 r + (l >> 4), r = 0 .. 3, of site l & 15; L, M, D [step][tile][NT][4][64] ----

// element r of this lane's rows at step `step`: down_at(..) + r * 64
template <int NT>
__device__ __forceinline__ size_t down_at(int step, long nblocks, long blk, int m, int lane)
{
    return ((size_t)step * nblocks + blk) * ((size_t)NT * 256) + (m * 4) * 64 + lane;
}

// v over the states: own rows are in v; the four lane groups by xor shuffles into part[m], then
// (after a barrier) down_total adds the waves in order -- a fixed order, the same bits every call
__device__ __forceinline__ void down_part(double (*part)[16], int m, int lane, double v)
{
    v += __shfl_xor(v, 16, 64);
    v += __shfl_xor(v, 32, 64);
    if (lane < 16) part[m][lane] = v;
}

template <int NT>
__device__ __forceinline__ double down_total(const double (*part)[16], int j)
{
    double t = 0.0;
#pragma unroll
    for (int mm = 0; mm < NT; ++mm) t += part[mm][j];
    return t;
}

// own rows of L at a step: what the upward pass stored (at o), or for an observed leaf (stream
// position k >= 0) its observation: the pairs q = 2m, 2m + 1 of og hold rows 4m .. 4m + 3
// (prune.hip)
template <int KP>
__device__ __forceinline__ void down_L(int k, const double *og, const double *Larr,
                              size_t o, int m, double (&L)[4])
{
    if (k >= 0) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = 2 * m + h;
            double2 v = {0.0, 0.0};
            if (q < KP) v = *(const double2 *)(og + ((size_t)k * KP + q) * 128);
            L[2 * h] = v.x;
            L[2 * h + 1] = v.y;
        }
    } else {
#pragma unroll
        for (int r = 0; r < 4; ++r) L[r] = Larr[o + r * 64];
    }
}

// u = D_p / M_v on own rows (parent's D at po, M at o); bad is set where a live parent state
// meets a denominator <= 0
__device__ __forceinline__ void down_u(const double *Darr, size_t po, const double *Marr, size_t o,
                                       double (&u)[4], bool &bad)
{
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const double dp = Darr[po + r * 64];
        const double den = Marr[o + r * 64];
        u[r] = 0.0;
        if (dp != 0.0) {
            if (den > 0.0) u[r] = dp / den;
            else bad = true;
        }
    }
}

// own rows of u into xb, the B operands of every wave's products, between two barriers (the
// first: every wave is done with the previous operands)
__device__ __forceinline__ void down_stage(double *xb, int m, int lane, const double (&u)[4])
{
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 4; ++r) xb[(4 * m + r) * 64 + lane] = u[r];
    __syncthreads();
}

// this wave's A fragments of step `step` of a rt_launch_pack_pt table
template <int KP>
__device__ __forceinline__ void down_frag(const double *ag, double (&a)[2 * KP])
{
#pragma unroll
    for (int q = 0; q < KP; ++q) {
        const double2 v = *(const double2 *)(ag + q * 128);
        a[2 * q] = v.x;
        a[2 * q + 1] = v.y;
    }
}

// own rows of A x for the staged x
template <int KS>
__device__ __forceinline__ double4_t down_product(const double (&a)[2 * ((KS + 1) / 2)], const double *xb, int lane)
{
    double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
    for (int kk = 0; kk < KS; ++kk)
        acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xb[kk * 64 + lane], acc, 0, 0, 0);
    return acc;
}

// ---- the division-free `up` pass (nni.hip, place.hip) ----

// The child tables of such a pass, over slots j = 0 .. cnt - 1 (n > 4: schedule steps; n <= 4:
// preorder nodes):
//   obs[j]          stream position of the slot's node, a leaf or an observed INTERNAL node (the
//                   shared step table has the leaves' only), or -1
//   cptr[j], cidx   the slots of its children in the CSR child order
//   first[j]        a per-slot number of the caller's (nni.hip: the index of its first move)
struct post_tab {
    const int *obs, *cptr, *first, *cidx;
    __host__ __device__ post_tab(const int *t, int cnt)
        : obs(t), cptr(t + cnt), first(t + 2 * cnt + 1), cidx(t + 3 * cnt + 1) {}
};

// the host image of a post_tab (4 cnt ints), by step (n > 4, after post_begin) or by node;
// first [nnodes] or null (zeros)
inline void post_tab_build(const post_pass *p, const int32_t *first, std::vector<int32_t> *tab)
{
    const rt_model *m = p->m;
    const int64_t N = p->N;
    const int cnt = p->lane ? (int)N : p->nops;
    const rt_sites *x = p->lane ? p->s : p->x;
    tab->assign((size_t)4 * cnt, 0);
    std::vector<int32_t> node_of((size_t)cnt), obs_of((size_t)N, -1), slot_of((size_t)N);
    for (int j = 0; j < cnt; ++j) node_of[(size_t)j] = p->lane ? j : x->ops[(size_t)j].node;
    for (int j = 0; j < cnt; ++j) slot_of[(size_t)node_of[(size_t)j]] = j;
    for (const rt_op &op : x->ops)
        if (op.obs >= 0) obs_of[(size_t)op.node] = op.obs;
    int32_t *t_obs = tab->data(), *t_cptr = t_obs + cnt, *t_first = t_cptr + cnt + 1;
    int32_t *t_cidx = t_first + cnt;
    int32_t e = 0;
    for (int j = 0; j < cnt; ++j) {
        const int64_t v = node_of[(size_t)j];
        t_obs[j] = obs_of[(size_t)v];
        t_first[j] = first ? first[(size_t)v] : 0;
        t_cptr[j] = e;
        for (int64_t k = m->indptr[(size_t)v]; k < m->indptr[(size_t)v + 1]; ++k)
            t_cidx[e++] = slot_of[(size_t)m->indices[(size_t)k]];
    }
    t_cptr[cnt] = e;
}

// n > 4.  The root: the site's likelihood sum_states(w L), true where it is not positive (the
// status is set), and with `make` up_root = w / it; then the `up` vectors of the nodes with
// children (steps[i].w), a parent before its children:
//     up_v[b] = sum_a P_v[a][b] up_p[a] obs_p[a] prod_{w child of p, w != v} M_w[a].
// make = false: a later launch that finds them in Uarr.  PfragT: [step] A fragments of the
// resident P^T; live: own rows that are states.
// MIX (one launch per rate set of a site-class mixture): up_root = ck w, whatever the sum is -- a
// set under which the resident tree is impossible may be live on a moved one -- and the sum goes
// to root_tot[site].
template <int NT, int KS, bool MIX = false>
__device__ __forceinline__ bool down_up_pass(bool make, double *xb, double (*red)[16],
                                             const post_tab &tab, const double *PfragT, int nops,
                                             const int4 *steps, const double *Larr,
                                             const double *Marr, double *Uarr, const double *og,
                                             const double *root_w, const bool (&live)[4], int m,
                                             int lane, long blk, long nblocks, bool writer,
                                             int *status, long site, double ck = 1.0,
                                             double *root_tot = nullptr)
{
    constexpr int KP = (KS + 1) / 2;
    const size_t frag = ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    bool zero;
    {
        const int i = nops - 1;
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        double w[4], s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            w[r] = live[r] ? (root_w ? root_w[16 * m + 4 * r + (lane >> 4)] : 1.0) : 0.0;
            s += w[r] * Larr[o + r * 64];
        }
        down_part(red, m, lane, s);
        __syncthreads();
        const double tot = down_total<NT>(red, lane & 15);
        zero = !(tot > 0.0);
        if (make) {
#pragma unroll
            for (int r = 0; r < 4; ++r) Uarr[o + r * 64] = MIX ? ck * w[r] : zero ? 0.0 : w[r] / tot;
        }
        if (writer && zero) atomicOr(&status[site], RT_SITE_ZERO_PROB);
        if constexpr (MIX)
            if (writer) root_tot[site] = tot;
    }
    if (!make) return zero;
    double a[2 * KP];
    for (int i = nops - 2; i >= 0; --i) {
        const int4 st = steps[i];
        if (!st.w) continue;
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        const size_t po = down_at<NT>(st.y, nblocks, blk, m, lane);
        double x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = Uarr[po + r * 64];
        const int kp = tab.obs[st.y];
        if (kp >= 0) {
            double ob[4];
            down_L<KP>(kp, og, Larr, po, m, ob);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] *= ob[r];
        }
        for (int e = tab.cptr[st.y]; e < tab.cptr[st.y + 1]; ++e) {
            const int w = tab.cidx[e];
            if (w == i) continue;
            const size_t wo = down_at<NT>(w, nblocks, blk, m, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] *= Marr[wo + r * 64];
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = live[r] ? x[r] : 0.0;     // (rows past the states)
        down_stage(xb, m, lane, x);
        down_frag<KP>(PfragT + (size_t)i * ASTRIDE + frag, a);
        const double4_t acc = down_product<KS>(a, xb, lane);
#pragma unroll
        for (int r = 0; r < 4; ++r) Uarr[o + r * 64] = acc[r];
    }
    return zero;
}

// n <= 4, after lane_up<N, true>: the site's likelihood (true where it is not positive; the status
// is set), and with `make` the `up` vectors of the root and of every node with children
// (MIX: as down_up_pass)
template <int N, bool MIX = false>
__device__ __forceinline__ bool lane_up_pass(bool make, int nnodes, long nsites, long site,
                                             const double *P, const int *parent, const int *node_k,
                                             const post_tab &tab, const void *obs, int compact, int K,
                                             int block_sites, const double *root_w,
                                             const double *Larr, const double *Marr, double *Uarr,
                                             int *status, double ck = 1.0, double *root_tot = nullptr)
{
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    double tot = 0.0;
#pragma unroll
    for (int s = 0; s < N; ++s) tot += (root_w ? root_w[s] : 1.0) * Larr[idx(0, s)];
    const bool zero = !(tot > 0.0);
    if (zero) status[site] |= RT_SITE_ZERO_PROB;
    if constexpr (MIX) root_tot[site] = tot;
    if (!make) return zero;
#pragma unroll
    for (int s = 0; s < N; ++s) {
        if constexpr (MIX) Uarr[idx(0, s)] = ck * (root_w ? root_w[s] : 1.0);
        else Uarr[idx(0, s)] = zero ? 0.0 : (root_w ? root_w[s] : 1.0) / tot;
    }
    for (int v = 1; v < nnodes; ++v) {
        if (tab.cptr[v + 1] == tab.cptr[v]) continue;
        const int p = parent[v];
        double x[N];
        const int k = node_k[p];
        if (k >= 0) lane_obs<N>(obs, compact, K, block_sites, site, k, x);
        else
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] = 1.0;
#pragma unroll
        for (int s = 0; s < N; ++s) x[s] *= Uarr[idx(p, s)];
        for (int e = tab.cptr[p]; e < tab.cptr[p + 1]; ++e) {
            const int w = tab.cidx[e];
            if (w == v) continue;
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] *= Marr[idx(w, s)];
        }
        const double *Pv = P + (size_t)v * N * N;
#pragma unroll
        for (int b = 0; b < N; ++b) {
            double y = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) y += Pv[a * N + b] * x[a];
            Uarr[idx(v, b)] = y;
        }
    }
    return zero;
}

// [row][site] -> [site][row] for a caller's per-site array, 32 x 32 tiles through LDS (TILE = 32;
// a template: only the translation units that launch it hold a copy)
template <int TILE>
__global__ void __launch_bounds__(256)
post_transpose_kernel(long nrows, long nsites, const double *__restrict__ in,
                      double *__restrict__ outT)
{
    static_assert(TILE == 32, "256 threads move 32 x 32 tiles");
    __shared__ double tile[TILE][TILE + 1];
    const long s0 = (long)blockIdx.x * 32, r0 = (long)blockIdx.y * 32;
    const int tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    for (int k = ty; k < 32; k += 8)
        if (r0 + k < nrows && s0 + tx < nsites) tile[k][tx] = in[(size_t)(r0 + k) * nsites + s0 + tx];
    __syncthreads();
    for (int k = ty; k < 32; k += 8)
        if (s0 + k < nsites && r0 + tx < nrows) outT[(size_t)(s0 + k) * nrows + r0 + tx] = tile[tx][k];
}

// ---- the result of a tree-search read (branch_profile.hip, nni.hip, place.hip, spr.hip): the
// kernels leave values [row][site] in the scratch, a chunk of rows at a time where all of them
// would not fit; the caller gets sums [row] and / or values [site][row] ----

// the site-weighted sum of every row, one workgroup per row: thread j adds sites j, j + BS, ... in
// order, then the BS partial sums by halves (fixed rounding).  Sites of zero likelihood and of
// weight 0 are skipped.  tlen (or null; rt_sites_branch_profiles: rows [node][np]): the row of an
// edge of resident length 0 is NaN.  (A template, BS = 256, as the mix_* kernels.)
template <int BS>
__global__ void __launch_bounds__(BS)
post_sums_kernel(long nsites, const double *__restrict__ values, const double *__restrict__ weights,
                 const int *__restrict__ status, int np, const double *__restrict__ tlen,
                 double *__restrict__ sums)
{
    __shared__ double part[BS];
    const size_t row = blockIdx.x;
    const int tid = threadIdx.x;
    const double *x = values + row * nsites;
    double acc = 0.0;
    for (long i = tid; i < nsites; i += BS) {
        const double w = weights ? weights[i] : 1.0;       // (w = 0: not -inf * 0 = NaN)
        if (w != 0.0 && !(status[i] & RT_SITE_ZERO_PROB)) acc += w * x[i];
    }
    part[tid] = acc;
    __syncthreads();
    for (int h = BS / 2; h > 0; h >>= 1) {
        if (tid < h) part[tid] += part[tid + h];
        __syncthreads();
    }
    if (tid != 0) return;
    const size_t v = tlen ? row / np : 0;
    sums[row] = (v > 0 && tlen[v] == 0.0) ? __builtin_nan("") : part[0];
}

constexpr size_t POST_CHUNK_BYTES = (size_t)4 << 30;     // result bytes of one chunk

// The units (moves, queries) of one chunk of `units`: their result within POST_CHUNK_BYTES at
// per_unit bytes each, and with `further` bytes a unit that are no result within what the plan so
// far leaves of the scratch's cap; at most max_units (a grid's y dimension), at least one.
// env: the variable that overrides the chunk's bytes (the tests: many chunks at small sizes).
inline int64_t post_chunk_units(const post_plan &plan, size_t per_unit, size_t further,
                                int64_t max_units, int64_t units, const char *env)
{
    size_t chunk_bytes = POST_CHUNK_BYTES;
    if (const char *e = getenv(env)) {
        const long long v = atoll(e);
        if (v > 0) chunk_bytes = (size_t)v;
    }
    const double room = POST_SCRATCH_CAP - (double)plan.total - 4096.0;
    const size_t fit = room > 0.0 ? (size_t)room / (per_unit + further) : 0;
    const int64_t CH = (int64_t)std::max<size_t>(1, std::min(chunk_bytes / per_unit, fit));
    return std::min(CH, std::max<int64_t>(1, std::min(max_units, units)));
}

struct post_result {
    double *values, *sums;                       // the caller's [site][rows] and [rows], or null
    size_t rows = 0, slab = 0;                   // rows of the whole result, of one transpose launch
    size_t o_sum = 0, o_val = 0, o_valT = 0;
    double *d_sum = nullptr, *d_val = nullptr, *d_valT = nullptr;

    post_result(double *v, double *s) : values(v), sums(s) {}
    // scratch bytes of one row: the values, and their transpose where the caller takes them
    size_t row_bytes(const post_pass *p) const { return (size_t)p->nsites * 8 * (values ? 2 : 1); }
    // after post_layout: the sums of all rows; then (the chunk planned with the sums in the plan)
    // the values of one chunk and the transpose of at most max_rows of them (a grid's y dimension)
    void take_sums(post_pass *p, size_t total_rows)
    {
        rows = total_rows;
        o_sum = p->plan.take(std::max<size_t>(rows, 1) * 8);
    }
    void take_chunk(post_pass *p, size_t chunk_rows, size_t max_rows = ~(size_t)0)
    {
        slab = std::min(chunk_rows, max_rows);
        o_val = p->plan.take(chunk_rows * p->nsites * 8);
        o_valT = p->plan.take(values ? slab * p->nsites * 8 : 8);
    }
    // after post_begin
    void place(const post_pass *p)
    {
        d_sum = (double *)(p->base + o_sum);
        d_val = (double *)(p->base + o_val);
        d_valT = (double *)(p->base + o_valT);
    }
    // the chunk's nrows rows at d_val are rows row0 .. of the result: their sums, and slab by slab
    // their transpose into the caller's array; only what was asked for crosses PCIe.
    // np, d_tlen: post_sums_kernel's.  (A template, as the kernels: only a translation unit that
    // calls it holds a copy of them.)
    template <int BS = 256>
    int chunk(post_pass *p, size_t row0, size_t nrows, int np = 1, const double *d_tlen = nullptr)
    {
        const long nsites = (long)p->nsites;
        if (sums) {
            hipLaunchKernelGGL(post_sums_kernel<BS>, dim3((unsigned)nrows), dim3(BS), 0, p->st, nsites,
                               (const double *)d_val, (const double *)p->s->d_weights,
                               (const int *)p->d_status, np, d_tlen, d_sum + row0);
            RT_HIP(hipGetLastError());
        }
        for (size_t r0 = 0; values && r0 < nrows; r0 += slab) {
            const size_t nr = std::min(slab, nrows - r0);
            hipLaunchKernelGGL(post_transpose_kernel<32>,
                               dim3((unsigned)((nsites + 31) / 32), (unsigned)((nr + 31) / 32)), dim3(256),
                               0, p->st, (long)nr, nsites, (const double *)(d_val + r0 * nsites), d_valT);
            RT_HIP(hipGetLastError());
            // [site][rows of the slab] into the caller's [site][rows]
            RT_HIP(hipMemcpy2DAsync(values + row0 + r0, rows * 8, d_valT, nr * 8, nr * 8, (size_t)nsites,
                                    hipMemcpyDeviceToHost, p->st));
        }
        return RT_OK;
    }
    // after the last chunk: the sums, the status (and log Lambda_i of a mixture) to the caller; the
    // stream is synchronised
    int finish(post_pass *p, int32_t *status, double *loglik = nullptr, const double *d_loglik = nullptr)
    {
        if (sums && rows) RT_HIP(hipMemcpyAsync(sums, d_sum, rows * 8, hipMemcpyDeviceToHost, p->st));
        if (loglik)
            RT_HIP(hipMemcpyAsync(loglik, d_loglik, (size_t)p->nsites * 8, hipMemcpyDeviceToHost, p->st));
        if (status)
            RT_HIP(hipMemcpyAsync(status, p->d_status, (size_t)p->nsites * 4, hipMemcpyDeviceToHost, p->st));
        RT_HIP(hipStreamSynchronize(p->st));
        return RT_OK;
    }
};

// ---- the same of a PARTITIONED batch (rt_sites_branch_profiles_partitioned,
// rt_sites_nni_scores_partitioned, rt_sites_spr_scores_partitioned,
// rt_sites_placements_partitioned): the kernels' PART forms leave values [row][slot]; the caller
// gets set_sums [set][row], sums [row] and / or values [site][row] in caller order ----

// stage 1 of the per-set sums (the shape of branch_expect.hip's part_sums_stage1_kernel, over rows
// [row][slot]): workgroup (row, b, k) adds a contiguous piece of set k's run, thread t every BS-th
// slot of it, then the BS partial sums by halves.  Pads, slots of zero likelihood and sites of
// weight 0 (not -inf * 0 = NaN) are skipped; the weights are in caller order, through `order`.  The
// shape comes from the plan alone: the same bits every call.
template <int BS>
__global__ void __launch_bounds__(BS)
post_part_sums_stage1_kernel(long nslots, const double *__restrict__ values,
                             const unsigned char *__restrict__ is_pad, const long *__restrict__ order,
                             const long *__restrict__ run_begin, const double *__restrict__ weights,
                             const int *__restrict__ status, double *__restrict__ part)
{
    __shared__ double sh[BS];
    const size_t row = blockIdx.x, nrows = gridDim.x;
    const int b = blockIdx.y, nblocks = gridDim.y, k = blockIdx.z, tid = threadIdx.x;
    const long r0 = run_begin[k], r1 = run_begin[k + 1];
    const long per = (r1 - r0 + nblocks - 1) / nblocks;
    const long lo = r0 + (long)b * per, hi = lo + per < r1 ? lo + per : r1;
    const double *x = values + row * nslots;
    double acc = 0.0;
    for (long slot = lo + tid; slot < hi; slot += BS) {
        if (is_pad[slot] || (status[slot] & RT_SITE_ZERO_PROB)) continue;
        const double w = weights ? weights[order[slot]] : 1.0;
        if (w != 0.0) acc += w * x[slot];
    }
    sh[tid] = acc;
    __syncthreads();
    for (int h = BS / 2; h > 0; h >>= 1) {
        if (tid < h) sh[tid] += sh[tid + h];
        __syncthreads();
    }
    if (tid == 0) part[((size_t)k * nblocks + b) * nrows + row] = sh[0];
}

// stage 2: workgroup (row, k) adds set k's stage-1 sums of the row -> set_sums[k][row0 + row].
// set_t (or null; rt_sites_branch_profiles_partitioned: rows [node][np], set_t [set][nnodes]): the
// row of an edge of resident length 0 under a set with a site is NaN.
template <int BS>
__global__ void __launch_bounds__(BS)
post_part_sums_stage2_kernel(const double *__restrict__ part, int nblocks, size_t total_rows,
                             size_t row0, int np, int nnodes, const double *__restrict__ set_t,
                             const long *__restrict__ run_begin, double *__restrict__ set_sums)
{
    __shared__ double sh[BS];
    const size_t row = blockIdx.x, nrows = gridDim.x;
    const int k = blockIdx.y, tid = threadIdx.x;
    double acc = 0.0;
    for (int b = tid; b < nblocks; b += BS) acc += part[((size_t)k * nblocks + b) * nrows + row];
    sh[tid] = acc;
    __syncthreads();
    for (int h = BS / 2; h > 0; h >>= 1) {
        if (tid < h) sh[tid] += sh[tid + h];
        __syncthreads();
    }
    if (tid != 0) return;
    const size_t v = set_t ? (row0 + row) / np : 0;
    const bool dead = v > 0 && run_begin[k + 1] > run_begin[k] && set_t[(size_t)k * nnodes + v] == 0.0;
    set_sums[(size_t)k * total_rows + row0 + row] = dead ? __builtin_nan("") : sh[0];
}

// sums[row]: the per-set rows added in set order (one thread per row)
template <int BS>
__global__ void __launch_bounds__(BS)
post_part_sums_total_kernel(int K, size_t total_rows, size_t row0, size_t nrows,
                            const double *__restrict__ set_sums, double *__restrict__ sums)
{
    const size_t j = (size_t)blockIdx.x * BS + threadIdx.x;
    if (j >= nrows) return;
    double t = 0.0;
    for (int k = 0; k < K; ++k) t += set_sums[(size_t)k * total_rows + row0 + j];
    sums[row0 + j] = t;
}

// slot order -> caller order: rows [row][slot] -> [row][site]; status (or null) with row 0
template <int BS>
__global__ void __launch_bounds__(BS)
post_part_gather_kernel(long nrows, long nslots, long nsites, const long *__restrict__ slot_of_site,
                        const double *__restrict__ val_slot, double *__restrict__ val,
                        const int *__restrict__ status_slot, int *__restrict__ status)
{
    const long i = (long)blockIdx.x * BS + threadIdx.x;
    if (i >= nsites) return;
    const long slot = slot_of_site[i];
    if (status && blockIdx.y == 0) status[i] = status_slot[slot];
    for (long r = blockIdx.y; r < nrows; r += gridDim.y)
        val[(size_t)r * nsites + i] = val_slot[(size_t)r * nslots + slot];
}

// What the PART instances of spr.hip's and place.hip's kernels take beside the plain ones'
// arguments, as ONE trailing argument that the other instances do not have (a parameter pack that
// is empty there: they keep their argument lists and their instruction streams).  A tile (n <= 4: a
// wave, whose 64 slots lie in one granule of 1 << gshift slots) reads its rate set once,
// wave-uniform, and moves its table bases on by set * s_p (the resident tables) and set * s_g (the
// grid's) doubles before anything else; read-only.
struct post_part_arg {
    const int *gset;                             // the set of every granule
    int gshift;
    long s_p, s_g;
};
// (the one argument of a pack that holds one)
template <class T>
__host__ __device__ __forceinline__ T post_pack_one(T x) { return x; }
__device__ __forceinline__ long post_part_set(const post_part_arg &a, long granule)
{
    return __builtin_amdgcn_readfirstlane(a.gset[granule]);
}

// What a tree-search read of a partitioned batch holds beside the single-set one: the sets of the
// batch, a "class weight" per set of the model for post_set_grid (1 for a set with a site, 0 for an
// empty one and for the model's sets past the batch's: no matrices are made for them) and the
// sets' P^T fragments.  The strides are what the kernels' PART forms add per set.
struct post_part {
    const rt_partition *pt = nullptr;
    int64_t K = 0;                               // the batch's sets
    post_set_pt PT;
    std::vector<double> live;                    // [the model's sets]
    size_t o_live = 0;

    // after post_layout
    int take(post_pass *p)
    {
        const rt_rate_sets &r = p->m->multi;
        RT_REQUIRE(r.P_stride == p->N * p->n * p->n, "unexpected stride of the sets' transition matrices");
        pt = p->s->part; K = pt->nsets;
        RT_REQUIRE((int64_t)pt->run_begin.size() == K + 1, "%s: the batch has no plan", p->who);
        RT_REQUIRE(pt->G >= 16 && (pt->G & (pt->G - 1)) == 0, "%s: unexpected granule %lld", p->who,
                   (long long)pt->G);
        live.assign((size_t)r.K, 0.0);
        for (int64_t k = 0; k < K; ++k)
            live[(size_t)k] = pt->run_begin[(size_t)k + 1] > pt->run_begin[(size_t)k] ? 1.0 : 0.0;
        PT.take(p, K);
        o_live = p->plan.take(live.size() * 8);
        return RT_OK;
    }
    // after post_begin
    int begin(post_pass *p)
    {
        PT.place(p);
        p->d_cw = (double *)(p->base + o_live);
        RT_HIP(hipMemcpyAsync(p->base + o_live, live.data(), live.size() * 8, hipMemcpyHostToDevice, p->st));
        return RT_OK;
    }
    long pt_stride() const { return (long)(PT.tab / 8); }
    post_part_arg arg(long s_p, long s_g) const { return {pt->d_granule_set, gshift(), s_p, s_g}; }
    // n <= 4: the granule (256 or 64 slots) as the shift that takes a slot to its granule
    int gshift() const
    {
        int sh = 0;
        while (((int64_t)1 << sh) < pt->G) ++sh;
        return sh;
    }
};

// post_result's interface for a partitioned batch: p->nsites counts the slots, the caller's arrays
// hold the pt->nsites real sites.
struct post_part_result {
    double *values, *sums, *set_sums;            // [site][rows], [rows], [set][rows], or null
    size_t rows = 0, slab = 0, chunk_rows = 0;
    size_t o_sum = 0, o_setsum = 0, o_part = 0, o_val = 0, o_valc = 0, o_valT = 0, o_statc = 0;
    double *d_sum = nullptr, *d_setsum = nullptr, *d_part = nullptr, *d_val = nullptr;
    double *d_valc = nullptr, *d_valT = nullptr;
    int *d_statc = nullptr;

    post_part_result(double *v, double *s, double *ss) : values(v), sums(s), set_sums(ss) {}
    // scratch bytes of one row: the values in slot order, the stage-1 sums, and where the caller
    // takes the values, those in caller order and their transpose
    size_t row_bytes(const post_pass *p) const
    {
        const rt_partition *pt = p->s->part;
        return (size_t)p->nsites * 8 + (size_t)pt->nsets * pt->nblocks * 8 +
               (values ? (size_t)pt->nsites * 16 : 0);
    }
    void take_sums(post_pass *p, size_t total_rows)
    {
        const rt_partition *pt = p->s->part;
        rows = total_rows;
        o_sum = p->plan.take(std::max<size_t>(rows, 1) * 8);
        o_setsum = p->plan.take(std::max<size_t>(rows, 1) * pt->nsets * 8);
        o_statc = p->plan.take((size_t)pt->nsites * 4);
    }
    void take_chunk(post_pass *p, size_t nrows, size_t max_rows = ~(size_t)0)
    {
        const rt_partition *pt = p->s->part;
        chunk_rows = nrows;
        slab = std::min(chunk_rows, max_rows);
        o_val = p->plan.take(chunk_rows * p->nsites * 8);
        o_part = p->plan.take(std::max<size_t>(chunk_rows, 1) * pt->nsets * pt->nblocks * 8);
        o_valc = p->plan.take(values ? chunk_rows * pt->nsites * 8 : 8);
        o_valT = p->plan.take(values ? slab * pt->nsites * 8 : 8);
    }
    // after post_begin
    void place(const post_pass *p)
    {
        d_sum = (double *)(p->base + o_sum); d_setsum = (double *)(p->base + o_setsum);
        d_part = (double *)(p->base + o_part); d_val = (double *)(p->base + o_val);
        d_valc = (double *)(p->base + o_valc); d_valT = (double *)(p->base + o_valT);
        d_statc = (int *)(p->base + o_statc);
    }
    // the chunk's nrows rows at d_val are rows row0 .. of the result.  np, d_set_t: the NaN rule of
    // post_part_sums_stage2_kernel.
    template <int BS = 256>
    int chunk(post_pass *p, size_t row0, size_t nrows, int np = 1, const double *d_set_t = nullptr)
    {
        const rt_partition *pt = p->s->part;
        const long nslots = (long)p->nsites, nreal = (long)pt->nsites;
        const int K = (int)pt->nsets, nb = pt->nblocks;
        if (sums || set_sums) {
            hipLaunchKernelGGL(post_part_sums_stage1_kernel<BS>, dim3((unsigned)nrows, (unsigned)nb, (unsigned)K),
                               dim3(BS), 0, p->st, nslots, (const double *)d_val,
                               (const unsigned char *)pt->d_is_pad, (const long *)pt->d_order,
                               (const long *)pt->d_run_begin, (const double *)p->s->d_weights,
                               (const int *)p->d_status, d_part);
            hipLaunchKernelGGL(post_part_sums_stage2_kernel<BS>, dim3((unsigned)nrows, (unsigned)K), dim3(BS),
                               0, p->st, (const double *)d_part, nb, rows, row0, np, (int)p->N, d_set_t,
                               (const long *)pt->d_run_begin, d_setsum);
            hipLaunchKernelGGL(post_part_sums_total_kernel<BS>, dim3((unsigned)((nrows + BS - 1) / BS)),
                               dim3(BS), 0, p->st, K, rows, row0, nrows, (const double *)d_setsum, d_sum);
            RT_HIP(hipGetLastError());
        }
        if (!values) return RT_OK;
        hipLaunchKernelGGL(post_part_gather_kernel<BS>,
                           dim3((unsigned)((nreal + BS - 1) / BS), (unsigned)std::min<size_t>(nrows, 1024)),
                           dim3(BS), 0, p->st, (long)nrows, nslots, nreal, (const long *)pt->d_slot_of_site,
                           (const double *)d_val, d_valc, (const int *)nullptr, (int *)nullptr);
        RT_HIP(hipGetLastError());
        for (size_t r0 = 0; r0 < nrows; r0 += slab) {
            const size_t nr = std::min(slab, nrows - r0);
            hipLaunchKernelGGL(post_transpose_kernel<32>,
                               dim3((unsigned)((nreal + 31) / 32), (unsigned)((nr + 31) / 32)), dim3(256),
                               0, p->st, (long)nr, nreal, (const double *)(d_valc + r0 * nreal), d_valT);
            RT_HIP(hipGetLastError());
            RT_HIP(hipMemcpy2DAsync(values + row0 + r0, rows * 8, d_valT, nr * 8, nr * 8, (size_t)nreal,
                                    hipMemcpyDeviceToHost, p->st));
        }
        return RT_OK;
    }
    // after the last chunk: the sums and the status (caller order) to the caller; the stream is
    // synchronised
    template <int BS = 256>
    int finish(post_pass *p, int32_t *status)
    {
        const rt_partition *pt = p->s->part;
        const long nreal = (long)pt->nsites;
        if (sums && rows) RT_HIP(hipMemcpyAsync(sums, d_sum, rows * 8, hipMemcpyDeviceToHost, p->st));
        if (set_sums && rows)
            RT_HIP(hipMemcpyAsync(set_sums, d_setsum, rows * pt->nsets * 8, hipMemcpyDeviceToHost, p->st));
        if (status) {
            hipLaunchKernelGGL(post_part_gather_kernel<BS>, dim3((unsigned)((nreal + BS - 1) / BS), 1u),
                               dim3(BS), 0, p->st, 0L, (long)p->nsites, nreal,
                               (const long *)pt->d_slot_of_site, (const double *)nullptr, (double *)nullptr,
                               (const int *)p->d_status, d_statc);
            RT_HIP(hipGetLastError());
            RT_HIP(hipMemcpyAsync(status, d_statc, (size_t)nreal * 4, hipMemcpyDeviceToHost, p->st));
        }
        RT_HIP(hipStreamSynchronize(p->st));
        return RT_OK;
    }
};

// parent [nnodes] of a caller's tree in CSR form (the root's: -1), or what is wrong with it: every
// node but the root is the child of exactly one node before it
inline int post_csr_parents(int64_t nnodes, const int64_t *idx, const int64_t *ptr,
                            std::vector<int32_t> *parent)
{
    RT_REQUIRE(nnodes >= 1 && ptr && (idx || nnodes == 1), "bad arguments");
    RT_REQUIRE(ptr[0] == 0 && ptr[nnodes] == nnodes - 1, "tree_csr_indptr does not describe a tree");
    parent->assign((size_t)nnodes, -1);
    for (int64_t v = 0; v < nnodes; ++v) {
        RT_REQUIRE(ptr[v + 1] >= ptr[v], "tree_csr_indptr not monotone");
        for (int64_t e = ptr[v]; e < ptr[v + 1]; ++e) {
            RT_REQUIRE(idx[e] > v && idx[e] < nnodes, "children not in preorder");
            RT_REQUIRE((*parent)[(size_t)idx[e]] < 0, "node %lld is listed as a child twice",
                       (long long)idx[e]);
            (*parent)[(size_t)idx[e]] = (int32_t)v;
        }
    }
    return RT_OK;
}

}  // namespace
