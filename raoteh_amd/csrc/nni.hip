// Every nearest-neighbour interchange of the model's tree scored on a RESIDENT batch
// (rt_sites_nni_scores): for every site i, every move (v, c, s) -- the subtrees of a child c of v
// and of a sibling s of v exchanged, each keeping its own edge -- and every trial length tau of
// the edge above v,
//     log L_i(tree after the move, t_v -> tau) - log L_i.
//
// With L_v, M_v = P_v L_v of every node from the stored upward pass, up_p the message into
// p = parent(v) from above (root_w at the root) and
//     W[a]    = up_p[a] obs_p[a] prod_{w child of p, w not in {v, s}} M_w[a]
//     L'_v[b] = obs_v[b] prod_{w child of v, w != c} M_w[b] M_s[b]
// the moved tree's likelihood is  sum_b L'_v[b] (P_v(tau)^T (W o M_c))[b].  Nothing is divided:
// the posterior D_p is 0 wherever M_v or M_s is, yet after the move such a state of p may be live,
// so the `up` vectors come from a downward pass of their own,
//     up_v[b] = sum_a P_v[a][b] up_p[a] obs_p[a] prod_{w child of p, w != v} M_w[a],
// normalised once at the root by 1 / L_i: everything after it is the ratio itself, exact where
// transition matrices or observations have zeros and at a resident t_v = 0.  Here:
//
//   1. lengths given: P_v(tau) of every edge and grid point in ONE launch of the model's own
//      exponential (post_grid, what rt_sites_branch_profiles runs); else the resident P_v;
//   2. n > 4: the upward pass with L and M of every step stored, then nni_kernel, one workgroup of
//      NT row-tile waves per 16-site tile: the `up` pass down the schedule, then per node v with
//      moves and per move the staged W o M_c, per grid point one n x n by n x 16 matrix-pipe
//      product dotted with L'_v and reduced over the states in a fixed order; the logs by all
//      lanes at the end.  n <= 4: nni_lane_kernel, one lane per site;
//   3. post_result (post_common.h): the site-weighted sums per (move, point) in a fixed order;
//      then, if the per-site array is asked for, its transpose to [site][move][point].
//
// Steps 2 and 3 run per chunk of moves where the result of all moves would not fit the scratch
// (post_chunk_units).  Nothing of the batch or the model is written; two calls give the same bits.
//
// rt_sites_nni_scores_mixture: the same scores of an ORDINARY batch under a site-class mixture over
// the model's K rate sets, trial lengths as factors of every set's own resident length of the edge
// above v -- the kernels' MIX forms once per set into one accumulator, the root scaled by the class
// weight instead of 1 / L_i.  One host body (nni_read, at the end) serves both calls, and
// rt_sites_nni_scores_partitioned: the same scores of a PARTITIONED batch, every site under its own
// rate set (under set k a moved subtree keeps its own edge of set k), trial lengths as factors -- one
// pass with the kernels' PART forms, every tile under the tables of its granule's set, then the
// per-set sums and the gather to caller order (post_part_result).
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int NNI_CHUNK = 8;                     // grid points between two barriers of nni_kernel

// the stored value: 0 at a site of zero likelihood, else the log of the ratio (-inf where it is
// not positive)
__device__ __forceinline__ double nni_value(double ratio, bool zero)
{
    if (zero) return 0.0;
    return ratio > 0.0 ? log(ratio) : -__builtin_inf();
}

// The move tables are a post_tab (post_common.h) whose first[j] is the index of the first move of
// slot j: moves go by node ascending, then by child of the node, then by sibling.

// n > 4.  steps[i] = {node, step of the parent, stream position of an observed leaf or -1, 1 if
// the node has children}; the root is the last step.  PfragT: [step] A fragments of the resident
// P^T; GfragT: [point][step] those of P(tau)^T (PfragT itself for the plain swap, np = 1);
// Uarr: the `up` vectors, laid out as L and M; out [move - mv0][point][site] for the moves
// mv0 .. mv1 - 1.  The first chunk (mv0 == 0) makes the `up` pass, later ones find it in Uarr.
// (NT = 7: four waves per SIMD asked for, as bp_down_kernel has them -- left alone KS = 28 takes
// 130 VGPRs.  NT = 8 takes 130 .. 136 and runs three: held to 128 it spills to scratch.)
// MIX (rt_sites_nni_scores_mixture, one launch per rate set k of weight ck > 0 and chunk against the
// set's fragments, in set order on one stream): the root is scaled by ck, not by 1 / L_ik -- a set
// under which the resident tree is impossible may be live after a move -- so a move's sum is the
// RAW term ck L_ik(moved tree, tau); it is written to `out` by the first set and added to it by the
// later ones (the same lane, launches in order: a fixed sum).  Every launch makes the `up` pass
// (the scratch is the current set's), L_ik goes to root_tot[site], the status word is the set's
// own, and the logs are mix_log_ratio_kernel's once the sets are in.
// PART (rt_sites_nni_scores_partitioned: sites are the batch's slots, the output is in slot order):
// the workgroup's tile is one granule; the fragment tables of its rate set are gset[tile] * (gs_pt,
// gs_gt) doubles further on (PfragT [set][step], GfragT [set][point][step]; the plain swap: both
// PfragT) -- wave-uniform, a scalar load and two scalar adds before the `up` pass, which takes the
// set's PfragT as it is.
template <int NT, int KS, bool MIX = false, bool PART = false>
__global__ void __launch_bounds__(64 * NT, NT == 7 ? 4 : 1)
nni_kernel(const double *__restrict__ PfragT, const double *__restrict__ GfragT, int np, int nops,
           const int4 *__restrict__ steps, const int *__restrict__ tabp,
           const double *__restrict__ Larr, const double *__restrict__ Marr,
           double *__restrict__ Uarr, const double *__restrict__ obs, int K,
           const double *__restrict__ root_w, int n, int mv0, int mv1, double *__restrict__ out,
           int *__restrict__ status, long nsites, long nblocks, double ck, int first,
           double *__restrict__ root_tot, const int *__restrict__ gset, long gs_pt, long gs_gt)
{
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double red[NT][16];
    __shared__ double sums[2][NNI_CHUNK][NT][16];
    const post_tab tab(tabp, nops);
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    if constexpr (PART) {
        const long gs = __builtin_amdgcn_readfirstlane(gset[blk]);
        PfragT += gs * gs_pt;
        GfragT += gs * gs_gt;
    }
    const long site = blk * 16 + (lane & 15);
    const bool site_ok = site < nsites;
    const bool writer = m == 0 && lane < 16 && site_ok;
    bool live[4];                                // own rows that are states
#pragma unroll
    for (int r = 0; r < 4; ++r) live[r] = 16 * m + 4 * r + (lane >> 4) < n;
    const size_t frag = ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    // 1. root: the site's likelihood sum_states(w L), up = w / it; then the `up` vectors of the
    // nodes with children, a parent before its children (shared with place.hip)
    [[maybe_unused]] const bool zero =
        down_up_pass<NT, KS, MIX>(MIX || mv0 == 0, xb, red, tab, PfragT, nops, steps, Larr, Marr, Uarr,
                                  og, root_w, live, m, lane, blk, nblocks, writer, status, site, ck,
                                  root_tot);
    double a[2 * KP];
    // 2. the moves about every node v with children and siblings
    int par = 0;                                 // the half of `sums` the next chunk writes
    for (int i = nops - 2; i >= 0; --i) {
        const int4 st = steps[i];
        if (!st.w) continue;
        const int pi = st.y;
        const int c0 = tab.cptr[i], c1 = tab.cptr[i + 1], s0 = tab.cptr[pi], s1 = tab.cptr[pi + 1];
        int k = tab.first[i];
        if (s1 - s0 < 2 || k >= mv1 || k + (c1 - c0) * (s1 - s0 - 1) <= mv0) continue;
        const size_t po = down_at<NT>(pi, nblocks, blk, m, lane);
        const int kp = tab.obs[pi], kv = tab.obs[i];
        for (int ec = c0; ec < c1; ++ec)
            for (int es = s0; es < s1; ++es) {
                const int c = tab.cidx[ec], s = tab.cidx[es];
                if (s == i) continue;
                const int mv = k++;
                if (mv < mv0 || mv >= mv1) continue;
                // x = W o M_c on own rows, staged; then lp = L'_v (x is dead by then: the
                // products below hold lp, one fragment table and the accumulator, as
                // bp_down_kernel's -- up_p and the observations are read again per move)
                {
                    double x[4];
                    const size_t co = down_at<NT>(c, nblocks, blk, m, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] = Uarr[po + r * 64] * Marr[co + r * 64];
                    if (kp >= 0) {
                        double ob[4];
                        down_L<KP>(kp, og, Larr, po, m, ob);
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[r] *= ob[r];
                    }
                    for (int e = s0; e < s1; ++e) {
                        const int w = tab.cidx[e];
                        if (w == i || w == s) continue;
                        const size_t wo = down_at<NT>(w, nblocks, blk, m, lane);
#pragma unroll
                        for (int r = 0; r < 4; ++r) x[r] *= Marr[wo + r * 64];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] = live[r] ? x[r] : 0.0;   // (rows past the states)
                    down_stage(xb, m, lane, x);
                }
                double lp[4];
                {
                    const size_t so = down_at<NT>(s, nblocks, blk, m, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) lp[r] = Marr[so + r * 64];
                    if (kv >= 0) {
                        double ob[4];
                        down_L<KP>(kv, og, Larr, so, m, ob);
#pragma unroll
                        for (int r = 0; r < 4; ++r) lp[r] *= ob[r];
                    }
                    for (int e = c0; e < c1; ++e) {
                        const int w = tab.cidx[e];
                        if (w == c) continue;
                        const size_t wo = down_at<NT>(w, nblocks, blk, m, lane);
#pragma unroll
                        for (int r = 0; r < 4; ++r) lp[r] *= Marr[wo + r * 64];
                    }
#pragma unroll
                    for (int r = 0; r < 4; ++r) lp[r] = live[r] ? lp[r] : 0.0;
                }
                double *row = out + (size_t)(mv - mv0) * np * nsites + site;
                // per grid point: sum_b L'_v[b] (P(tau)^T x)[b], one fragment table live at a
                // time.  A chunk of points goes into one half of `sums`; after the barrier wave 0
                // adds the waves in order and stores the ratio while the next chunk fills the
                // other half (the barrier after that chunk is behind these reads)
                for (int g0 = 0; g0 < np; g0 += NNI_CHUNK) {
                    const int cnt = min(NNI_CHUNK, np - g0);
                    for (int j = 0; j < cnt; ++j) {
                        down_frag<KP>(GfragT + ((size_t)(g0 + j) * nops + i) * ASTRIDE + frag, a);
                        const double4_t y = down_product<KS>(a, xb, lane);
                        double v = 0.0;
#pragma unroll
                        for (int r = 0; r < 4; ++r) v += y[r] * lp[r];
                        down_part(sums[par][j], m, lane, v);
                    }
                    __syncthreads();
                    if (writer)
                        for (int j = 0; j < cnt; ++j) {
                            double *x = row + (size_t)(g0 + j) * nsites;
                            const double t = down_total<NT>(sums[par][j], lane);
                            if constexpr (MIX) *x = first ? t : __dadd_rn(*x, t);
                            else *x = t;
                        }
                    par ^= 1;
                }
            }
    }
    if constexpr (MIX) return;
    // the tile's ratios -> values, by all waves: lane group q of the workgroup takes the rows
    // (move, point) q, q + 4 NT, ... of its site (the barrier: wave 0's stores are visible)
    __syncthreads();
    if (site_ok) {
        const long rows = (long)(mv1 - mv0) * np;
        for (long r = 4 * m + (lane >> 4); r < rows; r += 4 * NT) {
            double *x = out + (size_t)r * nsites + site;
            *x = nni_value(*x, zero);
        }
    }
}

// n <= 4: one lane per site; arrays [node][state][site], nodes in preorder; G [point][node][N][N]
// or null for the resident P (the same address in every lane: the scalar path).  MIX: as
// nni_kernel, P and G of the set.
// PART (sites are the batch's slots): a wave's 64 slots lie in one granule of 1 << gshift slots (256
// or 64); P and G of its rate set are gset[site >> gshift] * (gs_p, gs_g) doubles further on ([set][node],
// [set][point][node]) -- wave-uniform, so they stay scalar loads, in the `up` pass too.
template <int N, bool MIX = false, bool PART = false>
__global__ void __launch_bounds__(256)
nni_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const double *__restrict__ G,
                int np, const int *__restrict__ parent, const int *__restrict__ node_k,
                const int *__restrict__ tabp, const void *__restrict__ obs, int compact, int K,
                int block_sites, const double *__restrict__ root_w, double *__restrict__ Larr,
                double *__restrict__ Marr, double *__restrict__ Uarr, int mv0, int mv1,
                double *__restrict__ out, int *__restrict__ status, double ck, int first,
                double *__restrict__ root_tot, const int *__restrict__ gset, int gshift, long gs_p,
                long gs_g)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    if constexpr (PART) {
        const long gs = __builtin_amdgcn_readfirstlane(gset[site >> gshift]);
        P += gs * gs_p;
        G += gs * gs_g;                          // (the plain swap: the host gives P as G)
    }
    const post_tab tab(tabp, nnodes);
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    auto node_obs = [&](int v, double (&x)[N]) {
        const int k = node_k[v];
        if (k >= 0) lane_obs<N>(obs, compact, K, block_sites, site, k, x);
        else
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] = 1.0;
    };
    if (MIX || mv0 == 0)
        lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, K, block_sites, Larr,
                         Marr);
    // the `up` vectors: the root, then every node with children after its parent
    [[maybe_unused]] const bool zero =
        lane_up_pass<N, MIX>(MIX || mv0 == 0, nnodes, nsites, site, P, parent, node_k, tab, obs, compact,
                             K, block_sites, root_w, Larr, Marr, Uarr, status, ck, root_tot);
    for (int v = 1; v < nnodes; ++v) {
        const int p = parent[v];
        const int c0 = tab.cptr[v], c1 = tab.cptr[v + 1], s0 = tab.cptr[p], s1 = tab.cptr[p + 1];
        int k = tab.first[v];
        if (c1 == c0 || s1 - s0 < 2 || k >= mv1 || k + (c1 - c0) * (s1 - s0 - 1) <= mv0) continue;
        double base[N], lv[N];
        node_obs(p, base);
        node_obs(v, lv);
#pragma unroll
        for (int s = 0; s < N; ++s) base[s] *= Uarr[idx(p, s)];
        for (int ec = c0; ec < c1; ++ec)
            for (int es = s0; es < s1; ++es) {
                const int c = tab.cidx[ec], sb = tab.cidx[es];
                if (sb == v) continue;
                const int mv = k++;
                if (mv < mv0 || mv >= mv1) continue;
                double x[N], lp[N];
#pragma unroll
                for (int s = 0; s < N; ++s) {
                    x[s] = base[s] * Marr[idx(c, s)];
                    lp[s] = lv[s] * Marr[idx(sb, s)];
                }
                for (int e = s0; e < s1; ++e) {
                    const int w = tab.cidx[e];
                    if (w == v || w == sb) continue;
#pragma unroll
                    for (int s = 0; s < N; ++s) x[s] *= Marr[idx(w, s)];
                }
                for (int e = c0; e < c1; ++e) {
                    const int w = tab.cidx[e];
                    if (w == c) continue;
#pragma unroll
                    for (int s = 0; s < N; ++s) lp[s] *= Marr[idx(w, s)];
                }
                for (int g = 0; g < np; ++g) {
                    const double *Gv = G ? G + ((size_t)g * nnodes + v) * N * N : P + (size_t)v * N * N;
                    double t = 0.0;
#pragma unroll
                    for (int b = 0; b < N; ++b) {
                        double y = 0.0;
#pragma unroll
                        for (int a = 0; a < N; ++a) y += Gv[a * N + b] * x[a];
                        t += y * lp[b];
                    }
                    double *o = out + ((size_t)(mv - mv0) * np + g) * nsites + site;
                    if constexpr (MIX) *o = first ? t : __dadd_rn(*o, t);
                    else *o = nni_value(t, zero);
                }
            }
    }
}

// the moves in their order: v ascending, then the children c of v, then the siblings s of v, both
// in CSR order.  first (or null): [nnodes] the index of every node's first move; moves (or null):
// the triples
int64_t nni_enumerate(int64_t N, const int64_t *idx, const int64_t *ptr, const int32_t *parent,
                      int32_t *first, int32_t *moves)
{
    int64_t k = 0;
    for (int64_t v = 0; v < N; ++v) {
        if (first) first[v] = (int32_t)k;
        if (!v) continue;
        const int64_t p = parent[v];
        for (int64_t ec = ptr[v]; ec < ptr[v + 1]; ++ec)
            for (int64_t es = ptr[p]; es < ptr[p + 1]; ++es) {
                if (idx[es] == v) continue;
                if (moves) {
                    moves[3 * k] = (int32_t)v;
                    moves[3 * k + 1] = (int32_t)idx[ec];
                    moves[3 * k + 2] = (int32_t)idx[es];
                }
                ++k;
            }
    }
    return k;
}

int64_t nni_enumerate(const rt_model *m, int32_t *first, int32_t *moves)
{
    return nni_enumerate(m->nnodes, m->indices.data(), m->indptr.data(), m->parent.data(), first, moves);
}

int nni_moves_out(int64_t cnt, int32_t *moves, int64_t capacity, int64_t *nmoves)
{
    *nmoves = cnt;
    RT_REQUIRE(!moves || capacity >= cnt, "the tree has %lld moves, the array holds %lld",
               (long long)cnt, (long long)capacity);
    return RT_OK;
}

}  // namespace

extern "C" int rt_model_nni_moves(const rt_model *m, int32_t *moves, int64_t capacity, int64_t *nmoves)
{
    RT_REQUIRE(m && nmoves, "null pointer");
    RT_TRY(nni_moves_out(nni_enumerate(m, nullptr, nullptr), moves, capacity, nmoves));
    if (moves) nni_enumerate(m, nullptr, moves);
    return RT_OK;
}

extern "C" int rt_tree_nni_moves(int64_t nnodes, const int64_t *idx, const int64_t *ptr,
                                 int32_t *moves, int64_t capacity, int64_t *nmoves)
{
    RT_REQUIRE(nmoves, "bad arguments");
    // (the moves of v go through the children of its parent: every node but the root has one)
    std::vector<int32_t> parent;
    RT_TRY(post_csr_parents(nnodes, idx, ptr, &parent));
    RT_TRY(nni_moves_out(nni_enumerate(nnodes, idx, ptr, parent.data(), nullptr, nullptr), moves,
                         capacity, nmoves));
    if (moves) nni_enumerate(nnodes, idx, ptr, parent.data(), nullptr, moves);
    return RT_OK;
}

namespace {

// Both reads.  MIX = false: the pass runs once under the model's own matrices, `trial` are lengths
// (post_grid), the plain kernel instance divides by L_i at the root and makes the `up` pass in the
// first chunk only.  MIX = true: per chunk once per rate set of positive class weight over one L,
// M, U scratch -- the upward pass through a view of set k's tables (post_up_set), then the MIX
// instance, which makes the `up` pass every time and adds the term c_k L_ik(moved tree, tau) into
// ONE accumulator [move][point][site] in set order; `trial` are factors (post_set_grid), post_mix
// turns the accumulator into the values.  Nothing is divided before the end: exact where
// L_ik == 0 on the resident tree.  PART (a partitioned batch): as MIX = false, every tile under the
// tables of its own set -- `trial` are factors, the set grid makes matrices for the sets that have
// a site, the PART instance picks its tile's; the sums go per set over the runs of the plan and the
// result leaves in caller order (post_part_result).
template <bool MIX, bool PART = false>
int nni_read(const char *who, rt_model *m, rt_sites *s, int recompute_transitions,
             const double *class_weights, int64_t npoints, const double *trial, double *values,
             double *sums, double *set_sums, double *loglik, int32_t *status)
{
    static_assert(!(MIX && PART), "a mixture is read on an ordinary batch");
    using grid_t = std::conditional_t<MIX || PART, post_set_grid, post_grid>;
    using result_t = std::conditional_t<PART, post_part_result, post_result>;
    post_pass p;                                 // (alive until the synchronisation below)
    if (PART) RT_TRY(post_partitioned_only(who, s));
    RT_TRY(post_open(&p, who, m, s, PART));
    if (MIX) RT_TRY(post_class_weights(who, m, class_weights));
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    // the moves; the rows of `trial` that count are those of the nodes with one
    std::vector<int32_t> first((size_t)N + 1, 0);
    const int64_t nmoves = nni_enumerate(m, first.data(), nullptr);
    first[(size_t)N] = (int32_t)nmoves;
    std::vector<unsigned char> has_move((size_t)N, 0);
    for (int64_t v = 1; v < N; ++v) has_move[(size_t)v] = first[(size_t)v + 1] > first[(size_t)v];
    if (trial) RT_TRY(grid_t::check(&p, recompute_transitions, npoints, trial, has_move.data()));
    RT_REQUIRE(trial || npoints == 1, "%s: without %s the edge above v keeps its %s: 1 grid point "
               "(%lld here)", who, MIX || PART ? "factors" : "lengths", MIX || PART ? "matrices" : "matrix",
               (long long)npoints);
    RT_REQUIRE(nmoves * npoints < (int64_t)1 << 31, "%s: too many moves", who);
    const int np = (int)npoints;
    p.per_set = MIX;
    RT_TRY(post_layout(&p, true));
    grid_t grid;                                 // (alive until the synchronisation below)
    post_mix mix;
    post_part part;
    result_t res = [&] {
        if constexpr (PART) return post_part_result(values, sums, set_sums);
        else return post_result(values, sums);
    }();
    if (trial) RT_TRY(grid.take(&p, np));
    if (MIX) RT_TRY(mix.take(&p, class_weights));
    if (PART) RT_TRY(part.take(&p));
    const int cnt = p.lane ? (int)N : p.nops;    // slots of the move tables
    const size_t tab_ints = (size_t)4 * cnt;
    const size_t o_tab = p.plan.take(tab_ints * 4);
    res.take_sums(&p, (size_t)nmoves * np);
    // the chunks of moves: at most what the grids' y takes of (move, point) rows
    const int64_t CH = post_chunk_units(p.plan, np * res.row_bytes(&p), 0, ((int64_t)1 << 21) / np, nmoves,
                                        "RAOTEH_NNI_CHUNK_BYTES");
    res.take_chunk(&p, (size_t)CH * np);
    RT_TRY(post_begin(&p, recompute_transitions));
    res.place(&p);
    if (MIX) RT_TRY(mix.begin(&p));
    if (PART) RT_TRY(part.begin(&p));
    hipStream_t st = p.st;
    int *d_tab = (int *)(p.base + o_tab);
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    if (trial) RT_TRY(grid.launch(&p, trial, has_move.data()));
    RT_TRY(post_up(&p, internal.data(), !MIX && !PART));
    // the move tables, by step (n > 4) or by node
    std::vector<int32_t> tab;
    post_tab_build(&p, first.data(), &tab);
    RT_HIP(hipMemcpyAsync(d_tab, tab.data(), tab_ints * 4, hipMemcpyHostToDevice, st));
    if (!p.lane) {
        if (MIX) RT_TRY(mix.PT.pack(&p));
        if (PART) RT_TRY(part.PT.pack(&p));
        if (trial) RT_TRY(grid.pack(&p));
    }
    for (int64_t mv0 = 0; mv0 == 0 || mv0 < nmoves; mv0 += CH) {
        const int64_t mv1 = std::min(nmoves, mv0 + CH);
        const size_t rows = (size_t)(mv1 - mv0) * np;
        // the pass; MIX: set by set (a set of weight zero is never live: not run, never read)
        int first_set = 1;
        for (int64_t k = 0; k < (MIX ? mix.K : 1); ++k) {
            const double ck = MIX ? class_weights[k] : 1.0;
            if (!(ck > 0.0)) continue;
            // without trial lengths: the resident matrices (n <= 4: no G; else their fragments)
            const double *P = m->d_P, *G = trial ? grid.d_G : nullptr;
            const double *PT = p.d_PT, *GT = trial ? grid.d_GT : p.d_PT;
            int *stat = p.d_status;
            double *tot = nullptr;
            if constexpr (MIX) {
                P = mix.P_of(&p, k); G = trial ? grid.G_of_set(&p, k) : nullptr;
                PT = mix.PT.of_set(k); GT = trial ? grid.GT_of_set(k) : PT;
                stat = mix.status_of(&p, k); tot = mix.tot_of(&p, k);
            }
            const int *gset = nullptr;
            int gshift = 0;
            long gs_p = 0, gs_g = 0, gs_pt = 0, gs_gt = 0;
            if constexpr (PART) {
                P = m->multi.d_P; PT = part.PT.d_PT; GT = trial ? grid.d_GT : PT;
                gset = part.pt->d_granule_set; gshift = part.gshift();
                // (n <= 4, the plain swap: the sets' P as the one-point grid [set][node])
                if (!trial) G = P;
                gs_p = (long)m->multi.P_stride; gs_g = trial ? (long)((size_t)np * N * n * n) : gs_p;
                gs_pt = part.pt_stride(); gs_gt = trial ? (long)((size_t)np * grid.tab) : gs_pt;
            }
            if (p.lane) {
                const int *d_ptab = p.d_ptab;
                RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                    hipLaunchKernelGGL((nni_lane_kernel<decltype(nv)::value, MIX, PART>),
                                       dim3((unsigned)((nsites + 255) / 256)), dim3(256), 0, st, (int)N,
                                       (long)nsites, P, G, np, d_ptab, d_ptab + N, (const int *)d_tab,
                                       (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                                       s->block_sites, (const double *)m->d_root, p.d_L, p.d_M, p.d_D,
                                       (int)mv0, (int)mv1, res.d_val, stat, ck, first_set, tot, gset,
                                       gshift, gs_p, gs_g);
                    return RT_OK;
                }));
            } else {
                const rt_sites *x = p.x;
                if (MIX) RT_TRY(post_up_set(&p, k, nullptr));
                RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
                    constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
                    hipLaunchKernelGGL((nni_kernel<NT, KS, MIX, PART>), dim3((unsigned)x->nblocks),
                                       dim3(64 * NT), 0, st, PT, GT, np, p.nops, (const int4 *)p.d_steps,
                                       (const int *)d_tab, (const double *)p.d_L, (const double *)p.d_M,
                                       p.d_D, (const double *)x->d_obs, (int)x->nobs,
                                       (const double *)m->d_root, (int)n, (int)mv0, (int)mv1, res.d_val,
                                       stat, (long)x->nsites, (long)x->nblocks, ck, first_set, tot,
                                       gset, gs_pt, gs_gt);
                    return RT_OK;
                }));
            }
            RT_HIP(hipGetLastError());
            first_set = 0;
        }
        if (MIX && mv0 == 0) RT_TRY(mix.post(&p));           // (log Lambda_i, the status)
        if (!rows) break;                        // (no moves: the status, MIX: the log-likelihood)
        if (MIX && (values || sums)) RT_TRY(mix.log_ratio(&p, rows, np, nullptr, res.d_val));
        // the weighted site sums and the per-site array [site][nmoves][np]
        RT_TRY(res.chunk(&p, (size_t)mv0 * np, rows));
    }
    if constexpr (PART) RT_TRY(res.finish(&p, status));
    else RT_TRY(res.finish(&p, status, loglik, mix.d_ll));
    if (trial) RT_TRY(grid.result(&p));
    return RT_OK;
}

}  // namespace

extern "C" int rt_sites_nni_scores(rt_model *m, rt_sites *s, int recompute_transitions,
                                   int64_t npoints, const double *lengths, double *values,
                                   double *sums, int32_t *status)
{
    return nni_read<false>("rt_sites_nni_scores", m, s, recompute_transitions, nullptr, npoints, lengths,
                           values, sums, nullptr, nullptr, status);
}

extern "C" int rt_sites_nni_scores_mixture(rt_model *m, rt_sites *s, int recompute_transitions,
                                           const double *class_weights, int64_t npoints,
                                           const double *factors, double *values, double *sums,
                                           double *loglik, int32_t *status)
{
    return nni_read<true>("rt_sites_nni_scores_mixture", m, s, recompute_transitions, class_weights,
                          npoints, factors, values, sums, nullptr, loglik, status);
}

extern "C" int rt_sites_nni_scores_partitioned(rt_model *m, rt_sites *s, int recompute_transitions,
                                               int64_t npoints, const double *factors, double *values,
                                               double *sums, double *set_sums, int32_t *status)
{
    return nni_read<false, true>("rt_sites_nni_scores_partitioned", m, s, recompute_transitions, nullptr,
                                 npoints, factors, values, sums, set_sums, nullptr, status);
}

