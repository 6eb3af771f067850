// Per-branch likelihood profiles of a RESIDENT batch (rt_sites_branch_profiles): for every site i,
// every edge p -> v and every length tau of a grid of that edge,
//     log L_i(t_v -> tau) - log L_i,        every other branch at its resident length.
//
// The downward pass of posterior.hip / branch_expect.hip holds u = D_p / (P_v L_v) and L_v at
// every step.  The site's likelihood is linear in the edge's transition matrix, and with
// J[a][b] = u[a] P_v[a][b] L_v[b] the joint endpoint posterior,
//     L_i(t_v -> tau) / L_i = sum_{a,b} J[a][b] P_v(tau)[a][b] / P_v[a][b]
//                           = sum_b L_v[b] (P_v(tau)^T u)[b],      P_v(tau) = expm(tau Q_v):
// the contraction of be_down_kernel with P_v(tau)^T in the place of G_k^T.  (Exact while the
// resident t_v > 0: where (P_v L_v)[a] = 0, Q_v reaches no state of supp(L_v) from a at any
// length.  At t_v = 0, P_v = I and u has lost the states the other lengths would reach: such an
// edge's row is NaN.)  Here:
//
//   1. P_v(tau) of every edge and grid point in ONE launch of the model's own exponential
//      (rt_launch_expm, or rt_launch_spectral for spectral rates) over tiled qidx / tau arrays,
//      laid out [point][node][n][n] like the model's transition matrices;
//   2. n > 4: rt_launch_pack_pt per grid point, the upward pass with L and M of every step stored,
//      then bp_down_kernel: be_down_kernel with a run-time loop over the grid points; per step u
//      is staged once, per point one n x n by n x 16 matrix-pipe product reduced over the states
//      in a fixed order and stored (coalesced over the sites); the logs by all lanes at the end.
//      n <= 4: bp_lane_kernel, one lane per site;
//   3. post_result (post_common.h): the site-weighted sums per (node, point) in a fixed order;
//      then, if the per-site array is asked for, its transpose to [site][node][point].
//
// Nothing of the batch or the model is written; two calls give the same bits.
//
// rt_sites_branch_profiles_mixture: the same read of an ORDINARY batch under a site-class mixture
// over the model's K rate sets, trial lengths as factors of every set's own resident lengths.  One
// host body (bp_read) serves both; under the mixture
//   1. is P_kv(factor t_kv) of every set, point and edge in ONE launch of the sets' exponential
//      (post_set_grid), their transposes and the sets' P^T as A fragments (post_set_pt);
//   2. runs per set k with c_k > 0, on the one stream over one L, M, D scratch: the upward pass
//      through a view of set k's tables (post_up_set), then the MIX instance of the kernel against
//      set k's fragments -- the term c_k L_ik(tau) into ONE accumulator [node][point][site], the
//      sets added in set order, L_ik and a status word per set; then mix_post_kernel (log
//      Lambda_i, the status of the live sets) and mix_log_ratio_kernel (the accumulator -> values).
//
// rt_sites_branch_profiles_partitioned: the same read of a PARTITIONED batch, every site under its
// own rate set, trial lengths as factors of that set's resident lengths; bp_read again:
//   1. as under the mixture, for the sets that have a site (post_part: weight 1, an empty set 0);
//   2. ONE pass: the stored upward pass of the twin through the batch's granule_set (post_up), then
//      the PART instance of the kernel, every tile (n <= 4: every wave) against the fragments,
//      trial fragments and resident lengths of its granule's set;
//   3. post_part_result (post_common.h): per (set, node, point) the fixed-order two-stage sum over
//      the set's run with the pads skipped, the per-set rows added in set order, and the gather of
//      the values and the status into caller order.
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <cmath>
#include <limits>
#include <vector>

namespace {

constexpr int BP_CHUNK = 8;      // grid points between two barriers of bp_down_kernel

// the stored value: 0 at a site of zero likelihood, NaN on an edge of resident length 0, else the
// log of the ratio (-inf where it is not positive)
__device__ __forceinline__ double bp_value(double ratio, bool zero, double tv)
{
    if (zero) return 0.0;
    if (tv == 0.0) return __builtin_nan("");
    return ratio > 0.0 ? log(ratio) : -__builtin_inf();
}

// steps[i] = {node, step of the parent, stream position of an observed leaf or -1, 1 if the node
// has children}; the root is the last step.  GfragT: [point][step] A fragments of P(tau)^T;
// tlen: the resident lengths [node]; out [node][point][site].
// MIX (rt_sites_branch_profiles_mixture, one launch per rate set k of weight ck > 0 against the
// set's fragments, in set order on one stream): the root's sum L_ik goes to root_tot[site], the
// status word is the set's own, and the RAW term ck L_ik * ratio = ck L_ik(tau) is written to `out`
// by the first set and added to it by the later ones (the same lane, launches in order: a fixed
// sum); the logs are mix_log_ratio_kernel's, once the sets are in.
// PART (rt_sites_branch_profiles_partitioned: sites are the batch's slots, the output is in slot
// order): the workgroup's tile is one granule; the tables of its rate set are gset[tile] * (gs_pt,
// gs_gt, gs_t) doubles further on -- PfragT [set][step], GfragT [set][point][step], tlen
// [set][node] -- wave-uniform, a scalar load and three scalar adds before the first fragment load.
template <int NT, int KS, bool MIX = false, bool PART = false>
__global__ void __launch_bounds__(64 * NT)
bp_down_kernel(const double *__restrict__ PfragT, const double *__restrict__ GfragT, int np, int nops,
               const int4 *__restrict__ steps, const double *__restrict__ Larr,
               const double *__restrict__ Marr, double *__restrict__ Darr,
               const double *__restrict__ obs, int K, const double *__restrict__ root_w,
               const double *__restrict__ tlen, int n, double *__restrict__ out,
               int *__restrict__ status, long nsites, long nblocks, double ck, int first,
               double *__restrict__ root_tot, const int *__restrict__ gset, long gs_pt, long gs_gt,
               long gs_t)
{
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double red[NT][16];
    __shared__ double sums[2][BP_CHUNK][NT][16];
    [[maybe_unused]] double scale = 0.0;         // MIX: ck L_ik of the lane's site
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    if constexpr (PART) {
        const long gs = __builtin_amdgcn_readfirstlane(gset[blk]);
        PfragT += gs * gs_pt;
        GfragT += gs * gs_gt;
        tlen += gs * gs_t;
    }
    const long site = blk * 16 + (lane & 15);
    const bool site_ok = site < nsites;
    const bool writer = m == 0 && lane < 16 && site_ok;
    bool bad = false, zero;
    // root: D = w L / sum_states(w L); its row of the output is 0
    {
        const int i = nops - 1;
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        double wl[4], s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + 4 * r + (lane >> 4);
            const double w = row < n ? (root_w ? root_w[row] : 1.0) : 0.0;
            wl[r] = w * Larr[o + r * 64];
            s += wl[r];
        }
        down_part(red, m, lane, s);
        __syncthreads();
        const double tot = down_total<NT>(red, lane & 15);
        zero = !(tot > 0.0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Darr[o + r * 64] = zero ? 0.0 : wl[r] / tot;
        if constexpr (MIX) scale = zero ? 0.0 : __dmul_rn(ck, tot);
        if (writer) {
            if (zero) atomicOr(&status[site], RT_SITE_ZERO_PROB);
            if constexpr (MIX) root_tot[site] = tot;
            double *row = out + (size_t)steps[i].x * np * nsites + site;
            if (!MIX || first)
                for (int g = 0; g < np; ++g) row[(size_t)g * nsites] = 0.0;
        }
    }
    const size_t frag = ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    int par = 0;                                 // the half of `sums` the next chunk writes
    for (int i = nops - 2; i >= 0; --i) {
        const int4 st = steps[i];
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        double L[4], u[4];
        down_L<KP>(st.z, og, Larr, o, m, L);
        down_u(Darr, down_at<NT>(st.y, nblocks, blk, m, lane), Marr, o, u, bad);
        down_stage(xb, m, lane, u);
        double a[2 * KP];
        if (st.w) {                              // D_v = (P^T u) * L for the children's steps
            down_frag<KP>(PfragT + (size_t)i * ASTRIDE + frag, a);
            const double4_t acc = down_product<KS>(a, xb, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) Darr[o + r * 64] = acc[r] * L[r];
        }
        double *row = out + (size_t)st.x * np * nsites + site;
        // per grid point: sum_b L[b] (P(tau)^T u)[b], one fragment table live at a time.  A chunk
        // of points goes into one half of `sums`; after the barrier wave 0 adds the waves in
        // order and stores the ratio while the next chunk fills the other half (the barrier after
        // that chunk is behind these reads: one barrier per chunk).  The logs wait for the end
        // of the kernel, where nothing of the pass is live in registers
        for (int g0 = 0; g0 < np; g0 += BP_CHUNK) {
            const int cnt = min(BP_CHUNK, np - g0);
            for (int j = 0; j < cnt; ++j) {
                down_frag<KP>(GfragT + ((size_t)(g0 + j) * nops + i) * ASTRIDE + frag, a);
                const double4_t y = down_product<KS>(a, xb, lane);
                double v = 0.0;
#pragma unroll
                for (int r = 0; r < 4; ++r) v += y[r] * L[r];
                down_part(sums[par][j], m, lane, v);
            }
            __syncthreads();
            if (writer)
                for (int j = 0; j < cnt; ++j) {
                    double *x = row + (size_t)(g0 + j) * nsites;
                    const double t = down_total<NT>(sums[par][j], lane);
                    if constexpr (MIX) *x = first ? __dmul_rn(scale, t) : __dadd_rn(*x, __dmul_rn(scale, t));
                    else *x = t;
                }
            par ^= 1;
        }
    }
    if (bad && site_ok) atomicOr(&status[site], 2);
    if constexpr (MIX) return;
    // the tile's ratios -> values, by all waves: lane group q of the workgroup takes the rows
    // (node, point) q, q + 4 NT, ... of its site (the barrier: wave 0's stores are visible)
    __syncthreads();
    if (site_ok) {
        const long rows = (long)(nops - 1) * np;
        for (long k = 4 * m + (lane >> 4); k < rows; k += 4 * NT) {
            const int node = steps[k / np].x;
            double *x = out + ((size_t)node * np + k % np) * nsites + site;
            *x = bp_value(*x, zero, tlen[node]);
        }
    }
}

// n <= 4: one lane per site; arrays [node][state][site], nodes in preorder; G [point][node][N][N]
// (the same address in every lane: the scalar path).  MIX: as bp_down_kernel, P and G of the set.
// PART (sites are the batch's slots): a wave's 64 slots lie in one granule of 1 << gshift slots (256
// or 64); P, G and tlen of its rate set are gset[site >> gshift] * (gs_p, gs_g, nnodes) doubles further on
// ([set][node], [set][point][node], [set][node]) -- wave-uniform, so they stay scalar loads.
template <int N, bool MIX = false, bool PART = false>
__global__ void __launch_bounds__(256)
bp_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const double *__restrict__ G,
               int np, const int *__restrict__ parent, const int *__restrict__ node_k,
               const void *__restrict__ obs, int compact, int K, int block_sites,
               const double *__restrict__ root_w, const double *__restrict__ tlen,
               double *__restrict__ Larr, double *__restrict__ Marr, double *__restrict__ Darr,
               double *__restrict__ out, int *__restrict__ status, double ck, int first,
               double *__restrict__ root_tot, const int *__restrict__ gset, int gshift, long gs_p,
               long gs_g)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    if constexpr (PART) {
        const long gs = __builtin_amdgcn_readfirstlane(gset[site >> gshift]);
        P += gs * gs_p;
        G += gs * gs_g;
        tlen += gs * nnodes;
    }
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, K, block_sites, Larr, Marr);
    // down: the root, then every node after its parent
    bool zero;
    [[maybe_unused]] double scale = 0.0;         // MIX: ck L_ik
    {
        double d[N], tot = 0.0;
        zero = lane_root<N>(nsites, site, root_w, Larr, Darr, d, MIX ? &tot : nullptr);
        if (zero) status[site] |= RT_SITE_ZERO_PROB;
        if constexpr (MIX) {
            root_tot[site] = tot;
            scale = zero ? 0.0 : __dmul_rn(ck, tot);
        }
        if (!MIX || first)
            for (int g = 0; g < np; ++g) out[(size_t)g * nsites + site] = 0.0;
    }
    bool bad = false;
    for (int v = 1; v < nnodes; ++v) {
        const int p = parent[v];
        const double *Pv = P + (size_t)v * N * N;
        double u[N], L[N];
        lane_u<N>(nsites, site, p, v, Darr, Marr, u, bad);
#pragma unroll
        for (int b = 0; b < N; ++b) {
            L[b] = Larr[idx(v, b)];
            double y = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) y += Pv[a * N + b] * u[a];
            Darr[idx(v, b)] = y * L[b];
        }
        [[maybe_unused]] const double tv = MIX ? 1.0 : tlen[v];
        for (int g = 0; g < np; ++g) {
            const double *Gv = G + ((size_t)g * nnodes + v) * N * N;
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) {
                double y = 0.0;
#pragma unroll
                for (int a = 0; a < N; ++a) y += Gv[a * N + b] * u[a];
                t += y * L[b];
            }
            double *x = out + ((size_t)v * np + g) * nsites + site;
            if constexpr (MIX) *x = first ? __dmul_rn(scale, t) : __dadd_rn(*x, __dmul_rn(scale, t));
            else *x = bp_value(t, zero, tv);
        }
    }
    if (bad) status[site] |= 2;
}

}  // namespace

extern "C" int rt_model_get_branch_lengths(rt_model *m, double *t)
{
    RT_REQUIRE(m && t, "null pointer");
    RT_REQUIRE(post_model_has_rates(m),
               "rt_model_get_branch_lengths: no rates have been set (rt_model_set_rates or "
               "rt_model_set_rates_spectral)");
    std::copy(m->h_t.begin(), m->h_t.end(), t);
    return RT_OK;
}

namespace {

__global__ void __launch_bounds__(256)
set_grid_args_kernel(int K, int np, int nnodes, const int *__restrict__ set_qidx,
                     const double *__restrict__ set_t, const double *__restrict__ fac,
                     const double *__restrict__ cw, int nabs, const double *__restrict__ abs_tau,
                     const double *__restrict__ abs_scale, int *__restrict__ qidx,
                     double *__restrict__ tau)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= (long)K * np * nnodes) return;
    const int v = (int)(j % nnodes), g = (int)(j / nnodes % np), k = (int)(j / nnodes / np);
    const bool run = v > 0 && cw[k] > 0.0;
    qidx[j] = run ? set_qidx[(size_t)k * nnodes + v] : -1;
    double x = 0.0;
    if (run) {
        // (the last nabs points: an absolute length, the set's scale times the point's)
        if (g >= np - nabs) x = abs_scale[k] * abs_tau[g - (np - nabs)];
        else x = fac[(size_t)v * np + g] * set_t[(size_t)k * nnodes + v];
    }
    tau[j] = x;
}

}  // namespace

int rt_launch_set_grid_args(rt_ctx *ctx, int K, int np, int nnodes, const int32_t *d_set_qidx,
                            const double *d_set_t, const double *d_fac, const double *d_cw,
                            int nabs, const double *d_abs_tau, const double *d_abs_scale,
                            int32_t *d_qidx, double *d_tau)
{
    const long cnt = (long)K * np * nnodes;
    hipLaunchKernelGGL(set_grid_args_kernel, dim3((unsigned)((cnt + 255) / 256)), dim3(256), 0, ctx->stream,
                       K, np, nnodes, (const int *)d_set_qidx, d_set_t, d_fac, d_cw, nabs, d_abs_tau,
                       d_abs_scale, (int *)d_qidx, d_tau);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

namespace {

// The three reads.  MIX = false: the pass runs once under the model's own matrices, `trial` are
// lengths (post_grid), the plain kernel instance divides by L_i at the root.  MIX = true: once per
// rate set of positive class weight, `trial` are factors (post_set_grid), the MIX instances
// accumulate and post_mix turns the accumulator into the values.  PART (a partitioned batch): the
// pass runs once, every tile under the tables of its own set -- `trial` are factors, the set grid
// makes matrices for the sets that have a site, the PART instance picks its tile's; the sums go per
// set over the runs of the plan and the result leaves in caller order (post_part_result).
template <bool MIX, bool PART = false>
int bp_read(const char *who, rt_model *m, rt_sites *s, int recompute_transitions,
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
    RT_TRY(grid_t::check(&p, recompute_transitions, npoints, trial));
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    const int np = (int)npoints;
    p.per_set = MIX;
    RT_TRY(post_layout(&p, true));
    const size_t rows = (size_t)N * np;
    // scratch: L, M, D of every node and site (post_layout), the result, the grid matrices, their
    // fragments and the tiled arguments of the exponential (the grid), the mixture's pieces
    grid_t grid;                                 // (alive until the synchronisation below)
    post_mix mix;
    post_part part;
    result_t res = [&] {
        if constexpr (PART) return post_part_result(values, sums, set_sums);
        else return post_result(values, sums);
    }();
    res.take_sums(&p, rows);
    res.take_chunk(&p, rows);
    size_t o_dead = 0, o_tl = 0;
    if (MIX) {
        RT_TRY(mix.take(&p, class_weights));
        o_dead = p.plan.take((size_t)N * 4);
        o_tl = p.plan.take((size_t)N * 8);
    }
    if (PART) RT_TRY(part.take(&p));
    RT_TRY(grid.take(&p, np));
    RT_TRY(post_begin(&p, recompute_transitions));
    res.place(&p);
    hipStream_t st = p.st;
    // what the sums go by: the resident lengths; MIX: 0 on an edge that is dead under a live set;
    // PART: those of every set
    const double *d_tlen = PART ? m->multi.d_t : m->d_t;
    int *d_dead = nullptr;
    if (MIX) {
        RT_TRY(mix.begin(&p));
        d_dead = (int *)(p.base + o_dead);
        double *d_tl = (double *)(p.base + o_tl);
        hipLaunchKernelGGL(mix_dead_edge_kernel<256>, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st,
                           (int)mix.K, (int)N, p.d_cw, (const double *)m->multi.d_t, d_dead, d_tl);
        RT_HIP(hipGetLastError());
        d_tlen = d_tl;
    }
    if (PART) RT_TRY(part.begin(&p));
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    // 1. the trial matrices: one launch of the route the resident transitions take
    RT_TRY(grid.launch(&p, trial));
    RT_TRY(post_up(&p, internal.data(), !MIX && !PART));
    if (!p.lane) {
        if (MIX) RT_TRY(mix.PT.pack(&p));
        if (PART) RT_TRY(part.PT.pack(&p));
        RT_TRY(grid.pack(&p));
    }
    // 2. the pass; MIX: set by set (a set of weight zero is never live: not run, never read)
    int first = 1;
    for (int64_t k = 0; k < (MIX ? mix.K : 1); ++k) {
        const double ck = MIX ? class_weights[k] : 1.0;
        if (!(ck > 0.0)) continue;
        const double *P = m->d_P, *G = grid.d_G, *PT = p.d_PT, *GT = grid.d_GT, *tlen = m->d_t;
        int *stat = p.d_status;
        double *tot = nullptr;
        const int *gset = nullptr;
        int gshift = 0;
        long gs_p = 0, gs_g = 0, gs_pt = 0, gs_gt = 0;
        if constexpr (MIX) {
            P = mix.P_of(&p, k); G = grid.G_of_set(&p, k);
            PT = mix.PT.of_set(k); GT = grid.GT_of_set(k);
            tlen = nullptr; stat = mix.status_of(&p, k); tot = mix.tot_of(&p, k);
        }
        if constexpr (PART) {
            P = m->multi.d_P; PT = part.PT.d_PT; tlen = m->multi.d_t;
            gset = part.pt->d_granule_set; gshift = part.gshift();
            gs_p = (long)m->multi.P_stride; gs_g = (long)((size_t)np * N * n * n);
            gs_pt = part.pt_stride(); gs_gt = (long)((size_t)np * grid.tab);
        }
        if (p.lane) {
            const int *d_tab = p.d_ptab;
            RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                hipLaunchKernelGGL((bp_lane_kernel<decltype(nv)::value, MIX, PART>),
                                   dim3((unsigned)((nsites + 255) / 256)), dim3(256), 0, st, (int)N,
                                   (long)nsites, P, G, np, d_tab, d_tab + N, (const void *)s->d_obs,
                                   s->compact_states, (int)s->nobs, s->block_sites,
                                   (const double *)m->d_root, tlen, p.d_L, p.d_M, p.d_D, res.d_val, stat,
                                   ck, first, tot, gset, gshift, gs_p, gs_g);
                return RT_OK;
            }));
        } else {
            const rt_sites *x = p.x;
            if (MIX) RT_TRY(post_up_set(&p, k, nullptr));
            RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
                constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
                hipLaunchKernelGGL((bp_down_kernel<NT, KS, MIX, PART>), dim3((unsigned)x->nblocks),
                                   dim3(64 * NT), 0, st, PT, GT, np, p.nops, (const int4 *)p.d_steps,
                                   (const double *)p.d_L, (const double *)p.d_M, p.d_D,
                                   (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root, tlen,
                                   (int)n, res.d_val, stat, (long)x->nsites, (long)x->nblocks, ck, first,
                                   tot, gset, gs_pt, gs_gt, (long)N);
                return RT_OK;
            }));
        }
        RT_HIP(hipGetLastError());
        first = 0;
    }
    // MIX: log Lambda_i and the status, the accumulator -> values
    if (MIX) {
        RT_TRY(mix.post(&p));
        if (values || sums) RT_TRY(mix.log_ratio(&p, rows, np, d_dead, res.d_val));
    }
    // 3. the weighted site sums and the per-site array
    RT_TRY(res.chunk(&p, 0, rows, np, d_tlen));
    if constexpr (PART) RT_TRY(res.finish(&p, status));
    else RT_TRY(res.finish(&p, status, loglik, mix.d_ll));
    return grid.result(&p);
}

}  // namespace

extern "C" int rt_sites_branch_profiles(rt_model *m, rt_sites *s, int recompute_transitions,
                                        int64_t npoints, const double *lengths, double *values,
                                        double *sums, int32_t *status)
{
    return bp_read<false>("rt_sites_branch_profiles", m, s, recompute_transitions, nullptr, npoints,
                          lengths, values, sums, nullptr, nullptr, status);
}

extern "C" int rt_sites_branch_profiles_mixture(rt_model *m, rt_sites *s, int recompute_transitions,
                                                const double *class_weights, int64_t npoints,
                                                const double *factors, double *values, double *sums,
                                                double *loglik, int32_t *status)
{
    return bp_read<true>("rt_sites_branch_profiles_mixture", m, s, recompute_transitions,
                         class_weights, npoints, factors, values, sums, nullptr, loglik, status);
}

extern "C" int rt_sites_branch_profiles_partitioned(rt_model *m, rt_sites *s, int recompute_transitions,
                                                    int64_t npoints, const double *factors,
                                                    double *values, double *sums, double *set_sums,
                                                    int32_t *status)
{
    return bp_read<false, true>("rt_sites_branch_profiles_partitioned", m, s, recompute_transitions,
                                nullptr, npoints, factors, values, sums, set_sums, nullptr, status);
}
