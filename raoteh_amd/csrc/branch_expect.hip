// Per-site, per-branch expected history statistics of a RESIDENT batch
// (rt_sites_branch_expectations).
//
// The reference's examples/code2x3/extras.get_expected_ntransitions (extras.py:19-132) computes,
// for one site and every edge p -> v with rate matrix Q, length t and C = E * Q,
//     G = expm_frechet(t Q, t C),   value = sum_{a, b : J[a][b] != 0} J[a][b] G[a][b] / P[a][b]
// with J the joint endpoint posterior of the edge.  With J[a][b] = u[a] P[a][b] L_v[b],
// u = D_p / (P L_v) (what posterior.hip's downward pass holds at every step),
//     value = sum_b L_v[b] (G^T u)[b]:
// the edge-set sum of post_down_kernel with G^T in the place of P^T and no set masks.  Here:
//
//   1. per coefficient matrix k: W_e = C_e^T of every edge on the device (direction_kernel), ONE
//      derivative per edge by the routes of rt_expect_step (expect.hip's block exponential for
//      n <= 64, frechet_wide.hip's pair recurrence above; both give L(t Q^T, W) = L(t Q, C)^T),
//      extracted into G_k[node][n][n] laid out like the model's transition matrices;
//   2. n > 4: rt_launch_pack_pt on every G_k (G_k^T as A fragments), the upward pass with L and M
//      of every step stored, then be_down_kernel: post_down_kernel without sets and marginals;
//      per step and k one more n x n by n x 16 matrix-pipe product from the u already staged in
//      LDS, reduced over the states in a fixed order.  D is formed at internal nodes only (a
//      leaf's D has no reader).
//      n <= 4: be_lane_kernel, one lane per site (the upward pass, the root and u are
//      post_lane_kernel's: post_common.h);
//   3. edge_sums_kernel: the site-weighted sums per (node, k) in a fixed order.
//
// Nothing of the batch is written: its own pruning kernel, log-likelihoods, status and totals
// stay as they were; two calls give the same bits.
//
// rt_sites_branch_expectations_partitioned (at the end): the same read of a partitioned batch,
// every site under its own rate set -- the kernels' PART forms and the part_* kernels.
// rt_sites_branch_expectations_mixture (after it): an ordinary batch under a site-class mixture
// over the rate sets -- the kernels' TOT forms once per set, the mix_* kernels (mix_post_kernel:
// post_common.h, shared with the mixture reads of branch_profile.hip and nni.hip); set_tables is
// what the two share.
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int BC_MAX = RT_MAX_BRANCH_COEFS;

// W[e][r][c] = C_e[c][r]: C_e = E * Q_e off the diagonal, E on it (edge e is node e + 1).
// PART (the edges of all rate sets, set after set, per_set each): E of the edge's set, e_stride
// doubles per set further on (0: one E for all sets)
template <bool PART>
__global__ void __launch_bounds__(256)
direction_kernel(int n, const double *__restrict__ Q, const int *__restrict__ qidx,
                 const double *__restrict__ E, double *__restrict__ W, int per_set, long e_stride)
{
    const int e = blockIdx.x;
    const int nn = n * n;
    if constexpr (PART) E += (long)(e / per_set) * e_stride;
    const double *Qe = Q + (size_t)qidx[e] * nn;
    for (int k = threadIdx.x; k < nn; k += 256) {
        const int r = k / n, c = k - r * n;
        const double w = E[c * n + r];
        W[(size_t)e * nn + k] = r == c ? w : (w != 0.0 ? w * Qe[c * n + r] : 0.0);
    }
}

// steps[i] = {node, step of the parent, stream position of an observed leaf or -1, 1 if the node
// has children}; the root is the last step.  GfragT: [k][step] A fragments of G_k^T.
// PART (a partitioned batch: sites are its slots, the output is in slot order): the workgroup's
// tile is one granule; the tables of its rate set are gset[tile] * (gs_pt, gs_gt) doubles further
// on -- wave-uniform, a scalar load and two scalar adds before the first fragment load.
// TOT (the mixture call, one launch per rate set): the root's sum, the site's likelihood under the
// tables given, goes to root_tot[site] as well.
template <int NT, int KS, bool PART = false, bool TOT = false>
__global__ void __launch_bounds__(64 * NT)
be_down_kernel(const double *__restrict__ PfragT, const double *__restrict__ GfragT, int nk, int nops,
               const int4 *__restrict__ steps, const double *__restrict__ Larr,
               const double *__restrict__ Marr, double *__restrict__ Darr,
               const double *__restrict__ obs, int K, const double *__restrict__ root_w, int n,
               int nnodes, double *__restrict__ out, int *__restrict__ status, long nsites, long nblocks,
               const int *__restrict__ gset, long gs_pt, long gs_gt, double *__restrict__ root_tot)
{
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double red[NT][16];
    __shared__ double sums[BC_MAX][NT][16];
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
    bool bad = false;
    // root: D = w L / sum_states(w L); its slot of the output is 0
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
        const bool zero = !(tot > 0.0);
#pragma unroll
        for (int r = 0; r < 4; ++r) Darr[o + r * 64] = zero ? 0.0 : wl[r] / tot;
        if (m == 0 && lane < 16 && site_ok) {
            if (zero) atomicOr(&status[site], RT_SITE_ZERO_PROB);
            if constexpr (TOT) root_tot[site] = tot;
            for (int k = 0; k < nk; ++k) out[((size_t)site * nnodes + steps[i].x) * nk + k] = 0.0;
        }
    }
    const size_t frag = ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
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
        // per coefficient matrix: sum_b L[b] (G_k^T u)[b], one fragment table live at a time
        for (int k = 0; k < nk; ++k) {
            down_frag<KP>(GfragT + ((size_t)k * nops + i) * ASTRIDE + frag, a);
            const double4_t y = down_product<KS>(a, xb, lane);
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) v += y[r] * L[r];
            down_part(sums[k], m, lane, v);      // (then, below, the waves in order)
        }
        __syncthreads();
        if (m == 0 && lane < 16 && site_ok)
            for (int k = 0; k < nk; ++k)
                out[((size_t)site * nnodes + st.x) * nk + k] = down_total<NT>(sums[k], lane);
    }
    if (bad && site_ok) atomicOr(&status[site], 2);
}

// n <= 4: one lane per site; arrays [node][state][site], nodes in preorder; G [k][node][N][N]
// PART (a partitioned batch: sites are its slots): a wave's 64 slots lie in one granule of
// `granule` slots (256 or 64); P of its rate set is gset[granule] * gs_p doubles further on, its
// derivative tables are G [k][set][edge][N][N] (edge = node - 1, gs_g sets) -- wave-uniform, so P
// and G stay scalar loads.
// TOT (the mixture call, one launch per rate set with P and G of that set: G points at the set's
// edges in the PART layout, gs_g sets per coefficient matrix): the root's sum to root_tot[site].
template <int N, bool PART = false, bool TOT = false>
__global__ void __launch_bounds__(256)
be_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const double *__restrict__ G,
               int nk, const int *__restrict__ parent, const int *__restrict__ node_k,
               const void *__restrict__ obs, int compact, int K, int block_sites,
               const double *__restrict__ root_w, double *__restrict__ Larr,
               double *__restrict__ Marr, double *__restrict__ Darr, double *__restrict__ out,
               int *__restrict__ status, const int *__restrict__ gset, int granule, long gs_p, int gs_g,
               double *__restrict__ root_tot)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    long gs = 0;
    if constexpr (PART) {
        gs = __builtin_amdgcn_readfirstlane(gset[(site & ~63L) / granule]);
        P += gs * gs_p;
    }
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, K, block_sites, Larr, Marr);
    // down: the root, then every node after its parent
    {
        double d[N];
        double tot = 0.0;
        if (lane_root<N>(nsites, site, root_w, Larr, Darr, d, TOT ? &tot : nullptr))
            status[site] |= RT_SITE_ZERO_PROB;
        if constexpr (TOT) root_tot[site] = tot;
        for (int k = 0; k < nk; ++k) out[(size_t)site * nnodes * nk + k] = 0.0;
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
        for (int k = 0; k < nk; ++k) {
            const double *Gv = PART || TOT ? G + (((size_t)k * gs_g + gs) * (nnodes - 1) + (v - 1)) * N * N
                                    : G + ((size_t)k * nnodes + v) * N * N;
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) {
                double y = 0.0;
#pragma unroll
                for (int a = 0; a < N; ++a) y += Gv[a * N + b] * u[a];
                t += y * L[b];
            }
            out[((size_t)site * nnodes + v) * nk + k] = t;
        }
    }
    if (bad) status[site] |= 2;
}

// one workgroup per node: thread j adds sites j, j + 256, ... in order, then the 256 partial
// sums by halves (fixed rounding)
__global__ void __launch_bounds__(256)
edge_sums_kernel(int nnodes, int nk, long nsites, const double *__restrict__ values,
                 const double *__restrict__ weights, double *__restrict__ sums)
{
    __shared__ double part[BC_MAX][256];
    const int v = blockIdx.x, tid = threadIdx.x;
    double acc[BC_MAX];
#pragma unroll
    for (int k = 0; k < BC_MAX; ++k) acc[k] = 0.0;
    for (long i = tid; i < nsites; i += 256) {
        const double w = weights ? weights[i] : 1.0;
        const double *x = values + ((size_t)i * nnodes + v) * nk;
#pragma unroll
        for (int k = 0; k < BC_MAX; ++k)
            if (k < nk) acc[k] += w * x[k];
    }
#pragma unroll
    for (int k = 0; k < BC_MAX; ++k) part[k][tid] = acc[k];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            for (int k = 0; k < nk; ++k) part[k][tid] += part[k][tid + h];
        __syncthreads();
    }
    if (tid < nk) sums[(size_t)v * nk + tid] = part[tid][0];
}

// ---- a partitioned batch (rt_sites_branch_expectations_partitioned) ----

// the edges of the first K rate sets, set after set without the roots' entries: edge e is node
// e % (N - 1) + 1 of set e / (N - 1); ones / ident: what the block exponential's launch reads
__global__ void __launch_bounds__(256)
part_edges_kernel(int K, int N, const int *__restrict__ qidx, const double *__restrict__ t,
                  int *__restrict__ eq, double *__restrict__ et, double *__restrict__ ones,
                  int *__restrict__ ident)
{
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= K * (N - 1)) return;
    const int k = e / (N - 1), v = e - k * (N - 1) + 1;
    eq[e] = qidx[(size_t)k * N + v];
    et[e] = t[(size_t)k * N + v];
    ones[e] = 1.0;
    ident[e] = e;
}

// slot order -> caller order: values [site][row] (row = nnodes * nk doubles), status
__global__ void __launch_bounds__(256)
part_gather_kernel(const double *__restrict__ val_slot, const int *__restrict__ status_slot,
                   const long *__restrict__ slot_of_site, long nsites, long row,
                   double *__restrict__ val, int *__restrict__ status)
{
    const long total = nsites * row;
    for (long j = (long)blockIdx.x * 256 + threadIdx.x; j < total; j += (long)gridDim.x * 256) {
        const long i = j / row, c = j - i * row;
        const long slot = slot_of_site[i];
        if (val) val[j] = val_slot[slot * row + c];
        if (c == 0) status[i] = status_slot[slot];
    }
}

// stage 1 of the per-set sums: workgroup (b, k, v) adds a contiguous piece of set k's run for
// node v, thread t every 256th slot of it, pads skipped, the weights through `order`; then the
// 256 partial sums by halves.  The shape comes from the plan alone: the same bits every call.
__global__ void __launch_bounds__(256)
part_sums_stage1_kernel(int nnodes, int nk, const double *__restrict__ val_slot,
                        const unsigned char *__restrict__ is_pad, const long *__restrict__ order,
                        const long *__restrict__ run_begin, const double *__restrict__ weights,
                        int nblocks, double *__restrict__ part)
{
    __shared__ double sh[BC_MAX][256];
    const int b = blockIdx.x, k = blockIdx.y, v = blockIdx.z, tid = threadIdx.x;
    const long r0 = run_begin[k], r1 = run_begin[k + 1];
    const long per = (r1 - r0 + nblocks - 1) / nblocks;
    const long lo = r0 + (long)b * per, hi = lo + per < r1 ? lo + per : r1;
    double acc[BC_MAX];
#pragma unroll
    for (int c = 0; c < BC_MAX; ++c) acc[c] = 0.0;
    for (long slot = lo + tid; slot < hi; slot += 256) {
        if (is_pad[slot]) continue;
        const double w = weights ? weights[order[slot]] : 1.0;
        const double *x = val_slot + ((size_t)slot * nnodes + v) * nk;
#pragma unroll
        for (int c = 0; c < BC_MAX; ++c)
            if (c < nk) acc[c] += w * x[c];
    }
#pragma unroll
    for (int c = 0; c < BC_MAX; ++c) sh[c][tid] = acc[c];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            for (int c = 0; c < nk; ++c) sh[c][tid] += sh[c][tid + h];
        __syncthreads();
    }
    if (tid < nk) part[(((size_t)k * nblocks + b) * nnodes + v) * nk + tid] = sh[tid][0];
}

// stage 2: workgroup (k, v) adds set k's stage-1 sums of node v -> set_sums[k][v][.]
__global__ void __launch_bounds__(256)
part_sums_stage2_kernel(int nnodes, int nk, const double *__restrict__ part, int nblocks,
                        double *__restrict__ set_sums)
{
    __shared__ double sh[BC_MAX][256];
    const int k = blockIdx.x, v = blockIdx.y, tid = threadIdx.x;
    for (int c = 0; c < nk; ++c)
        sh[c][tid] = tid < nblocks ? part[(((size_t)k * nblocks + tid) * nnodes + v) * nk + c] : 0.0;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            for (int c = 0; c < nk; ++c) sh[c][tid] += sh[c][tid + h];
        __syncthreads();
    }
    if (tid < nk) set_sums[((size_t)k * nnodes + v) * nk + tid] = sh[tid][0];
}

// edge_sums[v][c]: the per-set rows added in set order (one thread per entry)
__global__ void __launch_bounds__(256)
part_sums_total_kernel(int K, long row, const double *__restrict__ set_sums, double *__restrict__ sums)
{
    const long j = (long)blockIdx.x * 256 + threadIdx.x;
    if (j >= row) return;
    double t = 0.0;
    for (int k = 0; k < K; ++k) t += set_sums[(size_t)k * row + j];
    sums[j] = t;
}

// ---- the tables of the model's first K rate sets, for the calls that read a batch under them
// (rt_sites_branch_expectations_partitioned, rt_sites_branch_expectations_mixture) ----

// Their pieces of the call's scratch and what fills them: the edge list of the K sets, the
// derivative route's buffers over all K (nnodes - 1) edges, the derivative tables G
// [coef][set][edge][n][n] and, for n > 4, per set the A fragments of P^T [set][step] and of every
// G^T [set][coef][step].  The step tables feed asynchronous copies: alive until the stream is
// synchronised.
struct set_tables {
    int64_t K = 0;
    int nk = 0;
    bool per_set = false, wide = false;
    size_t ne = 0, tab = 0;                      // K (nnodes - 1) edges; bytes of one step table
    size_t o_E = 0, o_G = 0, o_W = 0, o_B = 0, o_X = 0, o_scale = 0, o_ones = 0, o_ident = 0, o_eq = 0,
           o_et = 0, o_GT = 0, o_tabG = 0;
    double *E = nullptr, *G = nullptr, *PTs = nullptr, *GT = nullptr;
    post_set_pt PT;                              // the sets' P^T fragments (post_common.h)
    std::vector<int32_t> tabG;

    void take(post_pass *p, int64_t sets, int n_coefs, bool coefs_per_set)
    {
        K = sets; nk = n_coefs; per_set = coefs_per_set;
        const int64_t n = p->n, N = p->N;
        const size_t nn = (size_t)n * n;
        wide = 2 * n > RT_MAX_EXPM_STATES;
        ne = (size_t)K * (size_t)(N - 1);
        tab = (size_t)p->nops * p->NT * p->KP * 128 * 8;
        const size_t wide_edge = wide ? rt_frechet_wide_scratch_doubles(n, 1) : 0;
        post_plan &plan = p->plan;
        o_E = plan.take((size_t)(per_set ? K : 1) * nk * nn * 8);
        o_G = plan.take((size_t)nk * ne * nn * 8);
        o_W = plan.take(ne * nn * 8);
        o_B = wide ? plan.take(ne * wide_edge * 8) : plan.take(ne * 4 * nn * 8);
        o_X = wide ? plan.take(8) : plan.take(ne * 4 * nn * 8);
        o_scale = plan.take(ne * 8); o_ones = plan.take(ne * 8); o_ident = plan.take(ne * 4);
        o_eq = plan.take(ne * 4); o_et = plan.take(ne * 8);
        PT.take(p, K);
        o_GT = p->lane ? plan.take(8) : plan.take((size_t)K * nk * tab);
        o_tabG = plan.take((size_t)K * nk * p->nops * 4);
    }

    // after post_begin: the coefficients to the device; the edges of the K sets as one list; per
    // coefficient matrix one direction launch (E of the edge's set where the coefficients are per
    // set), ONE launch of the derivative route over the whole list -- the exponential's variant
    // chosen as for one set's edges -- and one extract straight into G (no root slots: an extract
    // writes its edges contiguously)
    int derivatives(post_pass *p, const double *coefs)
    {
        rt_ctx *ctx = p->ctx;
        hipStream_t st = p->st;
        const rt_rate_sets &r = p->m->multi;
        const int64_t n = p->n, N = p->N;
        const size_t nn = (size_t)n * n;
        unsigned char *base = p->base;
        E = (double *)(base + o_E); G = (double *)(base + o_G);
        PT.place(p);
        PTs = PT.d_PT; GT = (double *)(base + o_GT);
        double *d_W = (double *)(base + o_W), *d_B = (double *)(base + o_B), *d_X = (double *)(base + o_X);
        double *d_scale = (double *)(base + o_scale), *d_ones = (double *)(base + o_ones);
        double *d_et = (double *)(base + o_et);
        int *d_ident = (int *)(base + o_ident), *d_eq = (int *)(base + o_eq);
        RT_HIP(hipMemcpyAsync(E, coefs, (size_t)(per_set ? K : 1) * nk * nn * 8, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(part_edges_kernel, dim3((unsigned)((ne + 255) / 256)), dim3(256), 0, st, (int)K,
                           (int)N, (const int *)r.d_qidx, (const double *)r.d_t, d_eq, d_et, d_ones, d_ident);
        RT_HIP(hipGetLastError());
        for (int c = 0; c < nk; ++c) {
            double *Gc = G + (size_t)c * ne * nn;
            hipLaunchKernelGGL(direction_kernel<true>, dim3((unsigned)ne), dim3(256), 0, st, (int)n,
                               (const double *)r.d_Q, (const int *)d_eq,
                               (const double *)(E + (size_t)c * nn), d_W, (int)(N - 1),
                               (long)(per_set ? (size_t)nk * nn : 0));
            RT_HIP(hipGetLastError());
            if (wide) {
                RT_TRY(rt_frechet_wide_pairs_device(ctx, n, (int64_t)ne, r.d_Q, d_eq, d_et, d_W, d_B, d_scale,
                                                    nullptr));
                RT_TRY(rt_frechet_wide_extract_device(ctx, n, (int64_t)ne, d_et, d_B, d_scale, Gc));
            } else {
                RT_TRY(rt_frechet_blocks_device(ctx, n, (int64_t)ne, r.d_Q, d_eq, d_et, d_W, d_B, d_X, d_scale,
                                                d_ones, d_ident, N - 1));
                RT_TRY(rt_frechet_extract_device(ctx, n, (int64_t)ne, d_et, d_X, d_scale, Gc));
            }
        }
        return RT_OK;
    }

    // n > 4, after post_up (the step -> node table): P^T and G^T of every set as A fragments by two
    // rt_launch_pack_pt launches over step tables that span the sets -- step -> matrix of the table
    // it is packed from, P [set][node] (post_set_pt), G [coef][set][edge] (the root's step is never
    // read: any matrix of the set)
    int pack(post_pass *p)
    {
        const int64_t N = p->N, ne1 = N - 1;
        int *d_tabG = (int *)(p->base + o_tabG);
        tabG.resize((size_t)K * nk * p->nops);
        for (int64_t k = 0; k < K; ++k)
            for (int i = 0; i < p->nops; ++i) {
                const int64_t v = p->step_node[(size_t)i];
                for (int c = 0; c < nk; ++c)
                    tabG[(size_t)((k * nk + c) * p->nops + i)] =
                        (int32_t)((c * K + k) * ne1 + (v ? v - 1 : 0));
            }
        RT_HIP(hipMemcpyAsync(d_tabG, tabG.data(), tabG.size() * 4, hipMemcpyHostToDevice, p->st));
        RT_TRY(PT.pack(p));
        RT_TRY(rt_launch_pack_pt(p->ctx, (int)p->n, p->NT, p->KP, (int)(K * nk * p->nops), d_tabG, G, GT));
        return RT_OK;
    }
};

// ---- a site-class mixture over the rate sets (rt_sites_branch_expectations_mixture) ----

constexpr int MIX_POST_LDS = 2048;               // posteriors a combine workgroup stages (16 KB)

// values[i][j] = sum_k post[i][k] x[k][i][j] in set order, j over the site's (node, coefficient)
// row of `row` doubles; a set with post == 0 is skipped (nothing of a set that is not live is
// multiplied in); product and sum rounded separately, so post == 1 returns x bit for bit.
// A workgroup takes S consecutive sites (S row <= 256 where a row is short, S K <= MIX_POST_LDS):
// their posteriors go to LDS once, then thread t walks the S rows as one contiguous run -- for
// every set the loads of a wave are 64 consecutive doubles of x[k], the LDS reads broadcasts.
__global__ void __launch_bounds__(256)
mix_combine_kernel(int K, long nsites, long row, int S, const double *__restrict__ post,
                   const double *__restrict__ x, double *__restrict__ values)
{
    __shared__ double ps[MIX_POST_LDS];
    const long site0 = (long)blockIdx.x * S;
    const long left = nsites - site0;
    const int ns = left < S ? (int)left : S;
    for (int j = threadIdx.x; j < ns * K; j += 256) ps[j] = post[(size_t)site0 * K + j];
    __syncthreads();
    const size_t base = (size_t)site0 * row, set_stride = (size_t)nsites * row;
    const long len = (long)ns * row;
    for (long j = threadIdx.x; j < len; j += 256) {
        const double *pi = ps + (j / row) * K;
        double acc = 0.0;
        for (int k = 0; k < K; ++k) {
            const double pk = pi[k];
            if (pk != 0.0) acc = __dadd_rn(acc, __dmul_rn(pk, x[(size_t)k * set_stride + base + j]));
        }
        values[base + j] = acc;
    }
}

// stage 1 of the per-set sums of w_i post[i][k] x[k][i][v][.], in the shape of
// part_sums_stage1_kernel with the whole batch as the run and no pads: workgroup (b, k, v) adds a
// contiguous piece of the sites, thread t every 256th of it, then the 256 partial sums by halves
// (part_sums_stage2_kernel and part_sums_total_kernel finish).  A site where set k is not live
// adds nothing.  One piece (up to 4096 sites) and K = 1: edge_sums_kernel's order and bits.
__global__ void __launch_bounds__(256)
mix_sums_stage1_kernel(int nnodes, int nk, long nsites, int K, const double *__restrict__ x,
                       const double *__restrict__ post, const double *__restrict__ weights,
                       int nblocks, double *__restrict__ part)
{
    __shared__ double sh[BC_MAX][256];
    const int b = blockIdx.x, k = blockIdx.y, v = blockIdx.z, tid = threadIdx.x;
    const long per = (nsites + nblocks - 1) / nblocks;
    const long lo = (long)b * per, hi = lo + per < nsites ? lo + per : nsites;
    const double *xk = x + (size_t)k * nsites * nnodes * nk;
    double acc[BC_MAX];
#pragma unroll
    for (int c = 0; c < BC_MAX; ++c) acc[c] = 0.0;
    for (long i = lo + tid; i < hi; i += 256) {
        const double pk = post[(size_t)i * K + k];
        if (pk == 0.0) continue;
        const double w = (weights ? weights[i] : 1.0) * pk;
        const double *xi = xk + ((size_t)i * nnodes + v) * nk;
#pragma unroll
        for (int c = 0; c < BC_MAX; ++c)
            if (c < nk) acc[c] += w * xi[c];
    }
#pragma unroll
    for (int c = 0; c < BC_MAX; ++c) sh[c][tid] = acc[c];
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h)
            for (int c = 0; c < nk; ++c) sh[c][tid] += sh[c][tid + h];
        __syncthreads();
    }
    if (tid < nk) part[(((size_t)k * nblocks + b) * nnodes + v) * nk + tid] = sh[tid][0];
}

// class_sums[k] = sum_i w_i post[i][k]: one workgroup per set, thread t adds sites t, t + 256, ...
// in order, then the 256 partial sums by halves
__global__ void __launch_bounds__(256)
mix_class_sums_kernel(int K, long nsites, const double *__restrict__ post,
                      const double *__restrict__ weights, double *__restrict__ class_sums)
{
    __shared__ double sh[256];
    const int k = blockIdx.x, tid = threadIdx.x;
    double acc = 0.0;
    for (long i = tid; i < nsites; i += 256) acc += (weights ? weights[i] : 1.0) * post[(size_t)i * K + k];
    sh[tid] = acc;
    __syncthreads();
    for (int h = 128; h > 0; h >>= 1) {
        if (tid < h) sh[tid] += sh[tid + h];
        __syncthreads();
    }
    if (tid == 0) class_sums[k] = sh[0];
}

}  // namespace

extern "C" int rt_sites_branch_expectations(rt_model *m, rt_sites *s, int recompute_transitions,
                                            int64_t n_coefs, const double *coefs, double *values,
                                            double *edge_sums, int32_t *status)
{
    post_pass p;                                 // (alive until the synchronisation below)
    RT_TRY(post_open(&p, "rt_sites_branch_expectations", m, s));
    RT_REQUIRE(n_coefs >= 1 && coefs, "at least one coefficient matrix is needed");
    RT_REQUIRE(m->d_Q && !m->spectral,
               "rt_sites_branch_expectations: rt_model_set_rates has not been called (the "
               "derivative needs the rate matrices: a model with spectral rates or with "
               "transitions set directly has none)");
    RT_REQUIRE(m->rates_current || recompute_transitions,
               "%s: the transitions were set directly after the rates "
               "(rt_model_set_transitions): the resident rate matrices no longer describe them; "
               "set the rates again or pass recompute_transitions", "rt_sites_branch_expectations");
    if (n_coefs > RT_MAX_BRANCH_COEFS) {
        rt_set_error("rt_sites_branch_expectations: at most %d coefficient matrices (%lld here)",
                     RT_MAX_BRANCH_COEFS, (long long)n_coefs);
        return RT_ERR_UNSUPPORTED;
    }
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    RT_TRY(post_layout(&p, true));
    const size_t nn = (size_t)n * n, ne = (size_t)(N - 1);
    const int nk = (int)n_coefs;
    for (size_t j = 0; j < (size_t)nk * nn; ++j)
        RT_REQUIRE(std::isfinite(coefs[j]), "coefficient %lld of matrix %lld is not finite",
                   (long long)(j % nn), (long long)(j / nn));
    rt_ctx *ctx = p.ctx;
    const bool wide = 2 * n > RT_MAX_EXPM_STATES;
    // scratch: L, M, D of every node and site (post_layout), the values, the derivative route's
    // buffers, the derivative tables and their fragments
    const size_t tab = (size_t)p.nops * p.NT * p.KP * 128 * 8;
    post_plan &plan = p.plan;
    const size_t o_val = plan.take((size_t)nsites * N * nk * 8);
    const size_t o_sum = plan.take((size_t)N * nk * 8);
    const size_t o_E = plan.take((size_t)nk * nn * 8);
    const size_t o_G = plan.take((size_t)nk * N * nn * 8);
    const size_t o_W = plan.take(ne * nn * 8);
    const size_t o_B = wide ? plan.take(rt_frechet_wide_scratch_doubles(n, N - 1) * 8)
                            : plan.take(ne * 4 * nn * 8);
    const size_t o_X = wide ? plan.take(8) : plan.take(ne * 4 * nn * 8);
    const size_t o_scale = plan.take(ne * 8), o_ones = plan.take(ne * 8), o_ident = plan.take(ne * 4);
    const size_t o_GT = p.lane ? plan.take(8) : plan.take((size_t)nk * tab);
    RT_TRY(post_begin(&p, recompute_transitions));
    hipStream_t st = p.st;
    unsigned char *base = p.base;
    double *d_val = (double *)(base + o_val), *d_sum = (double *)(base + o_sum);
    double *d_E = (double *)(base + o_E), *d_G = (double *)(base + o_G), *d_W = (double *)(base + o_W);
    double *d_B = (double *)(base + o_B), *d_X = (double *)(base + o_X);
    double *d_scale = (double *)(base + o_scale), *d_ones = (double *)(base + o_ones);
    int *d_ident = (int *)(base + o_ident), *d_status = p.d_status;
    // (host buffers of the asynchronous copies: alive until the synchronisation below)
    std::vector<double> ones(ne, 1.0);
    std::vector<int32_t> ident(ne);
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    for (size_t e = 0; e < ne; ++e) ident[e] = (int32_t)e;
    RT_HIP(hipMemcpyAsync(d_E, coefs, (size_t)nk * nn * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_ones, ones.data(), ne * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_ident, ident.data(), ne * 4, hipMemcpyHostToDevice, st));
    // 1. the derivative tables: one launch of the derivative route per coefficient matrix (the
    //    root's slot of every table is zero)
    for (int k = 0; k < nk; ++k) {
        double *Gk = d_G + (size_t)k * N * nn;
        RT_HIP(hipMemsetAsync(Gk, 0, nn * 8, st));
        hipLaunchKernelGGL(direction_kernel<false>, dim3((unsigned)ne), dim3(256), 0, st, (int)n,
                           (const double *)m->d_Q, (const int *)(m->d_qidx + 1),
                           (const double *)(d_E + (size_t)k * nn), d_W, (int)ne, 0L);
        RT_HIP(hipGetLastError());
        if (wide) {
            RT_TRY(rt_frechet_wide_pairs_device(ctx, n, N - 1, m->d_Q, m->d_qidx + 1, m->d_t + 1, d_W,
                                                d_B, d_scale, nullptr));
            RT_TRY(rt_frechet_wide_extract_device(ctx, n, N - 1, m->d_t + 1, d_B, d_scale, Gk + nn));
        } else {
            RT_TRY(rt_frechet_blocks_device(ctx, n, N - 1, m->d_Q, m->d_qidx + 1, m->d_t + 1, d_W, d_B,
                                            d_X, d_scale, d_ones, d_ident));
            RT_TRY(rt_frechet_extract_device(ctx, n, N - 1, m->d_t + 1, d_X, d_scale, Gk + nn));
        }
    }
    RT_TRY(post_up(&p, internal.data(), true));
    if (p.lane) {
        const int *d_tab = p.d_ptab;
        RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
            hipLaunchKernelGGL((be_lane_kernel<decltype(nv)::value>), dim3((unsigned)((nsites + 255) / 256)),
                               dim3(256), 0, st, (int)N, (long)nsites, (const double *)m->d_P,
                               (const double *)d_G, nk, d_tab, d_tab + N, (const void *)s->d_obs,
                               s->compact_states, (int)s->nobs, s->block_sites,
                               (const double *)m->d_root, p.d_L, p.d_M, p.d_D, d_val, d_status,
                               (const int *)nullptr, 0, 0L, 0, (double *)nullptr);
            return RT_OK;
        }));
    } else {
        const rt_sites *x = p.x;
        double *d_GT = (double *)(base + o_GT);
        for (int k = 0; k < nk; ++k)
            RT_TRY(rt_launch_pack_pt(ctx, (int)n, p.NT, p.KP, p.nops, p.d_ptab, d_G + (size_t)k * N * nn,
                                     d_GT + (size_t)k * (tab / 8)));
        RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
            constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
            hipLaunchKernelGGL((be_down_kernel<NT, KS>), dim3((unsigned)x->nblocks), dim3(64 * NT), 0, st,
                               (const double *)p.d_PT, (const double *)d_GT, nk, p.nops,
                               (const int4 *)p.d_steps, (const double *)p.d_L, (const double *)p.d_M,
                               p.d_D, (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root,
                               (int)n, (int)N, d_val, d_status, (long)x->nsites, (long)x->nblocks,
                               (const int *)nullptr, 0L, 0L, (double *)nullptr);
            return RT_OK;
        }));
    }
    RT_HIP(hipGetLastError());
    // 3. the weighted site sums, whether or not the per-site array is returned
    if (edge_sums) {
        hipLaunchKernelGGL(edge_sums_kernel, dim3((unsigned)N), dim3(256), 0, st, (int)N, nk, (long)nsites,
                           (const double *)d_val, (const double *)s->d_weights, d_sum);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpyAsync(edge_sums, d_sum, (size_t)N * nk * 8, hipMemcpyDeviceToHost, st));
    }
    // only what was asked for crosses PCIe
    if (values)
        RT_HIP(hipMemcpyAsync(values, d_val, (size_t)nsites * N * nk * 8, hipMemcpyDeviceToHost, st));
    if (status) RT_HIP(hipMemcpyAsync(status, d_status, (size_t)nsites * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return RT_OK;
}

// The same read of a PARTITIONED batch: on the edge above node v, site i uses Q, t, P and the
// derivative of its own rate set (rt_model_set_rate_sets).  In the order of the data:
//   1. the edges of the batch's K sets as one list of K (nnodes - 1); per coefficient matrix one
//      direction launch (E of the edge's set where the coefficients are per set), ONE launch of
//      the derivative route over the whole list -- the exponential's variant chosen as for one
//      set's edges, so every derivative has the bits the ordinary call gives under that set -- and
//      one extract straight into G [coef][set][edge][n][n] (no root slots: an extract writes its
//      edges contiguously);
//   2. n > 4: P^T and G^T of every set as A fragments, [set][step] and [set][coef][step], by two
//      rt_launch_pack_pt launches over step tables that span the sets; the upward pass on the
//      twin through the batch's granule_set (post_up); be_down_kernel<.., true> per 16-slot tile.
//      n <= 4: be_lane_kernel<N, true>;
//   3. per (set, node, coefficient) the fixed-order two-stage sum over the set's run with the
//      pads skipped, the per-set rows added in set order, and the gather into caller order.
extern "C" int rt_sites_branch_expectations_partitioned(rt_model *m, rt_sites *s, int recompute_transitions,
                                                        int64_t n_coefs, int coefs_per_set,
                                                        const double *coefs, double *values,
                                                        double *edge_sums, double *set_edge_sums,
                                                        int32_t *status)
{
    static const char who[] = "rt_sites_branch_expectations_partitioned";
    post_pass p;                                 // (alive until the synchronisation below)
    RT_TRY(post_open(&p, who, m, s, true));
    RT_REQUIRE(n_coefs >= 1 && coefs, "at least one coefficient matrix is needed");
    if (n_coefs > RT_MAX_BRANCH_COEFS) {
        rt_set_error("%s: at most %d coefficient matrices (%lld here)", who, RT_MAX_BRANCH_COEFS,
                     (long long)n_coefs);
        return RT_ERR_UNSUPPORTED;
    }
    const rt_partition *pt = s->part;
    const rt_rate_sets &r = m->multi;
    const int64_t n = p.n, N = p.N, nslots = p.nsites, nreal = pt->nsites, K = pt->nsets;
    RT_TRY(post_layout(&p, true));
    RT_REQUIRE(r.P_stride == N * n * n, "unexpected stride of the sets' transition matrices");
    const size_t nn = (size_t)n * n;
    const int nk = (int)n_coefs;
    const size_t ncoef = (size_t)(coefs_per_set ? K : 1) * nk;
    for (size_t j = 0; j < ncoef * nn; ++j)
        RT_REQUIRE(std::isfinite(coefs[j]), "coefficient %lld of matrix %lld is not finite",
                   (long long)(j % nn), (long long)(j / nn));
    const int nb = pt->nblocks;
    const size_t row = (size_t)N * nk;
    // scratch: L, M, D of every node and slot (post_layout), the values in slot and in caller
    // order, the sums, the edge list, the derivative route's buffers over all K (nnodes - 1)
    // edges, the derivative tables, and per set the fragments of P^T and of every G^T
    post_plan &plan = p.plan;
    const size_t o_val = plan.take((size_t)nslots * row * 8);
    const size_t o_valc = plan.take(values ? (size_t)nreal * row * 8 : 8);
    const size_t o_statc = plan.take((size_t)nreal * 4);
    const size_t o_setsum = plan.take((size_t)K * row * 8), o_sum = plan.take(row * 8);
    const size_t o_part = plan.take((size_t)K * nb * row * 8);
    set_tables T;
    T.take(&p, K, nk, coefs_per_set != 0);
    RT_TRY(post_begin(&p, recompute_transitions));
    hipStream_t st = p.st;
    unsigned char *base = p.base;
    double *d_val = (double *)(base + o_val), *d_valc = (double *)(base + o_valc);
    double *d_setsum = (double *)(base + o_setsum), *d_sum = (double *)(base + o_sum);
    double *d_part = (double *)(base + o_part);
    int *d_status = p.d_status, *d_statc = (int *)(base + o_statc);
    // (host buffer of an asynchronous copy: alive until the synchronisation below)
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    // 1. the derivative tables
    RT_TRY(T.derivatives(&p, coefs));
    // 2. the passes
    RT_TRY(post_up(&p, internal.data(), false));
    const int *d_gset = pt->d_granule_set;
    if (p.lane) {
        const int *d_tab = p.d_ptab;
        RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
            hipLaunchKernelGGL((be_lane_kernel<decltype(nv)::value, true>),
                               dim3((unsigned)((nslots + 255) / 256)), dim3(256), 0, st, (int)N,
                               (long)nslots, (const double *)r.d_P, (const double *)T.G, nk, d_tab,
                               d_tab + N, (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                               s->block_sites, (const double *)m->d_root, p.d_L, p.d_M, p.d_D, d_val,
                               d_status, d_gset, (int)pt->G, (long)r.P_stride, (int)K, (double *)nullptr);
            return RT_OK;
        }));
    } else {
        const rt_sites *x = p.x;
        const size_t tab = T.tab;
        RT_TRY(T.pack(&p));
        RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
            constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
            hipLaunchKernelGGL((be_down_kernel<NT, KS, true>), dim3((unsigned)x->nblocks), dim3(64 * NT), 0,
                               st, (const double *)T.PTs, (const double *)T.GT, nk, p.nops,
                               (const int4 *)p.d_steps, (const double *)p.d_L, (const double *)p.d_M,
                               p.d_D, (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root,
                               (int)n, (int)N, d_val, d_status, (long)x->nsites, (long)x->nblocks, d_gset,
                               (long)(tab / 8), (long)((size_t)nk * (tab / 8)), (double *)nullptr);
            return RT_OK;
        }));
    }
    RT_HIP(hipGetLastError());
    // 3. the sums per set (pads masked, not merely weighted out: a pad repeats a real site), their
    //    total in set order, and what leaves the device in caller order
    if (edge_sums || set_edge_sums) {
        hipLaunchKernelGGL(part_sums_stage1_kernel, dim3((unsigned)nb, (unsigned)K, (unsigned)N), dim3(256),
                           0, st, (int)N, nk, (const double *)d_val, (const unsigned char *)pt->d_is_pad,
                           (const long *)pt->d_order, (const long *)pt->d_run_begin,
                           (const double *)s->d_weights, nb, d_part);
        hipLaunchKernelGGL(part_sums_stage2_kernel, dim3((unsigned)K, (unsigned)N), dim3(256), 0, st, (int)N,
                           nk, (const double *)d_part, nb, d_setsum);
        hipLaunchKernelGGL(part_sums_total_kernel, dim3((unsigned)((row + 255) / 256)), dim3(256), 0, st,
                           (int)K, (long)row, (const double *)d_setsum, d_sum);
        RT_HIP(hipGetLastError());
        if (set_edge_sums)
            RT_HIP(hipMemcpyAsync(set_edge_sums, d_setsum, (size_t)K * row * 8, hipMemcpyDeviceToHost, st));
        if (edge_sums) RT_HIP(hipMemcpyAsync(edge_sums, d_sum, row * 8, hipMemcpyDeviceToHost, st));
    }
    if (values || status) {
        const long grow = values ? (long)row : 1;
        const long blocks = std::min<long>(((long)nreal * grow + 255) / 256, 1 << 16);
        hipLaunchKernelGGL(part_gather_kernel, dim3((unsigned)blocks), dim3(256), 0, st,
                           (const double *)d_val, (const int *)d_status,
                           (const long *)pt->d_slot_of_site, (long)nreal, grow,
                           values ? d_valc : (double *)nullptr, d_statc);
        RT_HIP(hipGetLastError());
        if (values) RT_HIP(hipMemcpyAsync(values, d_valc, (size_t)nreal * row * 8, hipMemcpyDeviceToHost, st));
        if (status) RT_HIP(hipMemcpyAsync(status, d_statc, (size_t)nreal * 4, hipMemcpyDeviceToHost, st));
    }
    RT_HIP(hipStreamSynchronize(st));
    return RT_OK;
}

// The same read of an ORDINARY batch under a site-class mixture over the model's K rate sets:
// every site under every set, weighted by how much that set explains the site.
//   1. the derivative tables of all K (nnodes - 1) edges and, for n > 4, the per-set fragments of
//      P^T and G^T: set_tables, as the partitioned call -- every derivative has the bits
//      rt_sites_branch_expectations gives under that set;
//   2. per set k with c_k > 0, K launches on the one stream over one L, M, D scratch: the upward
//      pass of the twin through a view of set k's tables (post_up_set), then the ordinary downward
//      kernel's TOT instance against set k's fragments (n <= 4: the lane kernel's) -- the unweighted
//      x_k into [K][nsites][nnodes][n_coefs], the root total L_ik and a status word per set;
//   3. mix_post_kernel (posteriors, log-likelihood, the status of the live sets), mix_combine_kernel
//      (the per-site values, only where they are asked for), the two-stage per-set sums and their
//      total in set order, the class sums.
extern "C" int rt_sites_branch_expectations_mixture(rt_model *m, rt_sites *s, int recompute_transitions,
                                                    const double *class_weights, int64_t n_coefs,
                                                    int coefs_per_set, const double *coefs,
                                                    double *values, double *edge_sums,
                                                    double *set_edge_sums, double *class_post,
                                                    double *class_sums, double *loglik, int32_t *status)
{
    static const char who[] = "rt_sites_branch_expectations_mixture";
    post_pass p;                                 // (alive until the synchronisation below)
    RT_TRY(post_open(&p, who, m, s));
    RT_TRY(post_class_weights(who, m, class_weights));
    const rt_rate_sets &r = m->multi;
    const int64_t K = r.K;
    RT_REQUIRE(n_coefs >= 1 && coefs, "at least one coefficient matrix is needed");
    if (n_coefs > RT_MAX_BRANCH_COEFS) {
        rt_set_error("%s: at most %d coefficient matrices (%lld here)", who, RT_MAX_BRANCH_COEFS,
                     (long long)n_coefs);
        return RT_ERR_UNSUPPORTED;
    }
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    p.per_set = true;
    RT_TRY(post_layout(&p, true));
    RT_REQUIRE(r.P_stride == N * n * n, "unexpected stride of the sets' transition matrices");
    const size_t nn = (size_t)n * n;
    const int nk = (int)n_coefs;
    const size_t ncoef = (size_t)(coefs_per_set ? K : 1) * nk;
    for (size_t j = 0; j < ncoef * nn; ++j)
        RT_REQUIRE(std::isfinite(coefs[j]), "coefficient %lld of matrix %lld is not finite",
                   (long long)(j % nn), (long long)(j / nn));
    const size_t row = (size_t)N * nk;
    const bool sums = edge_sums || set_edge_sums || class_sums;
    const int nb = rt_partition_stage1_blocks(nsites);
    // scratch: L, M, D of every node and site, once (post_layout); x_k, the root totals and a status
    // word of every set; the posteriors, the combined values, the sums; the sets' tables
    post_plan &plan = p.plan;
    const size_t o_x = plan.take((size_t)K * nsites * row * 8);
    const size_t o_tot = plan.take((size_t)K * nsites * 8);
    const size_t o_stat = plan.take((size_t)K * nsites * 4);
    const size_t o_post = plan.take((size_t)nsites * K * 8), o_ll = plan.take((size_t)nsites * 8);
    const size_t o_val = plan.take(values ? (size_t)nsites * row * 8 : 8);
    const size_t o_setsum = plan.take((size_t)K * row * 8), o_sum = plan.take(row * 8);
    const size_t o_part = plan.take((size_t)K * nb * row * 8);
    const size_t o_csum = plan.take((size_t)K * 8), o_cw = plan.take((size_t)K * 8);
    set_tables T;
    T.take(&p, K, nk, coefs_per_set != 0);
    RT_TRY(post_begin(&p, recompute_transitions));
    hipStream_t st = p.st;
    unsigned char *base = p.base;
    double *d_x = (double *)(base + o_x), *d_tot = (double *)(base + o_tot);
    double *d_post = (double *)(base + o_post), *d_ll = (double *)(base + o_ll);
    double *d_val = (double *)(base + o_val);
    double *d_setsum = (double *)(base + o_setsum), *d_sum = (double *)(base + o_sum);
    double *d_part = (double *)(base + o_part), *d_csum = (double *)(base + o_csum);
    double *d_cw = (double *)(base + o_cw);
    int *d_stat = (int *)(base + o_stat);
    // (host buffer of an asynchronous copy: alive until the synchronisation below)
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    RT_HIP(hipMemcpyAsync(d_cw, class_weights, (size_t)K * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemsetAsync(d_stat, 0, (size_t)K * nsites * 4, st));
    // 1. the derivative tables
    RT_TRY(T.derivatives(&p, coefs));
    // 2. the passes, set by set (a set of weight zero is never live: not run, never read)
    RT_TRY(post_up(&p, internal.data(), false));
    if (!p.lane) RT_TRY(T.pack(&p));
    const size_t ne1 = (size_t)(N - 1);
    for (int64_t k = 0; k < K; ++k) {
        if (!(class_weights[k] > 0.0)) continue;
        double *xk = d_x + (size_t)k * nsites * row, *totk = d_tot + (size_t)k * nsites;
        int *statk = d_stat + (size_t)k * nsites;
        if (p.lane) {
            const int *d_tab = p.d_ptab;
            RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                hipLaunchKernelGGL((be_lane_kernel<decltype(nv)::value, false, true>),
                                   dim3((unsigned)((nsites + 255) / 256)), dim3(256), 0, st, (int)N,
                                   (long)nsites, (const double *)(r.d_P + k * r.P_stride),
                                   (const double *)(T.G + (size_t)k * ne1 * nn), nk, d_tab, d_tab + N,
                                   (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                                   s->block_sites, (const double *)m->d_root, p.d_L, p.d_M, p.d_D, xk,
                                   statk, (const int *)nullptr, 0, 0L, (int)K, totk);
                return RT_OK;
            }));
        } else {
            const rt_sites *x = p.x;
            RT_TRY(post_up_set(&p, k, nullptr));
            const double *PTk = T.PTs + (size_t)k * (T.tab / 8);
            const double *GTk = T.GT + (size_t)k * nk * (T.tab / 8);
            RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
                constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
                hipLaunchKernelGGL((be_down_kernel<NT, KS, false, true>), dim3((unsigned)x->nblocks),
                                   dim3(64 * NT), 0, st, PTk, GTk, nk, p.nops, (const int4 *)p.d_steps,
                                   (const double *)p.d_L, (const double *)p.d_M, p.d_D,
                                   (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root,
                                   (int)n, (int)N, xk, statk, (long)x->nsites, (long)x->nblocks,
                                   (const int *)nullptr, 0L, 0L, totk);
                return RT_OK;
            }));
        }
        RT_HIP(hipGetLastError());
    }
    // 3. posteriors, values, sums
    hipLaunchKernelGGL(mix_post_kernel<256>, dim3((unsigned)((nsites + 255) / 256)), dim3(256), 0, st, (int)K,
                       (long)nsites, (const double *)d_cw, (const double *)d_tot, (const int *)d_stat,
                       d_post, d_ll, p.d_status);
    RT_HIP(hipGetLastError());
    if (values) {
        const long by_row = row < 256 ? (long)(256 / row) : 1;
        const int S = (int)std::max<long>(1, std::min<long>(by_row, MIX_POST_LDS / K));
        hipLaunchKernelGGL(mix_combine_kernel, dim3((unsigned)((nsites + S - 1) / S)), dim3(256), 0, st,
                           (int)K, (long)nsites, (long)row, S, (const double *)d_post,
                           (const double *)d_x, d_val);
        RT_HIP(hipGetLastError());
        RT_HIP(hipMemcpyAsync(values, d_val, (size_t)nsites * row * 8, hipMemcpyDeviceToHost, st));
    }
    if (sums) {
        hipLaunchKernelGGL(mix_sums_stage1_kernel, dim3((unsigned)nb, (unsigned)K, (unsigned)N), dim3(256),
                           0, st, (int)N, nk, (long)nsites, (int)K, (const double *)d_x,
                           (const double *)d_post, (const double *)s->d_weights, nb, d_part);
        hipLaunchKernelGGL(part_sums_stage2_kernel, dim3((unsigned)K, (unsigned)N), dim3(256), 0, st, (int)N,
                           nk, (const double *)d_part, nb, d_setsum);
        hipLaunchKernelGGL(part_sums_total_kernel, dim3((unsigned)((row + 255) / 256)), dim3(256), 0, st,
                           (int)K, (long)row, (const double *)d_setsum, d_sum);
        hipLaunchKernelGGL(mix_class_sums_kernel, dim3((unsigned)K), dim3(256), 0, st, (int)K, (long)nsites,
                           (const double *)d_post, (const double *)s->d_weights, d_csum);
        RT_HIP(hipGetLastError());
        if (set_edge_sums)
            RT_HIP(hipMemcpyAsync(set_edge_sums, d_setsum, (size_t)K * row * 8, hipMemcpyDeviceToHost, st));
        if (edge_sums) RT_HIP(hipMemcpyAsync(edge_sums, d_sum, row * 8, hipMemcpyDeviceToHost, st));
        if (class_sums) RT_HIP(hipMemcpyAsync(class_sums, d_csum, (size_t)K * 8, hipMemcpyDeviceToHost, st));
    }
    if (class_post)
        RT_HIP(hipMemcpyAsync(class_post, d_post, (size_t)nsites * K * 8, hipMemcpyDeviceToHost, st));
    if (loglik) RT_HIP(hipMemcpyAsync(loglik, d_ll, (size_t)nsites * 8, hipMemcpyDeviceToHost, st));
    if (status) RT_HIP(hipMemcpyAsync(status, p.d_status, (size_t)nsites * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return RT_OK;
}
