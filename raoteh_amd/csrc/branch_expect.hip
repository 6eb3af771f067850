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
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <cmath>
#include <vector>

namespace {

constexpr int BC_MAX = RT_MAX_BRANCH_COEFS;

// W[e][r][c] = C_e[c][r]: C_e = E * Q_e off the diagonal, E on it (edge e is node e + 1)
__global__ void __launch_bounds__(256)
direction_kernel(int n, const double *__restrict__ Q, const int *__restrict__ qidx,
                 const double *__restrict__ E, double *__restrict__ W)
{
    const int e = blockIdx.x;
    const int nn = n * n;
    const double *Qe = Q + (size_t)qidx[e] * nn;
    for (int k = threadIdx.x; k < nn; k += 256) {
        const int r = k / n, c = k - r * n;
        const double w = E[c * n + r];
        W[(size_t)e * nn + k] = r == c ? w : (w != 0.0 ? w * Qe[c * n + r] : 0.0);
    }
}

// steps[i] = {node, step of the parent, stream position of an observed leaf or -1, 1 if the node
// has children}; the root is the last step.  GfragT: [k][step] A fragments of G_k^T.
template <int NT, int KS>
__global__ void __launch_bounds__(64 * NT)
be_down_kernel(const double *__restrict__ PfragT, const double *__restrict__ GfragT, int nk, int nops,
               const int4 *__restrict__ steps, const double *__restrict__ Larr,
               const double *__restrict__ Marr, double *__restrict__ Darr,
               const double *__restrict__ obs, int K, const double *__restrict__ root_w, int n,
               int nnodes, double *__restrict__ out, int *__restrict__ status, long nsites, long nblocks)
{
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double red[NT][16];
    __shared__ double sums[BC_MAX][NT][16];
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
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
template <int N>
__global__ void __launch_bounds__(256)
be_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const double *__restrict__ G,
               int nk, const int *__restrict__ parent, const int *__restrict__ node_k,
               const void *__restrict__ obs, int compact, int K, int block_sites,
               const double *__restrict__ root_w, double *__restrict__ Larr,
               double *__restrict__ Marr, double *__restrict__ Darr, double *__restrict__ out,
               int *__restrict__ status)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, K, block_sites, Larr, Marr);
    // down: the root, then every node after its parent
    {
        double d[N];
        if (lane_root<N>(nsites, site, root_w, Larr, Darr, d)) status[site] |= RT_SITE_ZERO_PROB;
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
            const double *Gv = G + ((size_t)k * nnodes + v) * N * N;
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
    std::vector<int32_t> ident(ne), internal((size_t)N, 0);
    for (size_t e = 0; e < ne; ++e) ident[e] = (int32_t)e;
    for (int64_t v = 1; v < N; ++v) internal[(size_t)m->parent[(size_t)v]] = 1;
    RT_HIP(hipMemcpyAsync(d_E, coefs, (size_t)nk * nn * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_ones, ones.data(), ne * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_ident, ident.data(), ne * 4, hipMemcpyHostToDevice, st));
    // 1. the derivative tables: one launch of the derivative route per coefficient matrix (the
    //    root's slot of every table is zero)
    for (int k = 0; k < nk; ++k) {
        double *Gk = d_G + (size_t)k * N * nn;
        RT_HIP(hipMemsetAsync(Gk, 0, nn * 8, st));
        hipLaunchKernelGGL(direction_kernel, dim3((unsigned)ne), dim3(256), 0, st, (int)n,
                           (const double *)m->d_Q, (const int *)(m->d_qidx + 1),
                           (const double *)(d_E + (size_t)k * nn), d_W);
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
                               (const double *)m->d_root, p.d_L, p.d_M, p.d_D, d_val, d_status);
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
                               (int)n, (int)N, d_val, d_status, (long)x->nsites, (long)x->nblocks);
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
