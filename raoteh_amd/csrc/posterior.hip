// Posterior node marginals and joint-endpoint set sums of a RESIDENT batch (rt_sites_posteriors).
//
// _mcy_dense.kitchen_sink (raoteh/sampler/_mcy_dense.py:57-230) computes, per site, the posterior
// marginal D_v of every node (mc0_esd_get_node_to_distn) and the joint endpoint posterior of every
// edge p -> v (mc0_esd_get_joint_endpoint_distn),
//     D_v = (P_v^T u) * L_v,   J_v[a][b] = u[a] P_v[a][b] L_v[b],   u = D_p / M_v,
// with L_v the subtree likelihood and M_v = P_v L_v the message to the parent.  A caller such as
// examples/p53/liwen-branch-expectation.py reads a few sums out of each: D_v summed over a state
// set, J_v summed over a block A x B.  Here those sums are formed on the device and only they (and
// the marginals asked for) come back:
//     node set S:      sum_{s in S} D_v[s]
//     edge set (A, B): sum_{b in B} L_v[b] (P_v^T (u * 1_A))[b]   (= sum_{b in B} D_v[b] when A
//                      is every state: no product)
//
//   n > 4   the split-M interpreter pruning kernel with L and M of every step stored (the upward
//           pass of expect_mfma.hip, prune.hip), then post_down_kernel: one workgroup of NT row-tile
//           waves per 16-site tile walks the steps in reverse with D through HBM, P^T as A
//           fragments, u exchanged through LDS as B operands.  Unlike the expectation pass every
//           step forms D (leaves included: their L is the batch's resident observation image).
//   n <= 4  post_lane_kernel: one lane per site, L, M and D in [node][state][site] scratch.
//
// Every sum is taken in a fixed order (the four lane groups by xor shuffles, then the waves in
// order), so two calls give the same bits.  Nothing of the batch is written: its own pruning
// kernel, log-likelihoods, status and totals stay as they were.  The checks, the scratch, the
// upward pass and the steps of the two kernels that rt_sites_branch_expectations and the sampling
// calls make as well are post_common.h's.
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int PS_MAX = RT_MAX_POSTERIOR_SETS;

// set masks on the device: [node sets | edge A | edge B][PS_MAX][2 words]
__device__ inline bool in_set(const unsigned long long *mask, int s)
{
    return (mask[s >> 6] >> (s & 63)) & 1ull;
}

// steps[i] = {node, step of the parent, stream position of an observed leaf or -1, marginal row
// or -1}; the root is the last step.  Per step: u = D_p / M_v, D_v = (P_v^T u) * L_v, the sums.
template <int NT, int KS>
__global__ void __launch_bounds__(64 * NT)
post_down_kernel(const double *__restrict__ PfragT, int nops, const int4 *__restrict__ steps,
                 const double *__restrict__ Larr, const double *__restrict__ Marr,
                 double *__restrict__ Darr, const double *__restrict__ obs, int K,
                 const double *__restrict__ root_w, int n, const unsigned long long *__restrict__ masks,
                 int nns, int nes, unsigned a_full, int nnodes, int nmarg,
                 double *__restrict__ node_out, double *__restrict__ edge_out,
                 double *__restrict__ marg_out, int *__restrict__ status, long nsites, long nblocks)
{
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double red[NT][16];
    __shared__ double sums[2 * PS_MAX][NT][16];
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    const long site = blk * 16 + (lane & 15);
    const bool site_ok = site < nsites;
    const unsigned long long *nmask = masks, *amask = masks + 2 * PS_MAX, *bmask = masks + 4 * PS_MAX;
    bool bad = false;
    // node sets of D (own rows d), into sums[0 .. nns): own rows, the four lane groups, then
    // (write_sums) the waves
    auto node_parts = [&](const double (&d)[4]) {
        for (int k = 0; k < nns; ++k) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (in_set(nmask + 2 * k, 16 * m + 4 * r + (lane >> 4))) v += d[r];
            down_part(sums[k], m, lane, v);
        }
    };
    // after a barrier: wave 0 adds the waves' parts in order and writes the site's row
    auto write_sums = [&](int v, bool edges) {
        if (m == 0 && lane < 16 && site_ok) {
            for (int k = 0; k < nns; ++k)
                node_out[((size_t)site * nnodes + v) * nns + k] = down_total<NT>(sums[k], lane);
            for (int k = 0; k < nes; ++k)
                edge_out[((size_t)site * nnodes + v) * nes + k] =
                    edges ? down_total<NT>(sums[PS_MAX + k], lane) : 0.0;
        }
    };
    auto write_marg = [&](int j, const double (&d)[4]) {
        if (j >= 0 && site_ok) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * m + 4 * r + (lane >> 4);
                if (row < n) marg_out[((size_t)site * nmarg + j) * n + row] = d[r];
            }
        }
    };
    // root: D = w L / sum_states(w L)  (_mc0_dense.py:400-489 with the prior weights)
    {
        const int4 st = steps[nops - 1];
        const size_t o = down_at<NT>(nops - 1, nblocks, blk, m, lane);
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
        double d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            d[r] = zero ? 0.0 : wl[r] / tot;
            Darr[o + r * 64] = d[r];
        }
        if (zero && m == 0 && lane < 16 && site_ok) atomicOr(&status[site], RT_SITE_ZERO_PROB);
        node_parts(d);
        __syncthreads();
        write_sums(st.x, false);                 // (the root has no edge: its slot is 0)
        write_marg(st.w, d);
    }
    const double *ag = PfragT + ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    for (int i = nops - 2; i >= 0; --i) {
        const int4 st = steps[i];
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        double a[2 * KP], L[4], u[4];
        down_frag<KP>(ag + (size_t)i * ASTRIDE, a);
        down_L<KP>(st.z, og, Larr, o, m, L);
        down_u(Darr, down_at<NT>(st.y, nblocks, blk, m, lane), Marr, o, u, bad);
        // D_v = (P^T u) * L
        down_stage(xb, m, lane, u);
        const double4_t acc = down_product<KS>(a, xb, lane);
        double d[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            d[r] = acc[r] * L[r];
            Darr[o + r * 64] = d[r];
        }
        node_parts(d);
        for (int k = 0; k < nes; ++k) {
            const unsigned long long *bm = bmask + 2 * k;
            double v = 0.0;
            if ((a_full >> k) & 1u) {            // A = every state: the node sum over B
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (in_set(bm, 16 * m + 4 * r + (lane >> 4))) v += d[r];
            } else {
                const unsigned long long *am = amask + 2 * k;
                __syncthreads();
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    xb[(4 * m + r) * 64 + lane] = in_set(am, 16 * m + 4 * r + (lane >> 4)) ? u[r] : 0.0;
                __syncthreads();
                const double4_t y = down_product<KS>(a, xb, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (in_set(bm, 16 * m + 4 * r + (lane >> 4))) v += y[r] * L[r];
            }
            down_part(sums[PS_MAX + k], m, lane, v);
        }
        __syncthreads();
        write_sums(st.x, true);
        write_marg(st.w, d);
    }
    if (bad && site_ok) atomicOr(&status[site], 2);
}

// n <= 4: one lane per site (the upward pass, the root and u: post_common.h);
// arrays [node][state][site]; nodes in preorder (a parent before its children)
template <int N>
__global__ void __launch_bounds__(256)
post_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const int *__restrict__ parent,
                 const int *__restrict__ node_k, const void *__restrict__ obs, int compact, int K,
                 int block_sites, const double *__restrict__ root_w,
                 const unsigned long long *__restrict__ masks, int nns, int nes,
                 const int *__restrict__ marg_row, int nmarg, double *__restrict__ Larr,
                 double *__restrict__ Marr, double *__restrict__ Darr, double *__restrict__ node_out,
                 double *__restrict__ edge_out, double *__restrict__ marg_out, int *__restrict__ status)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    const unsigned long long *nmask = masks, *amask = masks + 2 * PS_MAX, *bmask = masks + 4 * PS_MAX;
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, K, block_sites, Larr, Marr);
    auto sums = [&](int v, const double (&d)[N], const double (&u)[N], const double (&L)[N], const double *Pv) {
        for (int k = 0; k < nns; ++k) {
            double t = 0.0;
#pragma unroll
            for (int s = 0; s < N; ++s)
                if (in_set(nmask + 2 * k, s)) t += d[s];
            node_out[((size_t)site * nnodes + v) * nns + k] = t;
        }
        for (int k = 0; k < nes; ++k) {
            double t = 0.0;
            if (Pv) {
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    if (!in_set(bmask + 2 * k, b)) continue;
                    double y = 0.0;
#pragma unroll
                    for (int a = 0; a < N; ++a)
                        if (in_set(amask + 2 * k, a)) y += Pv[a * N + b] * u[a];
                    t += y * L[b];
                }
            }
            edge_out[((size_t)site * nnodes + v) * nes + k] = t;
        }
        const int j = marg_row[v];
        if (j >= 0)
#pragma unroll
            for (int s = 0; s < N; ++s) marg_out[((size_t)site * nmarg + j) * N + s] = d[s];
    };
    // down: the root, then every node after its parent
    {
        double d[N];
        if (lane_root<N>(nsites, site, root_w, Larr, Darr, d)) status[site] |= RT_SITE_ZERO_PROB;
        sums(0, d, d, d, nullptr);               // (no edge: u and L are not read)
    }
    bool bad = false;
    for (int v = 1; v < nnodes; ++v) {
        const int p = parent[v];
        const double *Pv = P + (size_t)v * N * N;
        double u[N], L[N], d[N];
        lane_u<N>(nsites, site, p, v, Darr, Marr, u, bad);
#pragma unroll
        for (int b = 0; b < N; ++b) {
            L[b] = Larr[idx(v, b)];
            double y = 0.0;
#pragma unroll
            for (int a = 0; a < N; ++a) y += Pv[a * N + b] * u[a];
            d[b] = y * L[b];
            Darr[idx(v, b)] = d[b];
        }
        sums(v, d, u, L, Pv);
    }
    if (bad) status[site] |= 2;
}

}  // namespace

extern "C" int rt_sites_posteriors(rt_model *m, rt_sites *s, int recompute_transitions,
                                   int64_t n_node_sets, const uint64_t *node_sets, int64_t n_edge_sets,
                                   const uint64_t *edge_sets, int64_t n_marginal_nodes,
                                   const int64_t *marginal_nodes, double *node_values,
                                   double *edge_values, double *marginals, int32_t *status)
{
    post_pass p;                                 // (alive until the synchronisation below)
    RT_TRY(post_open(&p, "rt_sites_posteriors", m, s));
    RT_REQUIRE(n_node_sets >= 0 && n_edge_sets >= 0 && n_marginal_nodes >= 0, "negative count");
    RT_REQUIRE(!n_node_sets || node_sets, "node_sets is null");
    RT_REQUIRE(!n_edge_sets || edge_sets, "edge_sets is null");
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    if (n_node_sets > RT_MAX_POSTERIOR_SETS || n_edge_sets > RT_MAX_POSTERIOR_SETS) {
        rt_set_error("rt_sites_posteriors: at most %d node sets and %d edge sets (%lld, %lld here)",
                     RT_MAX_POSTERIOR_SETS, RT_MAX_POSTERIOR_SETS, (long long)n_node_sets,
                     (long long)n_edge_sets);
        return RT_ERR_UNSUPPORTED;
    }
    RT_TRY(post_layout(&p, true));
    // the sets: no state beyond n
    const int words = 2;
    std::vector<unsigned long long> masks((size_t)3 * RT_MAX_POSTERIOR_SETS * words, 0ull);
    unsigned a_full = 0;
    auto check_mask = [&](const uint64_t *w) {
        for (int k = 0; k < words; ++k)
            for (int b = 0; b < 64; ++b)
                if (((w[k] >> b) & 1ull) && 64 * k + b >= n) return false;
        return true;
    };
    for (int64_t k = 0; k < n_node_sets; ++k) {
        RT_REQUIRE(check_mask(node_sets + 2 * k), "node set %lld holds a state >= n", (long long)k);
        masks[(size_t)k * 2] = node_sets[2 * k];
        masks[(size_t)k * 2 + 1] = node_sets[2 * k + 1];
    }
    for (int64_t k = 0; k < n_edge_sets; ++k) {
        const uint64_t *A = edge_sets + 4 * k, *B = A + 2;
        RT_REQUIRE(check_mask(A) && check_mask(B), "edge set %lld holds a state >= n", (long long)k);
        bool full = true;
        for (int64_t st = 0; st < n; ++st) full = full && ((A[st >> 6] >> (st & 63)) & 1ull);
        if (full) a_full |= 1u << k;
        for (int w = 0; w < 2; ++w) {
            masks[((size_t)RT_MAX_POSTERIOR_SETS + k) * 2 + w] = A[w];
            masks[((size_t)2 * RT_MAX_POSTERIOR_SETS + k) * 2 + w] = B[w];
        }
    }
    // the marginal rows: node -> row
    std::vector<int> marg_row((size_t)N, -1);
    int64_t nmarg = marginals ? n_marginal_nodes : 0;
    if (marginals) {
        if (!marginal_nodes) {
            RT_REQUIRE(n_marginal_nodes == N, "marginal_nodes = NULL means every node: "
                       "n_marginal_nodes must be nnodes");
            for (int64_t v = 0; v < N; ++v) marg_row[(size_t)v] = (int)v;
        } else {
            for (int64_t j = 0; j < n_marginal_nodes; ++j) {
                const int64_t v = marginal_nodes[j];
                RT_REQUIRE(v >= 0 && v < N, "marginal node %lld out of range", (long long)v);
                RT_REQUIRE(marg_row[(size_t)v] < 0, "marginal node %lld listed twice", (long long)v);
                marg_row[(size_t)v] = (int)j;
            }
        }
    }
    const int nns = node_values ? (int)n_node_sets : 0, nes = edge_values ? (int)n_edge_sets : 0;
    // scratch: L, M, D of every node and site (post_layout), the outputs, the masks
    const size_t o_node = p.plan.take((size_t)nsites * N * std::max(nns, 1) * 8);
    const size_t o_edge = p.plan.take((size_t)nsites * N * std::max(nes, 1) * 8);
    const size_t o_marg = p.plan.take((size_t)nsites * std::max<int64_t>(nmarg, 1) * n * 8);
    const size_t o_masks = p.plan.take(masks.size() * 8);
    RT_TRY(post_begin(&p, recompute_transitions));
    hipStream_t st = p.st;
    double *d_node = (double *)(p.base + o_node), *d_edge = (double *)(p.base + o_edge);
    double *d_marg = (double *)(p.base + o_marg);
    int *d_status = p.d_status;
    unsigned long long *d_masks = (unsigned long long *)(p.base + o_masks);
    RT_HIP(hipMemcpyAsync(d_masks, masks.data(), masks.size() * 8, hipMemcpyHostToDevice, st));
    RT_TRY(post_up(&p, marg_row.data(), true));
    if (p.lane) {
        const int *d_tab = p.d_ptab;
        RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
            hipLaunchKernelGGL((post_lane_kernel<decltype(nv)::value>), dim3((unsigned)((nsites + 255) / 256)),
                               dim3(256), 0, st, (int)N, (long)nsites, (const double *)m->d_P, d_tab,
                               d_tab + N, (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                               s->block_sites, (const double *)m->d_root,
                               (const unsigned long long *)d_masks, nns, nes, d_tab + 2 * N, (int)nmarg,
                               p.d_L, p.d_M, p.d_D, d_node, d_edge, d_marg, d_status);
            return RT_OK;
        }));
    } else {
        const rt_sites *x = p.x;
        RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
            constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
            hipLaunchKernelGGL((post_down_kernel<NT, KS>), dim3((unsigned)x->nblocks), dim3(64 * NT), 0, st,
                               (const double *)p.d_PT, p.nops, (const int4 *)p.d_steps,
                               (const double *)p.d_L, (const double *)p.d_M, p.d_D,
                               (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root, (int)n,
                               (const unsigned long long *)d_masks, nns, nes, a_full, (int)N, (int)nmarg,
                               d_node, d_edge, d_marg, d_status, (long)x->nsites, (long)x->nblocks);
            return RT_OK;
        }));
    }
    RT_HIP(hipGetLastError());
    // only what was asked for crosses PCIe
    if (node_values && n_node_sets)
        RT_HIP(hipMemcpyAsync(node_values, d_node, (size_t)nsites * N * nns * 8, hipMemcpyDeviceToHost, st));
    if (edge_values && n_edge_sets)
        RT_HIP(hipMemcpyAsync(edge_values, d_edge, (size_t)nsites * N * nes * 8, hipMemcpyDeviceToHost, st));
    if (marginals && nmarg)
        RT_HIP(hipMemcpyAsync(marginals, d_marg, (size_t)nsites * nmarg * n * 8, hipMemcpyDeviceToHost, st));
    if (status) RT_HIP(hipMemcpyAsync(status, d_status, (size_t)nsites * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return RT_OK;
}
