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
// kernel, log-likelihoods, status and totals stay as they were.
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
    const size_t tile_stride = (size_t)NT * 256;
    auto at = [&](int step) { return ((size_t)step * nblocks + blk) * tile_stride + (m * 4) * 64 + lane; };
    const unsigned long long *nmask = masks, *amask = masks + 2 * PS_MAX, *bmask = masks + 4 * PS_MAX;
    bool bad = false;
    // the sums of one node over the state layout: own rows, the four lane groups, then the waves
    auto wave_part = [&](int slot, double v) {
        v += __shfl_xor(v, 16, 64);
        v += __shfl_xor(v, 32, 64);
        if (lane < 16) sums[slot][m][lane] = v;
    };
    // node sets of D (own rows d), into sums[0 .. nns)
    auto node_parts = [&](const double (&d)[4]) {
        for (int k = 0; k < nns; ++k) {
            double v = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (in_set(nmask + 2 * k, 16 * m + 4 * r + (lane >> 4))) v += d[r];
            wave_part(k, v);
        }
    };
    // after a barrier: wave 0 adds the waves' parts in order and writes the site's row
    auto write_sums = [&](int v, bool edges) {
        if (m == 0 && lane < 16 && site_ok) {
            for (int k = 0; k < nns; ++k) {
                double t = 0.0;
#pragma unroll
                for (int mm = 0; mm < NT; ++mm) t += sums[k][mm][lane];
                node_out[((size_t)site * nnodes + v) * nns + k] = t;
            }
            for (int k = 0; k < nes; ++k) {
                double t = 0.0;
                if (edges)
#pragma unroll
                    for (int mm = 0; mm < NT; ++mm) t += sums[PS_MAX + k][mm][lane];
                edge_out[((size_t)site * nnodes + v) * nes + k] = t;
            }
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
        const int i = nops - 1;
        const int4 st = steps[i];
        const size_t o = at(i);
        double wl[4], s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + 4 * r + (lane >> 4);
            const double w = row < n ? (root_w ? root_w[row] : 1.0) : 0.0;
            wl[r] = w * Larr[o + r * 64];
            s += wl[r];
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        if (lane < 16) red[m][lane] = s;
        __syncthreads();
        double tot = 0.0;
#pragma unroll
        for (int mm = 0; mm < NT; ++mm) tot += red[mm][lane & 15];
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
    // observation pairs holding this wave's own rows 4m..4m+3: q = 2m, 2m+1 (prune.hip)
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    for (int i = nops - 2; i >= 0; --i) {
        const int4 st = steps[i];
        const size_t o = at(i), po = at(st.y);
        double a[2 * KP];
#pragma unroll
        for (int q = 0; q < KP; ++q) {
            const double2 v = *(const double2 *)(ag + (size_t)i * ASTRIDE + q * 128);
            a[2 * q] = v.x;
            a[2 * q + 1] = v.y;
        }
        double L[4], u[4];
        if (st.z >= 0) {                         // an observed leaf: L is its observation
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = 2 * m + h;
                double2 v = {0.0, 0.0};
                if (q < KP) v = *(const double2 *)(og + ((size_t)st.z * KP + q) * 128);
                L[2 * h] = v.x;
                L[2 * h + 1] = v.y;
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) L[r] = Larr[o + r * 64];
        }
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
        // D_v = (P^T u) * L
        __syncthreads();                         // every wave is done with the previous operands
#pragma unroll
        for (int r = 0; r < 4; ++r) xb[(4 * m + r) * 64 + lane] = u[r];
        __syncthreads();
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int kk = 0; kk < KS; ++kk)
            acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xb[kk * 64 + lane], acc, 0, 0, 0);
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
                double4_t y = {0.0, 0.0, 0.0, 0.0};
#pragma unroll
                for (int kk = 0; kk < KS; ++kk)
                    y = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], xb[kk * 64 + lane], y, 0, 0, 0);
#pragma unroll
                for (int r = 0; r < 4; ++r)
                    if (in_set(bm, 16 * m + 4 * r + (lane >> 4))) v += y[r] * L[r];
            }
            wave_part(PS_MAX + k, v);
        }
        __syncthreads();
        write_sums(st.x, true);
        write_marg(st.w, d);
    }
    if (bad && site_ok) atomicOr(&status[site], 2);
}

// n <= 4: one lane per site (lane_obs of post_common.h reads the observations);
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
    // up: L_v = observation, times the messages of the children (descending preorder index)
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
            Marr[idx(v, a)] = t;
            Larr[idx(p, a)] *= t;
        }
    }
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
        double wl[N], L[N], d[N], tot = 0.0;
#pragma unroll
        for (int s = 0; s < N; ++s) {
            L[s] = Larr[idx(0, s)];
            wl[s] = (root_w ? root_w[s] : 1.0) * L[s];
            tot += wl[s];
        }
        const bool zero = !(tot > 0.0);
#pragma unroll
        for (int s = 0; s < N; ++s) {
            d[s] = zero ? 0.0 : wl[s] / tot;
            Darr[idx(0, s)] = d[s];
        }
        if (zero) status[site] |= RT_SITE_ZERO_PROB;
        sums(0, d, d, L, nullptr);
    }
    bool bad = false;
    for (int v = 1; v < nnodes; ++v) {
        const int p = parent[v];
        const double *Pv = P + (size_t)v * N * N;
        double u[N], L[N], d[N];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            const double dp = Darr[idx(p, a)];
            const double den = Marr[idx(v, a)];
            u[a] = 0.0;
            if (dp != 0.0) {
                if (den > 0.0) u[a] = dp / den;
                else bad = true;
            }
        }
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

template <int NT, int KS>
int launch_down(rt_ctx *ctx, const double *d_PT, int nops, const int4 *d_steps, const double *d_L,
                const double *d_M, double *d_D, const rt_sites *x, const double *d_root, int n,
                const unsigned long long *d_masks, int nns, int nes, unsigned a_full, int nnodes,
                int nmarg, double *d_node, double *d_edge, double *d_marg, int *d_status)
{
    hipLaunchKernelGGL((post_down_kernel<NT, KS>), dim3((unsigned)x->nblocks), dim3(64 * NT), 0, ctx->stream,
                       d_PT, nops, d_steps, d_L, d_M, d_D, (const double *)x->d_obs, (int)x->nobs, d_root,
                       n, d_masks, nns, nes, a_full, nnodes, nmarg, d_node, d_edge, d_marg, d_status,
                       (long)x->nsites, (long)x->nblocks);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

}  // namespace

extern "C" int rt_sites_posteriors(rt_model *m, rt_sites *s, int recompute_transitions,
                                   int64_t n_node_sets, const uint64_t *node_sets, int64_t n_edge_sets,
                                   const uint64_t *edge_sets, int64_t n_marginal_nodes,
                                   const int64_t *marginal_nodes, double *node_values,
                                   double *edge_values, double *marginals, int32_t *status)
{
    RT_REQUIRE(m && s, "null pointer");
    RT_REQUIRE(s->model == m, "the site batch belongs to another model");
    RT_REQUIRE(n_node_sets >= 0 && n_edge_sets >= 0 && n_marginal_nodes >= 0, "negative count");
    RT_REQUIRE(!n_node_sets || node_sets, "node_sets is null");
    RT_REQUIRE(!n_edge_sets || edge_sets, "edge_sets is null");
    const int64_t n = m->n, N = m->nnodes, nsites = s->nsites;
    if (n_node_sets > RT_MAX_POSTERIOR_SETS || n_edge_sets > RT_MAX_POSTERIOR_SETS) {
        rt_set_error("rt_sites_posteriors: at most %d node sets and %d edge sets (%lld, %lld here)",
                     RT_MAX_POSTERIOR_SETS, RT_MAX_POSTERIOR_SETS, (long long)n_node_sets,
                     (long long)n_edge_sets);
        return RT_ERR_UNSUPPORTED;
    }
    const bool lane = s->layout == RT_LAYOUT_LANE;
    if (s->rescale || N < 2 || n < 2 || n > RT_MAX_STATES || s->d_scratch ||
        m->max_depth > RT_FAST_MAX_DEPTH || lane != (n <= 4)) {
        rt_set_error("rt_sites_posteriors: batches of 2..%d states without \"rescale\" on trees of "
                     "at least two nodes that the fast kernels take (n=%lld, nnodes=%lld, depth %d%s)",
                     RT_MAX_STATES, (long long)n, (long long)N, m->max_depth,
                     s->rescale ? ", rescale" : "");
        return RT_ERR_UNSUPPORTED;
    }
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
    rt_ctx *ctx = m->ctx;
    RT_HIP(hipSetDevice(ctx->device));
    const int NT = (int)((n + 15) / 16), KS = (int)((n + 3) / 4), KP = (KS + 1) / 2;
    const int nops = (int)s->ops.size();
    // scratch: L, M, D of every node and site, the outputs, the step table, the masks
    const size_t arr = lane ? (size_t)N * n * nsites * 8 : (size_t)nops * s->nblocks * NT * 256 * 8;
    post_plan plan;
    const size_t o_L = plan.take(arr), o_M = plan.take(arr), o_D = plan.take(arr);
    const size_t o_node = plan.take((size_t)nsites * N * std::max(nns, 1) * 8);
    const size_t o_edge = plan.take((size_t)nsites * N * std::max(nes, 1) * 8);
    const size_t o_marg = plan.take((size_t)nsites * std::max<int64_t>(nmarg, 1) * n * 8);
    const size_t o_status = plan.take((size_t)nsites * 4);
    const size_t o_masks = plan.take(masks.size() * 8);
    const size_t o_steps = plan.take((size_t)std::max<int64_t>(nops, N) * 16);
    const size_t o_PT = lane ? plan.take(8) : plan.take((size_t)nops * NT * KP * 128 * 8);
    const size_t o_ptab = plan.take((size_t)3 * N * 4);
    if ((double)plan.total > 96e9) {
        rt_set_error("rt_sites_posteriors: this batch needs %.0f GB of scratch; split the batch",
                     (double)plan.total / 1e9);
        return RT_ERR_UNSUPPORTED;
    }
    if (recompute_transitions) RT_TRY(rt_model_recompute_transitions(m));
    RT_REQUIRE(m->have_P, "the model has no transition matrices yet");
    hipStream_t st = ctx->stream;
    rt_sites *x = nullptr;
    if (!lane) {
        if (!s->expect_twin) RT_TRY(rt_sites_twin_interpreter(s, &s->expect_twin));
        x = s->expect_twin;
    }
    RT_TRY(rt_scratch_reserve(ctx, plan.total));
    unsigned char *base = ctx->d_scratch;
    double *d_L = (double *)(base + o_L), *d_M = (double *)(base + o_M), *d_D = (double *)(base + o_D);
    double *d_node = (double *)(base + o_node), *d_edge = (double *)(base + o_edge);
    double *d_marg = (double *)(base + o_marg);
    int *d_status = (int *)(base + o_status);
    unsigned long long *d_masks = (unsigned long long *)(base + o_masks);
    RT_HIP(hipMemsetAsync(d_status, 0, (size_t)nsites * 4, st));
    RT_HIP(hipMemcpyAsync(d_masks, masks.data(), masks.size() * 8, hipMemcpyHostToDevice, st));
    std::vector<int32_t> table, step_node;       // (alive until the synchronisation below)
    if (lane) {
        post_lane_table(m, s, marg_row.data(), &table);
        int *d_tab = (int *)(base + o_ptab);
        RT_HIP(hipMemcpyAsync(d_tab, table.data(), table.size() * 4, hipMemcpyHostToDevice, st));
        const unsigned grid = (unsigned)((nsites + 255) / 256);
#define RT_POST_LANE(NV)                                                                            \
        hipLaunchKernelGGL((post_lane_kernel<NV>), dim3(grid), dim3(256), 0, st, (int)N, (long)nsites,   \
                           (const double *)m->d_P, d_tab, d_tab + N, (const void *)s->d_obs,            \
                           s->compact_states, (int)s->nobs, s->block_sites, (const double *)m->d_root,  \
                           (const unsigned long long *)d_masks, nns, nes, d_tab + 2 * N, (int)nmarg,    \
                           d_L, d_M, d_D, d_node, d_edge, d_marg, d_status)
        switch ((int)n) {
        case 2: RT_POST_LANE(2); break;
        case 3: RT_POST_LANE(3); break;
        default: RT_POST_LANE(4); break;
        }
#undef RT_POST_LANE
        RT_HIP(hipGetLastError());
    } else {
        // the step table of the downward pass
        RT_TRY(post_step_table(m, x, marg_row.data(), &table, &step_node));
        int4 *d_steps = (int4 *)(base + o_steps);
        double *d_PT = (double *)(base + o_PT);
        int *d_step_node = (int *)(base + o_ptab);
        RT_HIP(hipMemcpyAsync(d_steps, table.data(), table.size() * 4, hipMemcpyHostToDevice, st));
        RT_HIP(hipMemcpyAsync(d_step_node, step_node.data(), (size_t)nops * 4, hipMemcpyHostToDevice, st));
        // upward pass: the split-M interpreter kernel with L and M of every step stored (its own
        // log-likelihoods and totals are the twin's, not the batch's)
        x->d_Lout = d_L;
        x->d_Mout = d_M;
        const int rc = rt_launch_prune(m, x, false);
        x->d_Lout = x->d_Mout = nullptr;
        RT_TRY(rc);
        RT_TRY(rt_launch_pack_pt(ctx, (int)n, NT, KP, nops, d_step_node, m->d_P, d_PT));
        int lrc = RT_ERR_UNSUPPORTED;
#define RT_PD(NTV, KSV)                                                                               \
        case KSV: lrc = launch_down<NTV, KSV>(ctx, d_PT, nops, d_steps, d_L, d_M, d_D, x, m->d_root,  \
                                              (int)n, d_masks, nns, nes, a_full, (int)N, (int)nmarg,   \
                                              d_node, d_edge, d_marg, d_status); break
        switch (KS) {
        RT_PD(1, 2); RT_PD(1, 3); RT_PD(1, 4);
        RT_PD(2, 5); RT_PD(2, 6); RT_PD(2, 7); RT_PD(2, 8);
        RT_PD(3, 9); RT_PD(3, 10); RT_PD(3, 11); RT_PD(3, 12);
        RT_PD(4, 13); RT_PD(4, 14); RT_PD(4, 15); RT_PD(4, 16);
        RT_PD(5, 17); RT_PD(5, 18); RT_PD(5, 19); RT_PD(5, 20);
        RT_PD(6, 21); RT_PD(6, 22); RT_PD(6, 23); RT_PD(6, 24);
        RT_PD(7, 25); RT_PD(7, 26); RT_PD(7, 27); RT_PD(7, 28);
        RT_PD(8, 29); RT_PD(8, 30); RT_PD(8, 31); RT_PD(8, 32);
        default: break;
        }
#undef RT_PD
        RT_TRY(lrc);
    }
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
