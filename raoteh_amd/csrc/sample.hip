// Joint draws of a state for every node from the posterior of a RESIDENT batch
// (rt_sites_sample_states).
//
// _sample_mcy_dense.resample_states (raoteh/sampler/_sample_mcy_dense.py:23-69) through
// _sample_mc0_dense.resample_states (_sample_mc0_dense.py:20-98): with L_v the subtree likelihood
// of node v (its own observation included), root ~ root_w * L_root, then every node after its
// parent, child ~ P_v[parent's state] * L_v.  Unlike rt_forest_resample_states (forest.hip: one P
// shared by every edge of every tree) each edge has its own P_v, the model's.
//
//   n > 4   the split-M interpreter pruning kernel with L of every step stored (post_up of
//           post_common.h, the upward pass of every read of a resident batch; its store variant
//           writes M unconditionally, so it is handed a buffer for M as well), then sample_down_kernel: one wave per (16-site tile, block of DB draws)
//           walks the steps in reverse.  A lane holds the rows of L the upward pass stored for it
//           (16 m + 4 r + (lane >> 4) of site lane & 15), so L_v is one coalesced load per draw
//           BLOCK; per draw the lane gathers its entries of the P row its site's parent state
//           selects, and a scan over the 4 NT chunks of four states picks the state.  The sampled
//           states of the block live in a wave-private LDS table [node][DB][16].
//   n <= 4  sample_lane_up_kernel (one lane per site, L in [node][state][site] scratch), then
//           sample_lane_down_kernel: one thread per (site, draw).
//
// The uniform of (draw d, site i, node v) is philox_uniform(seed, first_draw + d, i * nnodes + v):
// a draw does not depend on the launch shape, on ndraws or on how a call is split.  Nothing of the
// batch is written.
#include "common.h"
#include "philox.h"
#include "post_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int SAMPLE_MAX_DB = 16;              // draws per block at most
constexpr size_t SAMPLE_LDS_TARGET = 32 * 1024;    // the table of a wave, when DB can be chosen
constexpr unsigned char NO_STATE = 255;

__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// steps[i] = {node, -, stream position of an observed leaf or -1, parent node or -1}; the root is
// the last step (post_step_table with the parent table as its last column)
template <int NT>
__global__ void __launch_bounds__(64)
sample_down_kernel(const double *__restrict__ P, int nops, const int4 *__restrict__ steps,
                   const double *__restrict__ Larr, const double *__restrict__ obs, int K,
                   const double *__restrict__ root_w, int n, int nnodes, int DB,
                   unsigned long long seed, unsigned long long first_draw, long ndraws,
                   unsigned char *__restrict__ states, int *__restrict__ status, long nsites,
                   long nblocks)
{
    constexpr int NC = 4 * NT;                 // chunks of four states; rows of one lane
    extern __shared__ unsigned char tab[];     // [node][DB][16] sampled states of this block
    const int lane = threadIdx.x;
    const int g = lane >> 4, j = lane & 15;
    const long blk = (long)(blockIdx.x % (unsigned long)nblocks);
    const long d0 = (long)(blockIdx.x / (unsigned long)nblocks) * DB;
    const int nd = (int)(ndraws - d0 < DB ? ndraws - d0 : DB);
    const long site = blk * 16 + j;
    const bool site_ok = site < nsites;
    const int KP = ((n + 3) / 4 + 1) / 2;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    int flags = 0;
    for (int i = nops - 1; i >= 0; --i) {
        const int4 st = steps[i];
        const int v = st.x, p = st.w;
        const bool root = i == nops - 1;       // (uniform, as every branch on the schedule)
        // own rows of L_v: what the upward pass stored, or the observation of an observed leaf
        double L[NC];
        if (st.z >= 0) {
#pragma unroll
            for (int q = 0; q < 2 * NT; ++q) {
                double2 x = {0.0, 0.0};
                if (q < KP) x = *(const double2 *)(og + ((size_t)st.z * KP + q) * 128);
                L[2 * q] = x.x;
                L[2 * q + 1] = x.y;
            }
        } else {
            const double *lp = Larr + ((size_t)i * nblocks + blk) * (NT * 256) + lane;
#pragma unroll
            for (int k = 0; k < NC; ++k) L[k] = lp[k * 64];
        }
        // (rows at or above n are padding: an unobserved leaf stores ones there)
        if (root) {
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int row = 4 * k + g;
                L[k] = row < n ? (root_w ? root_w[row] : 1.0) * L[k] : 0.0;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NC; ++k)
                if (4 * k + g >= n) L[k] = 0.0;
        }
        const double *Pv = P + (size_t)v * n * n;
        for (int d = 0; d < nd; ++d) {
            int a = 0;
            bool dead = false;
            if (!root) {
                a = tab[((size_t)p * DB + d) * 16 + j];
                dead = a == NO_STATE;
                if (dead) a = 0;
            }
            const double *prow = Pv + (size_t)a * n;
            double w[NC], cum[NC];
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const int row = 4 * k + g;
                double x = L[k];
                if (!root) x *= row < n ? prow[row] : 0.0;
                w[k] = x > 0.0 ? x : 0.0;      // negative products (and NaN) count as 0
            }
            // chunk sums over the four lanes of the site (the same bits in all four), running sum
            double run = 0.0;
            int last = -1;                     // the last own state of positive weight
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                double c = w[k];
                c += __shfl_xor(c, 16, 64);
                c += __shfl_xor(c, 32, 64);
                run += c;
                cum[k] = run;
                if (w[k] > 0.0) last = 4 * k + g;
            }
            last = max(last, __shfl_xor(last, 16, 64));
            last = max(last, __shfl_xor(last, 32, 64));
            const double total = run;
            const double u = philox_uniform(seed, first_draw + (unsigned long long)(d0 + d),
                                            (unsigned long long)site * (unsigned long long)nnodes +
                                                (unsigned long long)v);
            const double target = u * total;
            // the first chunk whose cumulative weight exceeds the target (its own sum is then
            // positive), the sum before it and this lane's weight in it
            int ks = -1;
            double base = 0.0, wsel = 0.0;
#pragma unroll
            for (int k = 0; k < NC; ++k) {
                const bool hit = ks < 0 && cum[k] > target;
                if (hit) {
                    ks = k;
                    base = k ? cum[k - 1] : 0.0;
                    wsel = w[k];
                }
            }
            // ... then the state within the chunk, in index order
            int pick = -1, lastg = -1;
            double acc = base;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const double wg = __shfl(wsel, 16 * gg + j, 64);
                acc += wg;
                if (wg > 0.0) {
                    lastg = gg;
                    if (pick < 0 && acc > target) pick = gg;
                }
            }
            if (pick < 0) pick = lastg;        // (the chunk's sum was rounded another way)
            int state = ks >= 0 ? 4 * ks + pick : last;    // rounding left no chunk: the last state
            if (root) {
                if (!(total > 0.0 && total < INFINITY)) {
                    state = NO_STATE;
                    flags |= RT_SITE_ZERO_PROB;
                }
            } else if (dead) {
                state = NO_STATE;
            } else if (state < 0) {
                state = NO_STATE;
                flags |= 2;
            }
            if (g == 0) tab[((size_t)v * DB + d) * 16 + j] = (unsigned char)state;
        }
        wave_lds_order();
    }
    // the block's draws: [draw][site][node], the 16 sites of the tile contiguous per draw
    const long s0 = blk * 16;
    const long live = nsites - s0 < 16 ? nsites - s0 : 16;
    const long count = live * nnodes;
    for (int d = 0; d < nd; ++d) {
        unsigned char *out = states + ((size_t)(d0 + d) * nsites + s0) * nnodes;
        for (long idx = lane; idx < count; idx += 64) {
            const long jj = idx / nnodes;
            const long vv = idx - jj * nnodes;
            out[idx] = tab[((size_t)vv * DB + d) * 16 + jj];
        }
    }
    if (flags && g == 0 && site_ok) atomicOr(&status[site], flags);
}

// n <= 4, upward: one lane per site, L in [node][state][site]; nodes in preorder (lane_up of
// post_common.h: the upward part of post_lane_kernel without M)
template <int N>
__global__ void __launch_bounds__(256)
sample_lane_up_kernel(int nnodes, long nsites, const double *__restrict__ P,
                      const int *__restrict__ parent, const int *__restrict__ node_k,
                      const void *__restrict__ obs, int compact, int K, int block_sites,
                      double *__restrict__ Larr)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    lane_up<N, false>(nnodes, nsites, site, P, parent, node_k, obs, compact, K, block_sites, Larr, nullptr);
}

// n <= 4, downward: one thread per (site, draw); the thread reads the parent's state back from
// its own earlier stores
template <int N>
__global__ void __launch_bounds__(256)
sample_lane_down_kernel(int nnodes, long nsites, const double *__restrict__ P,
                        const int *__restrict__ parent, const double *__restrict__ Larr,
                        const double *__restrict__ root_w, unsigned long long seed,
                        unsigned long long first_draw, long ndraws, unsigned char *states,
                        int *__restrict__ status)
{
    const long t = (long)blockIdx.x * 256 + threadIdx.x;
    if (t >= nsites * ndraws) return;
    const long d = t / nsites;
    const long site = t - d * nsites;
    unsigned char *out = states + ((size_t)d * nsites + site) * nnodes;
    int flags = 0;
    for (int v = 0; v < nnodes; ++v) {
        double w[N];
        bool dead = false;
        if (v == 0) {
#pragma unroll
            for (int s = 0; s < N; ++s)
                w[s] = (root_w ? root_w[s] : 1.0) * Larr[((size_t)v * N + s) * nsites + site];
        } else {
            int a = out[parent[v]];
            dead = a == NO_STATE;
            if (dead) a = 0;
            const double *prow = P + ((size_t)v * N + a) * N;
#pragma unroll
            for (int s = 0; s < N; ++s) w[s] = prow[s] * Larr[((size_t)v * N + s) * nsites + site];
        }
        double total = 0.0;
#pragma unroll
        for (int s = 0; s < N; ++s) {
            w[s] = w[s] > 0.0 ? w[s] : 0.0;
            total += w[s];
        }
        const double u = philox_uniform(seed, first_draw + (unsigned long long)d,
                                        (unsigned long long)site * (unsigned long long)nnodes +
                                            (unsigned long long)v);
        const double target = u * total;
        int pick = -1, last = -1;
        double acc = 0.0;
#pragma unroll
        for (int s = 0; s < N; ++s) {
            acc += w[s];
            if (w[s] > 0.0) {
                last = s;
                if (pick < 0 && acc > target) pick = s;
            }
        }
        int state = pick >= 0 ? pick : last;
        if (v == 0) {
            if (!(total > 0.0 && total < INFINITY)) {
                state = NO_STATE;
                flags |= RT_SITE_ZERO_PROB;
            }
        } else if (dead) {
            state = NO_STATE;
        } else if (state < 0) {
            state = NO_STATE;
            flags |= 2;
        }
        out[v] = (unsigned char)state;
    }
    if (flags) atomicOr(&status[site], flags);
}

}  // namespace

extern "C" int rt_sample_states_draw_block(int64_t nnodes)
{
    if (nnodes < 1 || nnodes > RT_MAX_SAMPLE_NODES) return 0;
    const int64_t db = (int64_t)(SAMPLE_LDS_TARGET / 16) / nnodes;
    return (int)std::min<int64_t>(SAMPLE_MAX_DB, std::max<int64_t>(1, db));
}

// the checks and the scratch of the draws (post_common.h)
int rt_sample_states_plan(post_pass *p, int64_t ndraws, size_t *o_states)
{
    RT_TRY(post_layout(p, false));
    if (!p->lane && p->N > RT_MAX_SAMPLE_NODES) {
        rt_set_error("%s: trees of at most %d nodes (the sampled states of a "
                     "wave live in LDS; %lld nodes here)", p->who, RT_MAX_SAMPLE_NODES, (long long)p->N);
        return RT_ERR_UNSUPPORTED;
    }
    *o_states = p->plan.take((size_t)ndraws * p->nsites * p->N);
    return RT_OK;
}

// the upward pass and the draws on the context's stream, after post_begin: states
// [ndraws][nsites][nnodes] at d_states, status (OR-ed over the draws) at p->d_status
int rt_sample_states_enqueue(post_pass *p, uint64_t seed, uint64_t first_draw, int64_t ndraws,
                             unsigned char *d_states)
{
    const rt_model *m = p->m;
    const rt_sites *s = p->s, *x = p->x;
    const int64_t n = p->n, N = p->N, nsites = p->nsites;
    hipStream_t st = p->st;
    const double *d_L = p->d_L;
    int *d_status = p->d_status;
    // the table of the downward pass: the parent NODE in its last column
    RT_TRY(post_up(p, m->parent.data(), false));
    if (p->lane) {
        const int *d_tab = p->d_ptab;
        const unsigned grid_up = (unsigned)((nsites + 255) / 256);
        const int64_t threads = nsites * ndraws;
        RT_REQUIRE((threads + 255) / 256 < (int64_t)1 << 31, "too many draws for one call");
        const unsigned grid_down = (unsigned)((threads + 255) / 256);
        RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            hipLaunchKernelGGL((sample_lane_up_kernel<NV>), dim3(grid_up), dim3(256), 0, st, (int)N,
                               (long)nsites, (const double *)m->d_P, d_tab, d_tab + N,
                               (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                               s->block_sites, p->d_L);
            hipLaunchKernelGGL((sample_lane_down_kernel<NV>), dim3(grid_down), dim3(256), 0, st,
                               (int)N, (long)nsites, (const double *)m->d_P, d_tab, d_L,
                               (const double *)m->d_root, (unsigned long long)seed,
                               (unsigned long long)first_draw, (long)ndraws, d_states, d_status);
            return RT_OK;
        }));
    } else {
        // (a call of fewer draws than the tree's block keeps its table, and so its LDS, that small:
        // which draws share a block has no bearing on a draw)
        const int DB = (int)std::min<int64_t>(rt_sample_states_draw_block(N), ndraws);
        const size_t lds = (size_t)N * DB * 16;
        const int64_t dblocks = (ndraws + DB - 1) / DB;
        RT_REQUIRE(dblocks * x->nblocks < (int64_t)1 << 31, "too many draws for one call");
        const unsigned grid = (unsigned)(dblocks * x->nblocks);
        RT_TRY(post_dispatch<1, 8>(p->NT, [&](auto nt) {
            auto kern = sample_down_kernel<decltype(nt)::value>;
            if (lds > 64 * 1024)
                RT_HIP(hipFuncSetAttribute((const void *)kern,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, st, (const double *)m->d_P, p->nops,
                               (const int4 *)p->d_steps, d_L, (const double *)x->d_obs, (int)x->nobs,
                               (const double *)m->d_root, (int)n, (int)N, DB, (unsigned long long)seed,
                               (unsigned long long)first_draw, (long)ndraws, d_states, d_status,
                               (long)nsites, (long)x->nblocks);
            return RT_OK;
        }));
    }
    RT_HIP(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_sites_sample_states(rt_model *m, rt_sites *s, int recompute_transitions,
                                      uint64_t seed, uint64_t first_draw, int64_t ndraws,
                                      uint8_t *states, int32_t *status)
{
    post_pass p;                                 // (alive until the synchronisation below)
    RT_TRY(post_open(&p, "rt_sites_sample_states", m, s));
    RT_REQUIRE(ndraws >= 1, "ndraws must be at least 1");
    RT_REQUIRE(states, "states is null");
    size_t o_states = 0;
    RT_TRY(rt_sample_states_plan(&p, ndraws, &o_states));
    RT_TRY(post_begin(&p, recompute_transitions, true));
    unsigned char *d_states = p.base + o_states;
    RT_TRY(rt_sample_states_enqueue(&p, seed, first_draw, ndraws, d_states));
    // only the draws and the status cross PCIe
    const size_t nsites = (size_t)p.nsites;
    RT_HIP(hipMemcpyAsync(states, d_states, (size_t)ndraws * nsites * p.N, hipMemcpyDeviceToHost, p.st));
    if (status) RT_HIP(hipMemcpyAsync(status, p.d_status, nsites * 4, hipMemcpyDeviceToHost, p.st));
    RT_HIP(hipStreamSynchronize(p.st));
    return RT_OK;
}
