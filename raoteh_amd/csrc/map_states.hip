// The joint maximum-likelihood reconstruction of a RESIDENT batch (rt_sites_map_states): the one
// assignment of a state to every node of a site that maximises
//   J(x) = w[x_root] prod_v o_v[x_v] prod_{v != root} P_v[x_parent(v), x_v]
// (Pupko, Pe'er, Shamir, Graur 2000), with its log-probability.
//
// Upward, max-times instead of sum-times: L_v(b) = o_v(b) prod_{c child of v} M_c(b),
// M_c(a) = max_b P_c(a, b) L_c(b).  A maximum is no matrix product, so none of the MFMA upward
// passes serves: the pass is vector-ALU code of its own.  Downward, in preorder: the root takes the
// lowest a that maximises w(a) L_root(a), every other node the lowest b that maximises
// P_v(x_parent, b) L_v(b) -- recomputed from the stored L_v for the one parent state chosen, the
// same products the upward pass compared, so no back-pointers are kept.
//
// Scaling: every L_v is multiplied per site by the power of two that brings its largest entry into
// [0.5, 1) (frexp); the exponents are summed per site and log_joint = log(root maximum) + E ln 2.
// A power of two changes no product's mantissa and so no comparison; what deviates from arithmetic
// with an unbounded exponent is only an entry (or a product of the children's messages) more than
// about 2^1000 below the largest of its node, which may flush to zero.
//
//   n > 4   map_up_kernel: one workgroup of NT row-tile waves per 16-site tile walks the schedule of
//           the split-M twin (post_step_table).  Wave m, lane l owns rows 16 m + 4 r + (l >> 4) of
//           site l & 15 -- of M_v and of the parent's L alike, so the parent's accumulator lives in
//           the L scratch [step][tile][NT][4][64] (down_at) and only its owner touches it.  L_v over
//           all b is what the lanes share: staged in LDS between two barriers, with each wave's
//           maximum for the scale.  P_v is read row-major from the model's table (every tile reads
//           the same matrices: they stay in L2).  map_down_kernel: one wave per tile, the steps in
//           reverse, the arg-max over a lane's rows and then over the four lane groups by shuffles
//           (value first, then index: the lowest index wins an exact tie); the states of the tile
//           live in LDS as [node][16] bytes and leave in one coalesced store.
//   n <= 4  map_lane_up_kernel (one lane per site, L in [node][state][site] scratch), then
//           map_lane_down_kernel: one thread per site reads its own parent state back.
//
// A site's result depends on nothing but the site: no sums across lanes of other sites, the same
// order of operations in every launch shape.  Nothing of the batch is written.
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr unsigned char NO_STATE = 255;
constexpr int MAP_FIRST = 1 << 30;             // steps[i].w: the first child to reach its parent
constexpr int MAP_LEAF = 1 << 29;              //             a leaf (no accumulator of its own)
constexpr int MAP_NODE = MAP_LEAF - 1;         //             the parent NODE below the flags
constexpr int NO_INDEX = 0x7fffffff;

__device__ __forceinline__ void wave_lds_order()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

// the power of two that brings mx into [0.5, 1), and its exponent; 1 and 0 where mx is not
// positive and finite (such a vector stays as it is)
__device__ __forceinline__ double map_scale(double mx, int *e)
{
    *e = 0;
    if (!(mx > 0.0 && mx < INFINITY)) return 1.0;
    (void)frexp(mx, e);
    // (2^-e in two exact steps: e runs from -1073 to 1024, one ldexp of 1 would leave the range)
    const int h = *e / 2;
    return ldexp(1.0, -h) * ldexp(1.0, -(*e - h));
}

// x * sc for sc = map_scale(..): two exact factors where one would overflow or be subnormal
__device__ __forceinline__ double map_apply(double x, int e)
{
    const int h = e / 2;
    return x * ldexp(1.0, -h) * ldexp(1.0, -(e - h));
}

// own rows of the observation at stream position k: the pairs q = 2 m, 2 m + 1 of og hold rows
// 16 m + 4 r + (lane >> 4) (down_L of post_common.h with KP at run time)
__device__ __forceinline__ void map_obs(const double *og, int k, int KP, int m, double (&x)[4])
{
#pragma unroll
    for (int h = 0; h < 2; ++h) {
        const int q = 2 * m + h;
        double2 v = {0.0, 0.0};
        if (q < KP) v = *(const double2 *)(og + ((size_t)k * KP + q) * 128);
        x[2 * h] = v.x;
        x[2 * h + 1] = v.y;
    }
}

// steps[i] = {node, step of the parent, stream position of the node's observation or -1,
// parent node | MAP_FIRST | MAP_LEAF}; the root is the last step
template <int NT>
__global__ void __launch_bounds__(64 * NT)
map_up_kernel(const double *__restrict__ P, int nops, const int4 *__restrict__ steps,
              double *__restrict__ Larr, const double *__restrict__ obs, int K, int n,
              int *__restrict__ esum, long nsites, long nblocks)
{
    __shared__ double xb[NT * 16 * 16];        // L_v [state][site] of the step
    __shared__ double part[NT][16];            // each wave's largest entry per site
    const int m = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int g = lane >> 4, j = lane & 15;
    const long blk = blockIdx.x;
    const int KP = ((n + 3) / 4 + 1) / 2;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    bool rok[4];
    size_t prow[4];                            // own rows of a P_v (row 0 for the padding rows)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        const int row = 16 * m + 4 * r + g;
        rok[r] = row < n;
        prow[r] = rok[r] ? (size_t)row * n : 0;
    }
    int E = 0;
    for (int i = 0; i < nops; ++i) {
        const int4 st = steps[i];
        const bool leaf = (st.w & MAP_LEAF) != 0;      // (uniform, as every branch on the schedule)
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        // own rows of L_v: the children's messages (or ones) times the observation
        double L[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) L[r] = leaf ? 1.0 : Larr[o + r * 64];
        if (st.z >= 0) {
            double x[4];
            map_obs(og, st.z, KP, m, x);
#pragma unroll
            for (int r = 0; r < 4; ++r) L[r] *= fmax(x[r], 0.0);
        }
        double mx = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            L[r] = rok[r] ? fmax(L[r], 0.0) : 0.0;     // negative (and NaN) counts as 0
            mx = fmax(mx, L[r]);
        }
        mx = fmax(mx, __shfl_xor(mx, 16, 64));
        mx = fmax(mx, __shfl_xor(mx, 32, 64));
        __syncthreads();                       // every wave is done with the previous step's L
#pragma unroll
        for (int r = 0; r < 4; ++r) xb[(16 * m + 4 * r + g) * 16 + j] = L[r];
        if (lane < 16) part[m][j] = mx;
        __syncthreads();
        mx = 0.0;
#pragma unroll
        for (int mm = 0; mm < NT; ++mm) mx = fmax(mx, part[mm][j]);
        int e;
        (void)map_scale(mx, &e);
        E += e;
        if (!leaf)
#pragma unroll
            for (int r = 0; r < 4; ++r) Larr[o + r * 64] = map_apply(L[r], e);
        if (i == nops - 1) break;              // the root sends no message
        // own rows of M_v = max_b P_v(a, b) L_v(b), scaled, into the parent's accumulator
        const double *Pv = P + (size_t)st.x * n * n;
        double M[4] = {0.0, 0.0, 0.0, 0.0};
#pragma unroll 4
        for (int b = 0; b < n; ++b) {
            const double l = xb[b * 16 + j];
#pragma unroll
            for (int r = 0; r < 4; ++r) M[r] = fmax(M[r], Pv[prow[r] + b] * l);
        }
        const size_t po = down_at<NT>(st.y, nblocks, blk, m, lane);
        const bool first = (st.w & MAP_FIRST) != 0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const double t = rok[r] ? map_apply(M[r], e) : 0.0;
            Larr[po + r * 64] = first ? t : Larr[po + r * 64] * t;
        }
    }
    const long site = blk * 16 + j;
    if (m == 0 && g == 0 && site < nsites) esum[site] = E;
}

// one wave per tile, the steps in reverse (sample_down_kernel of sample.hip with the arg-max in
// place of the scan to a uniform, one "draw")
template <int NT>
__global__ void __launch_bounds__(64)
map_down_kernel(const double *__restrict__ P, int nops, const int4 *__restrict__ steps,
                const double *__restrict__ Larr, const double *__restrict__ obs, int K,
                const double *__restrict__ root_w, int n, int nnodes, const int *__restrict__ esum,
                unsigned char *__restrict__ states, double *__restrict__ log_joint,
                int *__restrict__ status, long nsites, long nblocks)
{
    constexpr int NC = 4 * NT;                 // rows of one lane: 4 k + g
    extern __shared__ unsigned char tab[];     // [node][16] states of this tile
    const int lane = threadIdx.x;
    const int g = lane >> 4, j = lane & 15;
    const long blk = blockIdx.x;
    const long site = blk * 16 + j;
    const bool site_ok = site < nsites;
    const int KP = ((n + 3) / 4 + 1) / 2;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    int flags = 0;
    for (int i = nops - 1; i >= 0; --i) {
        const int4 st = steps[i];
        const int v = st.x, p = st.w & MAP_NODE;
        const bool leaf = (st.w & MAP_LEAF) != 0;
        const bool root = i == nops - 1;
        // own rows of L_v: what the upward pass stored; a leaf's observation, or ones
        double L[NC];
        if (!leaf) {
            const double *lp = Larr + ((size_t)i * nblocks + blk) * (NT * 256) + lane;
#pragma unroll
            for (int k = 0; k < NC; ++k) L[k] = lp[k * 64];
        } else if (st.z >= 0) {
#pragma unroll
            for (int q = 0; q < 2 * NT; ++q) {
                double2 x = {0.0, 0.0};
                if (q < KP) x = *(const double2 *)(og + ((size_t)st.z * KP + q) * 128);
                L[2 * q] = x.x;
                L[2 * q + 1] = x.y;
            }
        } else {
#pragma unroll
            for (int k = 0; k < NC; ++k) L[k] = 1.0;
        }
        int a = 0;
        bool dead = false;
        if (!root) {
            a = tab[(size_t)p * 16 + j];
            dead = a == NO_STATE;
            if (dead) a = 0;
        }
        const double *prow = P + ((size_t)v * n + a) * n;
        // the largest product of the own rows, the lowest row first: only a larger one replaces it
        double bv = 0.0;
        int bi = NO_INDEX;
#pragma unroll
        for (int k = 0; k < NC; ++k) {
            const int row = 4 * k + g;
            double x = 0.0;
            if (row < n) {
                const double l = fmax(L[k], 0.0);
                x = root ? fmax(root_w ? root_w[row] : 1.0, 0.0) * l : prow[row] * l;
            }
            if (x > bv) {                      // (false for NaN)
                bv = x;
                bi = row;
            }
        }
        // ... then over the four lane groups: the value first, then the index
#pragma unroll
        for (int sh = 16; sh <= 32; sh *= 2) {
            const double ov = __shfl_xor(bv, sh, 64);
            const int oi = __shfl_xor(bi, sh, 64);
            if (ov > bv || (ov == bv && oi < bi)) {
                bv = ov;
                bi = oi;
            }
        }
        int state = bi == NO_INDEX ? (int)NO_STATE : bi;
        if (root) {
            const bool ok = bv > 0.0 && bv < INFINITY;
            if (!ok) {
                state = NO_STATE;
                flags |= RT_SITE_ZERO_PROB;
            }
            if (g == 0 && site_ok && log_joint)
                log_joint[site] = ok ? log(bv) + (double)esum[site] * 0.6931471805599453094 : -INFINITY;
        } else if (dead) {
            state = NO_STATE;
        } else if (state == NO_STATE) {
            flags |= 2;                        // (a live parent state without a child state)
        }
        if (g == 0) tab[(size_t)v * 16 + j] = (unsigned char)state;
        wave_lds_order();
    }
    // [site][node], the 16 sites of the tile contiguous
    const long s0 = blk * 16;
    const long live = nsites - s0 < 16 ? nsites - s0 : 16;
    const long count = live * nnodes;
    unsigned char *out = states + (size_t)s0 * nnodes;
    for (long idx = lane; idx < count; idx += 64) {
        const long jj = idx / nnodes;
        const long vv = idx - jj * nnodes;
        out[idx] = tab[(size_t)vv * 16 + jj];
    }
    if (flags && g == 0 && site_ok) atomicOr(&status[site], flags);
}

// n <= 4, upward: one lane per site, L in [node][state][site], nodes in preorder (lane_up of
// post_common.h with max-times and the scale)
template <int N>
__global__ void __launch_bounds__(256)
map_lane_up_kernel(int nnodes, long nsites, const double *__restrict__ P,
                   const int *__restrict__ parent, const int *__restrict__ node_k,
                   const void *__restrict__ obs, int compact, int K, int block_sites,
                   double *__restrict__ Larr, int *__restrict__ esum)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    for (int v = 0; v < nnodes; ++v) {
        double x[N];
        const int k = node_k[v];
        if (k >= 0) lane_obs<N>(obs, compact, K, block_sites, site, k, x);
        else
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] = 1.0;
#pragma unroll
        for (int s = 0; s < N; ++s) Larr[idx(v, s)] = fmax(x[s], 0.0);
    }
    int E = 0;
    for (int v = nnodes - 1; v >= 0; --v) {
        double x[N], mx = 0.0;
#pragma unroll
        for (int s = 0; s < N; ++s) {
            x[s] = fmax(Larr[idx(v, s)], 0.0);
            mx = fmax(mx, x[s]);
        }
        int e;
        (void)map_scale(mx, &e);
        E += e;
#pragma unroll
        for (int s = 0; s < N; ++s) {
            x[s] = map_apply(x[s], e);
            Larr[idx(v, s)] = x[s];
        }
        if (v == 0) break;
        const double *Pv = P + (size_t)v * N * N;
        const int p = parent[v];
#pragma unroll
        for (int a = 0; a < N; ++a) {
            double t = 0.0;
#pragma unroll
            for (int b = 0; b < N; ++b) t = fmax(t, Pv[a * N + b] * x[b]);
            Larr[idx(p, a)] *= t;
        }
    }
    esum[site] = E;
}

// n <= 4, downward: one thread per site; it reads the parent's state back from its own stores
template <int N>
__global__ void __launch_bounds__(256)
map_lane_down_kernel(int nnodes, long nsites, const double *__restrict__ P,
                     const int *__restrict__ parent, const double *__restrict__ Larr,
                     const double *__restrict__ root_w, const int *__restrict__ esum,
                     unsigned char *states, double *__restrict__ log_joint,
                     int *__restrict__ status)
{
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    unsigned char *out = states + (size_t)site * nnodes;
    int flags = 0;
    for (int v = 0; v < nnodes; ++v) {
        bool dead = false;
        int a = 0;
        if (v) {
            a = out[parent[v]];
            dead = a == NO_STATE;
            if (dead) a = 0;
        }
        const double *prow = P + ((size_t)v * N + a) * N;
        double bv = 0.0;
        int state = NO_STATE;
#pragma unroll
        for (int s = 0; s < N; ++s) {
            const double l = Larr[((size_t)v * N + s) * nsites + site];
            const double x = v ? prow[s] * l : fmax(root_w ? root_w[s] : 1.0, 0.0) * l;
            if (x > bv) {
                bv = x;
                state = s;
            }
        }
        if (v == 0) {
            const bool ok = bv > 0.0 && bv < INFINITY;
            if (!ok) {
                state = NO_STATE;
                flags |= RT_SITE_ZERO_PROB;
            }
            if (log_joint)
                log_joint[site] = ok ? log(bv) + (double)esum[site] * 0.6931471805599453094 : -INFINITY;
        } else if (dead) {
            state = NO_STATE;
        } else if (state == NO_STATE) {
            flags |= 2;
        }
        out[v] = (unsigned char)state;
    }
    if (flags) atomicOr(&status[site], flags);
}

}  // namespace

extern "C" int rt_sites_map_states(rt_model *m, rt_sites *s, int recompute_transitions,
                                   uint8_t *states, double *log_joint, int32_t *status)
{
    post_pass p;                                 // (alive until the synchronisation below)
    RT_TRY(post_open(&p, "rt_sites_map_states", m, s));
    RT_REQUIRE(states, "states is null");
    // L alone: the max-times pass writes no M (nothing here runs the MFMA store kernel)
    RT_TRY(post_layout(&p, false, false));
    if (!p.lane && p.N > RT_MAX_SAMPLE_NODES) {
        rt_set_error("%s: trees of at most %d nodes (the states of a tile live in LDS; %lld nodes "
                     "here)", p.who, RT_MAX_SAMPLE_NODES, (long long)p.N);
        return RT_ERR_UNSUPPORTED;
    }
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    const size_t o_esum = p.plan.take((size_t)nsites * 4);
    const size_t o_states = p.plan.take((size_t)nsites * N);
    const size_t o_joint = p.plan.take((size_t)nsites * 8);
    RT_TRY(post_begin(&p, recompute_transitions));
    int *d_esum = (int *)(p.base + o_esum);
    unsigned char *d_states = p.base + o_states;
    double *d_joint = (double *)(p.base + o_joint);
    hipStream_t st = p.st;
    if (p.lane) {
        RT_TRY(post_up(&p, m->parent.data(), false));         // (the lane table, nothing launched)
        const int *d_tab = p.d_ptab;
        const unsigned grid = (unsigned)((nsites + 255) / 256);
        RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
            constexpr int NV = decltype(nv)::value;
            hipLaunchKernelGGL((map_lane_up_kernel<NV>), dim3(grid), dim3(256), 0, st, (int)N,
                               (long)nsites, (const double *)m->d_P, d_tab, d_tab + N,
                               (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                               s->block_sites, p.d_L, d_esum);
            hipLaunchKernelGGL((map_lane_down_kernel<NV>), dim3(grid), dim3(256), 0, st, (int)N,
                               (long)nsites, (const double *)m->d_P, d_tab, (const double *)p.d_L,
                               (const double *)m->d_root, (const int *)d_esum, d_states, d_joint,
                               p.d_status);
            return RT_OK;
        }));
    } else {
        const rt_sites *x = p.x;
        RT_TRY(post_step_table(m, x, m->parent.data(), &p.table, &p.step_node));
        RT_REQUIRE(x->nblocks == s->nblocks, "%s: the twin's tiles do not match the batch's", p.who);
        // every observation (an internal node's too: this pass multiplies it in itself), and who
        // starts its parent's accumulator: the first step of each parent in schedule order
        std::vector<char> begun((size_t)p.nops, 0);
        for (int i = 0; i < p.nops; ++i) {
            const rt_op &op = x->ops[(size_t)i];
            int32_t *row = &p.table[(size_t)i * 4];
            row[2] = op.obs >= 0 ? op.obs : -1;
            if (i + 1 == p.nops) row[3] = 0;     // (the root has no parent)
            else if (!begun[(size_t)row[1]]) {
                begun[(size_t)row[1]] = 1;
                row[3] |= MAP_FIRST;
            }
            if (op.pop < 0) row[3] |= MAP_LEAF;
        }
        RT_REQUIRE(!(p.table[(size_t)(p.nops - 1) * 4 + 3] & MAP_LEAF), "unexpected schedule");
        RT_HIP(hipMemcpyAsync(p.d_steps, p.table.data(), p.table.size() * 4, hipMemcpyHostToDevice, st));
        const size_t lds = (size_t)N * 16;
        const unsigned grid = (unsigned)x->nblocks;
        RT_TRY(post_dispatch<1, 8>(p.NT, [&](auto nt) {
            constexpr int NTV = decltype(nt)::value;
            hipLaunchKernelGGL((map_up_kernel<NTV>), dim3(grid), dim3(64 * NTV), 0, st,
                               (const double *)m->d_P, p.nops, (const int4 *)p.d_steps, p.d_L,
                               (const double *)x->d_obs, (int)x->nobs, (int)n, d_esum, (long)nsites,
                               (long)x->nblocks);
            auto kern = map_down_kernel<NTV>;
            if (lds > 64 * 1024)
                RT_HIP(hipFuncSetAttribute((const void *)kern,
                                           hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(kern, dim3(grid), dim3(64), lds, st, (const double *)m->d_P, p.nops,
                               (const int4 *)p.d_steps, (const double *)p.d_L,
                               (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root,
                               (int)n, (int)N, (const int *)d_esum, d_states, d_joint, p.d_status,
                               (long)nsites, (long)x->nblocks);
            return RT_OK;
        }));
    }
    RT_HIP(hipGetLastError());
    // only the states, the log-probabilities and the status cross PCIe
    RT_HIP(hipMemcpyAsync(states, d_states, (size_t)nsites * N, hipMemcpyDeviceToHost, st));
    if (log_joint)
        RT_HIP(hipMemcpyAsync(log_joint, d_joint, (size_t)nsites * 8, hipMemcpyDeviceToHost, st));
    if (status) RT_HIP(hipMemcpyAsync(status, p.d_status, (size_t)nsites * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return RT_OK;
}
