// Query sequences placed on every branch of the model's tree on a RESIDENT batch
// (rt_sites_placements): for every site i, query q, non-root node v, fraction rho_r and pendant
// length tau_k,
//     log L_i(tree with q placed at (v, rho_r, tau_k)) - log L_i,
// the placement being a new node x that cuts the edge p -> v (p -> x of length rho t_v, x -> v of
// length (1 - rho) t_v) with a new leaf below x on an edge of length tau that carries the query's
// observation o_q; all three edges under the rate matrix Q_v of the cut edge.
//
// With L_w, M_w = P_w L_w of the stored upward pass and up_p the message into p = parent(v) from
// above, normalised once at the root by 1 / L_i (the division-free `up` pass of nni.hip):
//     A_v[a]       = up_p[a] obs_p[a] prod_{w child of p, w != v} M_w[a]
//     F_{v,r}[b]   = (P_v(rho_r t_v)^T A_v)[b] (P_v((1 - rho_r) t_v) L_v)[b]     the field
//     h_{d,k,q}[b] = sum_c expm(Q_d tau_k)[b][c] o_q[c]                        d = qidx(v)
//     ratio        = sum_b F_{v,r}[b] h_{d,k,q}[b]
// The field holds no query and the pendant vectors no edge: h is made once per DISTINCT rate
// matrix in use, never once per edge.  Here:
//
//   1. P_v(rho_r t_v), P_v((1 - rho_r) t_v) and expm(Q_v tau_k) of every node in ONE launch of
//      the model's own exponential (post_grid: 2 R + K points per node);
//   2. n > 4: the upward pass with L and M of every step stored; place_field_kernel, one
//      workgroup of NT row-tile waves per 16-site tile: the `up` pass, then per edge A_v and L_v
//      staged and per fraction two matrix-pipe products, F to the scratch as [edge][fraction];
//      per chunk of queries place_query_kernel (h per distinct matrix, pendant length and query:
//      a matrix-pipe product for dense queries, a column or the row sums of the matrix for state
//      queries) and place_score_kernel (PLACE_BLOCK vectors h in registers per walk of the
//      field, the dot products on the vector ALU, the states summed in the fixed order of
//      down_part / down_total, the logs by all lanes at the end);
//      n <= 4: place_lane_kernel, one lane per site, the same three stages;
//   3. post_result (post_common.h): the site-weighted sums per (query, node, fraction, pendant
//      length) in a fixed order; then, if the per-site array is asked for, its transpose.
//
// The field is made once; the queries go through 2 and 3 in chunks where the result of all of
// them would not fit the scratch (post_chunk_units).  The fraction grid (its checks, its lengths,
// its fragment tables) is post_fraction_*, shared with spr.hip.  Nothing of the batch or the model
// is written; two calls give the same bits, chunked or not.
//
// rt_sites_placements_mixture: the same placements of an ORDINARY batch under a site-class mixture
// over the model's K rate sets -- the cut edge at fractions of every set's own resident length, the
// pendant edge at pendant_scale[k] tau under the set's rate matrix; the kernels' MIX forms once per
// set and chunk of queries into one accumulator, the root scaled by the class weight instead of
// 1 / L_i; the field holds one set at a time.
// rt_sites_placements_partitioned: the same placements of a PARTITIONED batch, every site under its
// own rate set, the queries in the caller's site order -- the kernels' PART forms, every tile under
// the tables of its granule's set, one field and per chunk of queries one launch of each; the
// per-set sums and the gather to caller order are post_part_result's.  One host body (place_read,
// at the end) serves the three calls.
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int PLACE_BLOCK = 8;                   // (query, pendant) vectors held per walk of the field
constexpr int64_t PLACE_MAX_ROWS = (int64_t)1 << 21;     // rows of one transpose launch (grid y)

// the stored value: 0 at a site of zero likelihood, else the log of the ratio (-inf where it is
// not positive)
__device__ __forceinline__ double place_value(double ratio, bool zero)
{
    if (zero) return 0.0;
    return ratio > 0.0 ? log(ratio) : -__builtin_inf();
}

// What the MIX kernel instances (rt_sites_placements_mixture: one launch per rate set k of weight
// ck > 0 and chunk of queries, in set order on one stream) take beside the plain ones' arguments:
// the class weight the root is scaled by instead of 1 / L_ik, where L_ik goes (post_mix::tot_of),
// and whether the set is the first to run (it stores its terms, the later ones add to them).  It is
// an argument of the MIX instances ALONE (a parameter pack that is empty otherwise): the plain
// instances keep their argument lists and with them the parent's instruction streams.
struct place_mix {
    double ck;
    double *root_tot;
    int first;
};
struct place_plain {};
__device__ __forceinline__ place_plain place_args() { return {}; }
__device__ __forceinline__ place_mix place_args(place_mix a) { return a; }
// (a PART instance's pack holds the post_part_arg instead: post_common.h)
__device__ __forceinline__ post_part_arg place_args(post_part_arg a) { return a; }

// n > 4.  steps as in nni_kernel (steps[i].w: the node has children); PfragT: [step] A fragments
// of the resident P^T; GfragT: [fraction][step] those of P(rho t)^T; GfragA: [fraction][step]
// those of P((1 - rho) t) itself; Uarr: the `up` vectors; Farr: the field,
// [step * R + fraction] in the layout of L and M.
// MIX: the set's fragments; down_up_pass's MIX form (the root scaled by ck, L_ik to root_tot, the
// status word the set's own), so the field is c_k times the unnormalised one.
// PART (rt_sites_placements_partitioned: sites are the batch's slots): the plain field, the tile
// under the tables of its granule's set -- PfragT [set][step], GfragT / GfragA [set][fraction][step]
// moved on by set * (s_p, s_g) doubles before anything else.
template <int NT, int KS, bool MIX = false, bool PART = false, class... MX>
__global__ void __launch_bounds__(64 * NT)
place_field_kernel(const double *__restrict__ PfragT, const double *__restrict__ GfragT,
                   const double *__restrict__ GfragA, int R, int nops,
                   const int4 *__restrict__ steps, const int *__restrict__ tabp,
                   const double *__restrict__ Larr, const double *__restrict__ Marr,
                   double *__restrict__ Uarr, const double *__restrict__ obs, int K,
                   const double *__restrict__ root_w, int n, double *__restrict__ Farr,
                   int *__restrict__ status, long nsites, long nblocks, MX... mix)
{
    static_assert(sizeof...(MX) == (MIX || PART ? 1 : 0) && !(MIX && PART),
                  "place_mix: the MIX instance's alone; post_part_arg: the PART instance's");
    [[maybe_unused]] const auto mx = place_args(mix...);
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double lb[NT * 4 * 64];
    __shared__ double red[NT][16];
    const post_tab tab(tabp, nops);
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    if constexpr (PART) {
        const long gs = post_part_set(mx, blk);
        PfragT += gs * mx.s_p;
        GfragT += gs * mx.s_g;
        GfragA += gs * mx.s_g;
    }
    const long site = blk * 16 + (lane & 15);
    const bool writer = m == 0 && lane < 16 && site < nsites;
    bool live[4];                                // own rows that are states
#pragma unroll
    for (int r = 0; r < 4; ++r) live[r] = 16 * m + 4 * r + (lane >> 4) < n;
    const size_t frag = ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    // 1. the `up` pass (nni_kernel's)
    if constexpr (MIX)
        down_up_pass<NT, KS, true>(true, xb, red, tab, PfragT, nops, steps, Larr, Marr, Uarr, og, root_w,
                                   live, m, lane, blk, nblocks, writer, status, site, mx.ck,
                                   mx.root_tot);
    else
        down_up_pass<NT, KS>(true, xb, red, tab, PfragT, nops, steps, Larr, Marr, Uarr, og, root_w, live,
                             m, lane, blk, nblocks, writer, status, site);
    // 2. the field of every edge: A_v and L_v staged once, two products per fraction
    double a[2 * KP];
    for (int i = nops - 2; i >= 0; --i) {
        const int4 st = steps[i];
        const int pi = st.y;
        const size_t o = down_at<NT>(i, nblocks, blk, m, lane);
        const size_t po = down_at<NT>(pi, nblocks, blk, m, lane);
        double x[4], l[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) x[r] = Uarr[po + r * 64];
        const int kp = tab.obs[pi];
        if (kp >= 0) {
            double ob[4];
            down_L<KP>(kp, og, Larr, po, m, ob);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] *= ob[r];
        }
        for (int e = tab.cptr[pi]; e < tab.cptr[pi + 1]; ++e) {
            const int w = tab.cidx[e];
            if (w == i) continue;
            const size_t wo = down_at<NT>(w, nblocks, blk, m, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] *= Marr[wo + r * 64];
        }
        down_L<KP>(st.z, og, Larr, o, m, l);
        __syncthreads();                         // (every wave is done with the previous operands)
#pragma unroll
        for (int r = 0; r < 4; ++r) {            // (rows past the states: 0)
            xb[(4 * m + r) * 64 + lane] = live[r] ? x[r] : 0.0;
            lb[(4 * m + r) * 64 + lane] = live[r] ? l[r] : 0.0;
        }
        __syncthreads();
        for (int r = 0; r < R; ++r) {
            down_frag<KP>(GfragT + ((size_t)r * nops + i) * ASTRIDE + frag, a);
            const double4_t y = down_product<KS>(a, xb, lane);
            down_frag<KP>(GfragA + ((size_t)r * nops + i) * ASTRIDE + frag, a);
            const double4_t z = down_product<KS>(a, lb, lane);
            const size_t fo = down_at<NT>(i * R + r, nblocks, blk, m, lane);
#pragma unroll
            for (int e = 0; e < 4; ++e) Farr[fo + e * 64] = y[e] * z[e];
        }
    }
}

// n > 4, one workgroup per (tile, query of the chunk).  HfragA: [pendant][distinct] A fragments of
// expm(Q_d tau_k); Gtau: the same matrices as the exponential left them, [pendant][node][n][n],
// rep[d] the node that stands for distinct matrix d.  dense: queries f64[QC][nsites][n], staged
// and multiplied on the matrix pipe; else uint8[QC][nsites]: column o of the matrix, or its row
// sums where o >= n (unobserved).  Harr: [(d * K + k) * QC + q] in the layout of L and M.
// PART (queries in slot order: place_query_gather_kernel): HfragA [set][pendant][distinct] and Gtau
// [set][point][node] of the tile's set, moved on by set * (s_p, s_g) doubles.
template <int NT, int KS, bool PART = false, class... PX>
__global__ void __launch_bounds__(64 * NT)
place_query_kernel(int dense, const void *__restrict__ queries, const double *__restrict__ HfragA,
                   const double *__restrict__ Gtau, const int *__restrict__ rep, int nd, int K,
                   int QC, int N, int n, double *__restrict__ Harr, long nsites, long nblocks,
                   PX... part)
{
    static_assert(sizeof...(PX) == (PART ? 1 : 0), "post_part_arg: the PART instance's alone");
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    if constexpr (PART) {
        const post_part_arg px = post_pack_one(part...);
        const long gs = post_part_set(px, blk);
        HfragA += gs * px.s_p;
        Gtau += gs * px.s_g;
    }
    const int q = blockIdx.y;
    const long site = blk * 16 + (lane & 15);
    const bool site_ok = site < nsites;
    const size_t frag = ((size_t)m * KP * 64 + lane) * 2;
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    if (dense) {
        const double *qv = (const double *)queries + ((size_t)q * nsites + (site_ok ? site : 0)) * n;
        double x[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + 4 * r + (lane >> 4);
            x[r] = (site_ok && row < n) ? qv[row] : 0.0;
        }
        down_stage(xb, m, lane, x);
        double a[2 * KP];
        for (int d = 0; d < nd; ++d)
            for (int k = 0; k < K; ++k) {
                down_frag<KP>(HfragA + ((size_t)k * nd + d) * ASTRIDE + frag, a);
                const double4_t y = down_product<KS>(a, xb, lane);
                const size_t ho = down_at<NT>((d * K + k) * QC + q, nblocks, blk, m, lane);
#pragma unroll
                for (int e = 0; e < 4; ++e) Harr[ho + e * 64] = y[e];
            }
    } else {
        const int o = site_ok ? ((const unsigned char *)queries)[(size_t)q * nsites + site] : 255;
        for (int d = 0; d < nd; ++d)
            for (int k = 0; k < K; ++k) {
                const double *G = Gtau + ((size_t)k * N + rep[d]) * n * n;
                const size_t ho = down_at<NT>((d * K + k) * QC + q, nblocks, blk, m, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int row = 16 * m + 4 * r + (lane >> 4);
                    double y = 0.0;
                    if (row < n) {
                        if (o < n) y = G[(size_t)row * n + o];
                        else
                            for (int c = 0; c < n; ++c) y += G[(size_t)row * n + c];
                    }
                    Harr[ho + r * 64] = y;
                }
            }
    }
}

// n > 4, one workgroup per (tile, block of PLACE_BLOCK (query, pendant) pairs of the chunk; pair
// = q * K + k).  dslot[i]: the distinct matrix of step i's node.  Per distinct matrix the block's
// vectors h are held in registers (four doubles per lane and vector) and the field of the edges
// under that matrix is walked once: the dot products of own rows, the rows summed through the
// halves of `sums` as in nni_kernel (wave 0 adds the waves in order and stores the ratio while
// the next edge fills the other half).  out: [q][node][fraction][pendant][site]; the root's rows
// are not written.  (PLACE_BLOCK = 8: 64 VGPRs of vectors; see profiles/placements_resource_usage.txt)
// MIX: the field and the pendant vectors are the set's; the dot product is the RAW term
// c_k L_ik(tree with the query placed), stored by the first running set and added to by the later
// ones (the same lane of the same workgroup, launches in order: a fixed sum); no logs here and no
// look at the status -- mix_log_ratio_kernel's once the sets are in.
template <int NT, bool MIX = false, class... MX>
__global__ void __launch_bounds__(64 * NT)
place_score_kernel(int nops, int R, int K, int QC, int nd, const int4 *__restrict__ steps,
                   const int *__restrict__ dslot, const double *__restrict__ Farr,
                   const double *__restrict__ Harr, double *__restrict__ out,
                   const int *__restrict__ status, int N, long nsites, long nblocks, MX... mix)
{
    static_assert(sizeof...(MX) == (MIX ? 1 : 0), "place_mix: the MIX instance's alone");
    [[maybe_unused]] const auto mx = place_args(mix...);
    __shared__ double sums[2][PLACE_BLOCK][NT][16];
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    const long site = blk * 16 + (lane & 15);
    const bool site_ok = site < nsites;
    const bool writer = m == 0 && lane < 16 && site_ok;
    const int pairs = QC * K;
    const int j0 = blockIdx.y * PLACE_BLOCK;
    const int cnt = min(PLACE_BLOCK, pairs - j0);
    const size_t NRK = (size_t)N * R * K;
    int par = 0;                                 // the half of `sums` the next edge writes
    for (int d = 0; d < nd; ++d) {
        double h[PLACE_BLOCK][4];
#pragma unroll
        for (int j = 0; j < PLACE_BLOCK; ++j) {
            const int pair = min(j0 + j, pairs - 1);
            const int q = pair / K, k = pair - q * K;
            const size_t ho = down_at<NT>((d * K + k) * QC + q, nblocks, blk, m, lane);
#pragma unroll
            for (int e = 0; e < 4; ++e) h[j][e] = Harr[ho + e * 64];
        }
        for (int i = nops - 2; i >= 0; --i) {
            if (dslot[i] != d) continue;
            const int v = steps[i].x;
            for (int r = 0; r < R; ++r) {
                const size_t fo = down_at<NT>(i * R + r, nblocks, blk, m, lane);
                double f[4];
#pragma unroll
                for (int e = 0; e < 4; ++e) f[e] = Farr[fo + e * 64];
#pragma unroll
                for (int j = 0; j < PLACE_BLOCK; ++j) {
                    double t = 0.0;
#pragma unroll
                    for (int e = 0; e < 4; ++e) t += f[e] * h[j][e];
                    down_part(sums[par][j], m, lane, t);
                }
                __syncthreads();
                if (writer)
                    for (int j = 0; j < cnt; ++j) {
                        const int pair = j0 + j;
                        const int q = pair / K, k = pair - q * K;
                        double *x = out + ((size_t)q * NRK + ((size_t)v * R + r) * K + k) * nsites + site;
                        const double t = down_total<NT>(sums[par][j], lane);
                        if constexpr (MIX) *x = mx.first ? t : __dadd_rn(*x, t);
                        else *x = t;
                    }
                par ^= 1;
            }
        }
    }
    if constexpr (MIX) return;
    // the block's ratios -> values, by all waves: lane group g of the workgroup takes the rows
    // g, g + 4 NT, ... of its site (the barrier: wave 0's stores are visible)
    __syncthreads();
    if (site_ok) {
        const bool zero = status[site] & RT_SITE_ZERO_PROB;
        const long per = (long)(N - 1) * R;
        for (long t = 4 * m + (lane >> 4); t < (long)cnt * per; t += 4 * NT) {
            const int j = (int)(t / per);
            const long vr = t - (long)j * per + R;         // (v * R + r, v >= 1)
            const int pair = j0 + j;
            const int q = pair / K, k = pair - q * K;
            double *x = out + ((size_t)q * NRK + (size_t)vr * K + k) * nsites + site;
            *x = place_value(*x, zero);
        }
    }
}

// n <= 4: one lane per site; arrays [node][state][site], nodes in preorder; G [point][node][N][N]:
// the points 0 .. R - 1 are P(rho t), R .. 2 R - 1 are P((1 - rho) t), 2 R .. 2 R + K - 1 are
// expm(Q tau) (the same address in every lane: the scalar path); Farr [node * R + fraction][N][site];
// dnode[v] the distinct matrix of node v, rep[d] the node that stands for it.  make: the first
// chunk makes the upward pass, the `up` pass and the field, later ones find them.
// MIX: P and G of the set, make != 0 in every launch (the scratch is the current set's); the terms
// as in place_score_kernel.  PART (sites are the batch's slots, the queries in slot order): P
// [set][node] and G [set][point][node] of the set of the wave's granule, wave-uniform.
template <int N, bool MIX = false, bool PART = false, class... MX>
__global__ void __launch_bounds__(256)
place_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const double *__restrict__ G,
                  int R, int K, const int *__restrict__ parent, const int *__restrict__ node_k,
                  const int *__restrict__ tabp, const int *__restrict__ dnode,
                  const int *__restrict__ rep, int nd, const void *__restrict__ obs, int compact,
                  int Kobs, int block_sites, const double *__restrict__ root_w,
                  double *__restrict__ Larr, double *__restrict__ Marr, double *__restrict__ Uarr,
                  double *__restrict__ Farr, int dense, const void *__restrict__ queries, int QC,
                  int make, double *__restrict__ out, int *__restrict__ status, MX... mix)
{
    static_assert(sizeof...(MX) == (MIX || PART ? 1 : 0) && !(MIX && PART),
                  "place_mix: the MIX instance's alone; post_part_arg: the PART instance's");
    [[maybe_unused]] const auto mx = place_args(mix...);
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    if constexpr (PART) {
        const long gs = post_part_set(mx, site >> mx.gshift);
        P += gs * mx.s_p;
        G += gs * mx.s_g;
    }
    const post_tab tab(tabp, nnodes);
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    if (make)
        lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, Kobs, block_sites, Larr,
                         Marr);
    [[maybe_unused]] bool zero;
    if constexpr (MIX)
        zero = lane_up_pass<N, true>(make != 0, nnodes, nsites, site, P, parent, node_k, tab, obs,
                                     compact, Kobs, block_sites, root_w, Larr, Marr, Uarr, status,
                                     mx.ck, mx.root_tot);
    else
        zero = lane_up_pass<N>(make != 0, nnodes, nsites, site, P, parent, node_k, tab, obs, compact,
                               Kobs, block_sites, root_w, Larr, Marr, Uarr, status);
    if (make)
        for (int v = 1; v < nnodes; ++v) {
            const int p = parent[v];
            double x[N], l[N];
            const int kp = node_k[p];
            if (kp >= 0) lane_obs<N>(obs, compact, Kobs, block_sites, site, kp, x);
            else
#pragma unroll
                for (int s = 0; s < N; ++s) x[s] = 1.0;
#pragma unroll
            for (int s = 0; s < N; ++s) {
                x[s] *= Uarr[idx(p, s)];
                l[s] = Larr[idx(v, s)];
            }
            for (int e = tab.cptr[p]; e < tab.cptr[p + 1]; ++e) {
                const int w = tab.cidx[e];
                if (w == v) continue;
#pragma unroll
                for (int s = 0; s < N; ++s) x[s] *= Marr[idx(w, s)];
            }
            for (int r = 0; r < R; ++r) {
                const double *G1 = G + ((size_t)r * nnodes + v) * N * N;
                const double *G2 = G + ((size_t)(R + r) * nnodes + v) * N * N;
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    double y = 0.0, z = 0.0;
#pragma unroll
                    for (int a = 0; a < N; ++a) {
                        y += G1[a * N + b] * x[a];
                        z += G2[b * N + a] * l[a];
                    }
                    Farr[idx(v * R + r, b)] = y * z;
                }
            }
        }
    const size_t NRK = (size_t)nnodes * R * K;
    for (int q = 0; q < QC; ++q) {
        double oq[N];
        if (dense) {
            const double *qv = (const double *)queries + ((size_t)q * nsites + site) * N;
#pragma unroll
            for (int s = 0; s < N; ++s) oq[s] = qv[s];
        } else {
            const unsigned o = ((const unsigned char *)queries)[(size_t)q * nsites + site];
#pragma unroll
            for (int s = 0; s < N; ++s) oq[s] = (o >= (unsigned)N || o == (unsigned)s) ? 1.0 : 0.0;
        }
        for (int d = 0; d < nd; ++d)
            for (int k = 0; k < K; ++k) {
                const double *Gh = G + ((size_t)(2 * R + k) * nnodes + rep[d]) * N * N;
                double h[N];
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    double y = 0.0;
#pragma unroll
                    for (int c = 0; c < N; ++c) y += Gh[b * N + c] * oq[c];
                    h[b] = y;
                }
                for (int v = 1; v < nnodes; ++v) {
                    if (dnode[v] != d) continue;
                    for (int r = 0; r < R; ++r) {
                        double t = 0.0;
#pragma unroll
                        for (int b = 0; b < N; ++b) t += Farr[idx(v * R + r, b)] * h[b];
                        double *o = out + ((size_t)q * NRK + ((size_t)v * R + r) * K + k) * nsites + site;
                        if constexpr (MIX) *o = mx.first ? t : __dadd_rn(*o, t);
                        else *o = place_value(t, zero);
                    }
                }
            }
    }
}

// rt_sites_placements_partitioned: a chunk's queries from caller order [QC][nsites][width] to slot
// order [QC][nslots][width] (width: n doubles, or one byte) -- slot j takes the query of its source
// site order[j], a pad that of the site it repeats.
template <class T, int BS>
__global__ void __launch_bounds__(BS)
place_query_gather_kernel(long nslots, long nsites, int width, const long *__restrict__ order,
                          const T *__restrict__ in, T *__restrict__ out)
{
    const long j = (long)blockIdx.x * BS + threadIdx.x;
    if (j >= nslots * width) return;
    const long slot = j / width;
    const int e = (int)(j - slot * width);
    const size_t q = blockIdx.y;
    out[(q * nslots + slot) * width + e] = in[(q * nsites + order[slot]) * width + e];
}

// Both reads.  MIX = false: the grid of the model's own exponential (post_grid: 2 R + K points per
// node), the upward pass, the `up` pass and the field once, then the queries in chunks.  MIX = true:
// the sets' grid (post_set_grid: the factors rho_r, 1 - rho_r of every set's own length and K
// ABSOLUTE points pendant_scale[k] tau_j per set) and the sets' fragment tables once; then per chunk
// of queries, once per rate set of positive class weight over the one L / M / U / field / h scratch,
// the set's upward pass (post_up_set), the MIX field (the root scaled by c_k), the set's pendant
// vectors and the MIX scores, which add c_k L_ik(query placed) into ONE accumulator in set order;
// post_mix turns it into the values, the root's rows are cleared afterwards.  node_q is shared by
// the sets: the distinct matrices in use (dnode, rep) are found once.  PART (a partitioned batch):
// as MIX = false -- the sets' grid and fragment tables as for MIX, made for the sets that have a
// site; the field once and per chunk one launch of the PART instances, every tile under the tables
// of its own set; a chunk's queries arrive in caller order and are brought to slot order on the
// device (place_query_gather_kernel: the chunk's scratch holds both images); the sums go per set
// and the result leaves in caller order (post_part_result).
template <bool MIX, bool PART = false>
int place_read(const char *who, rt_model *m, rt_sites *s, int recompute_transitions,
               const double *class_weights, int64_t nqueries, int query_kind, const void *queries,
               int64_t nfractions, const double *fractions, int64_t npendant, const double *pendant,
               const double *pendant_scale, double *values, double *sums, double *set_sums,
               double *loglik, int32_t *status)
{
    static_assert(!(MIX && PART), "a mixture is read on an ordinary batch");
    constexpr bool SETS = MIX || PART;           // the tables are those of the model's rate sets
    using grid_t = std::conditional_t<SETS, post_set_grid, post_grid>;
    using result_t = std::conditional_t<PART, post_part_result, post_result>;
    post_pass p;                                 // (alive until the synchronisation below)
    if (PART) RT_TRY(post_partitioned_only(who, s));
    RT_TRY(post_open(&p, who, m, s, PART));
    if (MIX) RT_TRY(post_class_weights(who, m, class_weights));
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    RT_REQUIRE(nqueries >= 1, "%s: at least one query (%lld here)", who, (long long)nqueries);
    if (query_kind == RT_OBS_MASK) {
        rt_set_error("%s: RT_OBS_MASK queries are not taken (RT_OBS_DENSE or RT_OBS_STATE)", who);
        return RT_ERR_UNSUPPORTED;
    }
    RT_REQUIRE(query_kind == RT_OBS_DENSE || query_kind == RT_OBS_STATE, "%s: query_kind %d", who,
               query_kind);
    RT_REQUIRE(queries && fractions && pendant, "%s: queries, fractions or pendant is NULL", who);
    RT_TRY(post_fraction_count(who, nfractions));
    RT_REQUIRE(npendant >= 1 && npendant <= RT_MAX_PLACE_PENDANT,
               "%s: 1..%d pendant lengths (%lld here)", who, RT_MAX_PLACE_PENDANT, (long long)npendant);
    RT_REQUIRE(2 * nfractions + npendant <= 32, "%s: 2 nfractions + npendant is at most 32 "
               "(%lld here)", who, (long long)(2 * nfractions + npendant));
    RT_TRY(post_fraction_values(who, nfractions, fractions));
    for (int64_t k = 0; k < npendant; ++k)
        RT_REQUIRE(std::isfinite(pendant[k]) && pendant[k] >= 0.0,
                   "%s: pendant length %d is negative or not finite", who, (int)k);
    for (int64_t k = 0; SETS && pendant_scale && k < m->multi.K; ++k)
        RT_REQUIRE(std::isfinite(pendant_scale[k]) && pendant_scale[k] >= 0.0,
                   "%s: pendant_scale[%lld] is negative or not finite", who, (long long)k);
    const int R = (int)nfractions, K = (int)npendant, np = 2 * R + K;
    p.per_set = MIX;
    RT_TRY(post_layout(&p, true));
    // the grid of every node: rho_r t_v, (1 - rho_r) t_v, tau_k (MIX: factors, the pendant points
    // absolute)
    const std::vector<double> lengths = SETS ? post_set_fraction_factors(&p, R, fractions, K)
                                             : post_fraction_lengths(&p, R, fractions, K, pendant);
    RT_TRY(grid_t::check(&p, recompute_transitions, np, lengths.data()));
    const int64_t NRK = N * R * K;
    RT_REQUIRE(NRK < (int64_t)1 << 31, "%s: too many placements per query", who);
    post_plan &plan = p.plan;
    grid_t grid;                                 // (alive until the synchronisation below)
    post_mix mix;
    post_part part;
    post_set_fractions setfrac;
    result_t res = [&] {
        if constexpr (PART) return post_part_result(values, sums, set_sums);
        else return post_result(values, sums);
    }();
    if constexpr (SETS) RT_TRY(grid.take(&p, np, K));
    else RT_TRY(grid.take(&p, np));
    if (MIX) RT_TRY(mix.take(&p, class_weights));
    if (PART) RT_TRY(part.take(&p));
    // the sets the grid's tables span: every set the MODEL holds, also for a partitioned batch that
    // uses fewer (spr_read's batch_sets counts the batch's: its PfragA follows the PT table)
    const int64_t grid_sets = SETS ? m->multi.K : 1;
    // the distinct rate matrices in use: d of every node, the node that stands for d
    std::vector<int32_t> dnode((size_t)N, -1), rep;
    {
        const std::vector<int32_t> &node_q = SETS ? m->multi.h_node_q : m->h_qidx;
        RT_REQUIRE((int64_t)node_q.size() == N, "%s: the model's rate matrix indices are missing", who);
        std::vector<int32_t> d_of_q;
        for (int64_t v = 1; v < N; ++v) {
            const int64_t qi = node_q[(size_t)v];
            if (qi < 0) continue;
            if ((int64_t)d_of_q.size() <= qi) d_of_q.resize((size_t)qi + 1, -1);
            if (d_of_q[(size_t)qi] < 0) {
                d_of_q[(size_t)qi] = (int32_t)rep.size();
                rep.push_back((int32_t)v);
            }
            dnode[(size_t)v] = d_of_q[(size_t)qi];
        }
    }
    const int nd = (int)rep.size();
    RT_REQUIRE(nd >= 1 && (p.lane || (int64_t)nd <= (int64_t)p.nops), "%s: no rate matrix in use", who);
    const int cnt = p.lane ? (int)N : p.nops;    // slots of the tables
    const size_t o_tab = plan.take((size_t)4 * cnt * 4);
    const size_t o_dtab = plan.take(((size_t)cnt + nd) * 4);
    const size_t tile = p.lane ? 0 : (size_t)s->nblocks * p.NT * 256 * 8;    // one vector of every site
    const size_t o_F = plan.take(p.lane ? (size_t)N * R * n * nsites * 8 : (size_t)p.nops * R * tile);
    res.take_sums(&p, (size_t)nqueries * NRK);
    // the queries of one chunk (post_chunk_units): beside their result, their pendant vectors and
    // their own image (PART: in slot order, and beside it the caller's); at most what the grids' y
    // takes
    const size_t q_unit = query_kind == RT_OBS_DENSE ? (size_t)n * 8 : 1;
    const size_t q_bytes = (size_t)nsites * q_unit;
    const size_t qc_bytes = PART ? (size_t)s->part->nsites * q_unit : 0;     // a query as the caller has it
    const int64_t CH = post_chunk_units(plan, NRK * res.row_bytes(&p),
                                        q_bytes + qc_bytes + (PART ? 1024 : 512) +
                                            (p.lane ? 0 : (size_t)nd * K * tile),
                                        32768, nqueries, "RAOTEH_PLACE_CHUNK_BYTES");
    const size_t o_q = plan.take((size_t)CH * q_bytes);
    // (the other calls take nothing here: their scratch lies as it did)
    const size_t o_qc = PART ? plan.take((size_t)CH * qc_bytes) : 0;
    const size_t o_H = plan.take(p.lane ? 8 : (size_t)nd * K * CH * tile);
    res.take_chunk(&p, (size_t)CH * NRK, (size_t)PLACE_MAX_ROWS);
    RT_TRY(post_begin(&p, recompute_transitions));
    res.place(&p);
    if (MIX) RT_TRY(mix.begin(&p));
    if (PART) RT_TRY(part.begin(&p));
    hipStream_t st = p.st;
    unsigned char *base = p.base;
    double *d_val = res.d_val, *d_F = (double *)(base + o_F), *d_H = (double *)(base + o_H);
    int *d_tab = (int *)(base + o_tab), *d_dtab = (int *)(base + o_dtab);
    void *d_q = (void *)(base + o_q), *d_qc = (void *)(base + o_qc);
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    if constexpr (SETS) RT_TRY(grid.launch(&p, lengths.data(), nullptr, pendant, pendant_scale));
    else RT_TRY(grid.launch(&p, lengths.data()));
    RT_TRY(post_up(&p, internal.data(), !SETS));
    std::vector<int32_t> tab, dtab((size_t)cnt + nd, -1);
    post_tab_build(&p, nullptr, &tab);
    for (int j = 0; j < cnt; ++j) dtab[(size_t)j] = dnode[(size_t)(p.lane ? j : p.x->ops[(size_t)j].node)];
    for (int d = 0; d < nd; ++d) dtab[(size_t)cnt + d] = rep[(size_t)d];
    RT_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_dtab, dtab.data(), dtab.size() * 4, hipMemcpyHostToDevice, st));
    const size_t nn = (size_t)n * n;
    const int dense = query_kind == RT_OBS_DENSE;
    // n > 4: the fragment tables in the grid's own piece.  Plain, [point][step]: P(rho t)^T at the
    // points 0 .. R - 1, P((1 - rho) t) at R .. 2 R - 1, and expm(Q_d tau_k) as [k][d] from point
    // 2 R on.  MIX: the fraction tables of every set (post_set_fractions: [half][set][fraction][step])
    // and behind them expm(Q[set][d] s_set tau_k) as [set][k][d], each by one launch over a table
    // that spans the sets.
    const size_t ftab = p.lane ? 0 : (size_t)p.nops * p.NT * p.KP * 128;
    const size_t dfrag = p.lane ? 0 : (size_t)p.NT * p.KP * 128;
    std::vector<int32_t> htab;                   // (feeds an asynchronous copy)
    if (!p.lane) {
        if constexpr (SETS) {
            if constexpr (MIX) RT_TRY(mix.PT.pack(&p));
            else RT_TRY(part.PT.pack(&p));
            RT_TRY(setfrac.pack(&p, &grid, R));
            if (dense) {
                int *d_htab = (int *)(base + grid.o_tab) + (size_t)2 * grid_sets * R * p.nops;
                htab.resize((size_t)grid_sets * K * nd);
                for (int64_t k = 0; k < grid_sets; ++k)
                    for (int j = 0; j < K; ++j)
                        for (int d = 0; d < nd; ++d)
                            htab[(size_t)((k * K + j) * nd + d)] =
                                (int32_t)((k * np + 2 * R + j) * N + rep[(size_t)d]);
                RT_HIP(hipMemcpyAsync(d_htab, htab.data(), htab.size() * 4, hipMemcpyHostToDevice, st));
                RT_TRY(rt_launch_pack_p(p.ctx, (int)n, p.NT, p.KP, (int)htab.size(), d_htab, grid.d_G,
                                        grid.d_GT + (size_t)2 * grid_sets * R * ftab));
            }
        } else {
            RT_TRY(post_fraction_pack(&p, &grid, R));
            if (dense)
                for (int k = 0; k < K; ++k)
                    RT_TRY(rt_launch_pack_p(p.ctx, (int)n, p.NT, p.KP, nd, d_dtab + cnt,
                                            grid.d_G + (size_t)(2 * R + k) * N * nn,
                                            grid.d_GT + (size_t)2 * R * ftab + (size_t)k * nd * dfrag));
        }
    }
    // what set k's launches read and write (plain: the model's own, the batch's status)
    struct set_view {
        const double *P, *G, *PT, *GT, *GA, *HA;
        int *stat;
        place_mix mx;
    };
    auto view_of = [&](int64_t k, int first_set) {
        set_view v = {m->d_P, grid.d_G, p.d_PT, grid.d_GT, grid.d_GT + (size_t)R * ftab,
                      p.lane ? nullptr : grid.d_GT + (size_t)2 * R * ftab, p.d_status,
                      {1.0, nullptr, first_set}};
        if constexpr (MIX) {
            v.P = mix.P_of(&p, k); v.G = grid.G_of_set(&p, k); v.PT = mix.PT.of_set(k);
            v.GT = p.lane ? nullptr : setfrac.T_of_set(k);
            v.GA = p.lane ? nullptr : setfrac.A_of_set(k);
            v.HA = p.lane ? nullptr : grid.d_GT + (size_t)2 * grid_sets * R * ftab + (size_t)k * K * nd * dfrag;
            v.stat = mix.status_of(&p, k);
            v.mx = {class_weights[k], mix.tot_of(&p, k), first_set};
        }
        if constexpr (PART) {                    // (the tables of set 0: the kernels move on)
            v.P = m->multi.d_P; v.PT = part.PT.d_PT;
            v.GT = p.lane ? nullptr : setfrac.T_of_set(0);
            v.GA = p.lane ? nullptr : setfrac.A_of_set(0);
            v.HA = p.lane ? nullptr : grid.d_GT + (size_t)2 * grid_sets * R * ftab;
        }
        return v;
    };
    // what the PART instances add per set: n <= 4 to P [set][node] and G [set][point][node]; else
    // the field's to the fragments [set][step] and [set][fraction][step], the queries' to the
    // pendant fragments [set][pendant][distinct] and to G
    [[maybe_unused]] post_part_arg px = {}, pxq = {};
    if constexpr (PART) {
        const long s_G = (long)((size_t)np * N * nn);
        px = p.lane ? part.arg((long)m->multi.P_stride, s_G)
                    : part.arg(part.pt_stride(), (long)((size_t)R * grid.tab));
        pxq = part.arg((long)((size_t)K * nd * dfrag), s_G);
    }
    // n > 4: the upward pass (MIX: under set k), the `up` pass and the field
    auto field = [&](int64_t k) -> int {
        const set_view v = view_of(k, 0);
        const rt_sites *x = p.x;
        if (MIX) RT_TRY(post_up_set(&p, k, nullptr));
        RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
            constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
            auto launch = [&](auto kernel, auto... mx) {
                hipLaunchKernelGGL(kernel, dim3((unsigned)x->nblocks), dim3(64 * NT), 0, st, v.PT, v.GT,
                                   v.GA, R, p.nops, (const int4 *)p.d_steps, (const int *)d_tab,
                                   (const double *)p.d_L, (const double *)p.d_M, p.d_D,
                                   (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root,
                                   (int)n, d_F, v.stat, (long)x->nsites, (long)x->nblocks, mx...);
            };
            if constexpr (MIX) launch(place_field_kernel<NT, KS, true, false, place_mix>, v.mx);
            else if constexpr (PART) launch(place_field_kernel<NT, KS, false, true, post_part_arg>, px);
            else launch(place_field_kernel<NT, KS>);
            return RT_OK;
        }));
        RT_HIP(hipGetLastError());
        return RT_OK;
    };
    // the QC queries at d_q against the field (n <= 4: `make` first makes the passes and the field)
    auto score = [&](int64_t k, int QC, int make, int first_set) -> int {
        const set_view v = view_of(k, first_set);
        if (p.lane) {
            const int *d_ptab = p.d_ptab;
            RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                auto launch = [&](auto kernel, auto... mx) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)((nsites + 255) / 256)), dim3(256), 0, st,
                                       (int)N, (long)nsites, v.P, v.G, R, K, d_ptab, d_ptab + N,
                                       (const int *)d_tab, (const int *)d_dtab,
                                       (const int *)(d_dtab + cnt), nd, (const void *)s->d_obs,
                                       s->compact_states, (int)s->nobs, s->block_sites,
                                       (const double *)m->d_root, p.d_L, p.d_M, p.d_D, d_F, dense,
                                       (const void *)d_q, QC, make, d_val, v.stat, mx...);
                };
                if constexpr (MIX)
                    launch(place_lane_kernel<decltype(nv)::value, true, false, place_mix>, v.mx);
                else if constexpr (PART)
                    launch(place_lane_kernel<decltype(nv)::value, false, true, post_part_arg>, px);
                else launch(place_lane_kernel<decltype(nv)::value>);
                return RT_OK;
            }));
        } else {
            const rt_sites *x = p.x;
            RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
                constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
                auto launch = [&](auto kernel, auto... part_arg) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)x->nblocks, (unsigned)QC), dim3(64 * NT), 0,
                                       st, dense, (const void *)d_q, v.HA, v.G + (size_t)2 * R * N * nn,
                                       (const int *)(d_dtab + cnt), nd, K, QC, (int)N, (int)n, d_H,
                                       (long)x->nsites, (long)x->nblocks, part_arg...);
                };
                if constexpr (PART) launch(place_query_kernel<NT, KS, true, post_part_arg>, pxq);
                else launch(place_query_kernel<NT, KS>);
                return RT_OK;
            }));
            RT_HIP(hipGetLastError());
            RT_TRY(post_dispatch<1, 8>(p.NT, [&](auto nt) {
                constexpr int NT = decltype(nt)::value;
                auto launch = [&](auto kernel, auto... mx) {
                    hipLaunchKernelGGL(kernel,
                                       dim3((unsigned)x->nblocks,
                                            (unsigned)(((size_t)QC * K + PLACE_BLOCK - 1) / PLACE_BLOCK)),
                                       dim3(64 * NT), 0, st, p.nops, R, K, QC, nd,
                                       (const int4 *)p.d_steps, (const int *)d_dtab, (const double *)d_F,
                                       (const double *)d_H, d_val, (const int *)v.stat, (int)N,
                                       (long)x->nsites, (long)x->nblocks, mx...);
                };
                if constexpr (MIX) launch(place_score_kernel<NT, true, place_mix>, v.mx);
                else launch(place_score_kernel<NT>);
                return RT_OK;
            }));
        }
        RT_HIP(hipGetLastError());
        return RT_OK;
    };
    // PART: the chunk's queries at d_qc, caller order -> d_q, slot order
    auto gather = [&](int QC) -> int {
        const rt_partition *pt = s->part;
        const int width = dense ? (int)n : 1;
        const dim3 grid_dim((unsigned)(((size_t)nsites * width + 255) / 256), (unsigned)QC);
        if (dense)
            hipLaunchKernelGGL((place_query_gather_kernel<double, 256>), grid_dim, dim3(256), 0, st,
                               (long)nsites, (long)pt->nsites, width, (const long *)pt->d_order,
                               (const double *)d_qc, (double *)d_q);
        else
            hipLaunchKernelGGL((place_query_gather_kernel<unsigned char, 256>), grid_dim, dim3(256), 0,
                               st, (long)nsites, (long)pt->nsites, width, (const long *)pt->d_order,
                               (const unsigned char *)d_qc, (unsigned char *)d_q);
        RT_HIP(hipGetLastError());
        return RT_OK;
    };
    if (!MIX && !p.lane) RT_TRY(field(0));       // the field, once
    for (int64_t q0 = 0; q0 < nqueries; q0 += CH) {
        const int QC = (int)std::min<int64_t>(CH, nqueries - q0);
        const size_t rows = (size_t)QC * NRK;
        if constexpr (PART) {
            RT_HIP(hipMemcpyAsync(d_qc, (const unsigned char *)queries + (size_t)q0 * qc_bytes,
                                  (size_t)QC * qc_bytes, hipMemcpyHostToDevice, st));
            RT_TRY(gather(QC));
        } else {
            RT_HIP(hipMemcpyAsync(d_q, (const unsigned char *)queries + (size_t)q0 * q_bytes,
                                  (size_t)QC * q_bytes, hipMemcpyHostToDevice, st));
        }
        RT_HIP(hipMemsetAsync(d_val, 0, rows * nsites * 8, st));       // (the root's rows)
        // the pass; MIX: set by set, the field holds one set at a time (a set of weight zero is
        // never live: not run, never read)
        int first_set = 1;
        // (PART: one launch, every tile under its own set)
        for (int64_t k = 0; k < (MIX ? grid_sets : 1); ++k) {
            if (MIX && !(class_weights[k] > 0.0)) continue;
            if (MIX && !p.lane) RT_TRY(field(k));
            RT_TRY(score(k, QC, MIX || q0 == 0 ? 1 : 0, first_set));
            first_set = 0;
        }
        if constexpr (MIX) {
            if (q0 == 0) RT_TRY(mix.post(&p));   // (log Lambda_i, the status)
            if (values || sums) {
                RT_TRY(mix.log_ratio(&p, rows, K, nullptr, d_val));
                // the root's rows: log(0) there, 0 by the definition
                RT_HIP(hipMemset2DAsync(d_val, (size_t)NRK * nsites * 8, 0, (size_t)R * K * nsites * 8,
                                        (size_t)QC, st));
            }
        }
        // 3. the weighted site sums and the per-site array [site][nqueries][N][R][K]
        RT_TRY(res.chunk(&p, (size_t)q0 * NRK, rows));
    }
    if constexpr (PART) RT_TRY(res.finish(&p, status));
    else RT_TRY(res.finish(&p, status, loglik, mix.d_ll));
    return grid.result(&p);
}

}  // namespace

extern "C" int rt_sites_placements(rt_model *m, rt_sites *s, int recompute_transitions,
                                   int64_t nqueries, int query_kind, const void *queries,
                                   int64_t nfractions, const double *fractions, int64_t npendant,
                                   const double *pendant, double *values, double *sums,
                                   int32_t *status)
{
    return place_read<false>("rt_sites_placements", m, s, recompute_transitions, nullptr, nqueries,
                             query_kind, queries, nfractions, fractions, npendant, pendant, nullptr,
                             values, sums, nullptr, nullptr, status);
}

extern "C" int rt_sites_placements_mixture(rt_model *m, rt_sites *s, int recompute_transitions,
                                           const double *class_weights, int64_t nqueries,
                                           int query_kind, const void *queries, int64_t nfractions,
                                           const double *fractions, int64_t npendant,
                                           const double *pendant, const double *pendant_scale,
                                           double *values, double *sums, double *loglik,
                                           int32_t *status)
{
    return place_read<true>("rt_sites_placements_mixture", m, s, recompute_transitions, class_weights,
                            nqueries, query_kind, queries, nfractions, fractions, npendant, pendant,
                            pendant_scale, values, sums, nullptr, loglik, status);
}

extern "C" int rt_sites_placements_partitioned(rt_model *m, rt_sites *s, int recompute_transitions,
                                               int64_t nqueries, int query_kind, const void *queries,
                                               int64_t nfractions, const double *fractions,
                                               int64_t npendant, const double *pendant,
                                               const double *pendant_scale, double *values,
                                               double *sums, double *set_sums, int32_t *status)
{
    return place_read<false, true>("rt_sites_placements_partitioned", m, s, recompute_transitions,
                                   nullptr, nqueries, query_kind, queries, nfractions, fractions,
                                   npendant, pendant, pendant_scale, values, sums, set_sums, nullptr,
                                   status);
}
