// Every subtree pruning and regrafting (SPR) move of the model's tree scored on a RESIDENT batch
// (rt_sites_spr_scores): for every site i, every move (c, y) within the radius and every
// fraction rho_r,
//     log L_i(tree after the move) - log L_i,
// the move being: the subtree of the non-root node c leaves v = parent(c) with its own edge, a new
// unobserved node x cuts the edge q -> y (y non-root, outside the subtree of c; q -> x of length
// rho t_y, x -> y of length (1 - rho) t_y, both under Q_y) and c hangs below x.  v stays, with
// one child fewer.
//
// A move is a placement (place.hip) whose "query" is the stored message M_c of the pruned
// subtree; what is new is the field of the target edge on the tree WITHOUT the subtree.  With
// L_w, M_w = P_w L_w, obs_w of the stored upward pass, up_w of the division-free `up` pass
// (normalised once at the root by 1 / L_i) and a_0 = v, a_1 = parent(v), ... the path to the root:
//     L-_{a_0}[b] = obs_v[b] prod_{w child of v, w != c} M_w[b]
//     M-_{a_j}    = P_{a_j} L-_{a_j}
//     L-_{a_j}[b] = obs_{a_j}[b] M-_{a_{j-1}}[b] prod_{w child of a_j, w != a_{j-1}} M_w[b]
//     up-_{a_j}   = up_{a_j}                (an ancestor's message from above holds no c)
//     off the path: L-_x = L_x, M-_x = M_x,
//     A-_x[a]     = up-_q[a] obs_q[a] prod_{w child of q, w not in {x, c}} M-_w[a]    (q = parent(x))
//     up-_x       = P_x^T A-_x
//     F_{c,y,r}[b] = (P_y(rho_r t_y)^T A-_y)[b] (P_y((1 - rho_r) t_y) L-_y)[b]
//     ratio       = sum_b F_{c,y,r}[b] M_c[b]
// Nothing is divided.  The host plans the walk of every pruned node as a table of ops (spr_plan):
// path steps up from v as far as the radius needs them, then in depth-first order one op per
// target edge -- A-_y staged once, the `up-` product where targets lie below y, two products per
// fraction where y is a target itself.  L- / M- of the path and up- per depth level live in a
// scratch of the call in the layout of L and M: every lane reads back only what it wrote.  Here:
//
//   1. P_y(rho_r t_y) and P_y((1 - rho_r) t_y) of every node in ONE launch of the model's own
//      exponential (post_grid: 2 R points per node);
//   2. n > 4: the upward pass with L and M of every step stored; spr_up_kernel (the `up` pass,
//      down_up_pass unchanged); per chunk of pruned nodes spr_kernel, one workgroup of NT row-tile
//      waves per (16-site tile, group of pruned nodes): group g walks the ops of the pruned
//      nodes c0 + g, c0 + g + G, ... of the chunk in its own piece of the scratch;
//      n <= 4: spr_lane_up_kernel and spr_lane_kernel, one lane per site, the same walk;
//   3. post_result (post_common.h): the site-weighted sums per (move, fraction) in a fixed order;
//      then, if the per-site array is asked for, its transpose to [site][move][fraction].
//
// Steps 2 (the walk) and 3 run per chunk of pruned nodes where the result of all moves would not
// fit the scratch (post_chunk_units); a chunk never splits the moves of one pruned node.  The
// fraction grid (its checks, its lengths, its fragment tables) is post_fraction_*, shared with
// place.hip.  Nothing of the batch or the model is written; two calls give the same bits, chunked
// or not, whatever the number of groups.
//
// rt_sites_spr_scores_mixture: the same scores of an ORDINARY batch under a site-class mixture over
// the model's K rate sets, the cut edge at fractions of every set's own resident length -- the
// kernels' MIX forms once per set and chunk into one accumulator, the root scaled by the class
// weight instead of 1 / L_i; the plan of the walk is the same for every set.
// rt_sites_spr_scores_partitioned: the same scores of a PARTITIONED batch, every site under its own
// rate set (the cut edge at fractions of the set's own length, the pruned subtree with its own edge
// of the set) -- one pass with the kernels' PART forms, every tile under the tables of its granule's
// set, then the per-set sums and the gather to caller order (post_part_result).  One host body
// (spr_read, at the end) serves the three calls.
#include "common.h"
#include "post_common.h"

#include <algorithm>
#include <vector>

namespace {

constexpr int64_t SPR_MAX_ROWS = (int64_t)1 << 21;       // rows of one transpose launch (grid y)
constexpr size_t SPR_LEVEL_BYTES = (size_t)2 << 30;      // the level vectors of all groups
constexpr int SPR_R = RT_MAX_PLACE_FRACTIONS;

// the stored value: 0 at a site of zero likelihood, else the log of the ratio (-inf where it is
// not positive)
__device__ __forceinline__ double spr_value(double ratio, bool zero)
{
    if (zero) return 0.0;
    return ratio > 0.0 ? log(ratio) : -__builtin_inf();
}

// One op of the walk of a pruned node, three int4 on the device.  Slots are schedule steps (n > 4)
// or preorder nodes (n <= 4); levels index the group's scratch.
//   path step (kind 0): L- of the path node at slot i into level ldst, from the node's
//       observation and the messages of its children but the pruned one -- the path child at slot
//       pw (or -1) from level psrc instead of the stored pass; M- = P L- into level mdst (or -1)
//   edge (kind 1): A- of the node y at slot i below the parent at slot pi -- up- of the parent
//       from level usrc, or the stored `up` (usrc = -1: the parent is on the path); the parent's
//       children but y and the pruned node, the path child pw from level psrc; up-_y = P_y^T A-
//       into level udst (or -1); and the move itself (the planner makes an edge op for targets
//       only, so mv >= 0): L-_y from level lsrc (y on the path) or the stored pass (lsrc = -1),
//       the ratios of move mv at every fraction
struct spr_op {
    int32_t kind, i, pi, mv;
    int32_t usrc, udst, pw, psrc;                // (path step: usrc is mdst, udst is ldst)
    int32_t lsrc, pad0, pad1, pad2;
};
static_assert(sizeof(spr_op) == 48, "three int4 per op");

// the pruned node c on the device: {slot of c, first op, one past the last op, first move}
// (entry nnodes: the number of moves)

// n > 4: the `up` pass alone, for every group of spr_kernel to find.  MIX
// (rt_sites_spr_scores_mixture, one launch per rate set k of weight ck > 0 and chunk, after the
// set's upward pass): down_up_pass's MIX form -- the root scaled by ck, L_ik to root_tot[site], the
// status word the set's own.  PART (rt_sites_spr_scores_partitioned: sites are the batch's slots):
// the tile is one granule; PfragT [set][step] is moved on to the tile's set (post_part_arg, the PART
// instance's one further argument) and down_up_pass takes it as it is.
template <int NT, int KS, bool MIX = false, bool PART = false, class... PX>
__global__ void __launch_bounds__(64 * NT)
spr_up_kernel(const double *__restrict__ PfragT, int nops, const int4 *__restrict__ steps,
              const int *__restrict__ tabp, const double *__restrict__ Larr,
              const double *__restrict__ Marr, double *__restrict__ Uarr,
              const double *__restrict__ obs, int K, const double *__restrict__ root_w, int n,
              int *__restrict__ status, long nsites, long nblocks, double ck,
              double *__restrict__ root_tot, PX... part)
{
    static_assert(sizeof...(PX) == (PART ? 1 : 0) && !(MIX && PART), "post_part_arg: the PART instance's alone");
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double red[NT][16];
    const post_tab tab(tabp, nops);
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    if constexpr (PART) {
        const post_part_arg px = post_pack_one(part...);
        PfragT += post_part_set(px, blk) * px.s_p;
    }
    const long site = blk * 16 + (lane & 15);
    const bool writer = m == 0 && lane < 16 && site < nsites;
    bool live[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) live[r] = 16 * m + 4 * r + (lane >> 4) < n;
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;
    down_up_pass<NT, KS, MIX>(true, xb, red, tab, PfragT, nops, steps, Larr, Marr, Uarr, og, root_w,
                              live, m, lane, blk, nblocks, writer, status, site, ck, root_tot);
}

// n > 4, one workgroup per (tile, group).  steps as in nni_kernel; PfragT / PfragA: [step] A
// fragments of the resident P^T / P; GfragT: [fraction][step] those of P(rho t)^T; GfragA:
// [fraction][step] those of P((1 - rho) t); Uarr: the `up` vectors of spr_up_kernel; S: the level
// vectors, [group][level] in the layout of L and M; cut, ops: the plan; out
// [move - mvA][fraction][site] for the moves of the pruned nodes cA .. cB - 1.
// MIX (one launch per rate set of weight > 0 and chunk, against the set's P, P^T and fraction
// fragments; Uarr from the MIX spr_up_kernel, scaled by the class weight): a move's sum is the RAW
// term c_k L_ik(moved tree) -- no log, no look at the site's likelihood under the set, which may be
// 0 on the resident tree and positive on the moved one.  The first running set stores it, the
// later ones add to it (first == 0): the same lane of the same workgroup, launches in order on
// one stream -- a fixed sum.  The logs are mix_log_ratio_kernel's once the sets are in.
// (`first` is an argument of the MIX instance alone, FIRST = int: the plain instance keeps its
// argument list, and with it the offsets of the hidden arguments behind it -- gridDim.y.)
// PART (one launch per chunk; out in slot order): the plain walk, every tile under the tables of
// its granule's set -- PfragT / PfragA [set][step], GfragT / GfragA [set][fraction][step] are moved
// on by set * (s_p, s_g) doubles before anything else; the pack holds the post_part_arg instead.
template <int NT, int KS, bool MIX = false, bool PART = false, class... FIRST>
__global__ void __launch_bounds__(64 * NT)
spr_kernel(const double *__restrict__ PfragT, const double *__restrict__ PfragA,
           const double *__restrict__ GfragT, const double *__restrict__ GfragA, int R, int nops,
           const int4 *__restrict__ steps, const int *__restrict__ tabp,
           const int4 *__restrict__ cut, const int4 *__restrict__ ops,
           const double *__restrict__ Larr, const double *__restrict__ Marr,
           const double *__restrict__ Uarr, double *S, int nlevels,
           const double *__restrict__ obs, int K, const double *__restrict__ root_w, int n, int cA,
           int cB, int mvA, double *__restrict__ out, int *__restrict__ status, long nsites,
           long nblocks, FIRST... first_set)
{
    static_assert(sizeof...(FIRST) == (MIX || PART ? 1 : 0) && !(MIX && PART),
                  "first: the MIX instance's alone; post_part_arg: the PART instance's");
    [[maybe_unused]] int first = 0;
    if constexpr (MIX) first = post_pack_one(first_set...);
    constexpr int KP = (KS + 1) / 2;
    __shared__ double xb[NT * 4 * 64];
    __shared__ double lb[NT * 4 * 64];
    __shared__ double red[NT][16];
    __shared__ double sums[2][SPR_R][NT][16];
    const post_tab tab(tabp, nops);
    const int lane = threadIdx.x & 63;
    const int m = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long blk = blockIdx.x;
    if constexpr (PART) {
        const post_part_arg px = post_pack_one(first_set...);
        const long gs = post_part_set(px, blk);
        PfragT += gs * px.s_p;
        PfragA += gs * px.s_p;
        GfragT += gs * px.s_g;
        GfragA += gs * px.s_g;
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
    // the site's likelihood (the `up` vectors are spr_up_kernel's)
    [[maybe_unused]] bool zero = false;
    if constexpr (!MIX)
        zero = down_up_pass<NT, KS>(false, xb, red, tab, PfragT, nops, steps, Larr, Marr, nullptr, og,
                                    root_w, live, m, lane, blk, nblocks, writer, status, site);
    const int lv0 = blockIdx.y * nlevels;        // the group's levels
    double a[2 * KP];
    int par = 0;                                 // the half of `sums` the next move writes
    for (int c = cA + blockIdx.y; c < cB; c += gridDim.y) {
        const int4 ct = cut[c];
        if (ct.y == ct.z) continue;
        const int ci = ct.x;
        double mc[4];                            // the pruned subtree's message
        {
            const size_t co = down_at<NT>(ci, nblocks, blk, m, lane);
#pragma unroll
            for (int r = 0; r < 4; ++r) mc[r] = live[r] ? Marr[co + r * 64] : 0.0;
        }
        for (int o = ct.y; o < ct.z; ++o) {
            const int4 oa = ops[3 * o], ob4 = ops[3 * o + 1];
            const int kind = oa.x, i = oa.y, pi = oa.z, mv = oa.w;
            const int usrc = ob4.x, udst = ob4.y, pw = ob4.z, psrc = ob4.w;
            const size_t io = down_at<NT>(i, nblocks, blk, m, lane);
            const size_t pso = down_at<NT>(lv0 + max(psrc, 0), nblocks, blk, m, lane);
            double x[4];
            if (kind == 0) {
                // L- of a path node, then M- = P L-
                const int k = tab.obs[i];
                if (k >= 0) down_L<KP>(k, og, Larr, io, m, x);
                else
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] = 1.0;
                for (int e = tab.cptr[i]; e < tab.cptr[i + 1]; ++e) {
                    const int w = tab.cidx[e];
                    if (w == ci) continue;
                    const double *src = w == pw ? S + pso
                                                : Marr + down_at<NT>(w, nblocks, blk, m, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) x[r] *= src[r * 64];
                }
                const size_t lo = down_at<NT>(lv0 + udst, nblocks, blk, m, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    x[r] = live[r] ? x[r] : 0.0;     // (rows past the states)
                    S[lo + r * 64] = x[r];
                }
                if (usrc >= 0) {
                    down_stage(xb, m, lane, x);
                    down_frag<KP>(PfragA + (size_t)i * ASTRIDE + frag, a);
                    const double4_t y = down_product<KS>(a, xb, lane);
                    const size_t mo = down_at<NT>(lv0 + usrc, nblocks, blk, m, lane);
#pragma unroll
                    for (int r = 0; r < 4; ++r) S[mo + r * 64] = y[r];
                }
                continue;
            }
            // A- of the edge above the node at slot i
            const size_t po = down_at<NT>(pi, nblocks, blk, m, lane);
            {
                const double *us = usrc < 0 ? Uarr + po
                                            : S + down_at<NT>(lv0 + usrc, nblocks, blk, m, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = us[r * 64];
            }
            const int kp = tab.obs[pi];
            if (kp >= 0) {
                double ob[4];
                down_L<KP>(kp, og, Larr, po, m, ob);
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] *= ob[r];
            }
            for (int e = tab.cptr[pi]; e < tab.cptr[pi + 1]; ++e) {
                const int w = tab.cidx[e];
                if (w == i || w == ci) continue;
                const double *src = w == pw ? S + pso : Marr + down_at<NT>(w, nblocks, blk, m, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] *= src[r * 64];
            }
            double l[4];
            const int lsrc = ops[3 * o + 2].x;
            if (lsrc >= 0) {
                const size_t lo = down_at<NT>(lv0 + lsrc, nblocks, blk, m, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) l[r] = S[lo + r * 64];
            } else {
                down_L<KP>(steps[i].z, og, Larr, io, m, l);
            }
            __syncthreads();                     // (every wave is done with the previous operands)
#pragma unroll
            for (int r = 0; r < 4; ++r) {        // (rows past the states: 0)
                xb[(4 * m + r) * 64 + lane] = live[r] ? x[r] : 0.0;
                lb[(4 * m + r) * 64 + lane] = live[r] ? l[r] : 0.0;
            }
            __syncthreads();
            if (udst >= 0) {
                down_frag<KP>(PfragT + (size_t)i * ASTRIDE + frag, a);
                const double4_t y = down_product<KS>(a, xb, lane);
                const size_t uo = down_at<NT>(lv0 + udst, nblocks, blk, m, lane);
#pragma unroll
                for (int r = 0; r < 4; ++r) S[uo + r * 64] = y[r];
            }
            for (int r = 0; r < R; ++r) {
                down_frag<KP>(GfragT + ((size_t)r * nops + i) * ASTRIDE + frag, a);
                const double4_t y = down_product<KS>(a, xb, lane);
                down_frag<KP>(GfragA + ((size_t)r * nops + i) * ASTRIDE + frag, a);
                const double4_t z = down_product<KS>(a, lb, lane);
                double t = 0.0;
#pragma unroll
                for (int e = 0; e < 4; ++e) t += y[e] * z[e] * mc[e];
                down_part(sums[par][r], m, lane, t);
            }
            __syncthreads();
            if (writer) {
                double *row = out + (size_t)(mv - mvA) * R * nsites + site;
                for (int r = 0; r < R; ++r) {
                    const double t = down_total<NT>(sums[par][r], lane);
                    double *x = row + (size_t)r * nsites;
                    if constexpr (MIX) *x = first ? t : __dadd_rn(*x, t);
                    else *x = t;
                }
            }
            par ^= 1;
        }
        // the pruned node's ratios -> values, by all waves: lane group g of the workgroup takes
        // the rows g, g + 4 NT, ... of its site (the barrier: wave 0's stores are visible)
        if constexpr (MIX) continue;
        __syncthreads();
        if (site_ok) {
            const long r0 = (long)(ct.w - mvA) * R, r1 = (long)(cut[c + 1].w - mvA) * R;
            for (long r = r0 + 4 * m + (lane >> 4); r < r1; r += 4 * NT) {
                double *x = out + (size_t)r * nsites + site;
                *x = spr_value(*x, zero);
            }
        }
    }
}

// n <= 4: the upward pass and the `up` pass, one lane per site (MIX: as spr_up_kernel, P of the set;
// PART: P [set][node] moved on to the set of the wave's granule -- wave-uniform, so the matrices stay
// scalar loads)
template <int N, bool MIX = false, bool PART = false, class... PX>
__global__ void __launch_bounds__(256)
spr_lane_up_kernel(int nnodes, long nsites, const double *__restrict__ P,
                   const int *__restrict__ parent, const int *__restrict__ node_k,
                   const int *__restrict__ tabp, const void *__restrict__ obs, int compact, int Kobs,
                   int block_sites, const double *__restrict__ root_w, double *__restrict__ Larr,
                   double *__restrict__ Marr, double *__restrict__ Uarr, int *__restrict__ status,
                   double ck, double *__restrict__ root_tot, PX... part)
{
    static_assert(sizeof...(PX) == (PART ? 1 : 0) && !(MIX && PART), "post_part_arg: the PART instance's alone");
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    if constexpr (PART) {
        const post_part_arg px = post_pack_one(part...);
        P += post_part_set(px, site >> px.gshift) * px.s_p;
    }
    const post_tab tab(tabp, nnodes);
    lane_up<N, true>(nnodes, nsites, site, P, parent, node_k, obs, compact, Kobs, block_sites, Larr, Marr);
    lane_up_pass<N, MIX>(true, nnodes, nsites, site, P, parent, node_k, tab, obs, compact, Kobs,
                         block_sites, root_w, Larr, Marr, Uarr, status, ck, root_tot);
}

// n <= 4: one lane per (site, group); arrays [node][state][site], nodes in preorder; G
// [point][node][N][N]: the points 0 .. R - 1 are P(rho t), R .. 2 R - 1 are P((1 - rho) t) (the
// same address in every lane: the scalar path); S [group][level][state][site].  MIX: as spr_kernel,
// P and G of the set, `first` its argument alone.  PART: as spr_lane_up_kernel, P [set][node] and G
// [set][point][node] of the set of the wave's granule.
template <int N, bool MIX = false, bool PART = false, class... FIRST>
__global__ void __launch_bounds__(256)
spr_lane_kernel(int nnodes, long nsites, const double *__restrict__ P, const double *__restrict__ G,
                int R, const int *__restrict__ parent, const int *__restrict__ node_k,
                const int *__restrict__ tabp, const int4 *__restrict__ cut,
                const int4 *__restrict__ ops, const void *__restrict__ obs, int compact, int Kobs,
                int block_sites, const double *__restrict__ root_w, const double *__restrict__ Larr,
                const double *__restrict__ Marr, const double *__restrict__ Uarr, double *S,
                int nlevels, int cA, int cB, int mvA, double *__restrict__ out,
                int *__restrict__ status, FIRST... first_set)
{
    static_assert(sizeof...(FIRST) == (MIX || PART ? 1 : 0) && !(MIX && PART),
                  "first: the MIX instance's alone; post_part_arg: the PART instance's");
    [[maybe_unused]] int first = 0;
    if constexpr (MIX) first = post_pack_one(first_set...);
    const long site = (long)blockIdx.x * 256 + threadIdx.x;
    if (site >= nsites) return;
    if constexpr (PART) {
        const post_part_arg px = post_pack_one(first_set...);
        const long gs = post_part_set(px, site >> px.gshift);
        P += gs * px.s_p;
        G += gs * px.s_g;
    }
    const post_tab tab(tabp, nnodes);
    auto idx = [&](int v, int s) { return ((size_t)v * N + s) * nsites + site; };
    const int lv0 = blockIdx.y * nlevels;
    auto lev = [&](int level, int s) { return ((size_t)(lv0 + level) * N + s) * nsites + site; };
    auto node_obs = [&](int v, double (&x)[N]) {
        const int k = node_k[v];
        if (k >= 0) lane_obs<N>(obs, compact, Kobs, block_sites, site, k, x);
        else
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] = 1.0;
    };
    [[maybe_unused]] bool zero = false;
    if constexpr (!MIX)
        zero = lane_up_pass<N>(false, nnodes, nsites, site, P, parent, node_k, tab, obs, compact, Kobs,
                               block_sites, root_w, Larr, Marr, nullptr, status);
    for (int c = cA + blockIdx.y; c < cB; c += gridDim.y) {
        const int4 ct = cut[c];
        const int ci = ct.x;
        double mc[N];
#pragma unroll
        for (int s = 0; s < N; ++s) mc[s] = Marr[idx(ci, s)];
        for (int o = ct.y; o < ct.z; ++o) {
            const int4 oa = ops[3 * o], ob4 = ops[3 * o + 1];
            const int kind = oa.x, i = oa.y, pi = oa.z, mv = oa.w;
            const int usrc = ob4.x, udst = ob4.y, pw = ob4.z, psrc = ob4.w;
            double x[N];
            if (kind == 0) {
                node_obs(i, x);
                for (int e = tab.cptr[i]; e < tab.cptr[i + 1]; ++e) {
                    const int w = tab.cidx[e];
                    if (w == ci) continue;
#pragma unroll
                    for (int s = 0; s < N; ++s) x[s] *= w == pw ? S[lev(psrc, s)] : Marr[idx(w, s)];
                }
#pragma unroll
                for (int s = 0; s < N; ++s) S[lev(udst, s)] = x[s];
                if (usrc >= 0) {
                    const double *Pv = P + (size_t)i * N * N;
#pragma unroll
                    for (int a = 0; a < N; ++a) {
                        double t = 0.0;
#pragma unroll
                        for (int b = 0; b < N; ++b) t += Pv[a * N + b] * x[b];
                        S[lev(usrc, a)] = t;
                    }
                }
                continue;
            }
            node_obs(pi, x);
#pragma unroll
            for (int s = 0; s < N; ++s) x[s] *= usrc < 0 ? Uarr[idx(pi, s)] : S[lev(usrc, s)];
            for (int e = tab.cptr[pi]; e < tab.cptr[pi + 1]; ++e) {
                const int w = tab.cidx[e];
                if (w == i || w == ci) continue;
#pragma unroll
                for (int s = 0; s < N; ++s) x[s] *= w == pw ? S[lev(psrc, s)] : Marr[idx(w, s)];
            }
            if (udst >= 0) {
                const double *Pv = P + (size_t)i * N * N;
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    double y = 0.0;
#pragma unroll
                    for (int a = 0; a < N; ++a) y += Pv[a * N + b] * x[a];
                    S[lev(udst, b)] = y;
                }
            }
            const int lsrc = ops[3 * o + 2].x;
            double l[N];
#pragma unroll
            for (int s = 0; s < N; ++s) l[s] = lsrc >= 0 ? S[lev(lsrc, s)] : Larr[idx(i, s)];
            for (int r = 0; r < R; ++r) {
                const double *G1 = G + ((size_t)r * nnodes + i) * N * N;
                const double *G2 = G + ((size_t)(R + r) * nnodes + i) * N * N;
                double t = 0.0;
#pragma unroll
                for (int b = 0; b < N; ++b) {
                    double y = 0.0, z = 0.0;
#pragma unroll
                    for (int a = 0; a < N; ++a) {
                        y += G1[a * N + b] * x[a];
                        z += G2[b * N + a] * l[a];
                    }
                    t += y * z * mc[b];
                }
                double *o = out + ((size_t)(mv - mvA) * R + r) * nsites + site;
                if constexpr (MIX) *o = first ? t : __dadd_rn(*o, t);
                else *o = spr_value(t, zero);
            }
        }
    }
}

// ---- the host's side: the moves and the plan of the walk ----

// what the moves of one pruned node need of the tree (children after their parents, as every
// CSR the library takes)
struct spr_tree {
    int64_t N = 0;
    const int64_t *idx = nullptr, *ptr = nullptr;
    const int32_t *parent = nullptr;
    std::vector<int32_t> depth, size;            // edges from the root; nodes of the subtree
    std::vector<int32_t> dist, path;             // per pruned node: edges from v; j on the path, else -1
    std::vector<unsigned char> in, target;       // in the pruned subtree; a target of the pruned node

    spr_tree(int64_t n, const int64_t *i, const int64_t *p, const int32_t *par)
        : N(n), idx(i), ptr(p), parent(par), depth((size_t)n, 0), size((size_t)n, 1),
          dist((size_t)n, 0), path((size_t)n, -1), in((size_t)n, 0), target((size_t)n, 0)
    {
        for (int64_t v = 1; v < N; ++v) depth[(size_t)v] = depth[(size_t)parent[v]] + 1;
        for (int64_t v = N - 1; v >= 1; --v) size[(size_t)parent[v]] += size[(size_t)v];
    }

    // the path steps of the walk of the pruned node c: a_j, j = 0 .. J, the non-root ancestors
    // of c within the radius
    int64_t path_steps(int64_t c, int64_t radius) const
    {
        return std::min<int64_t>(radius < 0 ? N : radius, (int64_t)depth[(size_t)parent[c]] - 1) + 1;
    }

    // the targets y of the pruned node c within the radius (< 0: no limit), their number
    int64_t cut(int64_t c, int64_t radius)
    {
        std::fill(path.begin(), path.end(), -1);
        int32_t j = 0;
        for (int64_t a = parent[c]; a >= 0; a = parent[a]) {
            path[(size_t)a] = j;
            dist[(size_t)a] = j++;
        }
        int64_t cnt = 0;
        in[0] = target[0] = 0;
        for (int64_t y = 1; y < N; ++y) {
            const int64_t q = parent[y];
            in[(size_t)y] = y == c || in[(size_t)q];
            target[(size_t)y] = 0;
            if (in[(size_t)y]) continue;
            if (path[(size_t)y] < 0) dist[(size_t)y] = dist[(size_t)q] + 1;
            const int64_t d = std::min(dist[(size_t)y], dist[(size_t)q]);
            target[(size_t)y] = radius < 0 || d <= radius;
            cnt += target[(size_t)y];
        }
        return cnt;
    }
};

// the moves in their order: c ascending, then y ascending.  first (or null): [nnodes + 1] the
// index of every pruned node's first move; moves (or null): the pairs
int64_t spr_enumerate(spr_tree &t, int64_t radius, int32_t *first, int32_t *moves)
{
    int64_t k = 0;
    if (first) first[0] = 0;
    for (int64_t c = 1; c < t.N; ++c) {
        if (first) first[c] = (int32_t)std::min<int64_t>(k, INT32_MAX);
        // (without a limit and without the pairs the count needs no walk)
        const int64_t cnt = radius < 0 && !moves ? t.N - 1 - t.size[(size_t)c] : t.cut(c, radius);
        if (moves)
            for (int64_t y = 1, j = k; y < t.N; ++y)
                if (t.target[(size_t)y]) {
                    moves[2 * j] = (int32_t)c;
                    moves[2 * j + 1] = (int32_t)y;
                    ++j;
                }
        k += cnt;
    }
    if (first) first[t.N] = (int32_t)std::min<int64_t>(k, INT32_MAX);
    return k;
}

int spr_moves_out(int64_t cnt, int32_t *moves, int64_t capacity, int64_t *nmoves)
{
    *nmoves = cnt;
    RT_REQUIRE(!moves || capacity >= cnt, "the tree has %lld moves within the radius, the array "
               "holds %lld", (long long)cnt, (long long)capacity);
    return RT_OK;
}

int spr_list(int64_t N, const int64_t *idx, const int64_t *ptr, const int32_t *parent, int64_t radius,
             int32_t *moves, int64_t capacity, int64_t *nmoves)
{
    spr_tree t(N, idx, ptr, parent);
    RT_TRY(spr_moves_out(spr_enumerate(t, radius, nullptr, nullptr), moves, capacity, nmoves));
    if (moves) spr_enumerate(t, radius, nullptr, moves);
    return RT_OK;
}

// The ops of every pruned node (after spr_tree::cut of it, in `t`).  Levels of a group's
// scratch, D = 1 + the depth of the tree: L- of path node a_j at j, M- at D + j, up- of an
// off-path node of depth d at 2 D + d.  slot_of: node -> slot of the kernels' tables.
void spr_plan_one(const spr_tree &t, int64_t c, int64_t radius, int32_t mv0, int D,
                  const int32_t *slot_of, std::vector<spr_op> *ops, std::vector<int32_t> *rank,
                  std::vector<int32_t> *stack)
{
    const int64_t N = t.N;
    const int32_t *parent = t.parent;
    // the moves' indices: the rank of y among the targets, ascending
    int32_t k = mv0;
    for (int64_t y = 1; y < N; ++y) (*rank)[(size_t)y] = t.target[(size_t)y] ? k++ : -1;
    if (k == mv0) return;
    // the path: a_j, j = 0 .. J, the non-root ancestors whose L- a target or a later step needs
    const int64_t v = parent[c];
    const int64_t J = t.path_steps(c, radius) - 1;
    int64_t a = v, below = -1;                   // a_j and a_{j-1}
    for (int64_t j = 0; j <= J; ++j, below = a, a = parent[a]) {
        const int64_t q = parent[a];
        // M- of a_j: the next step's, or the A- of the siblings of a_j (d = j + 1)
        const bool others = t.ptr[q + 1] - t.ptr[q] > 1;
        const bool need_m = j < J || ((radius < 0 || j + 1 <= radius) && others);
        spr_op op = {};
        op.kind = 0;
        op.i = slot_of[a];
        op.pi = -1;
        op.mv = -1;
        op.usrc = need_m ? (int32_t)(D + j) : -1;
        op.udst = (int32_t)j;
        op.pw = j ? slot_of[below] : -1;
        op.psrc = j ? (int32_t)(D + j - 1) : -1;
        op.lsrc = -1;
        ops->push_back(op);
    }
    // the edges, depth first from the root in CSR child order
    size_t top = 0;
    auto push_children = [&](int64_t q) {
        for (int64_t e = t.ptr[q + 1] - 1; e >= t.ptr[q]; --e) (*stack)[top++] = (int32_t)t.idx[e];
    };
    push_children(0);
    while (top) {
        const int64_t y = (*stack)[--top];
        if (t.in[(size_t)y] || !t.target[(size_t)y]) {
            // not a target: below an off-path node nothing further down is one; a path node
            // past the radius may still have targets below it (nearer v)
            if (!t.in[(size_t)y] && t.path[(size_t)y] >= 0) push_children(y);
            continue;
        }
        const int64_t q = parent[y];
        const bool y_on = t.path[(size_t)y] >= 0, q_on = t.path[(size_t)q] >= 0;
        const bool kids = t.ptr[y + 1] > t.ptr[y];
        const bool up = !y_on && kids && (radius < 0 || t.dist[(size_t)y] <= radius);
        spr_op op = {};
        op.kind = 1;
        op.i = slot_of[y];
        op.pi = slot_of[q];
        op.mv = (*rank)[(size_t)y];
        op.usrc = q_on ? -1 : (int32_t)(2 * D + t.depth[(size_t)q]);
        op.udst = up ? (int32_t)(2 * D + t.depth[(size_t)y]) : -1;
        op.pw = -1;
        op.psrc = -1;
        op.lsrc = y_on ? t.path[(size_t)y] : -1;
        if (q_on && !y_on && t.path[(size_t)q] >= 1) {
            // q = a_j, j >= 1: its path child a_{j-1} comes without the pruned subtree
            int64_t b = v;
            while (parent[b] != q) b = parent[b];
            op.pw = slot_of[b];
            op.psrc = (int32_t)(D + t.path[(size_t)q] - 1);
        }
        ops->push_back(op);
        if (y_on || up) push_children(y);
    }
}

}  // namespace

extern "C" int rt_model_spr_moves(const rt_model *m, int64_t radius, int32_t *moves,
                                  int64_t capacity, int64_t *nmoves)
{
    RT_REQUIRE(m && nmoves, "null pointer");
    return spr_list(m->nnodes, m->indices.data(), m->indptr.data(), m->parent.data(), radius, moves,
                    capacity, nmoves);
}

extern "C" int rt_tree_spr_moves(int64_t nnodes, const int64_t *idx, const int64_t *ptr,
                                 int64_t radius, int32_t *moves, int64_t capacity, int64_t *nmoves)
{
    RT_REQUIRE(nmoves, "bad arguments");
    // (the walk goes up through the parents: every node but the root has exactly one)
    std::vector<int32_t> parent;
    RT_TRY(post_csr_parents(nnodes, idx, ptr, &parent));
    return spr_list(nnodes, idx, ptr, parent.data(), radius, moves, capacity, nmoves);
}

namespace {

// Both reads.  MIX = false: the grid of the model's own exponential (post_grid), the upward pass
// and the `up` pass once, then per chunk of pruned nodes the walk, whose plain instance takes the
// logs.  MIX = true: the sets' grid (post_set_grid at the factors rho_r, 1 - rho_r) and the sets'
// P, P^T and fraction fragments packed once; then per chunk, once per rate set of positive class
// weight over the one L / M / U / level scratch, the set's upward pass (post_up_set), the MIX `up`
// pass and the MIX walk, which adds c_k L_ik(moved tree) into ONE accumulator [move][fraction][site]
// in set order; post_mix turns it into the values.  PART (a partitioned batch): as MIX = false, one
// launch of the PART instances per chunk, every tile under the tables of its own set -- the sets'
// grid makes matrices for the sets that have a site, their fragments are packed once; the sums go
// per set over the runs of the plan and the result leaves in caller order (post_part_result).  The
// plan of the walk holds no matrix: it is made once per call.
template <bool MIX, bool PART = false>
int spr_read(const char *who, rt_model *m, rt_sites *s, int recompute_transitions,
             const double *class_weights, int64_t radius, int64_t nfractions, const double *fractions,
             double *values, double *sums, double *set_sums, double *loglik, int32_t *status)
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
    RT_REQUIRE(fractions, "%s: fractions is NULL", who);
    RT_TRY(post_fraction_count(who, nfractions));
    RT_TRY(post_fraction_values(who, nfractions, fractions));
    const int R = (int)nfractions, np = 2 * R;
    // the moves
    spr_tree tree(N, m->indices.data(), m->indptr.data(), m->parent.data());
    std::vector<int32_t> first((size_t)N + 1, 0);
    const int64_t nmoves = spr_enumerate(tree, radius, first.data(), nullptr);
    RT_REQUIRE(nmoves * R < (int64_t)1 << 31, "%s: too many moves (%lld at %d fractions)", who,
               (long long)nmoves, R);
    // the ops of the plan: one per move, and the path steps of every pruned node that has moves
    int64_t nplan = nmoves;
    for (int64_t c = 1; c < N; ++c)
        if (first[(size_t)c + 1] > first[(size_t)c]) nplan += tree.path_steps(c, radius);
    RT_REQUIRE(nplan < INT32_MAX / 4, "%s: too many moves (a plan of %lld ops)", who, (long long)nplan);
    p.per_set = MIX;
    RT_TRY(post_layout(&p, true));
    // the grid of every node: rho_r t_v, (1 - rho_r) t_v (MIX: the factors of every set's own t)
    const std::vector<double> lengths = SETS ? post_set_fraction_factors(&p, R, fractions)
                                             : post_fraction_lengths(&p, R, fractions);
    RT_TRY(grid_t::check(&p, recompute_transitions, np, lengths.data()));
    post_plan &plan = p.plan;
    grid_t grid;                                 // (alive until the synchronisation below)
    post_mix mix;
    post_part part;
    post_set_fractions setfrac;
    result_t res = [&] {
        if constexpr (PART) return post_part_result(values, sums, set_sums);
        else return post_result(values, sums);
    }();
    RT_TRY(grid.take(&p, np));
    if (MIX) RT_TRY(mix.take(&p, class_weights));
    if (PART) RT_TRY(part.take(&p));
    // the sets whose PfragA is packed, beside the PT table: the model's sets for a mixture, the
    // BATCH's sets for a partitioned batch (place_read's grid_sets counts the model's either way)
    const int64_t batch_sets = MIX ? mix.K : PART ? part.K : 1;
    const int cnt = p.lane ? (int)N : p.nops;    // slots of the tables
    const int D = 1 + *std::max_element(tree.depth.begin(), tree.depth.end()), nlevels = 3 * D;
    const size_t o_tab = plan.take((size_t)4 * cnt * 4);
    const size_t o_cut = plan.take(((size_t)N + 1) * 16);
    const size_t ftab = p.lane ? 0 : (size_t)p.nops * p.NT * p.KP * 128;
    const size_t o_PA = plan.take(p.lane ? 8 : (size_t)batch_sets * ftab * 8);
    res.take_sums(&p, (size_t)nmoves * R);
    // the groups of pruned nodes that walk side by side: enough workgroups to fill the device at
    // few sites, their level vectors within SPR_LEVEL_BYTES
    const size_t vec = p.lane ? (size_t)n * nsites * 8 : (size_t)s->nblocks * p.NT * 256 * 8;
    const int64_t wgs = p.lane ? (nsites + 255) / 256 : (int64_t)s->nblocks;
    int64_t G = (2048 + wgs - 1) / std::max<int64_t>(wgs, 1);
    G = std::min<int64_t>(G, (int64_t)(SPR_LEVEL_BYTES / std::max<size_t>((size_t)nlevels * vec, 1)));
    G = std::max<int64_t>(1, std::min<int64_t>(G, N - 1));
    const size_t o_S = plan.take((size_t)G * nlevels * vec);
    const size_t o_ops = plan.take((size_t)std::max<int64_t>(nplan, 1) * sizeof(spr_op));
    // the chunks of pruned nodes: the moves of a chunk by post_chunk_units (the rows go through the
    // transpose in slabs: no bound from a grid), a chunk never splits the moves of one pruned node
    const int64_t chunk_moves = post_chunk_units(plan, R * res.row_bytes(&p), 0, INT64_MAX, nmoves,
                                                 "RAOTEH_SPR_CHUNK_BYTES");
    std::vector<int32_t> chunks(1, 1);          // the first pruned node of every chunk, then nnodes
    int64_t max_moves = 1;
    for (int64_t c = 1, c0 = 1; c <= N; ++c)
        if (c == N || (c > c0 && first[(size_t)c + 1] - first[(size_t)c0] > chunk_moves)) {
            max_moves = std::max<int64_t>(max_moves, first[(size_t)c] - first[(size_t)c0]);
            if (c < N) chunks.push_back((int32_t)c);
            c0 = c;
        }
    chunks.push_back((int32_t)N);
    res.take_chunk(&p, (size_t)max_moves * R, (size_t)SPR_MAX_ROWS);
    // (the cap is checked here, before the host makes the plan)
    RT_TRY(post_begin(&p, recompute_transitions));
    // the plan of the walk (slots: by node here; n > 4 renumbers by step below)
    std::vector<spr_op> ops;
    ops.reserve((size_t)nplan);
    std::vector<int32_t> cut((size_t)(N + 1) * 4, 0);
    {
        std::vector<int32_t> ident((size_t)N), rank((size_t)N), stack((size_t)N + 1);
        for (int64_t v = 0; v < N; ++v) ident[(size_t)v] = (int32_t)v;
        for (int64_t c = 1; c < N; ++c) {
            tree.cut(c, radius);
            cut[(size_t)c * 4] = (int32_t)c;
            cut[(size_t)c * 4 + 1] = (int32_t)ops.size();
            spr_plan_one(tree, c, radius, first[(size_t)c], D, ident.data(), &ops, &rank, &stack);
            cut[(size_t)c * 4 + 2] = (int32_t)ops.size();
            cut[(size_t)c * 4 + 3] = first[(size_t)c];
        }
        cut[(size_t)N * 4 + 3] = (int32_t)nmoves;
        RT_REQUIRE((int64_t)ops.size() == nplan, "%s: the plan has %lld ops, %lld were counted", who,
                   (long long)ops.size(), (long long)nplan);
    }
    hipStream_t st = p.st;
    unsigned char *base = p.base;
    res.place(&p);
    if (MIX) RT_TRY(mix.begin(&p));
    if (PART) RT_TRY(part.begin(&p));
    double *d_val = res.d_val, *d_S = (double *)(base + o_S);
    double *d_PA = (double *)(base + o_PA);
    int *d_tab = (int *)(base + o_tab);
    int4 *d_cut = (int4 *)(base + o_cut), *d_ops = (int4 *)(base + o_ops);
    const std::vector<int32_t> internal = post_internal_nodes(&p);
    RT_TRY(grid.launch(&p, lengths.data()));
    RT_TRY(post_up(&p, internal.data(), !SETS));
    std::vector<int32_t> tab;
    post_tab_build(&p, nullptr, &tab);
    if (!p.lane) {                               // node -> step in the plan
        std::vector<int32_t> step_of((size_t)N, 0);
        for (int j = 0; j < p.nops; ++j) step_of[(size_t)p.x->ops[(size_t)j].node] = j;
        for (spr_op &op : ops) {
            op.i = step_of[(size_t)op.i];
            if (op.pi >= 0) op.pi = step_of[(size_t)op.pi];
            if (op.pw >= 0) op.pw = step_of[(size_t)op.pw];
        }
        for (int64_t c = 1; c < N; ++c) cut[(size_t)c * 4] = step_of[(size_t)c];
    }
    RT_HIP(hipMemcpyAsync(d_tab, tab.data(), tab.size() * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_cut, cut.data(), cut.size() * 4, hipMemcpyHostToDevice, st));
    if (!ops.empty())
        RT_HIP(hipMemcpyAsync(d_ops, ops.data(), ops.size() * sizeof(spr_op), hipMemcpyHostToDevice, st));
    if (!p.lane) {
        // the fragment tables: the resident P beside the resident P^T; the grid's (MIX: of every
        // set, each by one launch over the step table that spans the sets)
        if constexpr (SETS) {
            post_set_pt &PT = [&]() -> post_set_pt & {
                if constexpr (MIX) return mix.PT;
                else return part.PT;
            }();
            RT_TRY(PT.pack(&p));
            RT_TRY(rt_launch_pack_p(p.ctx, (int)n, p.NT, p.KP, (int)(batch_sets * p.nops),
                                    (const int *)(base + PT.o_tab), m->multi.d_P, d_PA));
            RT_TRY(setfrac.pack(&p, &grid, R));
        } else {
            RT_TRY(rt_launch_pack_p(p.ctx, (int)n, p.NT, p.KP, p.nops, p.d_ptab, m->d_P, d_PA));
            RT_TRY(post_fraction_pack(&p, &grid, R));
        }
    }
    // what set k's launches read and write (plain: the model's own, the batch's status)
    struct set_view {
        const double *P, *G, *PT, *PA, *GT, *GA;
        int *stat;
        double *tot, ck;
    };
    auto view_of = [&](int64_t k) {
        set_view v = {m->d_P, grid.d_G, p.d_PT, d_PA, grid.d_GT, grid.d_GT + (size_t)R * ftab,
                      p.d_status, nullptr, 1.0};
        if constexpr (MIX) {
            v.P = mix.P_of(&p, k); v.G = grid.G_of_set(&p, k);
            v.PT = mix.PT.of_set(k); v.PA = d_PA + (size_t)k * ftab;
            v.GT = p.lane ? nullptr : setfrac.T_of_set(k); v.GA = p.lane ? nullptr : setfrac.A_of_set(k);
            v.stat = mix.status_of(&p, k); v.tot = mix.tot_of(&p, k); v.ck = class_weights[k];
        }
        if constexpr (PART) {                    // (the tables of set 0: the kernels move on)
            v.P = m->multi.d_P; v.PT = part.PT.d_PT;
            v.GT = p.lane ? nullptr : setfrac.T_of_set(0); v.GA = p.lane ? nullptr : setfrac.A_of_set(0);
        }
        return v;
    };
    // what a PART instance adds per set: n <= 4 to P [set][node] and G [set][point][node], else to
    // the fragments [set][step] and [set][fraction][step]
    [[maybe_unused]] post_part_arg px = {};
    if constexpr (PART)
        px = p.lane ? part.arg((long)m->multi.P_stride, (long)((size_t)np * N * n * n))
                    : part.arg(part.pt_stride(), (long)((size_t)R * grid.tab));
    // the upward pass (MIX: under set k) and the `up` pass
    auto up_stage = [&](int64_t k) -> int {
        const set_view v = view_of(k);
        if (p.lane) {
            const int *d_ptab = p.d_ptab;
            RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                auto launch = [&](auto kernel, auto... part_arg) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)((nsites + 255) / 256)), dim3(256), 0, st,
                                       (int)N, (long)nsites, v.P, d_ptab, d_ptab + N, (const int *)d_tab,
                                       (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                                       s->block_sites, (const double *)m->d_root, p.d_L, p.d_M, p.d_D,
                                       v.stat, v.ck, v.tot, part_arg...);
                };
                if constexpr (PART)
                    launch(spr_lane_up_kernel<decltype(nv)::value, false, true, post_part_arg>, px);
                else launch(spr_lane_up_kernel<decltype(nv)::value, MIX>);
                return RT_OK;
            }));
        } else {
            const rt_sites *x = p.x;
            if (MIX) RT_TRY(post_up_set(&p, k, nullptr));
            RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
                constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
                auto launch = [&](auto kernel, auto... part_arg) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)x->nblocks), dim3(64 * NT), 0, st, v.PT,
                                       p.nops, (const int4 *)p.d_steps, (const int *)d_tab,
                                       (const double *)p.d_L, (const double *)p.d_M, p.d_D,
                                       (const double *)x->d_obs, (int)x->nobs, (const double *)m->d_root,
                                       (int)n, v.stat, (long)x->nsites, (long)x->nblocks, v.ck, v.tot,
                                       part_arg...);
                };
                if constexpr (PART) launch(spr_up_kernel<NT, KS, false, true, post_part_arg>, px);
                else launch(spr_up_kernel<NT, KS, MIX>);
                return RT_OK;
            }));
        }
        RT_HIP(hipGetLastError());
        return RT_OK;
    };
    // the walk of the pruned nodes cA .. cB - 1
    auto walk = [&](int64_t k, int cA, int cB, int mvA, unsigned groups, int first_set) -> int {
        const set_view v = view_of(k);
        if (p.lane) {
            const int *d_ptab = p.d_ptab;
            RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                auto launch = [&](auto kernel, auto... first) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)((nsites + 255) / 256), groups), dim3(256),
                                       0, st, (int)N, (long)nsites, v.P, v.G, R, d_ptab, d_ptab + N,
                                       (const int *)d_tab, (const int4 *)d_cut, (const int4 *)d_ops,
                                       (const void *)s->d_obs, s->compact_states, (int)s->nobs,
                                       s->block_sites, (const double *)m->d_root, (const double *)p.d_L,
                                       (const double *)p.d_M, (const double *)p.d_D, d_S, nlevels, cA,
                                       cB, mvA, d_val, v.stat, first...);
                };
                if constexpr (MIX) launch(spr_lane_kernel<decltype(nv)::value, true, false, int>, first_set);
                else if constexpr (PART)
                    launch(spr_lane_kernel<decltype(nv)::value, false, true, post_part_arg>, px);
                else launch(spr_lane_kernel<decltype(nv)::value>);
                return RT_OK;
            }));
        } else {
            const rt_sites *x = p.x;
            RT_TRY(post_dispatch<2, 32>(p.KS, [&](auto ks) {
                constexpr int KS = decltype(ks)::value, NT = (KS + 3) / 4;
                auto launch = [&](auto kernel, auto... first) {
                    hipLaunchKernelGGL(kernel, dim3((unsigned)x->nblocks, groups), dim3(64 * NT), 0, st,
                                       v.PT, v.PA, v.GT, v.GA, R, p.nops, (const int4 *)p.d_steps,
                                       (const int *)d_tab, (const int4 *)d_cut, (const int4 *)d_ops,
                                       (const double *)p.d_L, (const double *)p.d_M,
                                       (const double *)p.d_D, d_S, nlevels, (const double *)x->d_obs,
                                       (int)x->nobs, (const double *)m->d_root, (int)n, cA, cB, mvA,
                                       d_val, v.stat, (long)x->nsites, (long)x->nblocks, first...);
                };
                if constexpr (MIX) launch(spr_kernel<NT, KS, true, false, int>, first_set);
                else if constexpr (PART) launch(spr_kernel<NT, KS, false, true, post_part_arg>, px);
                else launch(spr_kernel<NT, KS>);
                return RT_OK;
            }));
        }
        RT_HIP(hipGetLastError());
        return RT_OK;
    };
    if (!MIX) RT_TRY(up_stage(0));
    bool have_ll = false;                        // (MIX: log Lambda_i and the status are in)
    for (size_t ch = 0; ch + 1 < chunks.size(); ++ch) {
        const int cA = chunks[ch], cB = chunks[ch + 1];
        const int mvA = first[(size_t)cA];
        const size_t rows = (size_t)(first[(size_t)cB] - mvA) * R;
        // (a chunk without moves: nothing, but the first one brings the mixture's likelihood)
        if (!rows && (!MIX || have_ll)) continue;
        const unsigned groups = (unsigned)std::min<int64_t>(G, cB - cA);
        // the pass; MIX: set by set (a set of weight zero is never live: not run, never read)
        int first_set = 1;
        // (PART: one launch, every tile under its own set)
        for (int64_t k = 0; k < (MIX ? batch_sets : 1); ++k) {
            if (MIX && !(class_weights[k] > 0.0)) continue;
            if (MIX) RT_TRY(up_stage(k));
            if (rows) RT_TRY(walk(k, cA, cB, mvA, groups, first_set));
            first_set = 0;
        }
        if (MIX && !have_ll) {
            RT_TRY(mix.post(&p));                // (log Lambda_i, the status)
            have_ll = true;
        }
        if (!rows) continue;
        if (MIX && (values || sums)) RT_TRY(mix.log_ratio(&p, rows, R, nullptr, d_val));
        // 3. the weighted site sums and the per-site array [site][nmoves][R]
        RT_TRY(res.chunk(&p, (size_t)mvA * R, rows));
    }
    if constexpr (PART) RT_TRY(res.finish(&p, status));
    else RT_TRY(res.finish(&p, status, loglik, mix.d_ll));
    return grid.result(&p);
}

}  // namespace

extern "C" int rt_sites_spr_scores(rt_model *m, rt_sites *s, int recompute_transitions,
                                   int64_t radius, int64_t nfractions, const double *fractions,
                                   double *values, double *sums, int32_t *status)
{
    return spr_read<false>("rt_sites_spr_scores", m, s, recompute_transitions, nullptr, radius,
                           nfractions, fractions, values, sums, nullptr, nullptr, status);
}

extern "C" int rt_sites_spr_scores_mixture(rt_model *m, rt_sites *s, int recompute_transitions,
                                           const double *class_weights, int64_t radius,
                                           int64_t nfractions, const double *fractions, double *values,
                                           double *sums, double *loglik, int32_t *status)
{
    return spr_read<true>("rt_sites_spr_scores_mixture", m, s, recompute_transitions, class_weights,
                          radius, nfractions, fractions, values, sums, nullptr, loglik, status);
}

extern "C" int rt_sites_spr_scores_partitioned(rt_model *m, rt_sites *s, int recompute_transitions,
                                               int64_t radius, int64_t nfractions,
                                               const double *fractions, double *values, double *sums,
                                               double *set_sums, int32_t *status)
{
    return spr_read<false, true>("rt_sites_spr_scores_partitioned", m, s, recompute_transitions, nullptr,
                                 radius, nfractions, fractions, values, sums, set_sums, nullptr, status);
}

