// Frechet derivative of the matrix exponential for 64 < n <= 128, without the order-2n block.
//
// expect.hip gets M_e = L(t_e Q_e^T, W_e) as the corner of exp([[A, W], [0, A]]), an expm of
// order 2n: 256 at 128 states, which no expm kernel here takes (the wide one keeps ONE order-128
// matrix in LDS).  The block exponential is [[X, L], [0, X]] with X = exp(A), and block upper
// triangular matrices of that shape multiply as pairs,
//     (X1, L1)(X2, L2) = (X1 X2, X1 L2 + L1 X2):
// three n x n products where the order-2n product does eight.  So the pair (X, L) is carried
// through the scaling and squaring around a Taylor polynomial of expm.hip's Taylor kernel:
//     (A, W) <- (t Q^T, W / |W| 2^-17) 2^-s        degree m = 3 q and s from |t Q^T|_1 alone
//     (A2, L2) = (A, W)^2,  (A3, L3) = (A, W)(A2, L2)
//     T = B_(q-1) + c_m (A3, L3),   T <- (A3, L3) T + B_j  (j = q - 2 .. 0),
//         B_j = (c_3j I + c_3j+1 A + c_3j+2 A2,  c_3j+1 W + c_3j+2 L2)
//     s times (X, L) <- (X X, X L + L X).
// W keeps expect.hip's scaling (largest entry 2^-17, undone in the contraction): L is linear in
// W, so its size is free, and it never enters the choice of m and s.
//
// One workgroup per edge, NT = ceil(n / 16) waves, wave w owns row tile w of every product
// C = X Y (+ addends):
//   X  its 16 rows as A operands in registers (4 NT doubles per lane), read from the edge's
//      scratch matrices (L2-resident: nine matrices of (16 NT)^2 doubles per edge, 1.2 MB at
//      128 states; the 126 edges of a tree are 145 MB, inside the Infinity Cache);
//   Y  the whole right operand staged in LDS (128 KB at NT = 8), shared by the waves: one
//      conflict-free ds_read_b64 per MFMA, against NT fetches of Y from L2 per product;
//   C  NT tiles of accumulators (4 NT doubles per lane), seeded with the addends.
// Every matrix is kept in B-fragment order, F(row, col) = (row / 4)(64 NT) + (col / 16) 64 +
// (row % 4) 16 + col % 16: the D layout of row tile w is rows 4 w .. 4 w + 3 of that image, so
// results are stored with plain coalesced stores and staging Y is a straight copy.  A wave
// reads and writes only its own rows of a left operand or a destination, and right operands are
// read from the LDS copy, so every product may run in place; one spare matrix (TMP) holds the
// first half of X1 L2 + L1 X2.  All sums are taken in a fixed order.
//
// Its own translation unit for the default MFMA register form (accumulators in the AGPR half
// of the file), as expm_wide.hip.
#include "common.h"

#include <cstdio>
#include <cstdlib>

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

// (the constants of expm.hip's Taylor kernel)
__constant__ double c_theta_taylor[5] = {1.3863479e-5, 9.0656564e-3, 8.9577602e-2,
                                         2.9961589e-1, 6.4108352e-1};
// 1 / i!, i = 0..15
__constant__ double c_inv_fact[16] = {
    1.0, 1.0, 0.5, 1.0 / 6.0, 1.0 / 24.0, 1.0 / 120.0, 1.0 / 720.0, 1.0 / 5040.0,
    1.0 / 40320.0, 1.0 / 362880.0, 1.0 / 3628800.0, 1.0 / 39916800.0, 1.0 / 479001600.0,
    1.0 / 6227020800.0, 1.0 / 87178291200.0, 1.0 / 1307674368000.0};

enum { FM_A = 0, FM_W, FM_A2, FM_L2, FM_A3, FM_L3, FM_TX, FM_TL, FM_TMP, FM_COUNT };

template <int NT>
struct pair_ops {
    static constexpr int TPB = 64 * NT, KS = 4 * NT, RS = 64 * NT, MS = KS * RS;

    // the right operand of the next products: Y (fragment order) -> LDS.  The barrier in front
    // also orders every wave's earlier stores to Y before the copy.
    static __device__ __forceinline__ void stage(double *Yl, const double *Y)
    {
        __syncthreads();
        for (int i = 2 * (int)threadIdx.x; i < MS; i += 2 * TPB)
            *(double2 *)(Yl + i) = *(const double2 *)(Y + i);
        __syncthreads();
    }

    // dst = X [Y in LDS] + c1 p1 + c2 p2 + c3 p3 + diag I, this wave's row tile (a null addend
    // is skipped; dst may be X or an addend)
    static __device__ __forceinline__ void mm(const double *Yl, double *dst, const double *X,
                                              const double *p1, double c1, const double *p2, double c2,
                                              const double *p3, double c3, double diag, int n)
    {
        const int lane = threadIdx.x & 63;
        const int w = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
        const int lr = lane & 15, lq = lane >> 4;
        // xop[kk] = X[16 w + lr][4 kk + lq]
        double xop[KS];
        {
            const double *xp = X + (4 * w + (lr >> 2)) * RS + (lr & 3) * 16 + lq;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) xop[kk] = xp[(kk >> 2) * 64 + 4 * (kk & 3)];
        }
        double4_t acc[NT];
        const int off0 = 4 * w * RS + lane;
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int off = off0 + r * RS + j * 64;
                double v = 0.0;
                if (p1) v = c1 * p1[off];
                if (p2) v = fma(c2, p2[off], v);
                if (p3) v = fma(c3, p3[off], v);
                const int row = 16 * w + 4 * r + lq, col = 16 * j + lr;
                if (row == col && row < n) v += diag;
                acc[j][r] = v;
            }
        const double *yp = Yl + lane;
        double bc[NT], bn[NT];
#pragma unroll
        for (int j = 0; j < NT; ++j) bc[j] = yp[j * 64];
#pragma unroll
        for (int kk = 0; kk < KS; ++kk) {
            const int kn = kk + 1 < KS ? kk + 1 : kk;
#pragma unroll
            for (int j = 0; j < NT; ++j) bn[j] = yp[kn * RS + j * 64];
#pragma unroll
            for (int j = 0; j < NT; ++j)
                acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(xop[kk], bc[j], acc[j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < NT; ++j) bc[j] = bn[j];
        }
#pragma unroll
        for (int j = 0; j < NT; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) dst[off0 + r * RS + j * 64] = acc[j][r];
    }
};

// scratch: [edge][FM_COUNT][(16 NT)^2]; the derivative is left in matrix FM_TL, scaled by
// 1 / scale[edge].  info (optional): {degree, squarings} per edge.
template <int NT>
__global__ void __launch_bounds__(64 * NT)
frechet_pair_kernel(int n, const double *__restrict__ Q, const int *__restrict__ qidx,
                    const double *__restrict__ tt, const double *__restrict__ W,
                    double *__restrict__ scratch, double *__restrict__ scale, int *__restrict__ info)
{
    using ops = pair_ops<NT>;
    constexpr int TPB = ops::TPB, RS = ops::RS, MS = ops::MS;
    extern __shared__ __attribute__((aligned(16))) double fw_sm[];
    double *Yl = fw_sm;                           // [4 NT][64 NT]
    __shared__ double red[TPB];
    const int e = blockIdx.x, tid = threadIdx.x;
    const int nn = n * n;
    const double *Qe = Q + (size_t)qidx[e] * nn;
    const double *We = W + (size_t)e * nn;
    const double t = tt[e];
    double *S = scratch + (size_t)e * FM_COUNT * MS;
    double *mA = S + FM_A * MS, *mW = S + FM_W * MS, *mA2 = S + FM_A2 * MS, *mL2 = S + FM_L2 * MS;
    double *mA3 = S + FM_A3 * MS, *mL3 = S + FM_L3 * MS, *mTX = S + FM_TX * MS, *mTL = S + FM_TL * MS;
    double *mTMP = S + FM_TMP * MS;
    // |t Q^T|_1: column c of t Q^T is row c of t Q (added in ascending order); max |W|
    double colsum = 0.0, mx = 0.0;
    if (tid < n)
        for (int r = 0; r < n; ++r) colsum += fabs(Qe[tid * n + r] * t);
    for (int k = tid; k < nn; k += TPB) mx = fmax(mx, fabs(We[k]));
    // block maximum, NaN kept (fmax drops it); TPB is not a power of two for NT = 5, 6, 7: the
    // tail is folded first
    constexpr int P2 = NT > 4 ? 256 : (NT > 2 ? 128 : 64);
    auto block_max = [&](double v) {
        red[tid] = v;
        __syncthreads();
        if (tid >= P2) {
            const double a = red[tid - P2], b = v;
            red[tid - P2] = (a != a || b != b) ? __builtin_nan("") : fmax(a, b);
        }
        __syncthreads();
        for (int h = P2 / 2; h > 0; h >>= 1) {
            if (tid < h) {
                const double a = red[tid], b = red[tid + h];
                red[tid] = (a != a || b != b) ? __builtin_nan("") : fmax(a, b);
            }
            __syncthreads();
        }
        const double out = red[0];
        __syncthreads();
        return out;
    };
    const double nrm = block_max(colsum);
    double sc = block_max(mx);
    if (!(sc > 0.0) || !(sc < 1e308 * 10.0)) sc = 1.0;
    sc = ldexp(sc, 17);
    if (!(sc < 1e308 * 10.0)) sc = ldexp(sc, -17);
    if (tid == 0) scale[e] = sc;
    if (!(nrm < 1e300)) {                         // inf / NaN in Q t (block-uniform)
        for (int i = tid; i < MS; i += TPB) mTL[i] = __builtin_nan("");
        if (info && tid == 0) { info[2 * e] = -1; info[2 * e + 1] = 0; }
        return;
    }
    int mdeg = 15, s = 0;
    if (nrm <= c_theta_taylor[0]) mdeg = 3;
    else if (nrm <= c_theta_taylor[1]) mdeg = 6;
    else if (nrm <= c_theta_taylor[2]) mdeg = 9;
    else if (nrm <= c_theta_taylor[3]) mdeg = 12;
    else if (nrm > c_theta_taylor[4]) {
        int ex;
        const double f = frexp(nrm / c_theta_taylor[4], &ex);    // ratio = f * 2^ex
        s = (f == 0.5) ? ex - 1 : ex;
        if (s < 0) s = 0;
    }
    mdeg = __builtin_amdgcn_readfirstlane(mdeg);
    s = __builtin_amdgcn_readfirstlane(s);
    if (info && tid == 0) { info[2 * e] = mdeg; info[2 * e + 1] = s; }
    const double sq = ldexp(1.0, -s), winv = 1.0 / sc;
    // (A, W) in fragment order, zero-padded: entry i is row 4 (i / RS) + (i % 64) / 16,
    // column 16 ((i % RS) / 64) + i % 16
    for (int i = tid; i < MS; i += TPB) {
        const int l = i & 63;
        const int row = 4 * (i / RS) + (l >> 4), col = 16 * ((i % RS) >> 6) + (l & 15);
        const bool in = row < n && col < n;
        const int rc = row < n ? row : n - 1, cc = col < n ? col : n - 1;
        const double a = Qe[cc * n + rc] * t * sq;             // t Q^T
        const double wv = We[rc * n + cc] * winv * sq;
        mA[i] = in ? a : 0.0;
        mW[i] = in ? wv : 0.0;
    }
    const int q = mdeg / 3;
    // The products as one list walked by one loop, so that the kernel holds ONE copy of the
    // product code (inlined at every step, the allocator spills):
    //   0..5     (A2, L2) = (A, W)(A, W), (A3, L3) = (A, W)(A2, L2)
    //   6        T = B_(q-1) + c_m (A3, L3): every lane the entries it wrote itself
    //   7..      T <- (A3, L3) T + B_j, three products a step, j = q - 2 .. 0
    //   then     (X, L) <- (X X, X L + L X), three products a squaring
    // Per product: the matrix to stage as the right operand first (-1: the one in LDS stays),
    // destination, left operand, up to three addends (-1: none) and the diagonal term.
    const int nhorner = 3 * (q - 1), total = 7 + nhorner + 3 * s;
    for (int i = 0; i < total; ++i) {
        int Y = -1, dst = 0, X = 0, p1 = -1, p2 = -1, p3 = -1;
        double c1 = 1.0, c2 = 0.0, c3 = 0.0, diag = 0.0;
        if (i == 6) {
            const int base = 3 * (q - 1);
            const double top0 = c_inv_fact[base], top1 = c_inv_fact[base + 1],
                         top2 = c_inv_fact[base + 2], top3 = c_inv_fact[mdeg];
            const int lane = tid & 63, w = tid >> 6;
            for (int j = 0; j < NT; ++j)
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int off = (4 * w + r) * RS + j * 64 + lane;
                    const int row = 16 * w + 4 * r + (lane >> 4), col = 16 * j + (lane & 15);
                    double x = top1 * mA[off];
                    x = fma(top2, mA2[off], x);
                    x = fma(top3, mA3[off], x);
                    if (row == col && row < n) x += top0;
                    double l = top1 * mW[off];
                    l = fma(top2, mL2[off], l);
                    l = fma(top3, mL3[off], l);
                    mTX[off] = x;
                    mTL[off] = l;
                }
            continue;
        }
        if (i < 6) {
            const bool cube = i >= 3;
            const int k = cube ? i - 3 : i;
            if (k == 0) { Y = cube ? FM_A2 : FM_A; dst = cube ? FM_A3 : FM_A2; X = FM_A; }
            else if (k == 1) { dst = cube ? FM_L3 : FM_L2; X = FM_W; }
            else { Y = cube ? FM_L2 : FM_W; dst = cube ? FM_L3 : FM_L2; X = FM_A; p1 = dst; }
        } else if (i < 7 + nhorner) {
            const int k = i - 7, jj = q - 2 - k / 3, sub = k % 3;
            const double b0 = c_inv_fact[3 * jj], b1 = c_inv_fact[3 * jj + 1], b2 = c_inv_fact[3 * jj + 2];
            if (sub == 0) { Y = FM_TX; dst = FM_TMP; X = FM_L3; }
            else if (sub == 1) { dst = FM_TX; X = FM_A3; p1 = FM_A; c1 = b1; p2 = FM_A2; c2 = b2; diag = b0; }
            else { Y = FM_TL; dst = FM_TL; X = FM_A3; p1 = FM_TMP; p2 = FM_W; c2 = b1; p3 = FM_L2; c3 = b2; }
        } else {
            const int sub = (i - 7 - nhorner) % 3;
            if (sub == 0) { Y = FM_TL; dst = FM_TMP; X = FM_TX; }
            else if (sub == 1) { Y = FM_TX; dst = FM_TL; X = FM_TL; p1 = FM_TMP; }
            else { dst = FM_TX; X = FM_TX; }
        }
        if (Y >= 0) ops::stage(Yl, S + Y * MS);
        ops::mm(Yl, S + dst * MS, S + X * MS, p1 >= 0 ? S + p1 * MS : nullptr, c1,
                p2 >= 0 ? S + p2 * MS : nullptr, c2, p3 >= 0 ? S + p3 * MS : nullptr, c3, diag, n);
    }
    (void)mTMP;
}

// one thread per (c, d): edges added in index order (fixed rounding); M_e = L_e scale[e]
__global__ void __launch_bounds__(256)
frechet_pair_contract_kernel(int n, int NT, int nedges, const double *__restrict__ Q,
                             const int *__restrict__ qidx, const double *__restrict__ t,
                             const double *__restrict__ scratch, const double *__restrict__ scale,
                             double *__restrict__ dwell, double *__restrict__ trans)
{
    const int k = blockIdx.x * 256 + threadIdx.x;
    const int nn = n * n;
    if (k >= nn) return;
    const int c = k / n, d = k - c * n;
    const size_t MS = (size_t)256 * NT * NT;
    const size_t at = (size_t)(c >> 2) * (64 * NT) + (d >> 4) * 64 + (c & 3) * 16 + (d & 15);
    const double *L = scratch + FM_TL * MS + at;
    double acc = 0.0, dw = 0.0;
#pragma unroll 8
    for (int e = 0; e < nedges; ++e) {
        const double q = Q[(size_t)qidx[e] * nn + k];
        const double Mcd = L[(size_t)e * FM_COUNT * MS] * scale[e];
        if (c == d) dw += t[e] * Mcd;
        if (q != 0.0) acc += t[e] * q * Mcd;
    }
    trans[k] = acc;
    if (c == d) dwell[c] = dw;
}

// rt_sites_branch_expectations: the derivative of every edge itself, transposed, unscaled and
// times the branch length, G[e][a][b] = t_e scale[e] M_e[b][a]  (M_e = L(t Q^T, C^T) = L(t Q, C)^T)
__global__ void __launch_bounds__(256)
frechet_pair_extract_kernel(int n, int NT, const double *__restrict__ t,
                            const double *__restrict__ scratch, const double *__restrict__ scale,
                            double *__restrict__ G)
{
    const int e = blockIdx.x;
    const int nn = n * n;
    const size_t MS = (size_t)256 * NT * NT;
    const double *L = scratch + ((size_t)e * FM_COUNT + FM_TL) * MS;
    const double f = t[e] * scale[e];
    for (int k = threadIdx.x; k < nn; k += 256) {
        const int a = k / n, b = k - a * n;      // M_e[b][a]: row b, column a of the fragment image
        G[(size_t)e * nn + k] = f * L[(size_t)(b >> 2) * (64 * NT) + (a >> 4) * 64 + (b & 3) * 16 + (a & 15)];
    }
}

}  // namespace

size_t rt_frechet_wide_scratch_doubles(int64_t n, int64_t nedges)
{
    const size_t nt = (size_t)((n + 15) / 16);
    return (size_t)nedges * FM_COUNT * 256 * nt * nt;
}

// 64 < n <= 128: the pair kernel on device-resident operands, asynchronously on the context's
// stream.  dS: rt_frechet_wide_scratch_doubles(n, nedges) doubles; dinfo (optional)
// int32[nedges][2] = {degree, squarings}.
int rt_frechet_wide_pairs_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dQ,
                                 const int32_t *dqidx, const double *dt, const double *dW, double *dS,
                                 double *dscale, int32_t *dinfo)
{
    RT_REQUIRE(n > 64 && n <= 128, "the pair kernel serves 64 < n <= 128 (n=%lld)", (long long)n);
    hipStream_t st = ctx->stream;
    const int nt = (int)((n + 15) / 16);
    const size_t lds = (size_t)256 * nt * nt * 8;
#define RT_FW(NTV)                                                                              \
    do {                                                                                        \
        RT_HIP(hipFuncSetAttribute((const void *)frechet_pair_kernel<NTV>,                      \
                                   hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));      \
        hipLaunchKernelGGL((frechet_pair_kernel<NTV>), dim3((unsigned)nedges), dim3(64 * NTV),  \
                           lds, st, (int)n, dQ, dqidx, dt, dW, dS, dscale, dinfo);              \
    } while (0)
    switch (nt) {
    case 5: RT_FW(5); break;
    case 6: RT_FW(6); break;
    case 7: RT_FW(7); break;
    default: RT_FW(8); break;
    }
#undef RT_FW
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// ... followed by the contraction over the edges
int rt_frechet_wide_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dQ,
                           const int32_t *dqidx, const double *dt, const double *dW, double *dS,
                           double *dscale, int32_t *dinfo, double *ddwell, double *dtrans)
{
    RT_TRY(rt_frechet_wide_pairs_device(ctx, n, nedges, dQ, dqidx, dt, dW, dS, dscale, dinfo));
    const int nt = (int)((n + 15) / 16);
    const size_t nn = (size_t)n * n;
    hipLaunchKernelGGL(frechet_pair_contract_kernel, dim3((unsigned)((nn + 255) / 256)), dim3(256), 0,
                       ctx->stream, (int)n, nt, (int)nedges, dQ, dqidx, dt, dS, dscale, ddwell, dtrans);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

// ... or by the derivatives themselves: dG [nedges][n][n], row = state at the parent
int rt_frechet_wide_extract_device(rt_ctx *ctx, int64_t n, int64_t nedges, const double *dt,
                                   const double *dS, const double *dscale, double *dG)
{
    hipLaunchKernelGGL(frechet_pair_extract_kernel, dim3((unsigned)nedges), dim3(256), 0, ctx->stream,
                       (int)n, (int)((n + 15) / 16), dt, dS, dscale, dG);
    RT_HIP(hipGetLastError());
    return RT_OK;
}
