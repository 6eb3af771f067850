// K rate sets against one resident batch (rt_step_multi): what follows the pruning launches.
//  - the K-fold reduce: workgroup k runs the fixed-order reduction of set k's per-wave partial
//    sums (reduce.h: the arithmetic of the batch's own reduction, so totals[k] has its bits);
//  - the weighted sums: sum_i w_i loglik[k][i] over the sites of non-zero likelihood, in two
//    stages whose shape depends on the number of sites only (bitwise reproducible);
//  - the per-site mixture over the sets, log sum_k c_k exp(loglik[k][i]).
#include "common.h"
#include "reduce.h"

namespace {

constexpr int WS_THREADS = 256;
constexpr int WS_SITES_PER_BLOCK = 4096;      // 16 sites per thread
constexpr int WS_MAX_BLOCKS = 256;

// fixed-order sum of one value per thread over a workgroup of 256 -> thread 0
__device__ __forceinline__ double block_sum_256(double v, double *sh)
{
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int w = 128; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    const double r = sh[0];
    __syncthreads();
    return r;
}

// stage 1: workgroup (b, k) sums a contiguous run of set k's sites, thread t every 256th of them
__global__ void __launch_bounds__(WS_THREADS)
multi_wsum_stage1_kernel(const double *__restrict__ loglik, const int *__restrict__ status,
                         long padded, long nsites, const double *__restrict__ weights,
                         int nblocks, double *__restrict__ wpart)
{
    __shared__ double sh[WS_THREADS];
    const int b = blockIdx.x, k = blockIdx.y;
    const long per = (nsites + nblocks - 1) / nblocks;
    const long lo = (long)b * per, hi = lo + per < nsites ? lo + per : nsites;
    const double *ll = loglik + (long)k * padded;
    const int *st = status + (long)k * padded;
    double acc = 0.0;
    for (long i = lo + threadIdx.x; i < hi; i += WS_THREADS) {
        if (st[i] & RT_SITE_ZERO_PROB) continue;
        acc += (weights ? weights[i] : 1.0) * ll[i];
    }
    const double r = block_sum_256(acc, sh);
    if (threadIdx.x == 0) wpart[(long)k * nblocks + b] = r;
}

// workgroup k: totals[k] from set k's partial sums, then stage 2 of its weighted sum
__global__ void __launch_bounds__(256)
multi_reduce_kernel(const double *__restrict__ partial, long npartials, double *__restrict__ totals,
                    double nsites, const double *__restrict__ wpart, int nblocks,
                    double *__restrict__ wsums)
{
    __shared__ double sh[WS_THREADS];
    const int k = blockIdx.x;
    rt_reduce_partials_body(partial + (long)k * npartials * 2, npartials, totals + 3 * k, nsites);
    __syncthreads();
    const double v = (int)threadIdx.x < nblocks ? wpart[(long)k * nblocks + threadIdx.x] : 0.0;
    const double r = block_sum_256(v, sh);
    if (threadIdx.x == 0) wsums[k] = r;
}

// one site per thread; logc[k] = log c_k (-inf: the set is out).  The workgroup leaves
// (sum of w_i value_i over its sites of non-zero likelihood, number of zero sites) in part[b]
__global__ void __launch_bounds__(256)
multi_mixture_kernel(int K, const double *__restrict__ logc, const double *__restrict__ loglik,
                     const int *__restrict__ status, long padded, long nsites,
                     const double *__restrict__ weights, double *__restrict__ out,
                     int *__restrict__ out_status, double *__restrict__ part)
{
    __shared__ double sh[256];
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    double contrib = 0.0, zero = 0.0;
    if (i < nsites) {
        const double ninf = -__builtin_huge_val();
        double mx = ninf;
        for (int k = 0; k < K; ++k) {
            const double lc = logc[k];
            if (lc == ninf || (status[(long)k * padded + i] & RT_SITE_ZERO_PROB)) continue;
            const double a = lc + loglik[(long)k * padded + i];
            mx = a > mx ? a : mx;
        }
        double val = ninf;
        if (mx > ninf) {
            double sum = 0.0;
            for (int k = 0; k < K; ++k) {
                const double lc = logc[k];
                if (lc == ninf || (status[(long)k * padded + i] & RT_SITE_ZERO_PROB)) continue;
                sum += exp(lc + loglik[(long)k * padded + i] - mx);
            }
            val = mx + log(sum);
            contrib = (weights ? weights[i] : 1.0) * val;
        } else {
            zero = 1.0;
        }
        out[i] = val;
        out_status[i] = mx > ninf ? RT_SITE_OK : RT_SITE_ZERO_PROB;
    }
    const double s = block_sum_256(contrib, sh);
    const double z = block_sum_256(zero, sh);
    if (threadIdx.x == 0) {
        part[2 * (long)blockIdx.x] = s;
        part[2 * (long)blockIdx.x + 1] = z;
    }
}

__global__ void __launch_bounds__(256)
multi_mixture_reduce_kernel(const double *__restrict__ part, long nparts, double *__restrict__ totals,
                            double nsites)
{
    rt_reduce_partials_body(part, nparts, totals, nsites);
}

}  // namespace

static int wsum_blocks(int64_t nsites)
{
    const int64_t b = (nsites + WS_SITES_PER_BLOCK - 1) / WS_SITES_PER_BLOCK;
    return (int)(b < 1 ? 1 : b > WS_MAX_BLOCKS ? WS_MAX_BLOCKS : b);
}

// doubles rt_multi_reduce_launch needs behind d_totals: [K][3] totals, [K] weighted sums,
// [K][blocks] stage-1 sums
int64_t rt_multi_totals_doubles(int64_t K, int64_t nsites)
{
    return K * (3 + 1 + wsum_blocks(nsites));
}

int rt_multi_reduce_launch(rt_ctx *ctx, int64_t K, const double *d_partial, int64_t npartials,
                           const double *d_loglik, const int32_t *d_status, int64_t padded,
                           int64_t nsites, const double *d_weights, double *d_totals,
                           double *d_wsums)
{
    const int nb = wsum_blocks(nsites);
    double *wpart = d_wsums + K;
    hipLaunchKernelGGL(multi_wsum_stage1_kernel, dim3((unsigned)nb, (unsigned)K), dim3(WS_THREADS), 0,
                       ctx->stream, d_loglik, (const int *)d_status, (long)padded, (long)nsites,
                       d_weights, nb, wpart);
    hipEvent_t ev = nullptr;
    rt_time_begin(ctx, RT_K_REDUCE, "reduce_partials_multi", &ev);
    RT_LAUNCH_TIMED(ctx, multi_reduce_kernel, dim3((unsigned)K), dim3(256), 0, d_partial,
                    (long)npartials, d_totals, (double)nsites, (const double *)wpart, nb, d_wsums);
    RT_HIP(hipGetLastError());
    rt_time_end(ctx, RT_K_REDUCE, ev);
    return RT_OK;
}

int rt_multi_mixture_launch(rt_ctx *ctx, int64_t K, const double *d_logc, const double *d_loglik,
                            const int32_t *d_status, int64_t padded, int64_t nsites,
                            const double *d_weights, double *d_out, int32_t *d_out_status,
                            double *d_partial, double *d_totals)
{
    const long nb = (long)((nsites + 255) / 256);
    hipLaunchKernelGGL(multi_mixture_kernel, dim3((unsigned)nb), dim3(256), 0, ctx->stream, (int)K,
                       d_logc, d_loglik, (const int *)d_status, (long)padded, (long)nsites, d_weights,
                       d_out, (int *)d_out_status, d_partial);
    hipLaunchKernelGGL(multi_mixture_reduce_kernel, dim3(1), dim3(256), 0, ctx->stream,
                       (const double *)d_partial, nb, d_totals, (double)nsites);
    RT_HIP(hipGetLastError());
    return RT_OK;
}
