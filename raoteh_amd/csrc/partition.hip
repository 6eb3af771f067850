// Partitioned likelihood (rt_sites_create_partitioned / rt_step_partitioned): what surrounds the
// pruning launch.
//  - rt_partition_plan: the host planner (partition_plan.h) behind the C ABI;
//  - the reductions: per set a fixed-order, two-stage sum over the slot-ordered loglik / status
//    of the batch -- log-likelihood sum, zero-probability count, site count, weighted sum -- with
//    the pad slots masked; the shape (workgroups per set, the run each one sums) comes from the
//    plan alone, so two calls give the same bits;
//  - the batch totals (the per-set totals added in set order) and the gather of loglik / status
//    into caller order, in one launch.
#include "common.h"
#include "partition_plan.h"

#include <algorithm>

namespace {

constexpr int PT_THREADS = 256;
constexpr int PT_SITES_PER_BLOCK = 4096;      // 16 slots per thread
constexpr int PT_MAX_BLOCKS = 256;            // (stage 2 reads one stage-1 sum per thread)

// fixed-order sums of four values per thread over a workgroup of 256 -> sh[q][0]
__device__ __forceinline__ void block_sum4_256(const double (&v)[4], double (*sh)[PT_THREADS])
{
#pragma unroll
    for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] = v[q];
    __syncthreads();
    for (int w = PT_THREADS / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) {
#pragma unroll
            for (int q = 0; q < 4; ++q) sh[q][threadIdx.x] += sh[q][threadIdx.x + w];
        }
        __syncthreads();
    }
}

// stage 1: workgroup (b, k) sums a contiguous piece of set k's run, thread t every 256th slot
__global__ void __launch_bounds__(PT_THREADS)
partition_stage1_kernel(const double *__restrict__ loglik, const int *__restrict__ status,
                        const unsigned char *__restrict__ is_pad, const long *__restrict__ order,
                        const long *__restrict__ run_begin, const double *__restrict__ weights,
                        int nblocks, double *__restrict__ part)
{
    __shared__ double sh[4][PT_THREADS];
    const int b = blockIdx.x, k = blockIdx.y;
    const long r0 = run_begin[k], r1 = run_begin[k + 1];
    const long per = (r1 - r0 + nblocks - 1) / nblocks;
    const long lo = r0 + (long)b * per, hi = lo + per < r1 ? lo + per : r1;
    double acc[4] = {0.0, 0.0, 0.0, 0.0};     // sum, zero-probability sites, sites, weighted sum
    for (long slot = lo + threadIdx.x; slot < hi; slot += PT_THREADS) {
        if (is_pad[slot]) continue;
        acc[2] += 1.0;
        if (status[slot] & RT_SITE_ZERO_PROB) {
            acc[1] += 1.0;
            continue;
        }
        const double ll = loglik[slot];
        acc[0] += ll;
        acc[3] += (weights ? weights[order[slot]] : 1.0) * ll;
    }
    block_sum4_256(acc, sh);
    if (threadIdx.x < 4) part[((long)k * nblocks + b) * 4 + threadIdx.x] = sh[threadIdx.x][0];
}

// stage 2: workgroup k adds set k's stage-1 sums -> totals[k][3], wsums[k]
__global__ void __launch_bounds__(PT_THREADS)
partition_stage2_kernel(const double *__restrict__ part, int nblocks, double *__restrict__ totals,
                        double *__restrict__ wsums)
{
    __shared__ double sh[4][PT_THREADS];
    const int k = blockIdx.x;
    double v[4] = {0.0, 0.0, 0.0, 0.0};
    if ((int)threadIdx.x < nblocks) {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[q] = part[((long)k * nblocks + threadIdx.x) * 4 + q];
    }
    block_sum4_256(v, sh);
    if (threadIdx.x < 3) totals[3 * k + threadIdx.x] = sh[threadIdx.x][0];
    if (threadIdx.x == 3) wsums[k] = sh[3][0];
}

// loglik / status into caller order (one site per thread); the first thread also adds the
// per-set totals in set order -> the batch's totals over its real sites
__global__ void __launch_bounds__(PT_THREADS)
partition_gather_kernel(const double *__restrict__ loglik, const int *__restrict__ status,
                        const long *__restrict__ slot_of_site, long nsites,
                        double *__restrict__ out, int *__restrict__ out_status,
                        const double *__restrict__ totals, int nsets,
                        double *__restrict__ batch_totals)
{
    const long i = (long)blockIdx.x * PT_THREADS + threadIdx.x;
    if (i < nsites) {
        const long slot = slot_of_site[i];
        out[i] = loglik[slot];
        out_status[i] = status[slot];
    }
    if (i == 0) {
        double t[3] = {0.0, 0.0, 0.0};
        for (int k = 0; k < nsets; ++k) {
#pragma unroll
            for (int q = 0; q < 3; ++q) t[q] += totals[3 * k + q];
        }
#pragma unroll
        for (int q = 0; q < 3; ++q) batch_totals[q] = t[q];
    }
}

}  // namespace

int rt_partition_stage1_blocks(int64_t longest_run)
{
    const int64_t b = (longest_run + PT_SITES_PER_BLOCK - 1) / PT_SITES_PER_BLOCK;
    return (int)(b < 1 ? 1 : b > PT_MAX_BLOCKS ? PT_MAX_BLOCKS : b);
}

// doubles behind rt_partition::d_totals: [nsets][3] totals, [nsets] weighted sums,
// [nsets][nblocks][4] stage-1 sums
int64_t rt_partition_totals_doubles(int64_t nsets, int nblocks)
{
    return nsets * (3 + 1 + 4 * (int64_t)nblocks);
}

int rt_partition_reduce_launch(rt_ctx *ctx, const rt_partition *part, const double *d_loglik,
                               const int32_t *d_status, const double *d_weights,
                               double *d_batch_totals)
{
    const int K = (int)part->nsets, nb = part->nblocks;
    double *totals = part->d_totals, *wsums = totals + 3 * K, *stage1 = wsums + K;
    hipLaunchKernelGGL(partition_stage1_kernel, dim3((unsigned)nb, (unsigned)K), dim3(PT_THREADS), 0,
                       ctx->stream, d_loglik, (const int *)d_status,
                       (const unsigned char *)part->d_is_pad, (const long *)part->d_order,
                       (const long *)part->d_run_begin, d_weights, nb, stage1);
    hipEvent_t ev = nullptr;
    rt_time_begin(ctx, RT_K_REDUCE, "reduce_partition", &ev);
    RT_LAUNCH_TIMED(ctx, partition_stage2_kernel, dim3((unsigned)K), dim3(PT_THREADS), 0,
                    (const double *)stage1, nb, totals, wsums);
    rt_time_end(ctx, RT_K_REDUCE, ev);
    hipLaunchKernelGGL(partition_gather_kernel, dim3((unsigned)((part->nsites + PT_THREADS - 1) / PT_THREADS)),
                       dim3(PT_THREADS), 0, ctx->stream, d_loglik, (const int *)d_status,
                       (const long *)part->d_slot_of_site, (long)part->nsites, part->d_loglik,
                       (int *)part->d_status, (const double *)totals, K, d_batch_totals);
    RT_HIP(hipGetLastError());
    return RT_OK;
}

extern "C" int rt_partition_plan(const int32_t *site_set, int64_t nsites, int64_t nsets,
                                 int64_t granule, int64_t capacity, int64_t *order,
                                 int64_t *slot_of_site, uint8_t *is_pad, int32_t *granule_set,
                                 int64_t *run_begin, int64_t *padded)
{
    RT_REQUIRE(site_set && padded, "null pointer");
    RT_REQUIRE(nsites >= 1 && nsets >= 1 && granule >= 1,
               "rt_partition_plan: nsites, nsets and the granule must be >= 1");
    rt_partition_layout plan;
    int64_t bad = -1;
    if (rt_partition_plan_build(site_set, nsites, nsets, granule, &plan, &bad) != 0) {
        rt_set_error("rt_partition_plan: site_set[%lld]=%d is outside 0..%lld", (long long)bad,
                     bad >= 0 ? (int)site_set[bad] : 0, (long long)nsets - 1);
        return RT_ERR_INVALID;
    }
    *padded = plan.padded;
    if (!order && !slot_of_site && !is_pad && !granule_set && !run_begin) return RT_OK;   // (the size only)
    RT_REQUIRE(capacity >= plan.padded, "rt_partition_plan: %lld slots needed, capacity %lld",
               (long long)plan.padded, (long long)capacity);
    if (order) std::copy(plan.order.begin(), plan.order.end(), order);
    if (slot_of_site) std::copy(plan.slot_of_site.begin(), plan.slot_of_site.end(), slot_of_site);
    if (is_pad) std::copy(plan.is_pad.begin(), plan.is_pad.end(), is_pad);
    if (granule_set) std::copy(plan.granule_set.begin(), plan.granule_set.end(), granule_set);
    if (run_begin) std::copy(plan.run_begin.begin(), plan.run_begin.end(), run_begin);
    return RT_OK;
}
