// What the downward passes over a RESIDENT batch share (posterior.hip, branch_expect.hip): the
// scratch plan, the step tables of the two layouts and the lane family's observation read.
#pragma once

#include "common.h"

namespace {

typedef double double4_t __attribute__((ext_vector_type(4)));

// byte offsets of the call's pieces in the context's scratch (256-byte aligned)
struct post_plan {
    size_t total = 0;
    size_t take(size_t bytes)
    {
        const size_t o = total;
        total += (bytes + 255) / 256 * 256;
        return o;
    }
};

// n > 4: steps[i] = {node, step of the parent, stream position of an observed leaf or -1,
// w_of_node[node]} in the schedule order of the split-M twin `x` (the root is the last step), and
// step -> node for rt_launch_pack_pt
inline int post_step_table(const rt_model *m, const rt_sites *x, const int *w_of_node,
                           std::vector<int32_t> *table, std::vector<int32_t> *step_node)
{
    const int64_t N = m->nnodes;
    const int nops = (int)x->ops.size();
    std::vector<int> step_of((size_t)N, -1);
    for (int i = 0; i < nops; ++i) step_of[(size_t)x->ops[(size_t)i].node] = i;
    RT_REQUIRE(nops == N && x->ops[(size_t)nops - 1].dst < 0, "unexpected schedule");
    table->assign((size_t)nops * 4, -1);
    step_node->assign((size_t)nops, 0);
    for (int i = 0; i < nops; ++i) {
        const rt_op &op = x->ops[(size_t)i];
        (*table)[(size_t)i * 4] = op.node;
        (*table)[(size_t)i * 4 + 1] = i + 1 < nops ? step_of[(size_t)m->parent[(size_t)op.node]] : 0;
        (*table)[(size_t)i * 4 + 2] = (op.pop < 0 && op.obs >= 0) ? op.obs : -1;
        (*table)[(size_t)i * 4 + 3] = w_of_node[(size_t)op.node];
        (*step_node)[(size_t)i] = op.node;
    }
    return RT_OK;
}

// n <= 4: [parent][stream position or -1][w_of_node] per node, in preorder
inline void post_lane_table(const rt_model *m, const rt_sites *s, const int *w_of_node,
                            std::vector<int32_t> *table)
{
    const int64_t N = m->nnodes;
    table->assign((size_t)3 * N, -1);
    for (int64_t v = 0; v < N; ++v) {
        (*table)[(size_t)v] = v ? m->parent[(size_t)v] : 0;
        (*table)[(size_t)2 * N + v] = w_of_node[(size_t)v];
    }
    for (const rt_op &op : s->ops)               // (the stream is in schedule order)
        if (op.obs >= 0) (*table)[(size_t)N + op.node] = op.obs;
}

// n <= 4: one lane per site.  The observation of stream position k from the batch's lane-family
// image (dense pairs, or one byte per leaf: a state or an allowed-set mask; passes.hip
// sets_from_lane_batch_kernel reads the same layouts).
template <int N>
__device__ inline void lane_obs(const void *obs, int compact, int K, int block_sites, long site, int k,
                                double (&x)[N])
{
    const long blk = site / block_sites;
    const int ln = (int)(site - blk * block_sites);
    if (compact) {
        const int KQ = (K + 3) / 4;
        const unsigned w = ((const unsigned *)obs)[((size_t)blk * KQ + (k >> 2)) * block_sites + ln];
        const unsigned b = (w >> (8 * (k & 3))) & 255u;
#pragma unroll
        for (int s = 0; s < N; ++s)
            x[s] = compact == 2 ? (double)((b >> s) & 1u) : (b >= (unsigned)N || b == (unsigned)s) ? 1.0 : 0.0;
    } else {
        constexpr int hp = ((N + 1) & ~1) / 2;
        const double *o = (const double *)obs + (((size_t)blk * K + k) * hp * block_sites + ln) * 2;
#pragma unroll
        for (int s = 0; s < N; ++s) x[s] = o[(size_t)(s >> 1) * block_sites * 2 + (s & 1)];
    }
}

}  // namespace
