// Body of prune_lane_kernel and, with RT_PART, of prune_lane_part_kernel (prune.hip): one text,
// so that the kernels ordinary batches run compile exactly as before the per-granule lookup.
{
#if RT_PART
    Pord += (long)((const RT_CONST_AS int *)gset)[blockIdx.x] * gstride;
#endif
    constexpr int NP = (N + 1) & ~1;
    constexpr int HP = NP / 2;                // 16-byte pairs per site
    // timing experiment only (RAOTEH_LANE_NOLOAD): skip the HBM stream
    const bool noload = depth_arg < 0;
    const int depth = noload ? -depth_arg : depth_arg;
    constexpr int WPB = PLDS ? 4 : 1;         // waves per workgroup
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const long gw = (long)blockIdx.x * WPB + wave;    // site block of this wave

    LaneCtx<N, PLDS, 1, RESC> C;
    unsigned char *stack_base = smem;
    if (PLDS) {
        double *pl = (double *)smem;
        for (int e = threadIdx.x; e < (nops + 1) * N * N; e += 256) pl[e] = Pord[e];
        stack_base = smem + (((size_t)(nops + 1) * N * N * 8 + 15) & ~(size_t)15);
        __syncthreads();
        if (gw >= nblocks) return;            // wave-uniform, after the only barrier
        C.P_l = pl;
    } else {
        C.P_l = nullptr;
    }
    const double2 *g = (const double2 *)obs + (size_t)gw * K * HP * 64 + lane;
    C.ops_c = (const RT_CONST_AS int4_t *)ops;
    C.P_c = (const RT_CONST_AS double *)Pord;
    C.w_c = (const RT_CONST_AS double *)root_w;
    C.stack[0] = stack_base + (size_t)wave * depth * N * 512 + lane * 8;
    C.nops = nops;
    C.nrec = nops;
    C.init();

    // prologue: R slots in flight
    double2 ring[R][HP];
#pragma unroll
    for (int j = 0; j < R; ++j) {
#pragma unroll
        for (int h = 0; h < HP; ++h) ring[j][h] = make_double2(1.0, 1.0);
        if (j < K && !noload) {
#pragma unroll
            for (int h = 0; h < HP; ++h) ring[j][h] = g[((size_t)j * HP + h) * 64];
        }
    }

    C.load_current();
    C.run_plain();
    for (int k0 = 0; k0 < K; k0 += R) {
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const int k = k0 + j;
            if (k < K) {              // wave-uniform; the current step consumes slot k
                double o[1][N];
#pragma unroll
                for (int q = 0; q < N; ++q)
                    o[0][q] = (q & 1) ? ring[j][q >> 1].y : ring[j][q >> 1].x;
                C.template step<true>(o);
                if (k + R < K && !noload) {
#pragma unroll
                    for (int h = 0; h < HP; ++h)
                        ring[j][h] = g[((size_t)(k + R) * HP + h) * 64];
                }
                C.run_plain();
            }
        }
    }

    const long site = gw * 64 + lane;
    double sum, nzero;
    finish_site(C.lik[0], C.negative[0], site < nsites, loglik, status, site, sum, nzero,
                C.escale[0]);
    sum = wave_sum(sum);
    nzero = wave_sum(nzero);
    if (lane == 0) {
        partial[gw * 2] = sum;
        partial[gw * 2 + 1] = nzero;
    }
}
