// The root combine of a root-halves batch (prune_mfma_combine_kernel of prune.hip, rt_jit_combine
// of jit.hip), ONE WAVE per 16-site tile: what the idle waves of an expm launch run for the batch
// the previous step left pending (expm.hip, rt_combine_args).  The stand-alone kernels give row
// tile m of a site tile to wave m and add the NT waves' sums through LDS; here the wave loops
// m = 0 .. NT - 1 itself with the statements of those kernels in their order, so the numbers are
// theirs bit for bit: x = ha * hb (* the root's observation), s = sum over r of w * fmax(x, 0) in
// r order, the two lane exchanges, tot = 0 + s_0 + s_1 + ..., then finish_site and wave_sum of
// site_epilogue.h as they do.  No LDS, no
// barrier.  Every load is issued before the first use.
template <int NT>
__device__ __forceinline__ void rt_combine_tile_body(const rt_combine_args &c, long tile)
{
    const int lane = threadIdx.x & 63;
    const double *ha = c.halfbuf + (size_t)tile * 2 * (NT * 256) + lane;
    double a[NT][4], b[NT][4], w[NT][4];
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            a[m][r] = ha[(m * 4 + r) * 64];
            b[m][r] = ha[NT * 256 + (m * 4 + r) * 64];
            const int row = 16 * m + 4 * r + (lane >> 4);
            w[m][r] = row < c.n ? c.root_w[row] : 0.0;
        }
    double x[NT][4];
#pragma unroll
    for (int m = 0; m < NT; ++m)
#pragma unroll
        for (int r = 0; r < 4; ++r) x[m][r] = a[m][r] * b[m][r];
    if (c.kroot >= 0) {                     // (uniform) the root's own observation
        const double *og = c.obs + (size_t)tile * c.K * (c.KP * 128) + lane * 2;
        double2 v[NT][2];
#pragma unroll
        for (int m = 0; m < NT; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = 2 * m + h;
                v[m][h] = make_double2(0.0, 0.0);
                if (q < c.KP) v[m][h] = *(const double2 *)(og + ((size_t)c.kroot * c.KP + q) * 128);
            }
#pragma unroll
        for (int m = 0; m < NT; ++m)
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                x[m][2 * h] *= v[m][h].x;
                x[m][2 * h + 1] *= v[m][h].y;
            }
    }
    double tot = 0.0;
    bool negative = false;                  // (of row tile 0: what the stand-alone kernels report)
#pragma unroll
    for (int m = 0; m < NT; ++m) {
        double s = 0.0;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int row = 16 * m + 4 * r + (lane >> 4);
            if (m == 0) negative |= (row < c.n) && (x[m][r] < 0.0);
            s += w[m][r] * fmax(x[m][r], 0.0);
        }
        s += __shfl_xor(s, 16, 64);
        s += __shfl_xor(s, 32, 64);
        tot += s;
    }
    const long site = tile * 16 + (lane & 15);
    double sum, nzero;
    finish_site(tot, negative, lane < 16 && site < c.nsites, c.loglik, c.status, site, sum, nzero);
    sum = wave_sum(sum);
    nzero = wave_sum(nzero);
    if (lane == 0) {
        // the batch's layout of partial sums: one entry per wave of the stand-alone kernel (the
        // interpreter's: the tile's value in wave 0's, zeros in the others) or one per tile
        double2 *p = (double2 *)c.partial + tile * c.wave_slots;
        p[0] = make_double2(sum, nzero);
        for (int mm = 1; mm < c.wave_slots; ++mm) p[mm] = make_double2(0.0, 0.0);
    }
}
