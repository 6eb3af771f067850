// The text of the Taylor / Paterson-Stockmeyer kernel of expm.hip (template parameters NT, GLOBAL,
// SPLIT, WAVES; parameters as expm_taylor_kernel), included once per kernel signature:
// RT_EXPM_CARRY = 0: expm_taylor_kernel; 1: expm_taylor_carry_kernel, whose launch may carry a
// root combine (rt_combine_args comb, comb.halfbuf == nullptr: none).
{
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
    if (red.partial && blockIdx.x == gridDim.x - 1) {      // the carried reduction
        rt_reduce_partials_body(red.partial, red.npartials, red.totals, red.nsites);
        return;
    }
#if RT_EXPM_CARRY
    // The carried root combine of the previous step's batch (combine_body.inc).  The load of Q
    // and the 1-norm below use the first TPB threads only: waves 4..7 of every matrix workgroup
    // have nothing to do until the first barrier -- one global round trip and the norm -- and
    // the combine of a tile is one global round trip and a few dozen flops on the vector ALU,
    // with no LDS and no barrier.  Wave 4 + k of workgroup g takes tile g + k G (rt_carry_tile);
    // this comes before every early return.  Waves 0..3 skip it on a scalar branch.
    static_assert(WAVES == 8 && NT == 4, "the carrying forms: eight waves, 49 <= n <= 64");
    if (comb.halfbuf) {
        const int cw = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) - 4;
        if (cw >= 0) {
            const long G = (long)gridDim.x - (red.partial ? 1 : 0);
            const long tile = rt_carry_tile((long)blockIdx.x, cw, G, comb.nblocks16);
            if (tile >= 0) rt_combine_tile_body<4>(comb, tile);
        }
    }
#endif
    constexpr int RN = 16 * NT;
    constexpr int LD = RN + 1;
    constexpr int MSZ = RN * LD;
    __shared__ double colsum[RN];
    const int trace_on = rt_expm_trace_on;
    RT_EXPM_STAMP(0);
    double *B0 = GLOBAL ? scratch + (size_t)blockIdx.x * 4 * MSZ : (double *)smem;   // A
    double *B1 = B0 + MSZ;                     // A^2
    double *B2 = B1 + MSZ;                     // A^3
    double *B3 = B2 + MSZ;                     // T

    static_assert(!SPLIT || (NT == 4 && !GLOBAL), "two workgroups per matrix: 49 <= n <= 64");
    static_assert(WAVES == 4 || (WAVES == 8 && !GLOBAL && (NT == 3 || NT == 4)),
                  "two waves per SIMD: LDS-resident, 33 <= n <= 64");
    // threads of the elementwise loops; the load and the norm stay on the first TPB threads
    // (row groups of TPB / RN: the order of the column sums is part of the result)
    constexpr int NTH = 64 * WAVES;
    const int b = SPLIT ? (int)(blockIdx.x >> 1) : (int)blockIdx.x;
    const int half = SPLIT ? (int)(blockIdx.x & 1) : 0;      // which columns this workgroup stores
    const int tid = threadIdx.x;
    const int nn = n * n;
    const int KSn = (n + 3) / 4, NTn = (n + 15) / 16;      // of the n x n matrix (Pfrag)
    double *Pb = P + (long)b * nn;
    const int qi = qidx[b];
    const int step = step_of_node ? step_of_node[b] : -1;
    // LDS-resident sizes: rate matrix 0 is fetched before the workgroup knows which matrix
    // it uses (one rate matrix for all edges is the common case; the others fetch again), so
    // that the index and the matrix are one memory round trip, not two
    constexpr int RP0 = GLOBAL ? 1 : TPB / RN;
    constexpr int PER0 = GLOBAL ? 1 : (RN + RP0 - 1) / RP0;
    double q0[PER0];
    if (!GLOBAL) {
        const int jc = tid % RN, g = tid / RN;
#pragma unroll
        for (int u = 0; u < PER0; ++u) {
            const int i = g + u * RP0;
            q0[u] = (g < RP0 && i < n && jc < n) ? Q[i * n + jc] : 0.0;
        }
    }
    const double t_early = tt[b];
    if (qi < 0) {                              // root slot: zeros (_density.py:171)
        for (int e = tid; e < nn; e += NTH) Pb[e] = 0.0;
        if (info && tid == 0) { info[2 * b] = 0; info[2 * b + 1] = 0; }
        if (step >= 0 && frag_kind == 0)
            for (int e = tid; e < nn; e += NTH) Pfrag[(long)step * nn + e] = 0.0;
        if (step >= 0 && frag_kind == 1) {
            const int total = NTn * ((KSn + 1) / 2) * 128;
            for (int e = tid; e < total; e += NTH) Pfrag[(long)step * total + e] = 0.0;
            if (Pquad)
                for (int e = tid; e < KSn * KSn * 16; e += NTH)
                    Pquad[(long)step * rt_quad_stride(n) + e] = 0.0;
        }
        return;
    }
    const double *Qb = Q + (long)qi * nn;
    const double t = t_early;
    // A = Q t, zero-padded.  Thread = (column j, row group g): rows g, g + RP, ... of one
    // column -- consecutive threads read consecutive addresses, no index division, all of a
    // thread's loads in flight together (n <= 64: 16 of them), and the column's |.| sum
    // falls out of the registers: ||A||_1 = max column sum without re-reading LDS.
    double nrm = 0.0;
    if (!GLOBAL) {
        constexpr int RP = TPB / RN;                 // row groups (4 at RN = 64)
        constexpr int PER = (RN + RP - 1) / RP;      // rows per thread
        __shared__ double colpart[RP][RN];
        const int jc = tid % RN, g = tid / RN;
        const bool active = g < RP;
        double v[PER];
        double part = 0.0;
        if (qi > 0) {                                // (block-uniform)
#pragma unroll
            for (int u = 0; u < PER; ++u) {
                const int i = g + u * RP;
                q0[u] = (active && i < n && jc < n) ? Qb[i * n + jc] : 0.0;
            }
        }
#pragma unroll
        for (int u = 0; u < PER; ++u) v[u] = q0[u] * t;
#pragma unroll
        for (int u = 0; u < PER; ++u) {
            const int i = g + u * RP;
            if (active && i < RN) B0[i * LD + jc] = v[u];
            part += fabs(v[u]);
        }
        if (active) colpart[g][jc] = part;
        __syncthreads();
        if (tid < RN) {
            double sum = 0.0;
#pragma unroll
            for (int r = 0; r < RP; ++r) sum += colpart[r][tid];
            colsum[tid] = sum;
        }
        __syncthreads();
        // max over the RN <= 64 column sums: one value per lane and a butterfly (a loop of RN
        // dependent LDS reads per thread was a quarter of this phase)
        {
            const int ln = tid & 63;
            nrm = ln < RN ? colsum[ln] : 0.0;
#pragma unroll
            for (int o = 32; o > 0; o >>= 1) nrm = fmax(nrm, __shfl_xor(nrm, o, 64));
        }
    } else {
        constexpr int PER = (MSZ + TPB - 1) / TPB;
        for (int c0 = 0; c0 < PER; c0 += 8) {
            double v[8];
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = (c0 + u) * TPB + tid;
                const int i = e / LD, jx = e - i * LD;
                v[u] = (e < MSZ && i < n && jx < n) ? Qb[i * n + jx] * t : 0.0;
            }
#pragma unroll
            for (int u = 0; u < 8; ++u) {
                const int e = (c0 + u) * TPB + tid;
                if (e < MSZ) B0[e] = v[u];
            }
        }
        __syncthreads();
        // ||A||_1 = max column sum
        for (int jx = tid; jx < RN; jx += TPB) {
            double sum = 0.0;
            for (int i = 0; i < n; ++i) sum += fabs(B0[i * LD + jx]);
            colsum[jx] = sum;
        }
        __syncthreads();
        for (int jj = 0; jj < RN; ++jj) nrm = fmax(nrm, colsum[jj]);
    }
    RT_EXPM_STAMP(1);
    if (!(nrm < 1e300)) {                      // inf / NaN in Q * t (block-uniform)
        for (int e = tid; e < nn; e += NTH) Pb[e] = __builtin_nan("");
        if (info && tid == 0) { info[2 * b] = -1; info[2 * b + 1] = 0; }
        return;
    }
    int m = 15, s = 0;
    if (nrm <= c_theta_taylor[0]) m = 3;
    else if (nrm <= c_theta_taylor[1]) m = 6;
    else if (nrm <= c_theta_taylor[2]) m = 9;
    else if (nrm <= c_theta_taylor[3]) m = 12;
    else if (nrm > c_theta_taylor[4]) {
        int e;
        const double f = frexp(nrm / c_theta_taylor[4], &e);    // ratio = f * 2^e
        s = (f == 0.5) ? e - 1 : e;
        if (s < 0) s = 0;
    }
    m = __builtin_amdgcn_readfirstlane(m);
    s = __builtin_amdgcn_readfirstlane(s);
    if (info && tid == 0) { info[2 * b] = m; info[2 * b + 1] = s; }
    if (s > 0) {
        const double sc = ldexp(1.0, -s);
        for (int e = tid; e < MSZ; e += NTH) B0[e] *= sc;
        __syncthreads();
    }
    const int q = m / 3;
    RT_EXPM_STAMP(2);
    if constexpr (WAVES == 8) {
        const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
        int wm, wj, wn;
        wave8_tiles<NT>(wave, wm, wj, wn);
        constexpr int NCF = NT == 4 ? 2 : 0;       // column tiles per wave of a full product
        const double nd = (double)n;
        // (m, q block-uniform: the coefficients are scalar loads from constant memory)
        const double tops8[5] = {c_inv_fact[3 * (q - 1)], c_inv_fact[3 * (q - 1) + 1],
                                 c_inv_fact[3 * (q - 1) + 2], c_inv_fact[m], nd};
        double left[4 * NT];
        half_tiles ra, ra2;
        load_left8<NT>(B0, wm, left);
        load_tiles8<NT>(B0, ra, wm, wj, wn);
        mm8<NT, NCF>(left, B0, B1, wm, wj, wn, false, 0.0, 0.0, 0.0, nd, nullptr, nullptr,
                     &ra2);                                                 // A^2
        // A^3 and the top block T = B_(q-1), as below
        mm8<NT, NCF>(left, B1, B2, wm, wj, wn, false, 0.0, 0.0, 0.0, nd, &ra, &ra2, nullptr,
                     tops8, B3);
        RT_EXPM_STAMP(3);
        RT_EXPM_STAMP(4);
        if (q >= 2) load_left8<NT>(B2, wm, left);                 // A^3: every Horner step
        if (SPLIT && s == 0) {
            if constexpr (SPLIT) {
                const int hj = 2 * half + (wave & 1);
                half_tiles ha, ha2;
                load_tiles8<NT>(B0, ha, wm, hj, 1);
                load_tiles8<NT>(B1, ha2, wm, hj, 1);
#pragma unroll
                for (int u = 3; u >= 0; --u)
                    if (u <= q - 2)        // T[:, half] = A^3 T[:, half] + B_u
                        mm8<NT, 1>(left, B3, B3, wm, hj, 1, true, c_inv_fact[3 * u],
                                   c_inv_fact[3 * u + 1], c_inv_fact[3 * u + 2], nd, &ha, &ha2,
                                   nullptr, nullptr, nullptr,
                                   trace_on && blockIdx.x == 2 && u == 0);
            }
        } else {
            for (int jj = q - 2; jj >= 0; --jj)                             // T = A^3 T + B_j
                mm8<NT, NCF>(left, B3, B3, wm, wj, wn, true, c_inv_fact[3 * jj],
                             c_inv_fact[3 * jj + 1], c_inv_fact[3 * jj + 2], nd, &ra, &ra2);
        }
        RT_EXPM_STAMP(5);
        for (int r = 0; r < s; ++r) {              // T = T T: no constant operand
            load_left8<NT>(B3, wm, left);
            mm8<NT, NCF>(left, B3, B3, wm, wj, wn, false, 0.0, 0.0, 0.0, nd, nullptr, nullptr);
        }
    } else {
        lane_tiles<NT> ra, ra2;
        load_tiles<NT>(B0, ra);
        mm_blocked<NT>(B0, B0, B1, nullptr, nullptr, nullptr, nullptr, nullptr, &ra2);     // A^2
        // A^3, and with it T = B_(q-1) = c I + c A + c A^2 + c_m A^3 (the degree-m polynomial
        // is sum_{j<q} A^(3j) B_j plus c_m A^m, and c_m A^m = A^(3(q-1)) (c_m A^3): the top
        // block carries the A^3 term)
        __shared__ double tops[5];
        {
            const int base = 3 * (q - 1);
            if (tid == 0) {
                tops[0] = c_inv_fact[base];
                tops[1] = c_inv_fact[base + 1];
                tops[2] = c_inv_fact[base + 2];
                tops[3] = c_inv_fact[m];
                tops[4] = (double)n;
            }
            __syncthreads();
        }
        mm_blocked<NT>(B0, B1, B2, nullptr, nullptr, nullptr, &ra, &ra2, nullptr, tops, B3);
        RT_EXPM_STAMP(3);
        RT_EXPM_STAMP(4);
        // the coefficients of every Horner step at once (one barrier, not one per step)
        __shared__ double cfs_all[5][4];
        if (tid < 20) cfs_all[tid >> 2][tid & 3] = (tid & 3) == 3 ? (double)n
                                                                 : c_inv_fact[3 * (tid >> 2) + (tid & 3)];
        __syncthreads();
        if (SPLIT && s == 0) {
            if constexpr (SPLIT) {
                half_tiles ha, ha2;
                load_half_tiles(B0, ha, half);
                load_half_tiles(B1, ha2, half);
                // (the coefficients of all four possible steps in registers: block-uniform loads
                // from constant memory, long before they are needed)
                double hc[4][3];
#pragma unroll
                for (int u = 0; u < 4; ++u)
#pragma unroll
                    for (int e = 0; e < 3; ++e) hc[u][e] = c_inv_fact[3 * u + e];
                const double nd = (double)n;
#pragma unroll
                for (int u = 3; u >= 0; --u)
                    if (u <= q - 2)            // T[:, half] = A^3 T[:, half] + B_u
                        mm_half(B2, B3, B3, hc[u][0], hc[u][1], hc[u][2], nd, ha, ha2, half,
                                trace_on && blockIdx.x == 2 && u == 0);
            }
        } else {
            for (int jj = q - 2; jj >= 0; --jj)
                mm_blocked<NT>(B2, B3, B3, cfs_all[jj], B0, B1, &ra, &ra2);    // T = A^3 T + B_j
        }
        RT_EXPM_STAMP(5);
        for (int r = 0; r < s; ++r) mm_blocked<NT>(B3, B3, B3, nullptr, nullptr, nullptr);
    }
    RT_EXPM_STAMP(6);

    const double *Xb = B3;
    if constexpr (SPLIT) {
        // this workgroup's columns only: P in the reference's order, the A fragments of its
        // k-pairs (column c of P is k-step c / 4: columns 32 h .. 32 h + 31 = pairs 4 h .. 4 h + 3)
        const int jc = 32 * half + (tid & 31), g = tid >> 5;
        if (jc < n)
            for (int i = g; i < n; i += NTH / 32) Pb[i * n + jc] = Xb[i * LD + jc];
        if (step >= 0 && frag_kind == 1) {
            const int KP = (KSn + 1) / 2;
            const int total = NTn * KP * 128;
            for (int blk = tid >> 7; blk < NTn * 4; blk += NTH >> 7) {
                const int mm = blk >> 2, qq = 4 * half + (blk & 3);
                if (qq < KP) {
                    const int e = (mm * KP + qq) * 128 + (tid & 127);
                    const int e2 = e & 1;
                    const int ln = (e >> 1) & 63;
                    const int row = 16 * mm + (ln & 15);
                    const int col = 4 * (2 * qq + e2) + (ln >> 4);
                    Pfrag[(long)step * total + e] = (col < RN) ? Xb[row * LD + col] : 0.0;
                }
            }
        }
        RT_EXPM_STAMP(7);
        return;
    }
    if (!GLOBAL) {               // thread = (column, row group) as in the load: no division
        constexpr int RP = NTH / RN;
        const int jc = tid % RN, g = tid / RN;
        if (g < RP && jc < n)
            for (int i = g; i < n; i += RP) Pb[i * n + jc] = Xb[i * LD + jc];
    } else {
        for (int e = tid; e < nn; e += TPB) {
            const int i = e / n, j = e - i * n;
            Pb[e] = Xb[i * LD + j];
        }
    }
    if (step >= 0 && frag_kind == 0) {
        for (int e = tid; e < nn; e += NTH) {
            const int i = e / n, j = e - i * n;
            Pfrag[(long)step * nn + e] = Xb[i * LD + j];
        }
    } else if (step >= 0 && frag_kind == 1) {
        // Pfrag[step][m][q][lane][e2] = P[16m + (lane&15)][4(2q+e2) + (lane>>4)]; the
        // padding of Xb is zero, so no bounds check (KP pairs cover <= RN columns)
        const int KP = (KSn + 1) / 2;
        const int total = NTn * KP * 128;
        // 128 entries per (row tile, k-pair): the block index is wave-uniform arithmetic
        for (int blk = tid >> 7; blk < NTn * KP; blk += NTH >> 7) {
            const int e = blk * 128 + (tid & 127);
            const int e2 = e & 1;
            const int ln = (e >> 1) & 63;
            const int qq = blk % KP;
            const int mm = blk / KP;
            const int row = 16 * mm + (ln & 15);
            const int col = 4 * (2 * qq + e2) + (ln >> 4);
            Pfrag[(long)step * total + e] = (col < RN) ? Xb[row * LD + col] : 0.0;
        }
        if (Pquad) {
            // Pquad[step][rq][kk][k][i] = P[4 rq + i][4 kk + k] (the padding is zero)
            const int tq = KSn * KSn * 16;
            for (int e = tid; e < tq; e += NTH) {
                const int i = e & 3, k = (e >> 2) & 3, blk = e >> 4;
                const int row = 4 * (blk / KSn) + i, col = 4 * (blk % KSn) + k;
                Pquad[(long)step * rt_quad_stride(n) + e] = Xb[row * LD + col];
            }
        }
    }
    RT_EXPM_STAMP(7);
}
