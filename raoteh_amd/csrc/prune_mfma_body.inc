// Body of prune_mfma_kernel and, with RT_PART, of prune_mfma_part_kernel (prune.hip): one text,
// so that the kernels ordinary batches run compile exactly as before the per-tile lookup.
{
    // (a compile-time switch: as a run-time one the leaf path cost the dense instance 35 %)
    const int sparse = SPARSE ? sparse_mode : 0;
    // sparse (1: one observed state per leaf, 2: allowed sets of one or two; batches whose
    // `sparse_ok` holds): a leaf step is a gathered column of P (or two, added) from the model's
    // leaf-column table instead of an x exchange and KS MFMAs -- what the tree-specialised
    // kernels do (jit.hip), for the trees that have none: more than 600 steps, or not compiled yet.
    // Lout / Mout (optional): own rows of L_v and of the message M_v = P_v L_v of every step,
    // [step][tile][m][r][lane] -- what the downward pass and the site sums of the expectation
    // path read back (csrc/expect_mfma.hip)
    constexpr int WAVES = rt_split_waves(NT);
    constexpr int TILES = WAVES / NT;
    constexpr int KP = (KS + 1) / 2;           // k-step pairs
    constexpr int XB = NT * 4 * 64;            // doubles of one x exchange buffer
    extern __shared__ __attribute__((aligned(16))) unsigned char smem[];

    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int tile = wave / NT;
    const int m = wave - tile * NT;
    const bool halves = !STORE && hv.halfbuf != nullptr;
    const int half = halves ? (int)(blockIdx.x & 1) : 0;
    const long bidx = halves ? (long)(blockIdx.x >> 1) : (long)blockIdx.x;
    const long gt = bidx * TILES + tile;                   // global site tile
    const bool live = gt < nblocks16;
    const long blk = live ? gt : nblocks16 - 1;           // keep barriers uniform
#if RT_PART
    {
        const long gs = ((const RT_CONST_AS int *)gset)[blk];
        Pfrag += gs * gs_frag;
        if constexpr (SPARSE) Pcol += gs * gs_pcol;
    }
#endif
    if (halves) {
        nops = half ? hv.nops1 : hv.nops0;
        if (half) prog = hv.prog1;
    }
    const int rec0 = half ? hv.rec1 : 0;                   // P record of this program's step 0
    const int kobs0 = half ? hv.kobs1 : 0;                 // stream position of its first leaf

    double *xb = (double *)smem + tile * XB;               // [TILES][XB], single buffer
    double *red = (double *)smem + TILES * XB;             // [TILES][NT][16]
    // this wave's rows of the spilled accumulators: [slot][4][64], + lane
    unsigned char *stack = (unsigned char *)(red + TILES * NT * 16) +
                           (size_t)wave * lds_slots * 2048 + lane * 8;

    const RT_CONST_AS int4_t *prog_c = (const RT_CONST_AS int4_t *)prog;
    // A fragments of this wave: [op][m][q][lane][2]
    constexpr size_t ASTRIDE = (size_t)NT * KP * 128;
    const double *ag = Pfrag + (size_t)rec0 * ASTRIDE + ((size_t)m * KP * 64 + lane) * 2;
    // observation pairs holding this wave's own rows 4m..4m+3: q = 2m, 2m+1
    const double *og = obs + (size_t)blk * K * (KP * 128) + lane * 2;

    double an[2 * KP];            // A fragments of the NEXT step
    double on[4];                 // own rows of the next observation in the stream
#pragma unroll
    for (int j = 0; j < 4; ++j) on[j] = 1.0;

    int4_t op = prog_c[0];
    int knext = kobs0;            // stream position `on` holds / will hold
#pragma unroll
    for (int q = 0; q < KP; ++q) {
        const double2 v = *(const double2 *)(ag + q * 128);
        an[2 * q] = v.x;
        an[2 * q + 1] = v.y;
    }
    if (!SPARSE && knext < K) {
#pragma unroll
        for (int h = 0; h < 2; ++h) {
            const int q = 2 * m + h;
            double2 v = {0.0, 0.0};
            if (q < KP) v = *(const double2 *)(og + ((size_t)knext * KP + q) * 128);
            on[2 * h] = v.x;
            on[2 * h + 1] = v.y;
        }
    }

    double lik = 0.0;
    bool negative = false;
    double cur[4] = {1.0, 1.0, 1.0, 1.0};      // register-cached top accumulator
    int escale = 0;               // rescaling: exponent tally of this lane's site (lane & 15)

    // ---- sparse leaves: the state words (two in flight) and the gathered column of the NEXT
    // leaf step, requested when the step before it starts its products
    const int per_word = sparse == 2 ? 2 : 4;
    const int KW = (K + per_word - 1) / per_word;
    const unsigned *lwp = SPARSE ? leafw + (size_t)blk * KW * 16 + (lane & 15) : nullptr;
    const double4_t *pcm = (const double4_t *)Pcol + (4 * m + (lane >> 4));
    int lwidx = SPARSE ? kobs0 / per_word : 0;
    unsigned lwcur = 0, lwnext = 0;
    if constexpr (SPARSE) {
        lwcur = lwp[(size_t)lwidx * 16];
        lwnext = lwp[(size_t)(lwidx + 1 < KW ? lwidx + 1 : lwidx) * 16];
    }
    double4_t pcn = {0.0, 0.0, 0.0, 0.0}, pcq = {0.0, 0.0, 0.0, 0.0};
    bool pair_on = false;
    // the column(s) of the leaf whose step is program index `step`, stream position kpos
    auto gather = [&](int step, int kpos) {
        const int wq = kpos / per_word;
        if (wq != lwidx) {                       // (uniform) the next word becomes the current one
            lwcur = lwnext;
            lwidx = wq;
            lwnext = lwp[(size_t)(wq + 1 < KW ? wq + 1 : wq) * 16];
        }
        const int sh = sparse == 2 ? 16 * (kpos & 1) : 8 * (kpos & 3);
        const int sa = (int)((lwcur >> sh) & 255u);
        pcn = pcm[((size_t)(rec0 + step) * n + sa) * (4 * NT)];
        if (sparse == 2) {
            const int sb = (int)((lwcur >> (sh + 8)) & 255u);
            pair_on = sb != 255;
            pcq = pcm[((size_t)(rec0 + step) * n + (sb != 255 ? sb : sa)) * (4 * NT)];
        }
    };
    auto is_sleaf = [&](int f) { return SPARSE && !(f & LOP_INTERNAL) && (f & LOP_OBS); };
    if constexpr (SPARSE) {
        if (is_sleaf(op.x)) gather(0, kobs0);
    }

    for (int i = 0; i < nops; ++i) {
        const int flags = op.x;
        const bool sleaf = SPARSE && is_sleaf(flags);      // (uniform)
        // own rows of L_v = (accumulator of v) * (observation at v)
        double x[4];
        if (flags & LOP_INTERNAL) {
            if (flags & LOP_X_CUR) {
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = cur[r];
            } else {
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] = *(const double *)(stack + op.y + r * 512);
            }
            if (flags & LOP_OBS) {
#pragma unroll
                for (int r = 0; r < 4; ++r) x[r] *= on[r];
            }
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) x[r] = (flags & LOP_OBS) ? on[r] : 1.0;
        }
        if (flags & LOP_OBS) knext += 1;
        // (L of an observed leaf is its observation vector, which is resident already: the site
        // sums read it from there, expect_mfma.hip -- a quarter of this pass's stores)
        if (STORE && live && ((flags & LOP_INTERNAL) || !(flags & LOP_OBS))) {
            double *lo = Lout + ((size_t)i * nblocks16 + gt) * (NT * 256) + (m * 4) * 64 + lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) lo[r * 64] = x[r];
        }
        if (flags & LOP_ROOT) {
            if (halves) {
                // this program's share of the root's accumulator (the root's own observation
                // is the combine kernel's: the half programs' root step carries none)
                if (live) {
                    double *hb = hv.halfbuf + ((size_t)gt * 2 + half) * (NT * 256) + (m * 4) * 64 + lane;
#pragma unroll
                    for (int r = 0; r < 4; ++r) hb[r * 64] = x[r];
                }
                return;
            }
            double s = 0.0;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int row = 16 * m + 4 * r + (lane >> 4);
                const double w = row < n ? root_w[row] : 0.0;
                negative |= (row < n) && (x[r] < 0.0);
                s += w * fmax(x[r], 0.0);
            }
            s += __shfl_xor(s, 16, 64);
            s += __shfl_xor(s, 32, 64);
            if (lane < 16) red[(tile * NT + m) * 16 + lane] = s;
            __syncthreads();
            if (m == 0 && lane < 16) {
                double tot = 0.0;
#pragma unroll
                for (int mm = 0; mm < NT; ++mm) tot += red[(tile * NT + mm) * 16 + lane];
                lik = tot;
            }
            break;
        }
        double a[2 * KP];
        double4_t acc = {0.0, 0.0, 0.0, 0.0};
        if (SPARSE && sleaf) {
            // the message of this leaf: its column(s), requested one step ago (one rounding for
            // two columns, as the chain of the matrix pipe adds two non-zero terms)
            acc = pcn;
            if (sparse == 2 && pair_on) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = pcn[r] + pcq[r];
            }
        } else {
            __syncthreads();      // every wave is done reading the previous step's x
#pragma unroll
            for (int r = 0; r < 4; ++r) xb[((4 * m + r) * 64) + lane] = x[r];
#pragma unroll
            for (int j = 0; j < 2 * KP; ++j) a[j] = an[j];
            __syncthreads();      // x of every wave of the tile is in LDS
        }

        // start everything the next step needs
        const int inext = (i + 1 < nops) ? i + 1 : i;
        const int4_t opn = prog_c[inext];
        if (SPARSE && is_sleaf(opn.x)) {
            if constexpr (SPARSE) {
                if (inext != i) gather(inext, knext);
            }
        } else if (!(opn.x & LOP_ROOT)) {
#pragma unroll
            for (int q = 0; q < KP; ++q) {
                const double2 v = *(const double2 *)(ag + (size_t)inext * ASTRIDE + q * 128);
                an[2 * q] = v.x;
                an[2 * q + 1] = v.y;
            }
        }
        if (!SPARSE && (flags & LOP_OBS) && knext < K) {
#pragma unroll
            for (int h = 0; h < 2; ++h) {
                const int q = 2 * m + h;
                double2 v = {0.0, 0.0};
                if (q < KP) v = *(const double2 *)(og + ((size_t)knext * KP + q) * 128);
                on[2 * h] = v.x;
                on[2 * h + 1] = v.y;
            }
        }

        if (!sleaf) {
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) {
                const double b = xb[kk * 64 + lane];
                acc = __builtin_amdgcn_mfma_f64_16x16x4f64(a[kk], b, acc, 0, 0, 0);
            }
        }
        if (rescale && !sleaf) {
            // every wave of the tile sees all of x as its B operands: the site's largest
            // entry, the same number in every lane of the site and in every wave
            double xmax = 0.0;
#pragma unroll
            for (int kk = 0; kk < KS; ++kk) xmax = fmax(xmax, xb[kk * 64 + lane]);
            xmax = fmax(xmax, __shfl_xor(xmax, 16, 64));
            xmax = fmax(xmax, __shfl_xor(xmax, 32, 64));
            const int e = rescale_exponent(xmax);
            if (e != 0) {
#pragma unroll
                for (int r = 0; r < 4; ++r) acc[r] = ldexp(acc[r], -e);
                escale += e;
            }
        }
        if (STORE && live) {
            double *mo = Mout + ((size_t)i * nblocks16 + gt) * (NT * 256) + (m * 4) * 64 + lane;
#pragma unroll
            for (int r = 0; r < 4; ++r) mo[r * 64] = acc[r];
        }

        if (flags & LOP_FIRST) {
            if (flags & LOP_SPILL) {
#pragma unroll
                for (int r = 0; r < 4; ++r) *(double *)(stack + op.w + r * 512) = cur[r];
            }
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] = acc[r];
        } else if (flags & LOP_DST_CUR) {
#pragma unroll
            for (int r = 0; r < 4; ++r) cur[r] *= acc[r];
        } else if (flags & LOP_FAST) {     // un-spill: the parent's step is next
#pragma unroll
            for (int r = 0; r < 4; ++r)
                cur[r] = *(const double *)(stack + op.z + r * 512) * acc[r];
        } else {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                double *d = (double *)(stack + op.z + r * 512);
                *d = *d * acc[r];
            }
        }
        op = opn;
    }

    // lanes 0..15 of wave m == 0 own the 16 sites of the tile
    const long site = blk * 16 + (lane & 15);
    const bool valid = live && m == 0 && lane < 16 && site < nsites;
    double sum, nzero;
    finish_site(lik, negative, valid, loglik, status, site, sum, nzero, escale);
    sum = wave_sum(sum);
    nzero = wave_sum(nzero);
    if (lane == 0) {
        const long gwv = (long)blockIdx.x * WAVES + wave;
        partial[gwv * 2] = sum;
        partial[gwv * 2 + 1] = nzero;
    }
}
