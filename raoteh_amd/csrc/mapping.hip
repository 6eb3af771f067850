// Stochastic mappings of every branch of a RESIDENT batch (rt_sites_sample_mappings): joint
// node states from the posterior (sample.hip's draws, left in scratch), then on every edge an
// endpoint-conditioned path by uniformization (Nielsen 2002; Hobolth & Stone 2009, section 2.3),
// reduced on the device to the linear history statistics of rt_sites_branch_expectations.
//
// With mu = max_c(-Q[c][c]), R = I + Q / mu and lam = mu t the law of the number of uniformized
// events k on an edge a -> b is pois(k; lam) (R^k)[a][b] / P[a][b], the states between the events
// are a bridge of the chain R, and the event times are uniform order statistics, whose spacings
// are normalised exponentials.  The sampling rule is pinned in include/raoteh_hip.h.
//
//   1. map_powers_*: R and its powers R^0 .. R^K per distinct rate matrix, stored TRANSPOSED
//      (T[m][b][c] = (R^m)[c][b]: the column a bridge pick needs is contiguous), plain f64;
//      map_pois_kernel: the Poisson weights of every edge.
//   2. n > 4: map_path_kernel, sample_down_kernel's layout: one wave per (16-site tile, draw),
//      the four lanes 16 g + j of site j hold states 4 k + g; the event count is a chunked scan
//      over k, every bridge pick two row gathers and the scan of sample_down_kernel.  The sites
//      of a wave draw different k: every loop with a cross-lane shuffle runs to the wave's
//      maximum, finished lanes are predicated; edges with k <= 1 everywhere skip the picks.
//      n <= 4: map_lane_kernel, one thread per (site, draw).
//   3. map_means_kernel: the sums over the draws in draw order.
//
// The draws go through the device in chunks (per-draw values and counts of a chunk live in
// scratch and cross PCIe only when asked for), so the scratch does not grow with ndraws beyond
// the node states.  Nothing of the batch is written.
#include "common.h"
#include "philox.h"
#include "post_common.h"

#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <vector>

namespace {

constexpr int BC_MAX = RT_MAX_BRANCH_COEFS;
constexpr int KCAP = RT_MAX_MAPPING_EVENTS;
constexpr unsigned char NO_STATE = 255;
constexpr unsigned long long BRANCH_STREAM = 1ull << 63;    // counters of the branch uniforms
constexpr size_t CHUNK_BYTES = (size_t)256 << 20;           // per-draw outputs of one chunk

// R[q] = I + Q[q] / mu[q] (row-major) and T[q][0] = I, T[q][1] = R^T
__global__ void __launch_bounds__(256)
map_powers_init_kernel(int n, const double *__restrict__ Q, const double *__restrict__ mu,
                       const long *__restrict__ powoff, double *__restrict__ R,
                       double *__restrict__ T)
{
    const int q = blockIdx.y, nn = n * n;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nn) return;
    const int r = k / n, c = k - r * n;
    const double m = mu[q];
    const double x = (r == c ? 1.0 : 0.0) + (m > 0.0 ? Q[(size_t)q * nn + k] / m : 0.0);
    R[(size_t)q * nn + k] = x;
    double *Tq = T + powoff[q];
    Tq[k] = r == c ? 1.0 : 0.0;
    Tq[(size_t)nn + c * n + r] = x;              // (every table holds at least R^0 and R^1)
}

// T[q][m][b][c] = sum_x T[q][m-1][x][c] R[q][x][b]  ((R^m)[c][b] = sum_x (R^(m-1))[c][x] R[x][b])
__global__ void __launch_bounds__(256)
map_powers_step_kernel(int n, int m, const int *__restrict__ Kq, const long *__restrict__ powoff,
                       const double *__restrict__ R, double *__restrict__ T)
{
    const int q = blockIdx.y, nn = n * n;
    if (m > Kq[q]) return;
    const int k = blockIdx.x * 256 + threadIdx.x;
    if (k >= nn) return;
    const int b = k / n, c = k - b * n;
    const double *prev = T + powoff[q] + (size_t)(m - 1) * nn;
    const double *Rq = R + (size_t)q * nn;
    double acc = 0.0;
    for (int x = 0; x < n; ++x) acc += prev[x * n + c] * Rq[x * n + b];
    T[powoff[q] + (size_t)m * nn + k] = acc;
}

// pois[v][k] = exp(-lam) lam^k / k!, k = 0 .. K_v, by the recurrence (lam <= 0: 1, 0, 0, ...)
__global__ void __launch_bounds__(256)
map_pois_kernel(int nnodes, int KS, const int *__restrict__ qidx, const double *__restrict__ t,
                const double *__restrict__ mu, const int *__restrict__ eK, double *__restrict__ pois)
{
    const int v = blockIdx.x * 256 + threadIdx.x;
    if (v < 1 || v >= nnodes) return;
    const double lam = mu[qidx[v]] * t[v];
    double *p = pois + (size_t)v * KS;
    const int K = eK[v];
    const bool some = lam > 0.0;
    double x = some ? exp(-lam) : 1.0;
    p[0] = x;
    for (int k = 1; k <= K; ++k) {
        x = some ? x * lam / (double)k : 0.0;
        p[k] = x;
    }
}

__device__ __forceinline__ int wave_max(int x)
{
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) x = max(x, __shfl_xor(x, o, 64));
    return x;
}

// the pick of sample_down_kernel: w[k] the weight of state 4 k + g of site j (lane 16 g + j), not
// negative; the first state in index order with w > 0 whose cumulative weight exceeds u * total,
// the last with w > 0 if rounding leaves none, -1 without a positive weight
template <int NC>
__device__ __forceinline__ int pick_chunked(const double (&w)[NC], double u, int g, int j)
{
    double cum[NC];
    double run = 0.0;
    int last = -1;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        double c = w[k];
        c += __shfl_xor(c, 16, 64);
        c += __shfl_xor(c, 32, 64);
        run += c;
        cum[k] = run;
        if (w[k] > 0.0) last = 4 * k + g;
    }
    last = max(last, __shfl_xor(last, 16, 64));
    last = max(last, __shfl_xor(last, 32, 64));
    const double target = u * run;
    int ks = -1;
    double base = 0.0, wsel = 0.0;
#pragma unroll
    for (int k = 0; k < NC; ++k) {
        const bool hit = ks < 0 && cum[k] > target;
        if (hit) {
            ks = k;
            base = k ? cum[k - 1] : 0.0;
            wsel = w[k];
        }
    }
    int pick = -1, lastg = -1;
    double acc = base;
#pragma unroll
    for (int gg = 0; gg < 4; ++gg) {
        const double wg = __shfl(wsel, 16 * gg + j, 64);
        acc += wg;
        if (wg > 0.0) {
            lastg = gg;
            if (pick < 0 && acc > target) pick = gg;
        }
    }
    if (pick < 0) pick = lastg;
    return ks >= 0 ? 4 * ks + pick : last;
}

// what the two path kernels read besides the draws
struct map_tables {
    const int *parent, *qidx, *eK;       // [nnodes]
    const double *t;                     // [nnodes]
    const long *powoff;                  // [nq] doubles into T
    const double *R, *T, *pois, *E;      // [nq][n][n], powers, [nnodes][KS], [nk][n][n]
    int KS, nk;
};

// n > 4.  grid: tiles * nd workgroups of one wave; draw d_begin + blockIdx / tiles of the call.
// values [nd][nsites][nnodes][nk], counts [nd][nsites][nnodes][2] or null: those of this chunk.
template <int NT>
__global__ void __launch_bounds__(64)
map_path_kernel(map_tables tb, int n, int nnodes, long nsites, long tiles,
                unsigned long long seed, unsigned long long first_draw, long d_begin,
                const unsigned char *__restrict__ states, double *__restrict__ values,
                int *__restrict__ counts, int *__restrict__ status)
{
    constexpr int NC = 4 * NT;
    const int lane = threadIdx.x;
    const int g = lane >> 4, j = lane & 15;
    const long tile = (long)(blockIdx.x % (unsigned long)tiles);
    const long dl = (long)(blockIdx.x / (unsigned long)tiles);
    const long site = tile * 16 + j;
    const bool site_ok = site < nsites;
    const unsigned long long draw = first_draw + (unsigned long long)(d_begin + dl);
    const unsigned char *srow = states + ((size_t)(d_begin + dl) * nsites + (site_ok ? site : 0)) * nnodes;
    const size_t out0 = ((size_t)dl * nsites + (site_ok ? site : 0)) * nnodes;
    const int nn = n * n, nk = tb.nk;
    const int c0 = g, c1 = g + 4;                // this lane's coefficient matrices
    const double *E0 = tb.E + (size_t)(c0 < nk ? c0 : 0) * nn;
    const double *E1 = tb.E + (size_t)(c1 < nk ? c1 : 0) * nn;
    int flags = 0;
    if (site_ok) {                               // the root's slot
        if (c0 < nk) values[out0 * nk + c0] = 0.0;
        if (c1 < nk) values[out0 * nk + c1] = 0.0;
        if (counts && g == 0) *(int2 *)(counts + out0 * 2) = make_int2(0, 0);
    }
    for (int v = 1; v < nnodes; ++v) {
        const int q = tb.qidx[v], Kv = tb.eK[v];
        const double tv = tb.t[v];
        const double *Rq = tb.R + (size_t)q * nn;
        const double *Tq = tb.T + tb.powoff[q];
        const double *po = tb.pois + (size_t)v * tb.KS;
        int a = site_ok ? srow[tb.parent[v]] : NO_STATE;
        int b = site_ok ? srow[v] : NO_STATE;
        bool live = a != NO_STATE && b != NO_STATE;
        if (!live) a = b = 0;
        const unsigned long long cb = BRANCH_STREAM +
            ((unsigned long long)site * (unsigned long long)nnodes + (unsigned long long)v) * 2048ull;
        // 1. the event count: weights pois[k] (R^k)[a][b], k = 4 kk + g
        const double *cell = Tq + (size_t)b * n + a;
        const int nch = (Kv + 4) >> 2;
        double total = 0.0;
        int lastk = -1;
        for (int kk = 0; kk < nch; ++kk) {
            const int k = 4 * kk + g;
            double w = k <= Kv ? po[k] * cell[(size_t)k * nn] : 0.0;
            w = w > 0.0 ? w : 0.0;
            if (w > 0.0) lastk = k;
            w += __shfl_xor(w, 16, 64);
            w += __shfl_xor(w, 32, 64);
            total += w;
        }
        lastk = max(lastk, __shfl_xor(lastk, 16, 64));
        lastk = max(lastk, __shfl_xor(lastk, 32, 64));
        if (live && !(total > 0.0 && total < INFINITY)) {
            live = false;
            flags |= 4;
        }
        const double target = philox_uniform(seed, draw, cb) * total;
        int kev = -1;
        double run = 0.0;
        for (int kk = 0; kk < nch; ++kk) {
            const int k = 4 * kk + g;
            double w = k <= Kv ? po[k] * cell[(size_t)k * nn] : 0.0;
            w = w > 0.0 ? w : 0.0;
            double c = w;
            c += __shfl_xor(c, 16, 64);
            c += __shfl_xor(c, 32, 64);
            double acc = run;
            int pick = -1, lastg = -1;
#pragma unroll
            for (int gg = 0; gg < 4; ++gg) {
                const double wg = __shfl(w, 16 * gg + j, 64);
                acc += wg;
                if (wg > 0.0) {
                    lastg = gg;
                    if (pick < 0 && acc > target) pick = gg;
                }
            }
            run += c;
            if (kev < 0 && run > target) kev = 4 * kk + (pick >= 0 ? pick : lastg);
            if (__all(kev >= 0)) break;          // (uniform: every site of the wave has its count)
        }
        if (kev < 0) kev = lastk;                // rounding left none: the last positive weight
        if (!live) kev = 0;
        // 2., 3. the states between the events and the dwell times, to the wave's largest count
        const int kmax = wave_max(kev);
        int x = a, changes = 0;
        double sum_e = 0.0, dw0 = 0.0, dw1 = 0.0, jm0 = 0.0, jm1 = 0.0;
        for (int l = 0; l <= kmax; ++l) {
            const bool act = live && l <= kev;
            const double e = -log1p(-philox_uniform(seed, draw, cb + 1024ull + (unsigned long long)l));
            if (act) {
                sum_e += e;
                dw0 += E0[x * n + x] * e;
                dw1 += E1[x * n + x] * e;
            }
            if (l < kmax) {
                int nx = b;
                if (l + 1 < kmax) {              // (uniform) some site has an inner state to pick
                    const bool need = act && l + 1 < kev;
                    const double *r1 = Rq + (size_t)(need ? x : 0) * n;
                    const double *r2 = Tq + (size_t)(need ? kev - (l + 1) : 0) * nn + (size_t)b * n;
                    double w[NC];
#pragma unroll
                    for (int k = 0; k < NC; ++k) {
                        const int row = 4 * k + g;
                        const double y = (need && row < n) ? r1[row] * r2[row] : 0.0;
                        w[k] = y > 0.0 ? y : 0.0;
                    }
                    const double u = philox_uniform(seed, draw, cb + (unsigned long long)(l + 1));
                    const int pk = pick_chunked<NC>(w, u, g, j);
                    if (need && pk >= 0) nx = pk;
                }
                if (act && l < kev) {
                    if (nx != x) {
                        jm0 += E0[x * n + nx];
                        jm1 += E1[x * n + nx];
                        ++changes;
                    }
                    x = nx;
                }
            }
        }
        // 4. the statistics of the edge
        double v0 = 0.0, v1 = 0.0;
        if (live) {
            if (sum_e > 0.0) {
                const double sc = tv / sum_e;
                v0 = dw0 * sc + jm0;
                v1 = dw1 * sc + jm1;
            } else {                             // every spacing 0: the whole length in x_0
                v0 = E0[a * n + a] * tv + jm0;
                v1 = E1[a * n + a] * tv + jm1;
            }
        } else {
            kev = changes = 0;
        }
        if (site_ok) {
            const size_t o = out0 + v;
            if (c0 < nk) values[o * nk + c0] = v0;
            if (c1 < nk) values[o * nk + c1] = v1;
            if (counts && g == 0) *(int2 *)(counts + o * 2) = make_int2(kev, changes);
        }
    }
    if (flags && g == 0 && site_ok) atomicOr(&status[site], flags);
}

// n <= 4: one thread per (site, draw of the chunk); the same rule with sequential sums
template <int N>
__global__ void __launch_bounds__(256)
map_lane_kernel(map_tables tb, int nnodes, long nsites, long nd, unsigned long long seed,
                unsigned long long first_draw, long d_begin,
                const unsigned char *__restrict__ states, double *__restrict__ values,
                int *__restrict__ counts, int *__restrict__ status)
{
    const long tix = (long)blockIdx.x * 256 + threadIdx.x;
    if (tix >= nsites * nd) return;
    const long dl = tix / nsites;
    const long site = tix - dl * nsites;
    const unsigned long long draw = first_draw + (unsigned long long)(d_begin + dl);
    const unsigned char *srow = states + ((size_t)(d_begin + dl) * nsites + site) * nnodes;
    const size_t out0 = ((size_t)dl * nsites + site) * nnodes;
    constexpr int nn = N * N;
    const int nk = tb.nk;
    int flags = 0;
    for (int c = 0; c < nk; ++c) values[out0 * nk + c] = 0.0;
    if (counts) *(int2 *)(counts + out0 * 2) = make_int2(0, 0);
    for (int v = 1; v < nnodes; ++v) {
        const int q = tb.qidx[v], Kv = tb.eK[v];
        const double tv = tb.t[v];
        const double *Rq = tb.R + (size_t)q * nn;
        const double *Tq = tb.T + tb.powoff[q];
        const double *po = tb.pois + (size_t)v * tb.KS;
        const size_t o = out0 + v;
        const int a = srow[tb.parent[v]], b = srow[v];
        bool live = a != NO_STATE && b != NO_STATE;
        int kev = 0, changes = 0;
        double val[BC_MAX];
#pragma unroll
        for (int c = 0; c < BC_MAX; ++c) val[c] = 0.0;
        if (live) {
            const unsigned long long cb = BRANCH_STREAM +
                ((unsigned long long)site * (unsigned long long)nnodes + (unsigned long long)v) * 2048ull;
            const double *cell = Tq + b * N + a;
            double total = 0.0;
            int lastk = -1;
            for (int k = 0; k <= Kv; ++k) {
                const double w = po[k] * cell[(size_t)k * nn];
                if (w > 0.0) {
                    total += w;
                    lastk = k;
                }
            }
            if (!(total > 0.0 && total < INFINITY)) {
                live = false;
                flags |= 4;
            } else {
                const double target = philox_uniform(seed, draw, cb) * total;
                double run = 0.0;
                kev = -1;
                for (int k = 0; k <= Kv; ++k) {
                    const double w = po[k] * cell[(size_t)k * nn];
                    if (w > 0.0) {
                        run += w;
                        if (run > target) {
                            kev = k;
                            break;
                        }
                    }
                }
                if (kev < 0) kev = lastk;
                int x = a;
                double sum_e = 0.0, dw[BC_MAX], jm[BC_MAX];
#pragma unroll
                for (int c = 0; c < BC_MAX; ++c) dw[c] = jm[c] = 0.0;
                for (int l = 0; l <= kev; ++l) {
                    const double e = -log1p(-philox_uniform(seed, draw, cb + 1024ull + (unsigned long long)l));
                    sum_e += e;
#pragma unroll
                    for (int c = 0; c < BC_MAX; ++c)
                        if (c < nk) dw[c] += tb.E[(size_t)c * nn + x * N + x] * e;
                    if (l < kev) {
                        int nx = b;
                        if (l + 1 < kev) {
                            const double *r1 = Rq + x * N;
                            const double *r2 = Tq + (size_t)(kev - (l + 1)) * nn + b * N;
                            double w[N], tot = 0.0;
#pragma unroll
                            for (int s = 0; s < N; ++s) {
                                const double y = r1[s] * r2[s];
                                w[s] = y > 0.0 ? y : 0.0;
                                tot += w[s];
                            }
                            const double tg = philox_uniform(seed, draw, cb + (unsigned long long)(l + 1)) * tot;
                            int pick = -1, last = -1;
                            double acc = 0.0;
#pragma unroll
                            for (int s = 0; s < N; ++s) {
                                acc += w[s];
                                if (w[s] > 0.0) {
                                    last = s;
                                    if (pick < 0 && acc > tg) pick = s;
                                }
                            }
                            if (pick < 0) pick = last;
                            if (pick >= 0) nx = pick;
                        }
                        if (nx != x) {
#pragma unroll
                            for (int c = 0; c < BC_MAX; ++c)
                                if (c < nk) jm[c] += tb.E[(size_t)c * nn + x * N + nx];
                            ++changes;
                        }
                        x = nx;
                    }
                }
                const double sc = sum_e > 0.0 ? tv / sum_e : 0.0;
#pragma unroll
                for (int c = 0; c < BC_MAX; ++c)
                    if (c < nk)
                        val[c] = (sum_e > 0.0 ? dw[c] * sc : tb.E[(size_t)c * nn + a * N + a] * tv) + jm[c];
            }
        }
        if (!live) kev = changes = 0;
#pragma unroll
        for (int c = 0; c < BC_MAX; ++c)
            if (c < nk) values[o * nk + c] = live ? val[c] : 0.0;
        if (counts) *(int2 *)(counts + o * 2) = make_int2(kev, changes);
    }
    if (flags) atomicOr(&status[site], flags);
}

// means[idx] (+)= values[0][idx] + values[1][idx] + ... in draw order; the last chunk divides
__global__ void __launch_bounds__(256)
map_means_kernel(long cells, long nd, int first, int last, double ndraws,
                 const double *__restrict__ values, double *__restrict__ means)
{
    const long idx = (long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= cells) return;
    double acc = first ? 0.0 : means[idx];
    for (long d = 0; d < nd; ++d) acc += values[(size_t)d * cells + idx];
    means[idx] = last ? acc / ndraws : acc;
}

}  // namespace

extern "C" int rt_sites_sample_mappings(rt_model *m, rt_sites *s, int recompute_transitions,
                                        uint64_t seed, uint64_t first_draw, int64_t ndraws,
                                        int64_t n_coefs, const double *coefs, uint8_t *states,
                                        double *values, int32_t *counts, double *means,
                                        int32_t *status)
{
    static const char who[] = "rt_sites_sample_mappings";
    post_pass p;                                 // (host buffers: alive until the synchronisation)
    RT_TRY(post_open(&p, who, m, s));
    RT_REQUIRE(ndraws >= 1, "ndraws must be at least 1");
    RT_REQUIRE(n_coefs >= 1 && coefs, "at least one coefficient matrix is needed");
    RT_REQUIRE(m->d_Q && !m->spectral,
               "rt_sites_sample_mappings: rt_model_set_rates has not been called (the paths need "
               "the rate matrices: a model with spectral rates or with transitions set directly "
               "has none)");
    RT_REQUIRE(m->rates_current || recompute_transitions,
               "%s: the transitions were set directly after the rates "
               "(rt_model_set_transitions): the resident rate matrices no longer describe them; "
               "set the rates again or pass recompute_transitions", "rt_sites_sample_mappings");
    if (n_coefs > RT_MAX_BRANCH_COEFS) {
        rt_set_error("%s: at most %d coefficient matrices (%lld here)", who, RT_MAX_BRANCH_COEFS,
                     (long long)n_coefs);
        return RT_ERR_UNSUPPORTED;
    }
    const int64_t n = p.n, N = p.N, nsites = p.nsites;
    size_t o_states = 0;
    RT_TRY(rt_sample_states_plan(&p, ndraws, &o_states));
    RT_REQUIRE((double)nsites * (double)N < 4503599627370496.0,
               "nsites * nnodes must be below 2^52 (the counters of the branch uniforms)");
    const bool lane = p.lane;
    const size_t nn = (size_t)n * n;
    const int nk = (int)n_coefs;
    for (size_t j = 0; j < (size_t)nk * nn; ++j)
        RT_REQUIRE(std::isfinite(coefs[j]), "coefficient %lld of matrix %lld is not finite",
                   (long long)(j % nn), (long long)(j / nn));
    RT_HIP(hipSetDevice(p.ctx->device));
    hipStream_t st = p.st;
    // the uniformization rate of every rate matrix in use and the event bound of every edge,
    // before anything is launched
    RT_REQUIRE((int64_t)m->h_qidx.size() == N && (int64_t)m->h_t.size() == N, "the model has no rates");
    int64_t nq = 1;
    for (int64_t v = 1; v < N; ++v) nq = std::max<int64_t>(nq, (int64_t)m->h_qidx[(size_t)v] + 1);
    std::vector<double> hQ((size_t)nq * nn), mu((size_t)nq, 0.0);
    RT_HIP(hipStreamSynchronize(st));
    RT_HIP(hipMemcpy(hQ.data(), m->d_Q, hQ.size() * 8, hipMemcpyDeviceToHost));
    for (int64_t q = 0; q < nq; ++q)
        for (int64_t c = 0; c < n; ++c) {
            const double r = -hQ[(size_t)q * nn + (size_t)c * n + c];
            if (r > mu[(size_t)q]) mu[(size_t)q] = r;
        }
    std::vector<int32_t> eK((size_t)N, 0), Kq((size_t)nq, 1), parent((size_t)N, 0);
    int KMAX = 1;
    for (int64_t v = 1; v < N; ++v) {
        const size_t q = (size_t)m->h_qidx[(size_t)v];
        double lam = mu[q] * m->h_t[(size_t)v];
        if (!(lam > 0.0)) lam = 0.0;
        const double kd = std::ceil(lam + 10.0 * std::sqrt(lam) + 20.0);
        if (!(kd <= (double)KCAP)) {
            rt_set_error("%s: the edge above node %lld needs up to %.0f uniformized events (rate "
                         "%g, length %g); at most %d", who, (long long)v, kd, mu[q],
                         m->h_t[(size_t)v], KCAP);
            return RT_ERR_UNSUPPORTED;
        }
        eK[(size_t)v] = (int32_t)kd;
        Kq[q] = std::max(Kq[q], (int32_t)kd);
        KMAX = std::max(KMAX, (int)kd);
        parent[(size_t)v] = m->parent[(size_t)v];
    }
    const int KS = KMAX + 1;
    std::vector<long> powoff((size_t)nq);
    size_t pow_doubles = 0;
    for (int64_t q = 0; q < nq; ++q) {
        powoff[(size_t)q] = (long)pow_doubles;
        pow_doubles += (size_t)(Kq[(size_t)q] + 1) * nn;
    }
    // the draws of one chunk
    const size_t per_draw = (size_t)nsites * N * ((size_t)nk * 8 + (counts ? 8 : 0));
    const int64_t tiles = (nsites + 15) / 16;
    size_t chunk_bytes = CHUNK_BYTES;
    if (const char *e = getenv("RAOTEH_MAPPING_CHUNK_BYTES")) {   // (tests: many chunks at small sizes)
        const long long v = atoll(e);
        if (v > 0) chunk_bytes = (size_t)v;
    }
    int64_t CH = (int64_t)std::max<size_t>(1, chunk_bytes / per_draw);
    CH = std::min<int64_t>(CH, ndraws);
    const int64_t per_draw_wgs = lane ? (nsites + 255) / 256 : tiles;         // workgroups per draw
    RT_REQUIRE(per_draw_wgs < (int64_t)1 << 31, "too many sites for one call");
    CH = std::max<int64_t>(1, std::min<int64_t>(CH, (((int64_t)1 << 31) - 1) / per_draw_wgs));
    RT_REQUIRE((int64_t)((size_t)nsites * N * nk + 255) / 256 < (int64_t)1 << 31,
               "too many sites for one call");
    post_plan &plan = p.plan;
    const size_t o_mu = plan.take((size_t)nq * 8), o_powoff = plan.take((size_t)nq * 8);
    const size_t o_Kq = plan.take((size_t)nq * 4), o_eK = plan.take((size_t)N * 4);
    const size_t o_parent = plan.take((size_t)N * 4);
    const size_t o_R = plan.take((size_t)nq * nn * 8), o_T = plan.take(pow_doubles * 8);
    const size_t o_pois = plan.take((size_t)N * KS * 8), o_E = plan.take((size_t)nk * nn * 8);
    const size_t cells = (size_t)nsites * N * nk;
    const size_t o_val = plan.take((size_t)CH * cells * 8);
    const size_t o_cnt = plan.take(counts ? (size_t)CH * nsites * N * 8 : 8);
    const size_t o_means = plan.take(cells * 8);
    RT_TRY(post_begin(&p, recompute_transitions, true));
    unsigned char *base = p.base;
    double *d_mu = (double *)(base + o_mu), *d_R = (double *)(base + o_R), *d_T = (double *)(base + o_T);
    double *d_pois = (double *)(base + o_pois), *d_E = (double *)(base + o_E);
    double *d_val = (double *)(base + o_val), *d_means = (double *)(base + o_means);
    long *d_powoff = (long *)(base + o_powoff);
    int *d_Kq = (int *)(base + o_Kq), *d_eK = (int *)(base + o_eK), *d_parent = (int *)(base + o_parent);
    int *d_cnt = counts ? (int *)(base + o_cnt) : nullptr;
    RT_HIP(hipMemcpyAsync(d_mu, mu.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_powoff, powoff.data(), (size_t)nq * 8, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_Kq, Kq.data(), (size_t)nq * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_eK, eK.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_parent, parent.data(), (size_t)N * 4, hipMemcpyHostToDevice, st));
    RT_HIP(hipMemcpyAsync(d_E, coefs, (size_t)nk * nn * 8, hipMemcpyHostToDevice, st));
    // 1. the tables (they depend on the rates alone: rebuilt by every call, never stale)
    {
        const dim3 grid((unsigned)((nn + 255) / 256), (unsigned)nq);
        hipLaunchKernelGGL(map_powers_init_kernel, grid, dim3(256), 0, st, (int)n,
                           (const double *)m->d_Q, (const double *)d_mu, (const long *)d_powoff, d_R, d_T);
        for (int k = 2; k <= KMAX; ++k)
            hipLaunchKernelGGL(map_powers_step_kernel, grid, dim3(256), 0, st, (int)n, k,
                               (const int *)d_Kq, (const long *)d_powoff, (const double *)d_R, d_T);
        hipLaunchKernelGGL(map_pois_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, (int)N,
                           KS, (const int *)m->d_qidx, (const double *)m->d_t, (const double *)d_mu,
                           (const int *)d_eK, d_pois);
        RT_HIP(hipGetLastError());
    }
    // 2. the node states: rt_sites_sample_states' own draws, left in scratch
    unsigned char *d_states = base + o_states;
    RT_TRY(rt_sample_states_enqueue(&p, seed, first_draw, ndraws, d_states));
    int *d_status = p.d_status;
    // 3. the paths, chunk by chunk
    map_tables tb;
    tb.parent = d_parent; tb.qidx = m->d_qidx; tb.eK = d_eK; tb.t = m->d_t; tb.powoff = d_powoff;
    tb.R = d_R; tb.T = d_T; tb.pois = d_pois; tb.E = d_E; tb.KS = KS; tb.nk = nk;
    for (int64_t d0 = 0; d0 < ndraws; d0 += CH) {
        const int64_t nd = std::min<int64_t>(CH, ndraws - d0);
        if (lane) {
            const unsigned grid = (unsigned)((nsites * nd + 255) / 256);
            RT_TRY(post_dispatch<2, 4>((int)n, [&](auto nv) {
                hipLaunchKernelGGL((map_lane_kernel<decltype(nv)::value>), dim3(grid), dim3(256), 0, st, tb,
                                   (int)N, (long)nsites, (long)nd, (unsigned long long)seed,
                                   (unsigned long long)first_draw, (long)d0,
                                   (const unsigned char *)d_states, d_val, d_cnt, d_status);
                return RT_OK;
            }));
        } else {
            const unsigned grid = (unsigned)(tiles * nd);
            RT_TRY(post_dispatch<1, 8>(p.NT, [&](auto nt) {
                hipLaunchKernelGGL((map_path_kernel<decltype(nt)::value>), dim3(grid), dim3(64), 0, st, tb,
                                   (int)n, (int)N, (long)nsites, (long)tiles, (unsigned long long)seed,
                                   (unsigned long long)first_draw, (long)d0,
                                   (const unsigned char *)d_states, d_val, d_cnt, d_status);
                return RT_OK;
            }));
        }
        RT_HIP(hipGetLastError());
        hipLaunchKernelGGL(map_means_kernel, dim3((unsigned)((cells + 255) / 256)), dim3(256), 0, st,
                           (long)cells, (long)nd, d0 == 0 ? 1 : 0, d0 + nd == ndraws ? 1 : 0,
                           (double)ndraws, (const double *)d_val, d_means);
        RT_HIP(hipGetLastError());
        // only what was asked for crosses PCIe
        if (values)
            RT_HIP(hipMemcpyAsync(values + (size_t)d0 * cells, d_val, (size_t)nd * cells * 8,
                                  hipMemcpyDeviceToHost, st));
        if (counts)
            RT_HIP(hipMemcpyAsync(counts + (size_t)d0 * nsites * N * 2, d_cnt,
                                  (size_t)nd * nsites * N * 8, hipMemcpyDeviceToHost, st));
    }
    if (states)
        RT_HIP(hipMemcpyAsync(states, d_states, (size_t)ndraws * nsites * N, hipMemcpyDeviceToHost, st));
    if (means) RT_HIP(hipMemcpyAsync(means, d_means, cells * 8, hipMemcpyDeviceToHost, st));
    if (status) RT_HIP(hipMemcpyAsync(status, d_status, (size_t)nsites * 4, hipMemcpyDeviceToHost, st));
    RT_HIP(hipStreamSynchronize(st));
    return RT_OK;
}
