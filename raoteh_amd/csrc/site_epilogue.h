// The end of a site in every pruning kernel of the library: the log-likelihood, the status and
// the site's contribution to the batch sums (finish_site), and the sum over a wave (wave_sum).
// One text for prune.hip's kernels and for the root combine that an expm launch carries
// (combine_body.inc), so that their numbers cannot drift apart.
#pragma once

__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// escale: the site's messages were multiplied by 2^-escale on the way up (opt-in rescaling:
// exact powers of two, so the mantissa of the likelihood is what it would have been)
__device__ __forceinline__ void finish_site(double lik, bool negative,
                                            bool valid, double *loglik,
                                            int *status, long site,
                                            double &sum, double &nzero, int escale = 0)
{
    const bool ok = lik > 0.0;
    if (valid) {
        double ll = ok ? log(lik) : -INFINITY;
        if (ok && escale != 0) {
            // in range: undo the scaling exactly and take the logarithm of the true value;
            // out of range: log(m 2^e) = log(m) + e ln 2
            const double back = ldexp(lik, escale);
            ll = (back > 0x1p-1000 && back < 0x1p1000) ? log(back)
                                                       : log(lik) + (double)escale * 0.6931471805599453094;
        }
        loglik[site] = ll;
        status[site] = (ok ? RT_SITE_OK : RT_SITE_ZERO_PROB) |
                       (negative ? RT_SITE_NEGATIVE : 0);
        sum = ok ? ll : 0.0;
        nzero = ok ? 0.0 : 1.0;
    } else {
        sum = 0.0;
        nzero = 0.0;
    }
}
