#!/usr/bin/env python
"""
L-BFGS-B on (kappa, omega, tree scale) of the codon configuration, the shape of the reference's
examples/p53/liwen-opt.py (fmin_l_bfgs_b with approx_grad over its parameters): the objective
and its forward differences are ONE step_multi -- K = 4 rate sets (the point and one step along
each parameter) against the resident alignment, one upload, one launch of exponentials, one
fetch of four totals.

    python examples/optimise_codon_lbfgs.py [nsites]

Synthetic data: configuration 3 of the benchmark (64-leaf tree, 61 codon states, sites simulated
with kappa = 3.176, omega = 0.219, scale 1), so the estimates should come back near those.
"""
import os
import sys
import time

import numpy as np
from scipy.optimize import fmin_l_bfgs_b

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import synth                      # noqa: E402
from raoteh_amd.device import TreeModel           # noqa: E402

EPS = 1e-6          # relative forward-difference step (parameters are optimised as logs)


def main(argv):
    nsites = int(argv[1]) if len(argv) > 1 else 10000
    cfg = synth.make_config('c3', nsites=nsites)
    model = TreeModel(cfg['T'], cfg['root'], cfg['nstates'])
    model.set_root_distn(cfg['root_distn'])
    batch = model.upload_sites(cfg['leaves'], cfg['leaf_states'].astype(np.uint8),
                               kind='state')                  # once
    t0 = model.tree.branch_lengths()
    calls = []

    def value_and_gradient(x):
        """x = log(kappa, omega, scale) -> (-log-likelihood, its forward differences)."""
        points = [x] + [x + EPS * np.eye(3)[j] for j in range(3)]
        Q = np.stack([synth.mg94(kappa=np.exp(p[0]), omega=np.exp(p[1]))[0] for p in points])
        t = np.stack([t0 * np.exp(p[2]) for p in points])
        start = time.perf_counter()
        model.set_rate_sets(Q, t=t)               # 4 x 126 exponentials, one launch
        model.step_multi(batch, recompute_transitions=False)    # 4 prunings, 4 sums
        tot = model.fetch_multi_totals(batch)
        calls.append(time.perf_counter() - start)
        if tot[:, 1].any():
            return np.inf, np.zeros(3)
        f = -tot[:, 0]
        return f[0], (f[1:] - f[0]) / EPS

    x0 = np.log([2.0, 0.5, 0.8])
    x, fmin, info = fmin_l_bfgs_b(value_and_gradient, x0, bounds=[(-3.0, 3.0)] * 3)
    lat = np.array(calls[2:]) * 1e6
    print('%d sites: kappa = %.4f, omega = %.4f, tree scale = %.4f (simulated with 3.1763, '
          '0.2193, 1), log-likelihood %.3f' % (nsites, np.exp(x[0]), np.exp(x[1]), np.exp(x[2]),
                                              -fmin))
    print('%d evaluations of value + gradient (%s), %.0f us each (median, host round trip and '
          'the four rate matrices built in numpy included; kernel %s)' % (
              len(calls), info['task'] if isinstance(info['task'], str) else info['task'].decode(),
              np.median(lat), batch.multi_kernel_name))


if __name__ == '__main__':
    main(sys.argv)
