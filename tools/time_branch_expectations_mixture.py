#!/usr/bin/env python
"""
Per-branch expectations under a site-class mixture over K rate sets (one coefficient matrix, edge
sums only): microseconds per evaluation of the whole alignment under K fresh parameter vectors, by

  mixture    set_rate_sets + branch_expectations_mixture(per_site=False) of one ordinary batch
  separate   K x (set_rates + branch_expectations(per_site=True)) of the same batch for the
             unweighted x_k, set_rate_sets + step_multi + fetch_multi_log_likelihoods for the
             L_ik, and the posteriors and the weighted sums in numpy on the host -- the only way
             to the same numbers without the call ("jit" = 0: the call runs its passes on the
             interpreter twin whichever kernel the batch has)

each the median of nine windows with the window minimum and maximum, the two forms alternating
window by window.  The separate form uses nothing this call added, so `--baseline-only` runs on a
checkout without it.  No cache flush is needed between calls: at 10 000 sites and 61 states the
stored L, M and D of one pass are 3 x 650 MB, several times the 256 MB Infinity Cache, and every
evaluation rewrites the transition and derivative tables.

    python tools/time_branch_expectations_mixture.py --workload c3 --K 4,16
        [--baseline-only] [--out profiles/branch_expect_mixture_c3.json] [--once K]

`--once K`: warm up, then ten mixture evaluations (the program to put behind
`rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from raoteh_amd import synth          # noqa: E402
from time_step_partitioned import new_model, rate_sets, summary          # noqa: E402
from time_branch_expectations_partitioned import window, WINDOWS          # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c3')
    ap.add_argument('--K', default='4,16')
    ap.add_argument('--reps', type=int, default=0, help='evaluations per window (0: 12 // K + 3)')
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--once', type=int, default=0)
    args = ap.parse_args()
    Ks = [args.once] if args.once else [int(k) for k in args.K.split(',')]
    cfg = synth.make_config(args.workload)
    dense = synth.leaf_likelihoods(cfg)
    nsites, n = dense.shape[0], cfg['nstates']
    E = np.ones((n, n))                 # every change counts once: expected changes per branch
    np.fill_diagonal(E, 0.0)
    result = dict(workload=args.workload, kind='dense', nsites=nsites, coefficient_matrices=1,
                  outputs='edge sums, per-set sums, class sums, posteriors, log-likelihoods',
                  windows=WINDOWS, rows=[])
    for K in Ks:
        reps = args.reps or 12 // K + 3
        ctx, model = new_model(cfg, 0)
        Q, t = rate_sets(cfg, K, model)
        c = np.arange(1.0, K + 1.0)
        c /= c.sum()
        row = dict(K=K, reps_per_window=reps)
        batch = model.upload_sites(cfg['leaves'], dense, kind='dense')

        def separate():
            x = []
            for k in range(K):
                model.set_rates(Q=Q[k], t=t[k])
                x.append(model.branch_expectations(batch, E, per_site=True).values)
            model.set_rate_sets(Q, t=t)
            model.step_multi(batch, recompute_transitions=False)
            ll, _ = model.fetch_multi_log_likelihoods(batch)
            a = ll + np.log(c)[:, None]
            post = np.exp(a - a.max(axis=0))
            post /= post.sum(axis=0)
            return np.array([np.einsum('i,ivc->vc', post[k], x[k]) for k in range(K)])
        forms = [('separate', separate)]
        if not args.baseline_only:
            def mixture():
                model.set_rate_sets(Q, t=t)
                return model.branch_expectations_mixture(batch, E, c, per_site=False).set_edge_sums
            forms.insert(0, ('mixture', mixture))
        last = {}
        for _ in range(2):
            for label, fn in forms:
                last[label] = fn()
        if args.once:
            for _ in range(10):
                mixture()
            print('ten mixture evaluations, K = %d' % K)
            return
        if 'mixture' in last:
            # the per-class sums are those of the separate form (another summation order only)
            assert np.allclose(last['mixture'], last['separate'], rtol=1e-10, atol=0)
        us = dict((label, []) for label, _ in forms)
        for _ in range(WINDOWS):
            for label, fn in forms:
                us[label].append(window(fn, reps))
        for label, _ in forms:
            row[label] = summary(us[label])
        if 'mixture' in us:
            row['ratio_separate_over_mixture'] = (row['separate']['median_us'] /
                                                  row['mixture']['median_us'])
        result['rows'].append(row)
        print(json.dumps(row))
        batch.close()
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
