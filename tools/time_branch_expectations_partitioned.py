#!/usr/bin/env python
"""
Per-branch expectations with each site under its own rate set (site i in set i % K, one
coefficient matrix, edge sums only): microseconds per evaluation of the whole alignment under K
fresh parameter vectors, by

  partitioned   set_rate_sets + branch_expectations_partitioned(per_site=False) of ONE
                partitioned batch
  subbatch      K x (set_rates + branch_expectations(per_site=False)) over K ordinary sub-batches
                holding the sites of one set each ("jit" = 0: the call runs its passes on the
                interpreter twin whichever kernel the batch has)

each the median of nine windows with the window minimum and maximum, the two forms alternating
window by window.  The sub-batch loop uses nothing this call added, so `--baseline-only` runs on
a checkout without it.  No cache flush is needed between calls: at 10 000 sites and 61 states
the stored L, M and D of one pass are 3 x 650 MB, several times the 256 MB Infinity Cache, and
every evaluation rewrites the transition and derivative tables.

    python tools/time_branch_expectations_partitioned.py --workload c3 --K 4,64
        [--baseline-only] [--out profiles/branch_expect_partitioned_c3.json] [--once K]

`--once K`: warm up, then ten partitioned evaluations (the program to put behind
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

WINDOWS = 9


def window(fn, reps):
    import time
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c3')
    ap.add_argument('--K', default='4,64')
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
                  assignment='site i in set i % K', windows=WINDOWS, rows=[])
    for K in Ks:
        reps = args.reps or 12 // K + 3
        site_sets = np.arange(nsites) % K
        ctx, model = new_model(cfg, 0)
        Q, t = rate_sets(cfg, K, model)
        row = dict(K=K, reps_per_window=reps)
        subs = [model.upload_sites(cfg['leaves'], np.ascontiguousarray(dense[site_sets == k]),
                                   kind='dense') for k in range(K)]

        def subbatch():
            out = []
            for k in range(K):
                model.set_rates(Q=Q[k], t=t[k])
                out.append(model.branch_expectations(subs[k], E, per_site=False).edge_sums)
            return np.array(out)
        forms = [('subbatch', subbatch)]
        if not args.baseline_only:
            part = model.upload_sites(cfg['leaves'], dense, kind='dense', site_sets=site_sets,
                                      nsets=K)

            def partitioned():
                model.set_rate_sets(Q, t=t)
                return model.branch_expectations_partitioned(part, E, per_site=False).set_edge_sums
            forms.insert(0, ('partitioned', partitioned))
        last = {}
        for _ in range(2):
            for label, fn in forms:
                last[label] = fn()
        if args.once:
            for _ in range(10):
                partitioned()
            print('ten partitioned evaluations, K = %d' % K)
            return
        if 'partitioned' in last:
            # the per-set sums are those of the sub-batch loop (another summation order only)
            assert np.allclose(last['partitioned'], last['subbatch'], rtol=1e-11, atol=0)
        us = dict((label, []) for label, _ in forms)
        for _ in range(WINDOWS):
            for label, fn in forms:
                us[label].append(window(fn, reps))
        for label, _ in forms:
            row[label] = summary(us[label])
        if 'partitioned' in us:
            row['ratio_subbatch_over_partitioned'] = (row['subbatch']['median_us'] /
                                                      row['partitioned']['median_us'])
        result['rows'].append(row)
        print(json.dumps(row))
        del subs
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
