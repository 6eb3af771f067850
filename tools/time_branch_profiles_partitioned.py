#!/usr/bin/env python
"""
Branch profiles with each site under its own rate set (site i in set i % K, eight factors per
branch, sums only): microseconds per evaluation of the whole alignment under K fresh parameter
vectors, by

  partitioned   set_rate_sets + branch_profiles_partitioned of ONE partitioned batch
  subbatch      K x (set_rates + branch_profiles(factors=...)) over K ordinary sub-batches holding
                the sites of one set each, the sums added on the host ("jit" = 0: the call runs
                its passes on the interpreter twin whichever kernel the batch has)

each the median of nine windows with the window minimum and maximum, the two forms alternating
window by window.  The sub-batch loop uses nothing this call added, so `--baseline-only` runs on
a checkout without it (copy this file and the time_*_partitioned.py that calls it into its tools/).
`--single` times the single-set call alone on the whole alignment as one ordinary batch (set_rates
+ the call), for a comparison of two builds.

    python tools/time_branch_profiles_partitioned.py --workload c3 --K 4,64
        [--baseline-only] [--single] [--out profiles/branch_profiles_partitioned_c3.json] [--once K]

`--once K`: warm up, then ten partitioned evaluations (the program to put behind
`rocprofv3 --kernel-trace --stats --`).  time_nni_scores_partitioned.py is the same program for
nni_scores_partitioned, at eight factors and for the plain swap; time_spr_scores_partitioned.py for
spr_scores_partitioned at radius 1 and 3 and one fraction; time_placements_partitioned.py for
place_queries_partitioned with 16 state queries on every edge at one fraction and one pendant
length.
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
from time_step_partitioned import new_model, summary          # noqa: E402
import time_step_partitioned          # noqa: E402

WINDOWS = 9
FACTORS = np.exp(np.linspace(-np.log(2.0), np.log(2.0), 8))


def window(fn, reps):
    import time
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps * 1e6


def rate_sets(cfg, K, model):
    """K parameter vectors around the configuration's own: c3 as time_step_partitioned has them,
    another workload its default rate matrix and tree, both scaled a little per set."""
    if cfg['name'] == 'c3':
        return time_step_partitioned.rate_sets(cfg, K, model)
    t0 = model.tree.branch_lengths()
    Q = np.array([np.asarray(cfg['Q_default']) * (1.0 + 0.02 * k) for k in range(K)])
    t = np.array([t0 * (1.0 + 0.005 * k) for k in range(K)])
    return Q, t


PLACE_QUERIES = 16
PLACE_PENDANT = (0.1,)


def calls(call, model, factors, nsites=0):
    """(the single-set call on a batch -> sums, the partitioned call on a batch -> set_sums); both
    take the batch and the sites it holds (an index array; None: all of them).  `factors`: the
    variant -- factors or None (profiles, nni), the radius (spr), nothing (place: PLACE_QUERIES
    state queries on every edge at one fraction and one pendant length)."""
    if call == 'profiles':
        return (lambda b, sites: model.branch_profiles(b, factors=factors).sums,
                lambda b, sites: model.branch_profiles_partitioned(b, factors).set_sums)
    if call == 'spr':
        return (lambda b, sites: model.spr_scores(b, radius=factors).sums,
                lambda b, sites: model.spr_scores_partitioned(b, radius=factors).set_sums)
    if call == 'place':
        q = np.random.RandomState(5).randint(0, model.nstates, size=(PLACE_QUERIES, nsites)).astype(np.uint8)
        cut = {}

        def mine(sites):                         # (the set's queries, sliced once per index array:
            if sites is None:                    # the entry keeps the array, so its id stays its own)
                return q
            if id(sites) not in cut:
                cut[id(sites)] = (sites, np.ascontiguousarray(q[:, sites]))
            return cut[id(sites)][1]
        return (lambda b, sites: model.place_queries(b, mine(sites), kind='state',
                                                     pendant=PLACE_PENDANT).sums,
                lambda b, sites: model.place_queries_partitioned(b, q, kind='state',
                                                                 pendant=PLACE_PENDANT).set_sums)
    if factors is None:
        return (lambda b, sites: model.nni_scores(b).sums,
                lambda b, sites: model.nni_scores_partitioned(b).set_sums)
    return (lambda b, sites: model.nni_scores(b, factors=factors).sums,
            lambda b, sites: model.nni_scores_partitioned(b, factors).set_sums)


def main(call='profiles', variants=(('8 factors', FACTORS),)):
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c3')
    ap.add_argument('--K', default='4,64')
    ap.add_argument('--reps', type=int, default=0, help='evaluations per window (0: 12 // K + 3)')
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--single', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--once', type=int, default=0)
    args = ap.parse_args()
    Ks = [args.once] if args.once else [int(k) for k in args.K.split(',')]
    cfg = synth.make_config(args.workload)
    dense = synth.leaf_likelihoods(cfg)
    nsites = dense.shape[0]
    result = dict(workload=args.workload, call=call, kind='dense', nsites=nsites,
                  assignment='site i in set i % K', windows=WINDOWS, rows=[])
    if args.single:
        ctx, model = new_model(cfg, 0)
        Q, t = rate_sets(cfg, 1, model)
        batch = model.upload_sites(cfg['leaves'], dense, kind='dense')
        for label, factors in variants:
            single, _ = calls(call, model, factors, nsites)

            def fn():
                model.set_rates(Q=Q[0], t=t[0])
                return single(batch, None)
            for _ in range(2):
                fn()
            row = dict(single=True, points=label, reps_per_window=args.reps or 6)
            row['single'] = summary([window(fn, args.reps or 6) for _ in range(WINDOWS)])
            result['rows'].append(row)
            print(json.dumps(row))
        Ks = []
    for K in Ks:
        reps = args.reps or 12 // K + 3
        site_sets = np.arange(nsites) % K
        members = [np.flatnonzero(site_sets == k) for k in range(K)]
        ctx, model = new_model(cfg, 0)
        Q, t = rate_sets(cfg, K, model)
        subs = [model.upload_sites(cfg['leaves'], np.ascontiguousarray(dense[site_sets == k]),
                                   kind='dense') for k in range(K)]
        part = None
        if not args.baseline_only:
            part = model.upload_sites(cfg['leaves'], dense, kind='dense', site_sets=site_sets, nsets=K)
        for label, factors in variants:
            single, partitioned_call = calls(call, model, factors, nsites)
            row = dict(K=K, points=label, reps_per_window=reps)

            def subbatch():
                out = []
                for k in range(K):
                    model.set_rates(Q=Q[k], t=t[k])
                    out.append(single(subs[k], members[k]))
                return np.array(out)

            def partitioned():
                model.set_rate_sets(Q, t=t)
                return partitioned_call(part, None)
            forms = [('subbatch', subbatch)]
            if part is not None:
                forms.insert(0, ('partitioned', partitioned))
            last = {}
            for _ in range(2):
                for name, fn in forms:
                    last[name] = fn()
            if args.once:
                for _ in range(10):
                    partitioned()
                print('ten partitioned evaluations, K = %d, %s' % (K, label))
                continue
            if 'partitioned' in last:
                # the per-set sums are those of the sub-batch loop (another summation order only)
                a, b = last['partitioned'], last['subbatch']
                assert np.allclose(a, b, rtol=1e-9, atol=1e-9 * np.abs(b).max(), equal_nan=True)
            us = dict((name, []) for name, _ in forms)
            for _ in range(WINDOWS):
                for name, fn in forms:
                    us[name].append(window(fn, reps))
            for name, _ in forms:
                row[name] = summary(us[name])
            if 'partitioned' in us:
                row['ratio_subbatch_over_partitioned'] = (row['subbatch']['median_us'] /
                                                          row['partitioned']['median_us'])
            result['rows'].append(row)
            print(json.dumps(row))
        del subs, part
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
