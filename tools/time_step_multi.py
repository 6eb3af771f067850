#!/usr/bin/env python
"""
K rate sets against one resident batch: microseconds per rate set of

  multi     set_rate_sets + step_multi + one fetch of the K totals
  baseline  K x (set_rates + step) + one fetch of the totals   (existing calls only)

each the median of nine windows, with the window minimum and maximum.  The baseline uses
nothing this feature added, so `--baseline-only` runs on a checkout without it.

    python tools/time_step_multi.py --workload c3 --K 1,2,4,8,31 [--kind dense|state]
        [--baseline-only] [--out profiles/step_multi_c3.json] [--once K]

RAOTEH_MULTI=loop in the environment times the loop form.  `--once K`: no timing, warm up and
run one multi step of K sets (the program to put behind `rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, synth          # noqa: E402

WINDOWS = 9


def rate_sets(cfg, K, model):
    """K parameter vectors around the configuration's own: (kappa, omega, tree scale) as a
    forward-difference gradient or a line search would ask for them."""
    if cfg['name'] != 'c3':
        raise SystemExit('workload %s: only c3 (the codon configuration) is set up here' % cfg['name'])
    t0 = model.tree.branch_lengths()
    Q = np.empty((K, cfg['nstates'], cfg['nstates']))
    t = np.empty((K, len(t0)))
    for k in range(K):
        Q[k] = synth.mg94(kappa=3.17632 * (1.0 + 0.01 * k), omega=0.21925 * (1.0 + 0.02 * k))[0]
        t[k] = t0 * (1.0 + 0.005 * k)
    return Q, t


def windows(fn, reps):
    out = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return out


def summary(us, K):
    per = np.array(us) / K
    return dict(median_us_per_set=float(np.median(per)), min_us_per_set=float(per.min()),
                max_us_per_set=float(per.max()), windows=len(us))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c3')
    ap.add_argument('--K', default='1,2,4,8,31')
    ap.add_argument('--kind', default='dense', choices=('dense', 'state'))
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--once', type=int, default=0)
    args = ap.parse_args()
    Ks = [args.once] if args.once else [int(k) for k in args.K.split(',')]
    cfg = synth.make_config(args.workload)
    ctx = device.get_context()
    model = device.TreeModel(cfg['T'], cfg['root'], cfg['nstates'], ctx=ctx)
    model.set_root_distn(cfg['root_distn'])
    model.set_rates(Q_default=cfg['Q_default'])
    if args.kind == 'state':
        batch = model.upload_sites(cfg['leaves'], cfg['leaf_states'].astype(np.uint8), kind='state')
    else:
        batch = model.upload_sites(cfg['leaves'], synth.leaf_likelihoods(cfg), kind='dense')
    batch.wait_for_kernel()
    model.step(batch)
    model.fetch_totals(batch)
    result = dict(workload=args.workload, kind=args.kind, nsites=batch.nsites,
                  kernel=batch.kernel_name, reps_per_window=args.reps,
                  form=os.environ.get('RAOTEH_MULTI', 'default'), rows=[])
    for K in Ks:
        Q, t = rate_sets(cfg, K, model)
        row = dict(K=K)

        def baseline():
            for k in range(K):
                model.set_rates(Q=Q[k], t=t[k])
                model.step(batch)
            return model.fetch_totals(batch)

        if not args.once:
            for _ in range(3):
                last = baseline()
            row['baseline'] = summary(windows(baseline, args.reps), K)
        if not args.baseline_only:
            def multi():
                model.set_rate_sets(Q, t=t)
                model.step_multi(batch)
                return model.fetch_multi_totals(batch)

            multi()
            batch.wait_for_kernel()           # the one-launch form, where the batch has one
            for _ in range(3):
                tot = multi()
            row['multi_kernel'] = batch.multi_kernel_name
            if args.once:
                print('one multi step of %d sets: %s' % (K, row['multi_kernel']))
                return
            # the last set's totals are those of the baseline's last step, bit for bit
            assert np.array_equal(tot[K - 1].view(np.int64), last.view(np.int64)), (tot[K - 1], last)
            row['multi'] = summary(windows(multi, args.reps), K)
            row['ratio_baseline_over_multi'] = (row['baseline']['median_us_per_set'] /
                                                row['multi']['median_us_per_set'])
        result['rows'].append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
