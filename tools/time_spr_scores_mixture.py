#!/usr/bin/env python
"""
SPR scores under a site-class mixture over K rate sets (every move within radius 1 and within
radius 3 at one fraction, sums only): milliseconds per evaluation of the whole alignment, by

  mixture    spr_scores_mixture(per_site=False) of one ordinary batch under the resident rate sets
  separate   K x (set_rates + step + spr_scores(per_site=True)) of the same batch for the per-set
             log ratios, one step_multi + fetch_multi_log_likelihoods for the L_ik, and the class
             posteriors, the combination and the weighted sums in numpy on the host
  single     one single-set spr_scores(per_site=False) call under the model's own rates: the
             yardstick that must not move against the parent commit

measured and reported as tools/time_branch_profiles_mixture.py does: the median of nine windows
with the window minimum and maximum, the forms alternating window by window; the separate and the
single form use nothing this call added, so `--baseline-only` runs on a checkout without it.  The
rate sets are a discrete-rate model, Q_k = r_k Q over the tree's own branch lengths, so every
L_ik is positive and the separate form is defined (it is not where a set is dead on the resident
tree and alive on the moved one).

    python tools/time_spr_scores_mixture.py [c2|c3|c6] [--K 4] [--rows r1,r3] [--baseline-only]
        [--out profiles/spr_scores_mixture_c3.json] [--once ROW] [--once-single ROW]

tools/time_placements_mixture.py runs the same comparison for place_queries_mixture (this
module's `main('place')`): the rows `small` (16 queries, 1 fraction, 1 pendant length) and `large`
(64 queries, 3 fractions, 4 pendant lengths).  `--once ROW` / `--once-single ROW`: warm up, then
five mixture / single-set evaluations of that row (the programs to put behind
`rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, synth                       # noqa: E402
from time_branch_profiles_mixture import WINDOWS, class_rates, combine   # noqa: E402

SPR_ROWS = {'r1': 1, 'r3': 3}
PLACE_ROWS = {'small': (16, (0.5,), (0.1,)), 'large': (64, (0.25, 0.5, 0.75), (0.02, 0.05, 0.1, 0.2))}


def main(call):
    ap = argparse.ArgumentParser()
    ap.add_argument('config', nargs='?', default='c3')
    ap.add_argument('--K', type=int, default=4)
    ap.add_argument('--sites', type=int, default=0)
    ap.add_argument('--window-ms', type=float, default=150.0)
    ap.add_argument('--rows', default='')
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--out', default='')
    ap.add_argument('--once', default='')
    ap.add_argument('--once-single', default='')
    args = ap.parse_args()
    K = args.K
    cfg = synth.make_config(args.config, nsites=args.sites or None)
    n = cfg['nstates']
    data = synth.leaf_likelihoods(cfg)
    ctx = device.get_context()
    model = device.TreeModel(cfg['T'], cfg['root'], n)
    model.set_root_distn(cfg['root_distn'])
    model.set_rates(Q_default=cfg['Q_default'])
    t = model.tree.branch_lengths()
    Q = np.array([r * cfg['Q_default'] for r in class_rates(K)])
    c = np.arange(1.0, K + 1.0)
    c /= c.sum()
    batch = model.upload_sites(cfg['leaves'], data, kind='dense')
    S = batch.nsites
    w = np.ones(S)
    model.set_rate_sets(Q, t=t)
    model.step(batch)
    ctx.sync()
    table = SPR_ROWS if call == 'spr' else PLACE_ROWS
    rows = [r for r in (args.rows.split(',') if args.rows else table)]
    queries = {}
    if call == 'place':
        rng = np.random.RandomState(5)
        for name in set(rows) | set(x for x in (args.once, args.once_single) if x):
            queries[name] = rng.randint(0, n, size=(table[name][0], S)).astype(np.uint8)

    def single(row, per_site):
        if call == 'spr':
            return model.spr_scores(batch, radius=table[row], per_site=per_site)
        nq, f, tau = table[row]
        return model.place_queries(batch, queries[row], kind='state', fractions=f, pendant=tau,
                                   per_site=per_site)

    def separate(row):
        ratios = []
        for k in range(K):
            model.set_rates(Q=Q[k], t=t)
            model.step(batch)
            v = single(row, True).values
            ratios.append(v.reshape(S, -1, v.shape[-1]))
        model.step_multi(batch, recompute_transitions=False)
        ll, _ = model.fetch_multi_log_likelihoods(batch)
        model.set_rates(Q_default=cfg['Q_default'])       # (the rates the single form runs under)
        return combine(ratios, ll, c, w)

    def mixture(row):
        if call == 'spr':
            return model.spr_scores_mixture(batch, c, radius=table[row]).sums
        nq, f, tau = table[row]
        sums = model.place_queries_mixture(batch, c, queries[row], kind='state', fractions=f,
                                           pendant=tau).sums
        return sums.reshape(-1, sums.shape[-1])

    if args.once or args.once_single:
        row = args.once or args.once_single
        fn = (lambda: mixture(row)) if args.once else (lambda: single(row, False))
        for _ in range(2):
            fn()
        ctx.sync()
        for _ in range(5):
            fn()
        ctx.sync()
        print('five %s evaluations of row %s' % ('mixture' if args.once else 'single-set', row))
        return
    out = dict(config=args.config, call=call, sites=S, states=n, nodes=model.tree.nnodes, K=K,
               windows=WINDOWS, outputs='sums only',
               what='wall ms per evaluation: median [min, max] of the windows')
    for label in rows:
        forms = [('separate', lambda r=label: separate(r)),
                 ('single', lambda r=label: single(r, False).sums)]
        if not args.baseline_only:
            forms.insert(0, ('mixture', lambda r=label: mixture(r)))
        last, reps = {}, {}
        for name, fn in forms:                   # warm-up: every shape the windows use
            fn()
            ctx.sync()
            t0 = time.perf_counter()
            last[name] = fn()
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            reps[name] = max(1, min(50, int(np.ceil(args.window_ms / ms))))
        out['%s_rows' % label] = int(np.prod(last['single'].shape))
        if 'mixture' in last:                    # the two forms agree on what they compute
            fin = np.isfinite(last['separate'])
            gap = np.abs(last['mixture'][fin] - last['separate'][fin]).max()
            out['%s_max_abs_gap' % label] = float(gap)
            assert gap <= 1e-8 * max(1.0, np.abs(last['separate'][fin]).max()), gap
        times = dict((name, []) for name, _ in forms)
        for _ in range(WINDOWS):
            for name, fn in forms:               # the forms alternate window by window
                t0 = time.perf_counter()
                for _ in range(reps[name]):
                    fn()
                ctx.sync()
                times[name].append((time.perf_counter() - t0) * 1e3 / reps[name])
        for name, ts in times.items():
            out['%s_%s' % (name, label)] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
        out['%s_per_window' % label] = reps
        if 'mixture' in times:
            a, b = out['mixture_' + label], out['separate_' + label]
            out['%s_separate_over_mixture' % label] = b[0] / a[0]
            # the ordering by DESIGN.md 3.4c: the medians further apart than the two window ranges
            out['%s_ordering_met' % label] = bool(b[0] - a[0] > max(a[2] - a[1], b[2] - b[1]))
            out['%s_mixture_over_K_single' % label] = a[0] / (K * out['single_' + label][0])
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f_:
            f_.write(line + '\n')


if __name__ == '__main__':
    main('spr')
