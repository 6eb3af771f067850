#!/usr/bin/env python
"""
Branch profiles under a site-class mixture over K rate sets (8 factors per branch, sums only):
milliseconds per evaluation of the whole alignment, by

  mixture    branch_profiles_mixture(per_site=False) of one ordinary batch under the resident
             rate sets
  separate   K x (set_rates + step + branch_profiles(per_site=True)) of the same batch for the
             per-set log ratios, one step_multi + fetch_multi_log_likelihoods for the L_ik, and the
             class posteriors, the combination and the weighted sums in numpy on the host -- the
             only way to the same numbers without the call

each the median of nine windows with the window minimum and maximum, the two forms alternating
window by window.  The separate form uses nothing this call added, so `--baseline-only` runs on a
checkout without it.  The rate sets are a discrete-rate model: Q_k = r_k Q of the workload's rate
matrix with the tree's own branch lengths for every class.

    python tools/time_branch_profiles_mixture.py [c2|c3|c6] [--K 4] [--baseline-only]
        [--out profiles/branch_profiles_mixture_c3.json] [--once] [--once-single]

`--once`: warm up, then five mixture evaluations; `--once-single`: five single-set
branch_profiles calls on the same batch (the programs to put behind
`rocprofv3 --kernel-trace --stats --`).

tools/time_nni_scores_mixture.py runs the same comparison for nni_scores_mixture (this module's
`main('nni')`).
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
F8 = np.exp(np.linspace(-np.log(4), np.log(4), 8))


def class_rates(K):
    """K rates with mean 1 over equal classes (the shape of a discrete gamma)."""
    r = np.exp(np.linspace(-1.5, 1.0, K))
    return r / r.mean()


def combine(ratios, ll, c, w):
    """sums[row, g] of log sum_k post[i, k] exp(ratios[k][i, row, g]) over the live sites: the
    mixture value from the per-set log ratios log L_ik(.) / L_ik and the L_ik of step_multi."""
    a = ll + np.log(c)[:, None]
    top = a.max(axis=0)
    live = np.isfinite(top)
    post = np.exp(a[:, live] - top[live])
    post /= post.sum(axis=0)
    mix = 0.0
    for k in range(len(c)):
        mix = mix + post[k][:, None, None] * np.exp(ratios[k][live])
    with np.errstate(divide='ignore'):
        return np.einsum('i,irg->rg', w[live], np.log(mix))


def main(call):
    ap = argparse.ArgumentParser()
    ap.add_argument('config', nargs='?', default='c3')
    ap.add_argument('--K', type=int, default=4)
    ap.add_argument('--sites', type=int, default=0)
    ap.add_argument('--window-ms', type=float, default=150.0)
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--out', default='')
    ap.add_argument('--once', action='store_true')
    ap.add_argument('--once-single', action='store_true')
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
    w = np.ones(batch.nsites)
    model.set_rate_sets(Q, t=t)
    model.step(batch)
    ctx.sync()
    grids = [('g8', F8)] if call == 'profile' else [('g1', None), ('g8', F8)]

    def single(f):
        if call == 'profile':
            return model.branch_profiles(batch, factors=f, per_site=True)
        return model.nni_scores(batch, factors=f, per_site=True)

    def separate(f):
        ratios = []
        for k in range(K):
            model.set_rates(Q=Q[k], t=t)
            model.step(batch)
            ratios.append(single(f).values)
        model.step_multi(batch, recompute_transitions=False)
        ll, _ = model.fetch_multi_log_likelihoods(batch)
        return combine(ratios, ll, c, w)

    def mixture(f):
        if call == 'profile':
            return model.branch_profiles_mixture(batch, c, f).sums
        return model.nni_scores_mixture(batch, c, f).sums

    if args.once or args.once_single:
        fn = (lambda: mixture(F8)) if args.once else (lambda: single(F8))
        for _ in range(2):
            fn()
        ctx.sync()
        for _ in range(5):
            fn()
        ctx.sync()
        print('five %s evaluations at 8 points' % ('mixture' if args.once else 'single-set'))
        return
    out = dict(config=args.config, call=call, sites=batch.nsites, states=n,
               nodes=model.tree.nnodes, K=K, windows=WINDOWS, outputs='sums only',
               rows=model.tree.nnodes if call == 'profile' else len(model.nni_moves()),
               what='wall ms per evaluation: median [min, max] of the windows')
    for label, f in grids:
        forms = [('separate', lambda f=f: separate(f))]
        if not args.baseline_only:
            forms.insert(0, ('mixture', lambda f=f: mixture(f)))
        last, reps = {}, {}
        for name, fn in forms:                   # warm-up: every shape the windows use
            fn()
            ctx.sync()
            t0 = time.perf_counter()
            last[name] = fn()
            ctx.sync()
            ms = (time.perf_counter() - t0) * 1e3
            reps[name] = max(1, min(50, int(np.ceil(args.window_ms / ms))))
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
    line = json.dumps(out)
    print(line)
    if args.out:
        with open(args.out, 'w') as f_:
            f_.write(line + '\n')


if __name__ == '__main__':
    main('profile')
