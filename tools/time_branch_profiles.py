"""Diagnostics: milliseconds per rt_sites_branch_profiles call (resident batch) for one bench
configuration, at G = 1, 8, 32 trial lengths per branch, sums only and with the per-site array;
beside it, on the same batch, the two comparators of DESIGN.md 3.5f:
  - the brute-force loop the call replaces, one set_rates + step (+ the fetch of the totals that
    ends it) per branch and trial length, for the same grid at G = 8 -- timed on --loop-branches
    branches and scaled to all nnodes - 1 (the loop's cost does not depend on the branch);
  - branch_expectations with 8 coefficient matrices, sums only: the same downward pass with 8
    extra products per step, with the derivative tables in the place of the exponentials.
Median wall ms per call of nine windows of --per-window calls after warm-up, each window ended
by a device synchronise.  Prints one JSON line (and writes it to --out); under
`rocprofv3 --kernel-trace --stats` (a run of its own, --windows 1 --no-loop) for the kernel split.
    python tools/time_branch_profiles.py [c2|c3|c6] [--sites N] [--windows 9] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth

ap = argparse.ArgumentParser()
ap.add_argument('config', nargs='?', default='c3')
ap.add_argument('--sites', type=int, default=0)
ap.add_argument('--windows', type=int, default=9)
ap.add_argument('--per-window', type=int, default=3)
ap.add_argument('--loop-branches', type=int, default=8)
ap.add_argument('--no-loop', action='store_true')
ap.add_argument('--out', default='')
args = ap.parse_args()
nsites = args.sites or {'c2': 100000}.get(args.config, 10000)
cfg = synth.make_config(args.config, nsites=nsites)
T, root, n = cfg['T'], cfg['root'], cfg['nstates']
model = device.TreeModel(T, root, n)
model.set_root_distn(cfg['root_distn'])
if cfg.get('Q_default') is not None:
    model.set_rates(Q_default=cfg['Q_default'])
else:
    model.set_rates()
batch = model.upload_sites(cfg['leaves'], synth.leaf_likelihoods(cfg), kind='dense')
ctx = device.get_context()
N = model.tree.nnodes
Q, t0 = model._rates
node_q = model.tree.rate_matrices(n, cfg.get('Q_default'))[1]
rng = np.random.RandomState(1)
coefs = (rng.uniform(size=(8, n, n)) < 0.5).astype(float)
for E in coefs:
    np.fill_diagonal(E, 0.0)


def factors(G):
    return np.exp(np.linspace(-np.log(4), np.log(4), G)) if G > 1 else np.array([1.5])


def median_ms(fn, per_window=None):
    per_window = per_window or args.per_window
    for _ in range(2):
        fn()
    ctx.sync()
    times = []
    for _ in range(args.windows):
        t0_ = time.perf_counter()
        for _ in range(per_window):
            fn()
        ctx.sync()
        times.append((time.perf_counter() - t0_) * 1e3 / per_window)
    return float(np.median(times))


out = dict(config=args.config, sites=batch.nsites, states=n, nodes=N, windows=args.windows,
           per_window=args.per_window, what='median wall ms per call')
model.prune(batch)
ctx.sync()
out['pruning_kernel'] = batch.kernel_name
for G in (1, 8, 32):
    f = factors(G)
    out['branch_profiles_g%d_sums_only' % G] = median_ms(
        lambda: model.branch_profiles(batch, factors=f))
    out['branch_profiles_g%d_per_site' % G] = median_ms(
        lambda: model.branch_profiles(batch, factors=f, per_site=True))
out['branch_expectations_k8_sums_only'] = median_ms(
    lambda: model.branch_expectations(batch, coefs, per_site=False))
out['step'] = median_ms(lambda: (model.step(batch), model.fetch_totals(batch)))
f8 = factors(8)
got = model.branch_profiles(batch, factors=f8)
out['status_nonzero'] = int(np.count_nonzero(got.status))
if not args.no_loop:
    branches = list(range(1, N))[:: max(1, (N - 1) // args.loop_branches)][:args.loop_branches]
    base = model.fetch_totals(batch)[0]
    loop_sums = np.zeros((len(branches), 8))

    def loop():
        for j, v in enumerate(branches):
            for g in range(8):
                t = t0.copy()
                t[v] = t0[v] * f8[g]
                model.set_rates(Q=Q, node_q=node_q, t=t)
                model.step(batch)
                loop_sums[j, g] = model.fetch_totals(batch)[0] - base

    sampled = median_ms(loop, per_window=1)
    model.set_rates(Q=Q, node_q=node_q, t=t0)
    model.step(batch)
    ctx.sync()
    out['loop_branches_timed'] = len(branches)
    out['loop_g8_sampled_ms'] = sampled
    out['loop_g8_all_branches_ms'] = sampled * (N - 1) / len(branches)
    out['loop_over_call_g8'] = out['loop_g8_all_branches_ms'] / out['branch_profiles_g8_sums_only']
    # the loop and the call agree on what they compute (the totals are sums of ~1e4 terms)
    out['loop_vs_call_max_abs_gap'] = float(np.abs(loop_sums - got.sums[branches]).max())
    out['total_log_likelihood'] = float(base)
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, 'w') as f_:
        f_.write(line + '\n')
