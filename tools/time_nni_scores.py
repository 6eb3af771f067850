"""Diagnostics: milliseconds per rt_sites_nni_scores call (resident batch) for one bench
configuration -- all moves of the tree, sums only and with the per-site array, each with the plain
swap (one point) and with 8 trial lengths of the edge above v -- beside two yardsticks on the same
batch that need nothing but older calls:
  - one branch_profiles call with the same number of points, sums only and per site: the same
    upward pass, exponentials and matrix-pipe products, over the nnodes - 1 edges instead of the
    moves;
  - the loop a caller would otherwise write, with the tree-specialised kernels off (jit = 0: a
    candidate tree is evaluated once, its kernel would never pay for its compile): per move
    nni_apply + TreeModel + set_rates + upload_sites + step and the fetch of the totals that ends
    it, timed on --loop-moves moves and scaled to all of them.
Median [minimum, maximum] wall ms per call of nine windows after warm-up, each window ended by a
device synchronise and sized from the warm-up to about --window-ms of work (at least
--per-window calls), the forms alternating window by window.  Prints one JSON line (and writes it
to --out).
    python tools/time_nni_scores.py [c2|c3|c6] [--sites N] [--windows 9] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth
from raoteh_amd._tree import nni_apply

ap = argparse.ArgumentParser()
ap.add_argument('config', nargs='?', default='c3')
ap.add_argument('--sites', type=int, default=0)
ap.add_argument('--windows', type=int, default=9)
ap.add_argument('--per-window', type=int, default=3)
ap.add_argument('--window-ms', type=float, default=100.0)
ap.add_argument('--loop-moves', type=int, default=8)
ap.add_argument('--no-loop', action='store_true')
ap.add_argument('--out', default='')
args = ap.parse_args()
nsites = args.sites or {'c2': 100000}.get(args.config, 10000)
cfg = synth.make_config(args.config, nsites=nsites)
T, root, n = cfg['T'], cfg['root'], cfg['nstates']
data = synth.leaf_likelihoods(cfg)
model = device.TreeModel(T, root, n)
model.set_root_distn(cfg['root_distn'])
model.set_rates(Q_default=cfg.get('Q_default'))
batch = model.upload_sites(cfg['leaves'], data, kind='dense')
ctx = device.get_context()
N = model.tree.nnodes
moves = model.nni_moves()
f8 = np.exp(np.linspace(-np.log(4), np.log(4), 8))
model.prune(batch)
ctx.sync()

forms = {
    'nni_scores_g1_sums_only': lambda: model.nni_scores(batch),
    'nni_scores_g1_per_site': lambda: model.nni_scores(batch, per_site=True),
    'nni_scores_g8_sums_only': lambda: model.nni_scores(batch, factors=f8),
    'nni_scores_g8_per_site': lambda: model.nni_scores(batch, factors=f8, per_site=True),
    'branch_profiles_g1_sums_only': lambda: model.branch_profiles(batch, factors=[1.0]),
    'branch_profiles_g1_per_site': lambda: model.branch_profiles(batch, factors=[1.0], per_site=True),
    'branch_profiles_g8_sums_only': lambda: model.branch_profiles(batch, factors=f8),
    'branch_profiles_g8_per_site': lambda: model.branch_profiles(batch, factors=f8, per_site=True),
}
per_window = dict((k, args.per_window) for k in forms)

got = model.nni_scores(batch)
base = float(model.fetch_totals(batch)[0])
if not args.no_loop:
    picked = list(range(len(moves)))[:: max(1, len(moves) // args.loop_moves)][:args.loop_moves]
    loop_sums = np.zeros(len(picked))
    labels = model.tree.preorder_nodes

    def loop():
        ctx.set_option('jit', 0)
        try:
            for j, k in enumerate(picked):
                v, c, s = (labels[int(x)] for x in moves[k])
                other = device.TreeModel(nni_apply(T, root, v, c, s), root, n)
                other.set_root_distn(cfg['root_distn'])
                other.set_rates(Q_default=cfg.get('Q_default'))
                ob = other.upload_sites(cfg['leaves'], data, kind='dense')
                other.step(ob)
                loop_sums[j] = other.fetch_totals(ob)[0] - base
                other.close()
        finally:
            ctx.set_option('jit', -1)

    forms['loop_sampled'] = loop
    per_window['loop_sampled'] = 1

for k, fn in forms.items():                      # warm-up: every shape the windows use
    fn()
    ctx.sync()
    t0 = time.perf_counter()
    fn()
    ctx.sync()
    ms = (time.perf_counter() - t0) * 1e3
    per_window[k] = max(per_window[k], min(100, int(np.ceil(args.window_ms / ms))))
times = dict((k, []) for k in forms)
for _ in range(args.windows):
    for k, fn in forms.items():                  # the forms alternate window by window
        t0 = time.perf_counter()
        for _ in range(per_window[k]):
            fn()
        ctx.sync()
        times[k].append((time.perf_counter() - t0) * 1e3 / per_window[k])

out = dict(config=args.config, sites=batch.nsites, states=n, nodes=N, moves=len(moves),
           windows=args.windows, per_window=per_window, pruning_kernel=batch.kernel_name,
           what='wall ms per call: median [min, max] of the windows',
           status_nonzero=int(np.count_nonzero(got.status)), total_log_likelihood=base)
for k, ts in times.items():
    out[k] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
for G in (1, 8):
    for what in ('sums_only', 'per_site'):
        out['nni_over_branch_profiles_g%d_%s' % (G, what)] = (
            out['nni_scores_g%d_%s' % (G, what)][0] / out['branch_profiles_g%d_%s' % (G, what)][0])
if not args.no_loop:
    scale = len(moves) / float(len(picked))
    out['loop_moves_timed'] = len(picked)
    out['loop_all_moves'] = [x * scale for x in out['loop_sampled']]
    out['loop_over_call_g1'] = out['loop_all_moves'][0] / out['nni_scores_g1_sums_only'][0]
    # the ordering by DESIGN.md 3.4c: the medians further apart than the two window ranges
    a, b = out['nni_scores_g1_sums_only'], out['loop_all_moves']
    out['loop_ordering_met'] = bool(b[0] - a[0] > max(a[2] - a[1], b[2] - b[1]))
    # the loop and the call agree on what they compute
    out['loop_vs_call_max_abs_gap'] = float(np.abs(loop_sums - got.sums[picked, 0]).max())
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, 'w') as f_:
        f_.write(line + '\n')
