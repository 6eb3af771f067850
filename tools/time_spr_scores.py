"""Diagnostics: milliseconds per rt_sites_spr_scores call (resident batch) for one bench
configuration -- every SPR move within radius 1, within radius 3 and without a limit, one
fraction, sums only, dense leaves -- beside two yardsticks on the same batch that need nothing but
older calls:
  - one nni_scores call (plain swap, sums only): the same upward pass and `up` pass, reported
    without a gate;
  - the loop a caller would otherwise write, with the tree-specialised kernels off (jit = 0: a
    candidate tree is evaluated once, its kernel would never pay for its compile): per candidate
    the rearranged tree (a helper of this tool) + TreeModel + set_rates + upload_sites + step and
    the fetch of the totals that ends it, timed on --loop-candidates candidates and scaled to the
    moves of every radius.
Median [minimum, maximum] wall ms per call of nine windows after warm-up, each window ended by a
device synchronise and sized from the warm-up to about --window-ms of work (at least
--per-window calls), the forms alternating window by window.  Prints one JSON line (and writes it
to --out).
    python tools/time_spr_scores.py [c2|c3|c6] [--sites N] [--windows 9] [--out FILE]"""
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
ap.add_argument('--window-ms', type=float, default=100.0)
ap.add_argument('--loop-candidates', type=int, default=8)
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
S = batch.nsites
FRACTION = 0.5
RADII = (('r1', 1), ('r3', 3), ('all', None))
model.prune(batch)
ctx.sync()


def regraft(c, y, fraction):
    """The tree with the subtree of node c (a label) hung on a new node that cuts the edge above
    y at `fraction` of its length: the loop's own rearrangement, in networkx alone."""
    ta = model.tree
    parent = dict((ta.preorder_nodes[i], ta.preorder_nodes[int(ta.parent[i])])
                  for i in range(1, ta.nnodes))
    out = T.copy()
    keep = dict(out[parent[c]][c])
    cut = dict(out[parent[y]][y])
    out.remove_edge(parent[c], c)
    out.remove_edge(parent[y], y)
    out.add_edge(parent[y], 'cut', **dict(cut, weight=fraction * cut['weight']))
    out.add_edge('cut', y, **dict(cut, weight=(1.0 - fraction) * cut['weight']))
    out.add_edge('cut', c, **keep)
    return out


forms = {}
for name, radius in RADII:
    forms['spr_%s_sums_only' % name] = \
        lambda radius=radius: model.spr_scores(batch, radius=radius, fractions=(FRACTION,))
forms['nni_scores_g1_sums_only'] = lambda: model.nni_scores(batch)
per_window = dict((k, args.per_window) for k in forms)

got = dict((name, forms['spr_%s_sums_only' % name]()) for name, _ in RADII)
base = float(model.fetch_totals(batch)[0])
if not args.no_loop:
    # candidates spread over the moves without a limit
    moves = got['all'].moves
    picked = moves[:: max(1, len(moves) // args.loop_candidates)][:args.loop_candidates]
    loop_sums = np.zeros(len(picked))
    labels = model.tree.preorder_nodes

    def loop():
        ctx.set_option('jit', 0)
        try:
            for j, (c, y) in enumerate(picked):
                T2 = regraft(labels[int(c)], labels[int(y)], FRACTION)
                other = device.TreeModel(T2, root, n)
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

out = dict(config=args.config, sites=S, states=n, nodes=N, fraction=FRACTION, windows=args.windows,
           per_window=per_window, pruning_kernel=batch.kernel_name,
           what='wall ms per call: median [min, max] of the windows',
           status_nonzero=int(np.count_nonzero(got['all'].status)), total_log_likelihood=base,
           nni_moves=int(len(model.nni_moves())))
for k, ts in times.items():
    out[k] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
for name, _ in RADII:
    call = out['spr_%s_sums_only' % name]
    count = int(len(got[name].moves))
    out['moves_%s' % name] = count
    out['ms_per_1000_moves_%s' % name] = call[0] * 1e3 / max(count, 1)
    out['spr_%s_over_nni_g1' % name] = call[0] / out['nni_scores_g1_sums_only'][0]
if not args.no_loop:
    out['loop_candidates_timed'] = len(picked)
    per_candidate = [x / len(picked) for x in out['loop_sampled']]
    out['loop_ms_per_candidate'] = per_candidate
    for name, _ in RADII:
        b = [x * out['moves_%s' % name] for x in per_candidate]
        a = out['spr_%s_sums_only' % name]
        out['loop_all_%s' % name] = b
        out['loop_over_call_%s' % name] = b[0] / a[0]
        # the ordering by DESIGN.md 3.4c: the medians further apart than the two window ranges
        out['loop_ordering_met_%s' % name] = bool(b[0] - a[0] > max(a[2] - a[1], b[2] - b[1]))
    # the loop and the call agree on what they compute
    where = [got['all'].moves.tolist().index(mv) for mv in picked.tolist()]
    out['loop_vs_call_max_abs_gap'] = float(np.abs(loop_sums - got['all'].sums[where, 0]).max())
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, 'w') as f_:
        f_.write(line + '\n')
