"""Diagnostics: milliseconds per rt_sites_placements call (resident batch) for one bench
configuration -- queries placed on every edge (state queries; dense 0/1 vectors at c6, whose
leaves are allowed sets), sums only, for 16 queries x 1 fraction x 1 pendant length and for
64 x 3 x 4 -- beside two yardsticks on the same batch that need nothing but
older calls:
  - one nni_scores call (plain swap, sums only): the same upward pass and `up` pass, reported
    without a gate;
  - the loop a caller would otherwise write, with the tree-specialised kernels off (jit = 0: a
    candidate tree is evaluated once, its kernel would never pay for its compile): per candidate
    (query, edge, fraction, pendant length) place_apply + TreeModel + set_rates + upload_sites of
    reference plus query + step and the fetch of the totals that ends it, timed on
    --loop-candidates candidates and scaled to all of them.
Median [minimum, maximum] wall ms per call of nine windows after warm-up, each window ended by a
device synchronise and sized from the warm-up to about --window-ms of work (at least
--per-window calls), the forms alternating window by window.  Prints one JSON line (and writes it
to --out).
    python tools/time_placements.py [c2|c3|c6] [--sites N] [--windows 9] [--out FILE]"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth
from raoteh_amd._tree import place_apply

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
t = model.branch_lengths()
# the queries: the leaves' own columns, shuffled over the leaves site by site (sequences like the
# alignment's, none of them a copy of a leaf)
rng = np.random.RandomState(5)
leaf_states = np.asarray(cfg['leaf_states'])
pick = rng.randint(0, leaf_states.shape[1], size=(64, S))
if cfg['obs_kind'] == 'state':
    kind = 'state'
    queries = leaf_states[np.arange(S)[None, :], pick].astype(np.uint8)
    as_leaf = lambda q: np.eye(n)[queries[q]]
else:                                            # (allowed sets: dense 0/1 vectors, as the leaves)
    kind = 'dense'
    queries = data[np.arange(S)[None, :], pick]
    as_leaf = lambda q: queries[q]
small = dict(fractions=(0.5,), pendant=(float(np.mean(t[1:])),))
large = dict(fractions=(0.25, 0.5, 0.75), pendant=tuple(float(np.mean(t[1:])) * x for x in (0.25, 0.5, 1.0, 2.0)))
model.prune(batch)
ctx.sync()

forms = {
    'place_q16_r1_k1_sums_only': lambda: model.place_queries(batch, queries[:16], kind=kind, **small),
    'place_q64_r3_k4_sums_only': lambda: model.place_queries(batch, queries, kind=kind, **large),
    'nni_scores_g1_sums_only': lambda: model.nni_scores(batch),
}
per_window = dict((k, args.per_window) for k in forms)

got_small = forms['place_q16_r1_k1_sums_only']()
got_large = forms['place_q64_r3_k4_sums_only']()
base = float(model.fetch_totals(batch)[0])
if not args.no_loop:
    # candidates of the large call, spread over queries, edges, fractions and pendant lengths
    R, K = len(large['fractions']), len(large['pendant'])
    total = 64 * (N - 1) * R * K
    flat = np.arange(total)[:: max(1, total // args.loop_candidates)][:args.loop_candidates]
    picked = [np.unravel_index(int(x), (64, N - 1, R, K)) for x in flat]
    picked = [(int(q), int(v) + 1, int(r), int(k)) for q, v, r, k in picked]
    loop_sums = np.zeros(len(picked))
    labels = model.tree.preorder_nodes

    def loop():
        ctx.set_option('jit', 0)
        try:
            for j, (q, v, r, k) in enumerate(picked):
                T2 = place_apply(T, root, labels[v], large['fractions'][r], large['pendant'][k], 'query')
                other = device.TreeModel(T2, root, n)
                other.set_root_distn(cfg['root_distn'])
                other.set_rates(Q_default=cfg.get('Q_default'))
                both = np.concatenate([data, as_leaf(q)[:, None, :]], axis=1)
                ob = other.upload_sites(list(cfg['leaves']) + ['query'], both, kind='dense')
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

out = dict(config=args.config, sites=S, states=n, nodes=N, query_kind=kind, windows=args.windows,
           per_window=per_window, pruning_kernel=batch.kernel_name,
           what='wall ms per call: median [min, max] of the windows',
           status_nonzero=int(np.count_nonzero(got_large.status)), total_log_likelihood=base,
           placements_small=16 * (N - 1), placements_large=64 * (N - 1) * 12)
for k, ts in times.items():
    out[k] = [float(np.median(ts)), float(np.min(ts)), float(np.max(ts))]
out['place_q16_over_nni_g1'] = out['place_q16_r1_k1_sums_only'][0] / out['nni_scores_g1_sums_only'][0]
if not args.no_loop:
    out['loop_candidates_timed'] = len(picked)
    per_candidate = [x / len(picked) for x in out['loop_sampled']]
    out['loop_ms_per_candidate'] = per_candidate
    for name, count, call in (('small', 16 * (N - 1), 'place_q16_r1_k1_sums_only'),
                              ('large', 64 * (N - 1) * 12, 'place_q64_r3_k4_sums_only')):
        b = [x * count for x in per_candidate]
        a = out[call]
        out['loop_all_%s' % name] = b
        out['loop_over_call_%s' % name] = b[0] / a[0]
        # the ordering by DESIGN.md 3.4c: the medians further apart than the two window ranges
        out['loop_ordering_met_%s' % name] = bool(b[0] - a[0] > max(a[2] - a[1], b[2] - b[1]))
    # the loop and the call agree on what they compute
    want = np.array([got_large.sums[q, v, r, k] for q, v, r, k in picked])
    out['loop_vs_call_max_abs_gap'] = float(np.abs(loop_sums - want).max())
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, 'w') as f_:
        f_.write(line + '\n')
