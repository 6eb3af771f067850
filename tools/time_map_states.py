"""Diagnostics: milliseconds per rt_sites_map_states call (resident batch) for one bench
configuration, next to rt_sites_sample_states with one draw (the sum-product call of the same
shape: an upward pass with L of every node stored, then one downward walk) and rt_prune on the
same batch: the median, minimum and maximum of nine windows of `calls` calls each; under
`rocprofv3 --kernel-trace --stats` for the split between the upward and the downward kernel.
One JSON line at the end.
    python tools/time_map_states.py [c2|c3|c5|c6] [calls] [sites]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth
name = sys.argv[1] if len(sys.argv) > 1 else 'c3'
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
nsites = int(sys.argv[3]) if len(sys.argv) > 3 else None     # (None: the bench size)
WINDOWS = 9
cfg = synth.make_config(name, nsites=nsites)
T, root, n = cfg['T'], cfg['root'], cfg['nstates']
model = device.TreeModel(T, root, n)
model.set_root_distn(cfg['root_distn'])
if cfg.get('Q_default') is not None:
    model.set_rates(Q_default=cfg['Q_default'])
else:                                       # per-edge rate matrices on the tree (C5)
    model.set_rates()
batch = model.upload_sites(cfg['leaves'], synth.leaf_likelihoods(cfg), kind='dense')


def windows(fn):
    """(median, min, max) over WINDOWS windows of the milliseconds per call."""
    for _ in range(2):
        fn()
    out = []
    for _ in range(WINDOWS):
        device.get_context().sync()
        t0 = time.perf_counter()
        for _ in range(calls):
            fn()
        device.get_context().sync()
        out.append((time.perf_counter() - t0) / calls * 1e3)
    return float(np.median(out)), float(min(out)), float(max(out))


def prune():
    model.prune(batch)
    model.fetch_totals(batch)


N = model.tree.nnodes
prune()                                     # (the batch has its kernel's name from here on)
res = {'config': name, 'sites': batch.nsites, 'states': n, 'nodes': N,
       'kernel': batch.kernel_name, 'calls_per_window': calls, 'windows': WINDOWS,
       # the upward pass: one multiply and one compare per (site, edge, a, b)
       'multiply_compare_pairs': int(batch.nsites) * (N - 1) * n * n,
       'prune_ms': windows(prune),
       'sample_states_1_ms': windows(lambda: model.sample_states(batch, ndraws=1, seed=1)),
       'map_states_ms': windows(lambda: model.map_states(batch))}
got = model.map_states(batch)
ll, _ = model.log_likelihoods(batch)
live = got.status == 0
res['status_nonzero'] = int(np.count_nonzero(got.status))
res['median_posterior_of_reconstruction'] = float(np.median(np.exp(got.log_joint[live] - ll[live])))
res['map_over_sample_1'] = res['map_states_ms'][0] / res['sample_states_1_ms'][0]
print('%s: %d sites, %d states, %d nodes, kernel %s: rt_prune %.3f ms' % (
    name, batch.nsites, n, N, batch.kernel_name, res['prune_ms'][0]))
print('  sample_states, 1 draw: %.3f ms [%.3f, %.3f]' % res['sample_states_1_ms'])
print('  map_states:            %.3f ms [%.3f, %.3f]  (%.2f x; %.3g multiply-compare pairs)' % (
    res['map_states_ms'] + (res['map_over_sample_1'], res['multiply_compare_pairs'])))
print(json.dumps(res))
