"""Diagnostics: milliseconds per rt_sites_sample_states call (resident batch) for one bench
configuration at 1, 16 and 128 draws (or the one count given), next to rt_sites_posteriors with
one node set on the same batch: the median of nine windows of `calls` calls each; under
`rocprofv3 --kernel-trace --stats` for the kernel split.  One JSON line at the end.
    python tools/time_sample_states.py [c2|c3|c5|c6] [calls] [sites] [ndraws]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth
name = sys.argv[1] if len(sys.argv) > 1 else 'c3'
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 5
nsites = int(sys.argv[3]) if len(sys.argv) > 3 else None     # (None: the bench size)
draws = [int(sys.argv[4])] if len(sys.argv) > 4 else [1, 16, 128]
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
lo = list(range(n // 2))


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


res = {'config': name, 'sites': batch.nsites, 'states': n, 'nodes': model.tree.nnodes,
       'kernel': batch.kernel_name, 'calls_per_window': calls, 'windows': WINDOWS,
       'draw_block': device._lib.lib().rt_sample_states_draw_block(model.tree.nnodes),
       'prune_ms': windows(prune),
       'posteriors_one_node_set_ms': windows(lambda: model.posteriors(batch, node_sets=[lo]))}
for nd in draws:
    res['sample_states_%d_ms' % nd] = windows(lambda: model.sample_states(batch, ndraws=nd, seed=1))
got = model.sample_states(batch, ndraws=draws[0], seed=1)
res['status_nonzero'] = int(np.count_nonzero(got.status))
print('%s: %d sites, %d states, %d nodes, kernel %s: rt_prune %.3f ms, posteriors (one node set) '
      '%.3f ms [%.3f, %.3f]' % ((name, batch.nsites, n, model.tree.nnodes, batch.kernel_name,
                                 res['prune_ms'][0]) + res['posteriors_one_node_set_ms']))
for nd in draws:
    print('  sample_states, %4d draws: %.3f ms [%.3f, %.3f]' % ((nd,) + res['sample_states_%d_ms' % nd]))
print(json.dumps(res))
