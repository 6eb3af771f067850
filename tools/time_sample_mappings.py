"""Diagnostics: milliseconds per rt_sites_sample_mappings call (resident batch) for one bench
configuration with one and four coefficient matrices, means only (per_draw=False) and with the
per-draw values and counts, next to rt_sites_sample_states for the same draws and
rt_sites_branch_expectations for the same coefficients on the same batch: the median of nine
windows of `calls` calls each; under `rocprofv3 --kernel-trace --stats` for the kernel split.
One JSON line at the end.
    python tools/time_sample_mappings.py [c2|c3|c5|c6] [calls] [sites] [ndraws]"""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth
name = sys.argv[1] if len(sys.argv) > 1 else 'c3'
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 3
nsites = int(sys.argv[3]) if len(sys.argv) > 3 else None     # (None: the bench size)
ndraws = int(sys.argv[4]) if len(sys.argv) > 4 else 16
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
rng = np.random.RandomState(1)
coefs = (rng.uniform(size=(4, n, n)) < 0.5).astype(float)    # indicators of labelled changes
for E in coefs:
    np.fill_diagonal(E, 0.0)


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


res = {'config': name, 'sites': batch.nsites, 'states': n, 'nodes': model.tree.nnodes,
       'kernel': batch.kernel_name, 'calls_per_window': calls, 'windows': WINDOWS,
       'ndraws': ndraws,
       'sample_states_ms': windows(lambda: model.sample_states(batch, ndraws=ndraws, seed=1))}
for nk in (1, 4):
    E = coefs[:nk]
    res['branch_expectations_%d_ms' % nk] = windows(
        lambda: model.branch_expectations(batch, E, per_site=False))
    res['means_only_%d_ms' % nk] = windows(
        lambda: model.sample_mappings(batch, E, ndraws=ndraws, seed=1, per_draw=False))
    res['per_draw_%d_ms' % nk] = windows(
        lambda: model.sample_mappings(batch, E, ndraws=ndraws, seed=1))
    res['paths_over_states_%d' % nk] = res['means_only_%d_ms' % nk][0] / res['sample_states_ms'][0]
    res['draws_per_expectation_call_%d' % nk] = (
        ndraws * res['branch_expectations_%d_ms' % nk][0] / res['means_only_%d_ms' % nk][0])
got = model.sample_mappings(batch, coefs, ndraws=ndraws, seed=1)
res['status_nonzero'] = int(np.count_nonzero(got.status))
res['mean_events'] = float(got.counts[:, :, 1:, 0].mean())
res['max_events'] = int(got.counts[..., 0].max())
res['mean_changes'] = float(got.counts[:, :, 1:, 1].mean())
print('%s: %d sites, %d states, %d nodes, kernel %s, %d draws: sample_states %.3f ms'
      % (name, batch.nsites, n, model.tree.nnodes, batch.kernel_name, ndraws,
         res['sample_states_ms'][0]))
for nk in (1, 4):
    print('  %d coefficient matrices: means only %.3f ms [%.3f, %.3f], per draw %.3f ms, '
          'branch_expectations %.3f ms; %.2f x sample_states, one expectation call buys %.1f draws'
          % ((nk,) + res['means_only_%d_ms' % nk] + (res['per_draw_%d_ms' % nk][0],
             res['branch_expectations_%d_ms' % nk][0], res['paths_over_states_%d' % nk],
             res['draws_per_expectation_call_%d' % nk])))
print(json.dumps(res))
