"""Diagnostics: milliseconds per rt_sites_branch_expectations call (resident batch) for one
bench configuration, for 1 and 4 coefficient matrices, with and without the per-site array;
beside it, on the same batch, rt_sites_posteriors with the same number of edge sets whose A is
not every state (the same pass with the same number of extra products, plus re-staging) and one
rt_expect_step (which holds one derivative launch).  Median of nine calls after warm-up.  Prints
one JSON line (and writes it to --out); under `rocprofv3 --kernel-trace --stats` (a run of its
own, --calls 3) for the kernel split.
    python tools/time_branch_expectations.py [c2|c3|c6] [--sites N] [--calls 9] [--out FILE]"""
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
ap.add_argument('--calls', type=int, default=9)
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
rng = np.random.RandomState(1)
coefs = (rng.uniform(size=(4, n, n)) < 0.5).astype(float)
for E in coefs:
    np.fill_diagonal(E, 0.0)
h = n // 2
lo, hi = list(range(h)), list(range(h, n))
sets = [(lo, hi), (hi, lo), (lo, lo), (hi, hi)]


def median_ms(fn):
    for _ in range(3):
        fn()
    device.get_context().sync()
    times = []
    for _ in range(args.calls):
        t0 = time.perf_counter()
        fn()
        device.get_context().sync()
        times.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(times))


out = dict(config=args.config, sites=batch.nsites, states=n, nodes=model.tree.nnodes,
           calls=args.calls, what='median wall ms per call')
model.prune(batch)
out['pruning_kernel'] = batch.kernel_name
for k in (1, 4):
    out['branch_expectations_k%d_sums_only' % k] = median_ms(
        lambda: model.branch_expectations(batch, coefs[:k], per_site=False))
    out['branch_expectations_k%d_per_site' % k] = median_ms(
        lambda: model.branch_expectations(batch, coefs[:k], per_site=True))
    out['posteriors_%d_edge_sets' % k] = median_ms(
        lambda: model.posteriors(batch, edge_sets=sets[:k]))
out['expect_step'] = median_ms(
    lambda: model.expected_history_statistics(batch, recompute_transitions=False))
got = model.branch_expectations(batch, coefs, per_site=False)
out['status_nonzero'] = int(np.count_nonzero(got.status))
out['edge_sums_total'] = [float(x) for x in got.edge_sums.sum(axis=0)]
line = json.dumps(out)
print(line)
if args.out:
    with open(args.out, 'w') as f:
        f.write(line + '\n')
