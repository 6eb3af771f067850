"""Diagnostics: milliseconds per rt_sites_posteriors call (resident batch) for one bench
configuration, next to rt_prune on the same batch; under `rocprofv3 --kernel-trace --stats` for
the kernel split.  Sets: the lower half of the states (node set) and the two blocks lower x upper,
upper x lower (edge sets: the switch probabilities of examples/p53/liwen-branch-expectation.py
for the 122-state model).
    python tools/time_posteriors.py [c2|c3|c5|c6] [calls] [sites]"""
import os, sys, time
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from raoteh_amd import device, synth
name = sys.argv[1] if len(sys.argv) > 1 else 'c3'
calls = int(sys.argv[2]) if len(sys.argv) > 2 else 20
nsites = int(sys.argv[3]) if len(sys.argv) > 3 else 10000
cfg = synth.make_config(name, nsites=nsites)
T, root, n = cfg['T'], cfg['root'], cfg['nstates']
model = device.TreeModel(T, root, n)
model.set_root_distn(cfg['root_distn'])
if cfg.get('Q_default') is not None:
    model.set_rates(Q_default=cfg['Q_default'])
else:                                       # per-edge rate matrices on the tree (C5)
    model.set_rates()
batch = model.upload_sites(cfg['leaves'], synth.leaf_likelihoods(cfg), kind='dense')
h = n // 2
lo, hi = list(range(h)), list(range(h, n))


def per_call(fn):
    for _ in range(3):
        fn()
    device.get_context().sync()
    t0 = time.perf_counter()
    for _ in range(calls):
        fn()
    device.get_context().sync()
    return (time.perf_counter() - t0) / calls * 1e3


def prune():
    model.prune(batch)
    model.fetch_totals(batch)


def sets_only():
    return model.posteriors(batch, node_sets=[lo], edge_sets=[(lo, hi), (hi, lo)])


def all_marginals():
    return model.posteriors(batch, node_sets=[lo], edge_sets=[(lo, hi), (hi, lo)], marginals=True)


t_prune = per_call(prune)
t_sets = per_call(sets_only)
t_marg = per_call(all_marginals)
post = sets_only()
print('%s: %d sites, %d states, %d nodes, kernel %s: rt_prune %.3f ms, posteriors (sets only) %.3f '
      'ms, with all marginals %.3f ms; status != 0: %d, node-set sum %.12g, edge-set sum %.12g'
      % (name, batch.nsites, n, model.tree.nnodes, batch.kernel_name, t_prune, t_sets, t_marg,
         int(np.count_nonzero(post.status)), post.node_values.sum(), post.edge_values.sum()))
