#!/usr/bin/env python
"""
Joint ancestral reconstruction draws on the GPU (TreeModel.sample_states, the device form of
raoteh/sampler/_sample_mcy_dense.resample_states): for the p53 codon alignment under the MG94
model of examples/branch_site_map.py, 100 joint draws of a codon for every node of the tree at
every column, conditional on the alignment.  Per branch, the fraction of (draw, column) pairs
whose two endpoints differ is printed next to the same probability from the posterior joint
endpoint law (TreeModel.posteriors, the edge sets {a} x not-{a} summed over the codons a).

    python examples/sample_ancestral_states.py [ndraws [seed]]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, io      # noqa: E402


def main(argv):
    ndraws = int(argv[1]) if len(argv) > 1 else 100
    seed = int(argv[2]) if len(argv) > 2 else 1
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    n = len(code)
    Q, distn = io.mg94_from_code(
        code, kappa=3.17632, omega=0.21925,
        nt_freqs=dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883))
    T, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)

    model = device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    model.set_root_distn(distn)
    batch = model.upload_sites(leaves, states, kind='state')
    t0 = time.time()
    got = model.sample_states(batch, ndraws=ndraws, seed=seed)
    dt = time.time() - t0
    live = got.status == 0
    print('%d draws of %d codon columns, %d nodes, %d states: %.3f s; %d columns of zero '
          'likelihood' % (ndraws, batch.nsites, len(got.nodes), n, dt, int((~live).sum())))
    # the same from the posterior joint endpoint law: sum over a of P(parent = a, child != a),
    # eight edge sets per call
    every = set(range(n))
    differ = np.zeros((batch.nsites, len(got.nodes)))
    lim = 8
    for lo in range(0, n, lim):
        esets = [([a], sorted(every - {a})) for a in range(lo, min(n, lo + lim))]
        differ += model.posteriors(batch, edge_sets=esets).edge_values.sum(axis=2)
    parent = model.tree.parent
    t = model.tree.branch_lengths()
    st = got.states[:, live]
    print('%6s %8s %10s %12s %12s' % ('branch', 'node', 'length', 'sampled', 'posterior'))
    for v in range(1, len(got.nodes)):
        sampled = (st[:, :, v] != st[:, :, parent[v]]).mean()
        print('%6d %8s %10.5f %12.5f %12.5f' % (v, got.nodes[v], t[v], sampled,
                                               differ[live, v].mean()))


if __name__ == '__main__':
    main(sys.argv)
