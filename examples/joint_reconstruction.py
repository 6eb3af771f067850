#!/usr/bin/env python
"""
The joint maximum-likelihood ancestral reconstruction on the GPU (TreeModel.map_states; Pupko,
Pe'er, Shamir & Graur 2000): for the p53 codon alignment under the MG94 model of
examples/branch_site_map.py, the single most probable assignment of a codon to every node of the
tree at every column -- what codeml prints next to the marginal reconstruction.  Per column: the
posterior probability of the joint reconstruction, exp(log_joint - log-likelihood), and the
number of nodes at which it differs from the arg-max of the marginals
(TreeModel.posteriors(..., marginals=True)), which is another object and need not even be a
possible history.  For one column the reconstructed codons are printed.

    python examples/joint_reconstruction.py [column]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, io      # noqa: E402


def main(argv):
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
    got = model.map_states(batch)
    dt = time.time() - t0
    ll, _ = model.log_likelihoods(batch)
    live = got.status == 0
    print('joint reconstruction of %d codon columns, %d nodes, %d states: %.3f s; %d columns of '
          'zero likelihood' % (batch.nsites, len(got.nodes), n, dt, int((~live).sum())))
    marg = model.posteriors(batch, marginals=True).marginals       # [column, node, codon]
    best = marg.argmax(axis=2)
    differ = (best != got.states).sum(axis=1)
    post = np.exp(got.log_joint - ll)
    print('%6s %12s %12s %10s' % ('column', 'log joint', 'posterior', 'differing'))
    for i in range(batch.nsites):
        if live[i]:
            print('%6d %12.5f %12.5f %10d' % (i, got.log_joint[i], post[i], differ[i]))
        else:
            print('%6d %12s %12s %10s' % (i, '-inf', '-', '-'))
    print('columns whose joint reconstruction differs from the arg-max of the marginals: %d of %d'
          % (int((differ[live] > 0).sum()), int(live.sum())))
    # one column: the least certain one unless the caller names one
    col = int(argv[1]) if len(argv) > 1 else int(np.argmin(np.where(live, post, np.inf)))
    print('column %d (posterior %.5f): node, joint codon, marginal codon (its probability)'
          % (col, post[col]))
    for v, node in enumerate(got.nodes):
        a, b = int(got.states[col, v]), int(best[col, v])
        print('%8s  %s %s  %s %s  (%.4f)%s' % (node, code[a][2], code[a][1], code[b][2], code[b][1],
                                              marg[col, v, b], '' if a == b else '  *'))


if __name__ == '__main__':
    main(sys.argv)
