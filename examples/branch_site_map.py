#!/usr/bin/env python
"""
The reference's branch-site map (examples/p53/liwen-branch-expectation.py, "the posterior
expected number of changes at the site"; examples/code2x3/extras.get_expected_ntransitions) on
the GPU: for the p53 codon alignment under the MG94 model of examples/p53_loglik.py, the
expected number of synonymous and of non-synonymous substitutions at every codon column on
every branch, conditional on the alignment -- one device call for all columns, branches and
both kinds (TreeModel.branch_expectations), plus the analytic gradient of the log-likelihood
in the branch lengths from the same pass (TreeModel.branch_length_gradient).

    python examples/branch_site_map.py [branch [top]]

branch: preorder index of the node below the branch whose top sites are listed (default: the
branch with the most expected non-synonymous changes); top: how many sites (default 10).
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
    # coefficient matrices: 1 where the amino acid stays resp. changes (zero diagonal: counts)
    residue = np.array([r for _, r, _ in code])
    syn = (residue[:, None] == residue[None, :]).astype(float)
    np.fill_diagonal(syn, 0.0)
    nonsyn = 1.0 - syn
    np.fill_diagonal(nonsyn, 0.0)

    model = device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    model.set_root_distn(distn)
    batch = model.upload_sites(leaves, states, kind='state')
    t0 = time.time()
    got = model.branch_expectations(batch, [syn, nonsyn])
    grad = model.branch_length_gradient(batch)
    dt = time.time() - t0
    t = model.tree.branch_lengths()
    print('%d codon columns, %d branches, %d states: %.3f s; %d columns of zero likelihood' % (
        batch.nsites, len(got.nodes) - 1, n, dt, int((got.status & 1).sum())))
    print('%6s %8s %10s %10s %10s %12s' % ('branch', 'node', 'length', 'syn', 'nonsyn',
                                          'dlogL/dt'))
    for v in range(1, len(got.nodes)):
        print('%6d %8s %10.5f %10.4f %10.4f %12.4f' % (
            v, got.nodes[v], t[v], got.edge_sums[v, 0], got.edge_sums[v, 1], grad[v]))
    print('%6s %8s %10.5f %10.4f %10.4f' % ('all', '', t[1:].sum(), got.edge_sums[:, 0].sum(),
                                           got.edge_sums[:, 1].sum()))
    branch = int(argv[1]) if len(argv) > 1 else int(np.argmax(got.edge_sums[:, 1]))
    top = int(argv[2]) if len(argv) > 2 else 10
    order = np.argsort(-got.values[:, branch, 1])[:top]
    print('branch %d (above node %s): the %d columns with the most expected non-synonymous '
          'changes' % (branch, got.nodes[branch], len(order)))
    for i in order:
        print('  column %4d: syn %.4f  nonsyn %.4f' % (i + 1, got.values[i, branch, 0],
                                                      got.values[i, branch, 1]))


if __name__ == '__main__':
    main(sys.argv)
