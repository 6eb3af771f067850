#!/usr/bin/env python
"""
Stochastic mappings of the p53 codon alignment (Nielsen 2002; the uniformization sampler of
Hobolth & Stone 2009) on the GPU: under the MG94 model of examples/p53_loglik.py, independent
draws of a substitution history on every branch at every codon column, conditional on the
alignment (TreeModel.sample_mappings), each reduced to its number of synonymous and of
non-synonymous changes.  Per branch the mean over the draws and columns is printed next to the
exact expectation of examples/branch_site_map.py (TreeModel.branch_expectations), which it
converges to, with the standard deviation over the draws -- the spread behind that mean, which
the expectation alone does not give.

    python examples/sample_mappings.py [ndraws [seed]]
"""
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, io      # noqa: E402


def main(argv):
    ndraws = int(argv[1]) if len(argv) > 1 else 200
    seed = int(argv[2]) if len(argv) > 2 else 2002
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    n = len(code)
    Q, distn = io.mg94_from_code(
        code, kappa=3.17632, omega=0.21925,
        nt_freqs=dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883))
    T, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)
    residue = np.array([r for _, r, _ in code])
    syn = (residue[:, None] == residue[None, :]).astype(float)
    np.fill_diagonal(syn, 0.0)
    nonsyn = 1.0 - syn
    np.fill_diagonal(nonsyn, 0.0)

    model = device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    model.set_root_distn(distn)
    batch = model.upload_sites(leaves, states, kind='state')
    want = model.branch_expectations(batch, [syn, nonsyn])
    t0 = time.time()
    got = model.sample_mappings(batch, [syn, nonsyn], ndraws=ndraws, seed=seed)
    dt = time.time() - t0
    # per draw: the changes of a kind on a branch, summed over the columns
    per_draw = got.values.sum(axis=1)                       # [ndraws, nnodes, 2]
    mean, sd = per_draw.mean(axis=0), per_draw.std(axis=0, ddof=1 if ndraws > 1 else 0)
    t = model.tree.branch_lengths()
    print('%d draws of %d codon columns, %d branches, %d states: %.3f s; %.2f uniformized events '
          'and %.3f changes per branch and column' % (
              ndraws, batch.nsites, len(got.nodes) - 1, n, dt, got.counts[:, :, 1:, 0].mean(),
              got.counts[:, :, 1:, 1].mean()))
    print('%6s %8s %9s | %9s %9s %8s | %9s %9s %8s' % (
        'branch', 'node', 'length', 'E[syn]', 'mean', 'sd', 'E[nonsyn]', 'mean', 'sd'))
    for v in range(1, len(got.nodes)):
        print('%6d %8s %9.5f | %9.3f %9.3f %8.3f | %9.3f %9.3f %8.3f' % (
            v, got.nodes[v], t[v], want.edge_sums[v, 0], mean[v, 0], sd[v, 0],
            want.edge_sums[v, 1], mean[v, 1], sd[v, 1]))
    tot = per_draw.sum(axis=1)
    print('%6s %8s %9.5f | %9.3f %9.3f %8.3f | %9.3f %9.3f %8.3f' % (
        'all', '', t[1:].sum(), want.edge_sums[:, 0].sum(), tot[:, 0].mean(), tot[:, 0].std(),
        want.edge_sums[:, 1].sum(), tot[:, 1].mean(), tot[:, 1].std()))
    ratio = tot[:, 1] / np.maximum(tot[:, 0], 1.0)
    print('non-synonymous per synonymous change over the tree: %.3f +- %.3f over the draws' % (
        ratio.mean(), ratio.std()))
    # every change is of one kind or the other
    assert np.array_equal(np.rint(got.values.sum(axis=3)).astype(np.int64), got.counts[..., 1])
    dev = np.abs(mean - want.edge_sums) / np.maximum(sd / np.sqrt(ndraws), 1e-12)
    print('largest deviation of a branch mean from its expectation: %.2f standard errors' % (
        dev[1:].max()))


if __name__ == '__main__':
    main(sys.argv)
