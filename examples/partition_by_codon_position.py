#!/usr/bin/env python
"""
A partition model on the GPU: the p53 alignment read as nucleotides, its three codon positions
as three 4-state partitions with their own rates -- HKY85 with the nucleotide frequencies the
reference quotes (examples/p53/p53.py:22-27), a transition / transversion ratio and a relative
rate per position (third positions fast, second positions slow) -- evaluated in ONE pruning
launch: column i reads the transition tables of partition i % 3.

    python examples/partition_by_codon_position.py [alignment.phylip tree.newick] [--check]

Defaults to the copies of the reference's data under tests/golden/p53/.  --check evaluates
the three partitions as three ordinary batches as well and compares.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, io, synth      # noqa: E402

NT_FREQS = (0.25039, 0.30126, 0.25952, 0.18883)          # A, C, G, T
# per codon position: (kappa, relative rate); the rates average to one
POSITIONS = ((2.6, 0.55), (2.2, 0.35), (4.1, 2.10))


def main(argv):
    check = '--check' in argv
    argv = [a for a in argv if a != '--check']
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    aln = argv[1] if len(argv) > 1 else os.path.join(data, 'alignment.for.codeml.phylip')
    tree = argv[2] if len(argv) > 2 else os.path.join(data, 'p53S.const.tree')

    T, root, leaf_name_pairs = io.read_newick(open(tree).read())
    codons = dict(io.read_phylip(aln))
    leaves = [leaf for leaf, _ in leaf_name_pairs]
    # nucleotide states uint8[columns, taxa]; anything but A, C, G, T is unobserved
    code = dict(A=0, C=1, G=2, T=3)
    states = np.array([[code.get(ch, 255) for ch in ''.join(codons[name])]
                       for _, name in leaf_name_pairs], dtype=np.uint8).T.copy()
    ncols = states.shape[0]
    position = np.arange(ncols) % 3
    Q = np.array([synth.hky85(kappa, NT_FREQS)[0] * rate for kappa, rate in POSITIONS])
    distn = np.array(NT_FREQS) / np.sum(NT_FREQS)

    model = device.TreeModel(T, root, 4)
    model.set_root_distn(distn)
    batch = model.upload_sites(leaves, states, kind='state', site_sets=position, nsets=3)
    model.set_rate_sets(Q)                       # the tree's branch lengths for every partition
    model.step_partitioned(batch, recompute_transitions=False)
    ll, status = model.fetch_log_likelihoods(batch)
    totals = model.fetch_totals(batch)
    per = model.fetch_partition_totals(batch)
    print('%d taxa, %d nucleotide columns, kernel %s' % (len(leaves), ncols, batch.kernel_name))
    for k, (kappa, rate) in enumerate(POSITIONS):
        print('codon position %d (kappa %.2f, rate %.2f): %4d columns, log likelihood %.10f' % (
            k + 1, kappa, rate, int(per[k, 2]), per[k, 0]))
    print('total log likelihood: %.10f  (%d zero-probability columns)' % (totals[0], int(totals[1])))
    if check:
        for k in range(3):
            model.set_rates(Q_default=Q[k])
            sub = model.upload_sites(leaves, np.ascontiguousarray(states[position == k]), kind='state')
            want, _ = model.log_likelihoods(sub)
            err = np.max(np.abs(ll[position == k] - want) / np.abs(want))
            print('position %d against an ordinary batch: max rel err %.2e' % (k + 1, err))
            assert err < 1e-10
            sub.close()
    batch.close()
    model.close()


if __name__ == '__main__':
    main(sys.argv)
