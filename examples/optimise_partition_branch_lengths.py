#!/usr/bin/env python
"""
Fitting a partition model on the GPU: the p53 alignment read as nucleotides, its three codon
positions as three 4-state HKY85 partitions (the set-up of partition_by_codon_position.py) on ONE
tree shared by the partitions.  Branch v of partition k has length t[k][v] = r_k * tau_v; the
shared lengths tau and the multipliers r_k (r_1 = 1 fixes the scale) are fitted with L-BFGS-B.
Each iteration takes the value from step_partitioned -- one pruning launch for all columns -- and
the gradient from branch_length_gradient_partitioned -- one call for d / d t[k][v] of every
partition and branch -- through the chain rule d / d tau_v = sum_k r_k g[k, v], d / d r_k =
sum_v tau_v g[k, v] (device.partition_chain_rule).

    python examples/optimise_partition_branch_lengths.py [alignment.phylip tree.newick]

Defaults to the copies of the reference's data under tests/golden/p53/.
"""
import os
import sys

import numpy as np
import scipy.optimize

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, io, synth      # noqa: E402

NT_FREQS = (0.25039, 0.30126, 0.25952, 0.18883)          # A, C, G, T
KAPPAS = (2.6, 2.2, 4.1)                                 # per codon position
START_RATES = (1.0, 1.0, 1.0)
FLOOR = 1e-8                                             # shortest branch the fit may reach


def main(argv):
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    aln = argv[1] if len(argv) > 1 else os.path.join(data, 'alignment.for.codeml.phylip')
    tree = argv[2] if len(argv) > 2 else os.path.join(data, 'p53S.const.tree')

    T, root, leaf_name_pairs = io.read_newick(open(tree).read())
    codons = dict(io.read_phylip(aln))
    leaves = [leaf for leaf, _ in leaf_name_pairs]
    code = dict(A=0, C=1, G=2, T=3)
    states = np.array([[code.get(ch, 255) for ch in ''.join(codons[name])]
                       for _, name in leaf_name_pairs], dtype=np.uint8).T.copy()
    ncols = states.shape[0]
    position = np.arange(ncols) % 3
    Q = np.array([synth.hky85(kappa, NT_FREQS)[0] for kappa in KAPPAS])
    distn = np.array(NT_FREQS) / np.sum(NT_FREQS)

    model = device.TreeModel(T, root, 4)
    model.set_root_distn(distn)
    batch = model.upload_sites(leaves, states, kind='state', site_sets=position, nsets=3)
    N = model.tree.nnodes
    tau0 = np.maximum(model.tree.branch_lengths()[1:], 1e-4)
    evaluations = [0]

    def lengths(x):
        tau = np.concatenate([[0.0], np.exp(x[:N - 1])])
        r = np.concatenate([[1.0], np.exp(x[N - 1:])])
        return tau, r

    def objective(x):
        """-(log likelihood) and its gradient in (log tau_1.., log r_2, log r_3)."""
        tau, r = lengths(x)
        model.set_rate_sets(Q, t=r[:, None] * tau[None, :])
        model.step_partitioned(batch, recompute_transitions=False)
        total, nzero, _ = model.fetch_totals(batch)
        if nzero:
            raise SystemExit('%d columns of zero likelihood' % nzero)
        g = model.branch_length_gradient_partitioned(batch)
        d_tau, d_r = device.partition_chain_rule(g, r, tau)
        evaluations[0] += 1
        return -total, -np.concatenate([tau[1:] * d_tau[1:], r[1:] * d_r[1:]])

    x0 = np.concatenate([np.log(tau0), np.log(START_RATES[1:])])
    start, _ = objective(x0)
    print('%d taxa, %d nucleotide columns in 3 partitions, %d branches; start %.6f'
          % (len(leaves), ncols, N - 1, -start))
    bounds = [(np.log(FLOOR), np.log(50.0))] * (N - 1) + [(np.log(1e-3), np.log(1e3))] * 2
    fit = scipy.optimize.minimize(objective, x0, jac=True, method='L-BFGS-B', bounds=bounds,
                                  options=dict(maxiter=500, ftol=1e-12, gtol=1e-6))
    tau, r = lengths(fit.x)
    # the same model with the rates averaging to one over the columns
    counts = np.bincount(position, minlength=3)
    mean = float(np.dot(r, counts)) / ncols
    print('%s after %d iterations, %d evaluations (each: one step_partitioned + one gradient call)'
          % ('converged' if fit.success else 'stopped: %s' % fit.message, fit.nit, evaluations[0]))
    print('log likelihood %.6f (start %.6f); largest |gradient| %.2e'
          % (-fit.fun, -start, np.abs(fit.jac).max()))
    print('relative rates of the codon positions: %s; tree length %.4f'
          % (', '.join('%.4f' % (x / mean) for x in r), tau.sum() * mean))
    assert -fit.fun >= -start
    batch.close()
    model.close()


if __name__ == '__main__':
    main(sys.argv)
