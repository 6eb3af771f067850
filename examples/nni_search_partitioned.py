#!/usr/bin/env python
"""
The NNI search of examples/nni_search.py on a partitioned alignment: the p53 alignment read as
nucleotides, its three codon positions as three 4-state HKY85 partitions on ONE shared tree (the
set-up of examples/optimise_partition_branch_lengths.py), branch v of partition k at length
t[k][v] = r_k * tau_v with fixed relative rates r.  The start is the fixture's tree with two leaves
exchanged.  Each round:

  1. ONE nni_scores_partitioned call: every NNI neighbour of the current tree, every column under
     its own partition's rates, the edge above v at a small grid of factors of its length (the
     same factor in every partition) -- nothing but the sums leaves the device;
  2. the best improving (move, factor) is adopted with _tree.nni_apply, a new model is built for
     the tree and the alignment uploaded;
  3. the shared lengths tau are fitted again with branch_profiles_partitioned: one common factor
     per branch for all partitions, chosen from a grid per fitting round.

The log-likelihood of step_partitioned is printed per round.

    python examples/nni_search_partitioned.py [leaf_a leaf_b]
"""
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from raoteh_amd import io, synth                   # noqa: E402
from raoteh_amd._tree import nni_apply             # noqa: E402
from raoteh_amd.device import TreeModel            # noqa: E402
from nni_search import splits                      # noqa: E402

NT_FREQS = (0.25039, 0.30126, 0.25952, 0.18883)    # A, C, G, T
KAPPAS = (2.6, 2.2, 4.1)                           # per codon position
RATES = (0.75, 0.5, 1.75)                          # relative rates of the codon positions
FACTORS = np.exp(np.linspace(-np.log(4.0), np.log(4.0), 5))     # of the length of the edge above v
FIT_ROUNDS = 4
MIN_GAIN = 1e-3


class Fit(object):
    """A model with the three rate sets and a resident partitioned batch for one tree; the shared
    lengths tau live in the tree's 'weight's."""

    def __init__(self, T, root, Q, distn, leaves, states, position):
        self.T, self.root, self.Q = T, root, Q
        self.r = np.array(RATES)
        self.model = TreeModel(T, root, 4)
        self.model.set_root_distn(distn)
        self.tau = self.model.tree.branch_lengths()
        self.batch = self.model.upload_sites(leaves, states, kind='state', site_sets=position,
                                             nsets=len(RATES))
        self.calls = 1
        self.set_lengths(self.tau)

    def set_lengths(self, tau):
        self.model.set_rate_sets(self.Q, t=self.r[:, None] * tau[None, :])
        self.calls += 1

    def total(self):
        """The log-likelihood of the batch at the resident lengths: one pruning launch."""
        self.model.step_partitioned(self.batch, recompute_transitions=False)
        self.calls += 1
        total, nzero, _ = self.model.fetch_totals(self.batch)
        return -np.inf if nzero else float(total)

    def fit_lengths(self, rounds):
        """Per round one branch_profiles_partitioned call over a grid of factors: every branch moved
        to its best grid point at once, the move halved while the total does not improve.  -> the
        log-likelihood."""
        best = self.total()
        span = np.log(2.0)
        for _ in range(rounds):
            x = np.linspace(-span, span, 9)
            prof = self.model.branch_profiles_partitioned(self.batch, np.exp(x))
            self.calls += 1
            move = np.zeros(len(self.tau))
            for v in range(1, len(self.tau)):
                if self.tau[v] > 0 and np.isfinite(prof.sums[v]).any():
                    move[v] = x[int(np.nanargmax(prof.sums[v]))]
            scale, accepted = 1.0, False
            for _ in range(5):
                trial = self.tau * np.exp(scale * move)
                self.set_lengths(trial)
                now = self.total()
                if now > best:
                    self.tau, best, accepted = trial, now, True
                    break
                scale *= 0.5
            if not accepted:
                self.set_lengths(self.tau)
                break
            span = max(0.5 * span, 0.02)
        ta = self.model.tree
        for i in range(1, ta.nnodes):            # the fitted lengths back into the tree
            self.T[ta.preorder_nodes[int(ta.parent[i])]][ta.preorder_nodes[i]]['weight'] = float(self.tau[i])
        return best

    def close(self):
        self.batch.close()
        self.model.close()


def main(argv):
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    T0, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    codons = dict(io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')))
    leaves = [leaf for leaf, _ in leaf_name_pairs]
    code = dict(A=0, C=1, G=2, T=3)
    states = np.array([[code.get(ch, 255) for ch in ''.join(codons[name])]
                       for _, name in leaf_name_pairs], dtype=np.uint8).T.copy()
    position = np.arange(states.shape[0]) % 3
    Q = np.array([synth.hky85(kappa, NT_FREQS)[0] for kappa in KAPPAS])
    distn = np.array(NT_FREQS) / np.sum(NT_FREQS)
    names = dict(leaf_name_pairs)
    by_name = dict((name, v) for v, name in leaf_name_pairs)
    a, b = (by_name[x] for x in (argv[1:3] if len(argv) > 2 else ('Has', 'Ppy')))
    truth = splits(T0, root)
    T = nx.relabel_nodes(T0, {a: b, b: a}, copy=True)
    args = (Q, distn, leaves, states, position)
    print('%d taxa, %d nucleotide columns in %d partitions; %s and %s exchanged: %d of %d splits of '
          'the fixture\'s tree are missing'
          % (len(leaves), len(states), len(RATES), names[a], names[b],
             len(truth - splits(T, root)), len(truth)))
    fit = Fit(T, root, *args)
    best = fit.fit_lengths(FIT_ROUNDS)
    calls, rnd = fit.calls, 0
    print('start: log-likelihood %.6f after the length fit' % best)
    while True:
        rnd += 1
        scores = fit.model.nni_scores_partitioned(fit.batch, FACTORS)       # every neighbour
        calls += 1
        k, g = np.unravel_index(int(np.nanargmax(scores.sums)), scores.sums.shape)
        gain = float(scores.sums[k, g])
        if not gain > MIN_GAIN:
            print('round %d: %d moves scored, none improves (best %.3g): done; log-likelihood %.6f'
                  % (rnd, len(scores.moves), gain, best))
            break
        labels = fit.model.tree.preorder_nodes
        iv = int(scores.moves[k, 0])
        v, c, s = (labels[int(x)] for x in scores.moves[k])
        p = labels[int(fit.model.tree.parent[iv])]
        T = nni_apply(fit.T, root, v, c, s)
        T[p][v]['weight'] = float(scores.factors[iv, g] * fit.tau[iv])
        fit.close()
        fit = Fit(T, root, *args)
        moved = fit.total() - best
        best = fit.fit_lengths(FIT_ROUNDS)
        calls += fit.calls
        print('round %d: %d moves scored; the best, %s, promised %+.6f and gave %+.6f; '
              'log-likelihood %.6f after the length fit; %d splits missing'
              % (rnd, len(scores.moves), [int(x) for x in scores.moves[k]], gain, moved, best,
                 len(truth - splits(T, root))))
    recovered = splits(fit.T, root) == truth
    print('final log-likelihood %.6f after %d device calls; the fixture\'s tree was %s'
          % (best, calls, 'recovered' if recovered else 'NOT recovered'))
    fit.close()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
