#!/usr/bin/env python
"""
A tree search by nearest-neighbour interchanges on the p53 codon alignment (tests/golden/p53/,
MG94 with the PAML estimates of examples/p53_loglik.py).  The start is the fixture's tree with two
leaves exchanged.  Each round:

  1. ONE nni_scores call: every NNI neighbour of the current tree, with the edge above v at a
     grid of factors of its length, from one upward and one downward pass on the resident batch;
  2. the best improving (move, length) is adopted: _tree.nni_apply rearranges the tree, a new
     TreeModel is built for it and the alignment uploaded;
  3. the branch lengths are fitted again, one branch_profiles call per fitting round (the scheme
     of examples/optimise_branch_lengths.py).

It stops when no move improves by more than MIN_GAIN, and says whether the fixture's tree (as an
unrooted topology) was recovered; the fixture's own tree with its lengths fitted the same way is
printed first, for comparison (the fixture's topology need not be the best one under this model).

    python examples/nni_search.py [leaf_a leaf_b]
"""
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import io                          # noqa: E402
from raoteh_amd._tree import TreeArrays, nni_apply  # noqa: E402
from raoteh_amd.device import TreeModel            # noqa: E402

FACTORS = np.exp(np.linspace(-np.log(4.0), np.log(4.0), 9))     # of the length of the edge above v
FIT_ROUNDS = 4
MIN_GAIN = 1e-3     # log-likelihood units: below it a move only flips a branch of length ~0


def splits(T, root):
    """The unrooted topology: the non-trivial bipartitions of the leaves, each as the side that
    does not hold the first leaf."""
    ta = TreeArrays(T, root)
    kids = np.diff(ta.indptr)
    below = [set() for _ in range(ta.nnodes)]
    for v in range(ta.nnodes - 1, -1, -1):
        if kids[v] == 0:
            below[v].add(ta.preorder_nodes[v])
        if v:
            below[int(ta.parent[v])] |= below[v]
    leaves = frozenset(below[0])
    first = min(leaves)
    out = set()
    for v in range(1, ta.nnodes):
        side = frozenset(below[v])
        if first in side:
            side = leaves - side
        if 1 < len(side) < len(leaves) - 1:
            out.add(side)
    return out


class Fit(object):
    """A model and a resident batch for one tree; the lengths live in the tree's 'weight's."""

    def __init__(self, T, root, n, Q, distn, leaves, patterns, weights):
        self.T, self.root, self.Q, self.weights = T, root, Q, weights
        self.model = TreeModel(T, root, n)
        self.model.set_root_distn(distn)
        self.t = self.model.tree.branch_lengths()
        self.model.set_rates(Q=Q, t=self.t)
        self.batch = self.model.upload_sites(leaves, patterns, kind='state')
        self.batch.set_weights(weights)
        self.calls = 1

    def total(self):
        ll, status = self.model.log_likelihoods(self.batch)
        return float(np.dot(self.weights, ll)) if not (status & 1).any() else -np.inf

    def fit_lengths(self, rounds):
        """Per round one branch_profiles call over a grid of factors, every branch moved to its
        best grid point at once, the move halved while the total does not improve."""
        best = self.total()
        span = np.log(2.0)
        for _ in range(rounds):
            x = np.linspace(-span, span, 9)
            prof = self.model.branch_profiles(self.batch, factors=np.exp(x))
            self.calls += 1
            move = np.zeros(len(self.t))
            for v in range(1, len(self.t)):
                if self.t[v] > 0 and np.isfinite(prof.sums[v]).any():
                    move[v] = x[int(np.nanargmax(prof.sums[v]))]
            scale, accepted = 1.0, False
            for _ in range(5):
                trial = self.t * np.exp(scale * move)
                self.model.set_rates(Q=self.Q, t=trial)
                self.calls += 1
                now = self.total()
                if now > best:
                    self.t, best, accepted = trial, now, True
                    break
                scale *= 0.5
            if not accepted:
                self.model.set_rates(Q=self.Q, t=self.t)
                break
            span = max(0.5 * span, 0.02)
        ta = self.model.tree
        for i in range(1, ta.nnodes):            # the fitted lengths back into the tree
            self.T[ta.preorder_nodes[int(ta.parent[i])]][ta.preorder_nodes[i]]['weight'] = float(self.t[i])
        return best

    def close(self):
        self.model.close()


def main(argv):
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    Q, distn = io.mg94_from_code(
        code, kappa=3.17632, omega=0.21925,
        nt_freqs=dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883))
    T0, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)
    patterns, _, counts = io.compress_patterns(states)
    weights = counts.astype(np.float64)
    names = dict(leaf_name_pairs)
    by_name = dict((name, v) for v, name in leaf_name_pairs)
    a, b = (by_name[x] for x in (argv[1:3] if len(argv) > 2 else ('Has', 'Ppy')))
    truth = splits(T0, root)
    # the start: the two leaves change places (the edge lengths stay where they are)
    T = nx.relabel_nodes(T0, {a: b, b: a}, copy=True)
    args = (len(code), Q, distn, leaves, patterns, weights)
    print('%d taxa, %d patterns of %d columns; %s and %s exchanged: %d of %d splits of the '
          'fixture\'s tree are missing' % (len(leaves), len(patterns), len(states), names[a],
                                          names[b], len(truth - splits(T, root)), len(truth)))
    fit = Fit(T0.copy(), root, *args)
    print('the fixture\'s tree: log-likelihood %.6f, %.6f after the length fit'
          % (fit.total(), fit.fit_lengths(2 * FIT_ROUNDS)))
    fit.close()
    fit = Fit(T, root, *args)
    best = fit.fit_lengths(FIT_ROUNDS)
    calls, rnd = fit.calls, 0
    print('start: log-likelihood %.6f after the length fit' % best)
    while True:
        rnd += 1
        scores = fit.model.nni_scores(fit.batch, factors=FACTORS)      # one call: every neighbour
        calls += 1
        k, g = np.unravel_index(int(np.nanargmax(scores.sums)), scores.sums.shape)
        gain = float(scores.sums[k, g])
        if not gain > MIN_GAIN:
            print('round %d: %d moves scored, none improves (best %.3g): done'
                  % (rnd, len(scores.moves), gain))
            break
        labels = fit.model.tree.preorder_nodes
        v, c, s = (labels[int(x)] for x in scores.moves[k])
        p = labels[int(fit.model.tree.parent[int(scores.moves[k, 0])])]
        T = nni_apply(fit.T, root, v, c, s)
        T[p][v]['weight'] = float(scores.lengths[int(scores.moves[k, 0]), g])
        fit.close()
        fit = Fit(T, root, *args)
        moved = fit.total()
        best = fit.fit_lengths(FIT_ROUNDS)
        calls += fit.calls
        print('round %d: %d moves scored; the best, %s, promised %+.6f and gave %.6f; after the '
              'length fit %.6f; %d splits missing'
              % (rnd, len(scores.moves), [int(x) for x in scores.moves[k]], gain, moved, best,
                 len(truth - splits(T, root))))
    recovered = splits(fit.T, root) == truth
    print('final log-likelihood %.6f after %d device calls; the fixture\'s tree was %s'
          % (best, calls, 'recovered' if recovered else 'NOT recovered'))
    fit.close()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
