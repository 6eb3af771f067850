#!/usr/bin/env python
"""
The NNI search of examples/nni_search.py under a site-class model: the p53 codon alignment
(tests/golden/p53/) under the three omega classes of examples/optimise_codon_site_classes.py --
MG94 with one kappa, an omega per class and class weights c, every class on the same tree.  The
start is the fixture's tree with two leaves exchanged.  Each round:

  1. ONE nni_scores_mixture call: every NNI neighbour of the current tree under the mixture, the
     edge above v at a small grid of factors of its length (the same factor in every class), from
     one upward and one downward pass per class on the resident batch -- nothing but the sums
     leaves the device;
  2. the best improving (move, factor) is adopted with _tree.nni_apply, a new model is built for
     the tree and the alignment uploaded;
  3. the branch lengths are fitted again with branch_profiles_mixture: one common factor per
     branch, applied to every class, chosen from a grid per fitting round.

The mixture log-likelihood sum_i w_i log sum_k c_k L_ik is printed per round.

    python examples/nni_search_site_classes.py [leaf_a leaf_b]
"""
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from raoteh_amd import io                          # noqa: E402
from raoteh_amd._tree import nni_apply             # noqa: E402
from raoteh_amd.device import TreeModel            # noqa: E402
from nni_search import splits                      # noqa: E402

NT_FREQS = dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883)
KAPPA = 3.17632
OMEGA = (0.02, 0.25, 1.2)                          # three classes: constrained, relaxed, fast
CLASS_WEIGHTS = (0.6, 0.3, 0.1)
FACTORS = np.exp(np.linspace(-np.log(4.0), np.log(4.0), 5))     # of the length of the edge above v
FIT_ROUNDS = 4
MIN_GAIN = 1e-3


class Fit(object):
    """A model with the K rate sets and a resident batch for one tree; the lengths live in the
    tree's 'weight's and are shared by the classes."""

    def __init__(self, T, root, n, Qs, distn, leaves, patterns, weights):
        self.T, self.root, self.Qs, self.weights = T, root, Qs, weights
        self.c = np.array(CLASS_WEIGHTS)
        self.model = TreeModel(T, root, n)
        self.model.set_root_distn(distn)
        self.t = self.model.tree.branch_lengths()
        self.model.set_rate_sets(Qs, t=self.t)
        self.batch = self.model.upload_sites(leaves, patterns, kind='state')
        self.batch.set_weights(weights)
        self.calls = 1

    def fit_lengths(self, rounds):
        """Per round one branch_profiles_mixture call over a grid of factors: every branch moved to
        its best grid point at once, the move halved while the total does not improve.  -> the
        mixture log-likelihood."""
        best = self.total()
        span = np.log(2.0)
        for _ in range(rounds):
            x = np.linspace(-span, span, 9)
            prof = self.model.branch_profiles_mixture(self.batch, self.c, np.exp(x))
            self.calls += 1
            move = np.zeros(len(self.t))
            for v in range(1, len(self.t)):
                if self.t[v] > 0 and np.isfinite(prof.sums[v]).any():
                    move[v] = x[int(np.nanargmax(prof.sums[v]))]
            scale, accepted = 1.0, False
            for _ in range(5):
                trial = self.t * np.exp(scale * move)
                self.model.set_rate_sets(self.Qs, t=trial)
                self.calls += 1
                now = self.total()
                if now > best:
                    self.t, best, accepted = trial, now, True
                    break
                scale *= 0.5
            if not accepted:
                self.model.set_rate_sets(self.Qs, t=self.t)
                break
            span = max(0.5 * span, 0.02)
        ta = self.model.tree
        for i in range(1, ta.nnodes):            # the fitted lengths back into the tree
            self.T[ta.preorder_nodes[int(ta.parent[i])]][ta.preorder_nodes[i]]['weight'] = float(self.t[i])
        return best

    def total(self):
        """sum_i w_i log sum_k c_k L_ik, from the loglik output of the profile call at the
        resident lengths (one point, factor 1)."""
        res = self.model.branch_profiles_mixture(self.batch, self.c, [1.0])
        self.calls += 1
        if (res.status & 1).any():
            return -np.inf
        return float(np.dot(self.weights, res.loglik))

    def close(self):
        self.model.close()


def main(argv):
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    parts = [io.mg94_from_code(code, kappa=KAPPA, omega=w, nt_freqs=NT_FREQS) for w in OMEGA]
    Qs, distn = np.array([p[0] for p in parts]), parts[0][1]
    T0, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)
    patterns, _, counts = io.compress_patterns(states)
    weights = counts.astype(np.float64)
    names = dict(leaf_name_pairs)
    by_name = dict((name, v) for v, name in leaf_name_pairs)
    a, b = (by_name[x] for x in (argv[1:3] if len(argv) > 2 else ('Has', 'Ppy')))
    truth = splits(T0, root)
    T = nx.relabel_nodes(T0, {a: b, b: a}, copy=True)
    args = (len(code), Qs, distn, leaves, patterns, weights)
    print('%d taxa, %d patterns of %d columns, %d omega classes; %s and %s exchanged: %d of %d '
          'splits of the fixture\'s tree are missing'
          % (len(leaves), len(patterns), len(states), len(OMEGA), names[a], names[b],
             len(truth - splits(T, root)), len(truth)))
    fit = Fit(T, root, *args)
    best = fit.fit_lengths(FIT_ROUNDS)
    calls, rnd = fit.calls, 0
    print('start: mixture log-likelihood %.6f after the length fit' % best)
    while True:
        rnd += 1
        scores = fit.model.nni_scores_mixture(fit.batch, fit.c, FACTORS)    # every neighbour
        calls += 1
        k, g = np.unravel_index(int(np.nanargmax(scores.sums)), scores.sums.shape)
        gain = float(scores.sums[k, g])
        if not gain > MIN_GAIN:
            print('round %d: %d moves scored, none improves (best %.3g): done; mixture '
                  'log-likelihood %.6f' % (rnd, len(scores.moves), gain, best))
            break
        labels = fit.model.tree.preorder_nodes
        iv = int(scores.moves[k, 0])
        v, c, s = (labels[int(x)] for x in scores.moves[k])
        p = labels[int(fit.model.tree.parent[iv])]
        T = nni_apply(fit.T, root, v, c, s)
        T[p][v]['weight'] = float(scores.factors[iv, g] * fit.t[iv])
        fit.close()
        fit = Fit(T, root, *args)
        moved = fit.total()
        best = fit.fit_lengths(FIT_ROUNDS)
        calls += fit.calls
        print('round %d: %d moves scored; the best, %s, promised %+.6f and gave %.6f; mixture '
              'log-likelihood %.6f after the length fit; %d splits missing'
              % (rnd, len(scores.moves), [int(x) for x in scores.moves[k]], gain, moved, best,
                 len(truth - splits(T, root))))
    recovered = splits(fit.T, root) == truth
    print('final mixture log-likelihood %.6f after %d device calls; the fixture\'s tree was %s'
          % (best, calls, 'recovered' if recovered else 'NOT recovered'))
    fit.close()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
