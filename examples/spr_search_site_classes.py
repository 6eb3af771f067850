#!/usr/bin/env python
"""
The SPR search of examples/spr_search.py under a site-class model: the p53 codon alignment
(tests/golden/p53/) under the three omega classes of examples/nni_search_site_classes.py -- MG94
with one kappa, an omega per class and class weights c, every class on the same tree.  The start
is the fixture's tree with one subtree cut off and hung three edges away, which no single
interchange undoes.  Each round:

  1. ONE spr_scores_mixture call: every move within radius 3 at three fractions of the target
     edge under the mixture, from one upward pass and one bounded walk per pruned node and class
     on the resident batch -- nothing but the sums leaves the device;
  2. the best improving (move, fraction) is adopted with _tree.spr_apply, a new model is built for
     the tree and the alignment uploaded;
  3. the branch lengths are fitted again with branch_profiles_mixture (the Fit of
     examples/nni_search_site_classes.py: one common factor per branch, applied to every class).

The mixture log-likelihood sum_i w_i log sum_k c_k L_ik is printed per round.  (A pruned subtree
leaves its parent as a single-child node and every adopted move adds a cut node: neither changes a
likelihood or a split.)

    python examples/spr_search_site_classes.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from raoteh_amd import device, io                  # noqa: E402
from raoteh_amd._tree import TreeArrays, spr_apply  # noqa: E402
from nni_search import splits                      # noqa: E402
from nni_search_site_classes import (FIT_ROUNDS, KAPPA, MIN_GAIN, NT_FREQS, OMEGA,  # noqa: E402
                                     Fit)

RADIUS = 3
FRACTIONS = (0.25, 0.5, 0.75)
MAX_ROUNDS = 8


def main(argv):
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    parts = [io.mg94_from_code(code, kappa=KAPPA, omega=w, nt_freqs=NT_FREQS) for w in OMEGA]
    Qs, distn = np.array([p[0] for p in parts]), parts[0][1]
    T0, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)
    patterns, _, counts = io.compress_patterns(states)
    args = (len(code), Qs, distn, leaves, patterns, counts.astype(np.float64))
    truth = splits(T0, root)
    # the start: the first internal subtree with a target edge exactly three edges away
    ta = TreeArrays(T0, root)
    near = set(map(tuple, device.tree_spr_moves(ta, RADIUS - 1).tolist()))
    far = [mv for mv in map(tuple, device.tree_spr_moves(ta, RADIUS).tolist()) if mv not in near]
    kids = np.diff(ta.indptr)
    c, y = ([mv for mv in far if kids[mv[0]] > 0] or far)[0]
    T = spr_apply(T0, root, ta.preorder_nodes[c], ta.preorder_nodes[y], 0.5, cut_label=('cut', 0))
    print('%d taxa, %d patterns of %d columns, %d omega classes; the subtree of node %d hung on '
          'the edge above node %d, three edges away: %d of %d splits of the fixture\'s tree are '
          'missing' % (len(leaves), len(patterns), len(states), len(OMEGA), c, y,
                       len(truth - splits(T, root)), len(truth)))
    fit = Fit(T, root, *args)
    best = fit.fit_lengths(FIT_ROUNDS)
    calls = fit.calls
    print('start: mixture log-likelihood %.6f after the length fit' % best)
    for rnd in range(1, MAX_ROUNDS + 1):
        scores = fit.model.spr_scores_mixture(fit.batch, fit.c, radius=RADIUS, fractions=FRACTIONS)
        calls += 1
        if scores.best is None:
            break
        k, g = scores.best
        gain = float(scores.sums[k, g])
        if not gain > MIN_GAIN:
            print('round %d: %d moves scored, none improves (best %.3g): done; mixture '
                  'log-likelihood %.6f' % (rnd, len(scores.moves), gain, best))
            break
        labels = fit.model.tree.preorder_nodes
        pruned, target = (labels[int(x)] for x in scores.moves[k])
        T = spr_apply(fit.T, root, pruned, target, FRACTIONS[g], cut_label=('cut', rnd))
        fit.close()
        fit = Fit(T, root, *args)
        moved = fit.total()
        before, best = best, fit.fit_lengths(FIT_ROUNDS)
        calls += fit.calls
        print('round %d: %d moves scored; the best, %s at fraction %g, promised %+.6f and gave '
              '%+.6f; mixture log-likelihood %.6f after the length fit; %d splits missing'
              % (rnd, len(scores.moves), [int(x) for x in scores.moves[k]], FRACTIONS[g], gain,
                 moved - before, best, len(truth - splits(T, root))))
    recovered = splits(fit.T, root) == truth
    print('final mixture log-likelihood %.6f after %d device calls; the fixture\'s tree was %s'
          % (best, calls, 'recovered' if recovered else 'NOT recovered'))
    fit.close()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
