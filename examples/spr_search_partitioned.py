#!/usr/bin/env python
"""
The search of examples/nni_search_partitioned.py by subtree pruning and regrafting: the p53
alignment read as nucleotides, its three codon positions as three 4-state HKY85 partitions on ONE
shared tree, branch v of partition k at length t[k][v] = r_k * tau_v with fixed relative rates r.
The start is the fixture's tree with one subtree cut off and hung three edges away, which no single
interchange undoes.  Each round:

  1. ONE spr_scores_partitioned call: every move within radius 3 at three fractions of the target
     edge, every column under its own partition's rates (a fraction of tau_y is the same fraction
     of every partition's t[k][y]) -- nothing but the sums leaves the device;
  2. the best improving (move, fraction) is adopted with _tree.spr_apply, a new model is built for
     the tree and the alignment uploaded;
  3. the shared lengths tau are fitted again with branch_profiles_partitioned (the Fit of
     examples/nni_search_partitioned.py: one common factor per branch for all partitions).

The log-likelihood of step_partitioned is printed per round.  (A pruned subtree leaves its parent
as a single-child node and every adopted move adds a cut node: neither changes a likelihood or a
split.)

    python examples/spr_search_partitioned.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from raoteh_amd import device, io, synth            # noqa: E402
from raoteh_amd._tree import TreeArrays, spr_apply  # noqa: E402
from nni_search import splits                       # noqa: E402
from nni_search_partitioned import (FIT_ROUNDS, KAPPAS, MIN_GAIN, NT_FREQS, RATES,  # noqa: E402
                                    Fit)

RADIUS = 3
FRACTIONS = (0.25, 0.5, 0.75)
MAX_ROUNDS = 8


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
    args = (Q, distn, leaves, states, position)
    truth = splits(T0, root)
    # the start: the first internal subtree with a target edge exactly three edges away
    ta = TreeArrays(T0, root)
    near = set(map(tuple, device.tree_spr_moves(ta, RADIUS - 1).tolist()))
    far = [mv for mv in map(tuple, device.tree_spr_moves(ta, RADIUS).tolist()) if mv not in near]
    kids = np.diff(ta.indptr)
    c, y = ([mv for mv in far if kids[mv[0]] > 0] or far)[0]
    T = spr_apply(T0, root, ta.preorder_nodes[c], ta.preorder_nodes[y], 0.5, cut_label=('cut', 0))
    print('%d taxa, %d nucleotide columns in %d partitions; the subtree of node %d hung on the edge '
          'above node %d, three edges away: %d of %d splits of the fixture\'s tree are missing'
          % (len(leaves), len(states), len(RATES), c, y, len(truth - splits(T, root)), len(truth)))
    fit = Fit(T, root, *args)
    best = fit.fit_lengths(FIT_ROUNDS)
    calls = fit.calls
    print('start: log-likelihood %.6f after the length fit' % best)
    for rnd in range(1, MAX_ROUNDS + 1):
        scores = fit.model.spr_scores_partitioned(fit.batch, radius=RADIUS, fractions=FRACTIONS)
        calls += 1
        if scores.best is None:
            break
        k, g = scores.best
        gain = float(scores.sums[k, g])
        if not gain > MIN_GAIN:
            print('round %d: %d moves scored, none improves (best %.3g): done; log-likelihood %.6f'
                  % (rnd, len(scores.moves), gain, best))
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
              '%+.6f; log-likelihood %.6f after the length fit; %d splits missing'
              % (rnd, len(scores.moves), [int(x) for x in scores.moves[k]], FRACTIONS[g], gain,
                 moved - before, best, len(truth - splits(T, root))))
    recovered = splits(fit.T, root) == truth
    print('final log-likelihood %.6f after %d device calls; the fixture\'s tree was %s'
          % (best, calls, 'recovered' if recovered else 'NOT recovered'))
    fit.close()
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
