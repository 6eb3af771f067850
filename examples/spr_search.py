#!/usr/bin/env python
"""
A tree search by subtree pruning and regrafting on the p53 codon alignment (tests/golden/p53/,
MG94 with the PAML estimates of examples/p53_loglik.py), next to the search by nearest-neighbour
interchanges of examples/nni_search.py from the same start.  The start is the fixture's tree with
one subtree cut off and hung three edges away, which no single interchange undoes.  Each round of
the SPR search:

  1. ONE spr_scores call: every move within radius 3 at three fractions of the target edge, from
     one upward pass and a bounded walk per pruned node on the resident batch;
  2. the best improving (move, fraction) is adopted: _tree.spr_apply rearranges the tree, a new
     TreeModel is built for it and the alignment uploaded;
  3. the branch lengths are fitted again, one branch_profiles call per fitting round (the scheme
     of examples/optimise_branch_lengths.py).

The NNI search does the same with one nni_scores call per round.  Both stop when no move improves
by more than MIN_GAIN or after MAX_ROUNDS; the log-likelihoods are printed round by round, side by
side.  (A pruned subtree leaves its parent as a single-child node and every adopted move adds a
cut node: neither changes a likelihood or a split.)

    python examples/spr_search.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

from raoteh_amd import device, io                  # noqa: E402
from raoteh_amd._tree import TreeArrays, nni_apply, spr_apply  # noqa: E402
from nni_search import FACTORS, FIT_ROUNDS, MIN_GAIN, Fit, splits  # noqa: E402

RADIUS = 3
FRACTIONS = (0.25, 0.5, 0.75)
MAX_ROUNDS = 8


def search(kind, T, root, args, truth):
    """[(log-likelihood, splits missing)] per round of the search of `kind` from the tree T, the
    start (after its length fit) first; the number of device calls."""
    fit = Fit(T, root, *args)
    trace = [(fit.fit_lengths(FIT_ROUNDS), len(truth - splits(T, root)))]
    calls = fit.calls
    for rnd in range(1, MAX_ROUNDS + 1):
        labels = fit.model.tree.preorder_nodes
        if kind == 'spr':
            scores = fit.model.spr_scores(fit.batch, radius=RADIUS, fractions=FRACTIONS)
        else:
            scores = fit.model.nni_scores(fit.batch, factors=FACTORS)
        calls += 1
        k, g = np.unravel_index(int(np.nanargmax(scores.sums)), scores.sums.shape)
        gain = float(scores.sums[k, g])
        if not gain > MIN_GAIN:
            print('  %s round %d: %d moves scored, none improves (best %.3g)'
                  % (kind, rnd, len(scores.moves), gain))
            break
        if kind == 'spr':
            c, y = (labels[int(x)] for x in scores.moves[k])
            T = spr_apply(fit.T, root, c, y, FRACTIONS[g], cut_label=('cut', rnd))
        else:
            v, c, s = (labels[int(x)] for x in scores.moves[k])
            p = labels[int(fit.model.tree.parent[int(scores.moves[k, 0])])]
            T = nni_apply(fit.T, root, v, c, s)
            T[p][v]['weight'] = float(scores.lengths[int(scores.moves[k, 0]), g])
        fit.close()
        fit = Fit(T, root, *args)
        moved = fit.total()
        best = fit.fit_lengths(FIT_ROUNDS)
        calls += fit.calls
        trace.append((best, len(truth - splits(T, root))))
        print('  %s round %d: %d moves scored; the best, %s, promised %+.6f and gave %+.6f; after '
              'the length fit %.6f' % (kind, rnd, len(scores.moves),
                                       [int(x) for x in scores.moves[k]], gain,
                                       moved - trace[-2][0], best))
    fit.close()
    return trace, calls


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
    args = (len(code), Q, distn, leaves, patterns, counts.astype(np.float64))
    truth = splits(T0, root)
    # the start: the first internal subtree with a target edge exactly three edges away
    ta = TreeArrays(T0, root)
    near = set(map(tuple, device.tree_spr_moves(ta, RADIUS - 1).tolist()))
    far = [mv for mv in map(tuple, device.tree_spr_moves(ta, RADIUS).tolist()) if mv not in near]
    kids = np.diff(ta.indptr)
    c, y = ([mv for mv in far if kids[mv[0]] > 0] or far)[0]
    T = spr_apply(T0, root, ta.preorder_nodes[c], ta.preorder_nodes[y], 0.5, cut_label=('cut', 0))
    print('%d taxa, %d patterns of %d columns; the subtree of node %d hung on the edge above node '
          '%d, three edges away: %d of %d splits of the fixture\'s tree are missing'
          % (len(leaves), len(patterns), len(states), c, y, len(truth - splits(T, root)),
             len(truth)))
    fit = Fit(T0.copy(), root, *args)
    print('the fixture\'s tree: log-likelihood %.6f, %.6f after the length fit'
          % (fit.total(), fit.fit_lengths(2 * FIT_ROUNDS)))
    fit.close()
    traces = {}
    for kind in ('nni', 'spr'):
        traces[kind], calls = search(kind, T.copy(), root, args, truth)
        print('  %s: %d device calls' % (kind, calls))
    print('round   nni log-likelihood (splits missing)   spr log-likelihood (splits missing)')
    for rnd in range(max(len(x) for x in traces.values())):
        cells = []
        for kind in ('nni', 'spr'):
            tr = traces[kind]
            ll, missing = tr[min(rnd, len(tr) - 1)]
            cells.append('%16.6f (%d)%s' % (ll, missing, '' if rnd < len(tr) else ' done'))
        print('%5d   %-37s %s' % (rnd, cells[0], cells[1]))
    return 0


if __name__ == '__main__':
    sys.exit(main(sys.argv))
