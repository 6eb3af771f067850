#!/usr/bin/env python
"""
Evolutionary placement on the p53 codon alignment (tests/golden/p53/, MG94 with the PAML estimates
of examples/p53_loglik.py): three taxa are taken out of the tree and the alignment (a removed
leaf leaves a single-child node, which is spliced out and its lengths added), the branch lengths
of the reduced tree are fitted with branch_profiles as examples/optimise_branch_lengths.py does,
and the three sequences are placed back with ONE place_queries call -- every edge of the reduced
tree at 3 attachment fractions and 4 pendant lengths.  Printed for each: the best edge and its
score, the score of the edge the taxon was cut from, and the next best edge.  The placements are
then adopted one by one with place_apply.

    python examples/place_queries.py [rounds]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import io                          # noqa: E402
from raoteh_amd._tree import TreeArrays, place_apply    # noqa: E402
from raoteh_amd.device import TreeModel            # noqa: E402
from optimise_branch_lengths import GRID, parabola_argmax     # noqa: E402


def remove_leaf(T, root, leaf):
    """T without `leaf`; a node left with a single child (and a parent) is spliced out and its two
    lengths added.  -> the node BELOW the edge the leaf hung on (the child of the spliced node),
    or the node the leaf hung on where it keeps two children or more."""
    ta = TreeArrays(T, root)
    idx = ta.node_to_index
    p = ta.preorder_nodes[int(ta.parent[idx[leaf]])]
    T.remove_node(leaf)
    if p == root:
        return p
    g = ta.preorder_nodes[int(ta.parent[idx[p]])]
    kids = [x for x in T[p] if x != g]
    if len(kids) != 1:
        return p
    c = kids[0]
    data = dict(T[p][c])
    data['weight'] = T[g][p]['weight'] + T[p][c]['weight']
    # (the spliced node's place among the children of g is the end of g's adjacency: the order
    # of the children does not enter the likelihood)
    T.remove_node(p)
    T.add_edge(g, c, **data)
    return c


def fit_branch_lengths(model, batch, weights, Q, t, rounds):
    def total():
        ll, status = model.log_likelihoods(batch)
        return float(np.dot(weights, ll)) if not (status & 1).any() else -np.inf

    N = model.tree.nnodes
    best, span = total(), np.log(4.0)
    for _ in range(rounds):
        x = np.linspace(-span, span, GRID)
        prof = model.branch_profiles(batch, factors=np.exp(x))
        move = np.zeros(N)
        for v in range(1, N):
            if t[v] > 0 and np.isfinite(prof.sums[v]).any():
                move[v] = parabola_argmax(x, prof.sums[v], int(np.nanargmax(prof.sums[v])))
        scale, accepted = 1.0, False
        for _ in range(6):
            trial = t * np.exp(scale * move)
            model.set_rates(Q=Q, t=trial)
            now = total()
            if now > best:
                t, best, accepted = trial, now, True
                break
            scale *= 0.5
        if not accepted:
            model.set_rates(Q=Q, t=t)
            break
        if scale == 1.0:
            span = max(0.5 * span, 0.02)
    return t, best


def main(argv):
    rounds = int(argv[1]) if len(argv) > 1 else 4
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    Q, distn = io.mg94_from_code(
        code, kappa=3.17632, omega=0.21925,
        nt_freqs=dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883))
    T, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)
    names = dict(leaf_name_pairs)
    patterns, _, counts = io.compress_patterns(states)
    weights = counts.astype(np.float64)

    # three taxa out of the tree and the alignment
    out = [leaves[k] for k in (1, len(leaves) // 2, len(leaves) - 2)]
    keep = [k for k, v in enumerate(leaves) if v not in out]
    cut_from = dict((v, remove_leaf(T, root, v)) for v in out)
    queries = np.ascontiguousarray(patterns[:, [leaves.index(v) for v in out]].T)

    model = TreeModel(T, root, len(code))
    model.set_root_distn(distn)
    model.set_rates(Q=Q, t=model.tree.branch_lengths())
    batch = model.upload_sites([leaves[k] for k in keep], patterns[:, keep], kind='state')
    batch.set_weights(weights)
    t, total = fit_branch_lengths(model, batch, weights, Q, model.tree.branch_lengths(), rounds)
    N = model.tree.nnodes
    print('%d taxa kept, %d taken out, %d patterns, %d branches; total %.6f after the fit'
          % (len(keep), len(out), len(patterns), N - 1, total))

    # one call: 3 queries x every edge x 3 fractions x 4 pendant lengths
    mean = float(np.mean(t[1:]))
    got = model.place_queries(batch, queries, kind='state', fractions=(0.25, 0.5, 0.75),
                              pendant=(0.25 * mean, 0.5 * mean, mean, 2.0 * mean))
    labels = model.tree.preorder_nodes
    per_edge = got.sums.reshape(len(out), N, -1).max(axis=2)
    per_edge[:, 0] = -np.inf
    placed = T
    for q, v in enumerate(out):
        b, r, k = (int(x) for x in got.best[q])
        order = np.argsort(-per_edge[q], kind='stable')
        home = model.tree.node_to_index.get(cut_from[v], 0)     # (0: its edge is gone, too)
        print('%s: best edge above node %d at fraction %.2f, pendant %.4f: %.4f; the edge it was '
              'cut from (above node %d): %.4f; next best edge (above node %d): %.4f'
              % (names[v], b, got.fractions[r], got.pendant[k], got.sums[q, b, r, k], home,
                 per_edge[q, home], int(order[1]), per_edge[q, int(order[1])]))
        # adopt it: the label of the node below the edge is the same in every tree along the way
        # (an edge cut by an earlier placement keeps its lower part above that node)
        placed = place_apply(placed, root, labels[b], got.fractions[r], got.pendant[k], v)
    print('the tree with the three taxa placed has %d nodes' % placed.number_of_nodes())


if __name__ == '__main__':
    main(sys.argv)
