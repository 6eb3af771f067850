#!/usr/bin/env python
"""
Branch lengths of the p53 codon alignment (tests/golden/p53/, MG94 with the PAML estimates of
examples/p53_loglik.py) from perturbed starting lengths, by per-branch likelihood profiles: each
round is ONE branch_profiles call -- every branch at a geometric grid of factors of its current
length, from one upward and one downward pass -- then per branch a parabola in log t through the
best grid point and its neighbours, all branches moved at once, and one step to accept the move
(halved while the total does not improve).

    python examples/optimise_branch_lengths.py [rounds]

Beside the total of every round: the device calls made, and the set_rates + step pairs the same
grids would have cost one branch and one trial length at a time.
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import io                          # noqa: E402
from raoteh_amd.device import TreeModel            # noqa: E402

GRID = 9            # trial lengths per branch and round (odd: the middle one is the current length)


def parabola_argmax(x, y, k):
    """The maximiser of the parabola through (x, y)[k - 1 .. k + 1], kept inside that interval;
    x[k] when k is an end of the grid or the three points are not concave."""
    if k == 0 or k == len(x) - 1 or not np.isfinite(y[k - 1:k + 2]).all():
        return x[k]
    x0, x1, x2 = x[k - 1:k + 2]
    y0, y1, y2 = y[k - 1:k + 2]
    den = (x1 - x0) * (y1 - y2) - (x1 - x2) * (y1 - y0)
    if den == 0.0:
        return x1
    num = (x1 - x0) ** 2 * (y1 - y2) - (x1 - x2) ** 2 * (y1 - y0)
    return float(np.clip(x1 - 0.5 * num / den, x0, x2))


def main(argv):
    rounds = int(argv[1]) if len(argv) > 1 else 8
    data = os.path.join(os.path.dirname(HERE), 'tests', 'golden', 'p53')
    code = io.read_genetic_code(os.path.join(data, 'universal.code.txt'))
    Q, distn = io.mg94_from_code(
        code, kappa=3.17632, omega=0.21925,
        nt_freqs=dict(A=0.25039, C=0.30126, G=0.25952, T=0.18883))
    T, root, leaf_name_pairs = io.read_newick(open(os.path.join(data, 'p53S.const.tree')).read())
    leaves, states = io.alignment_to_states(
        io.read_phylip(os.path.join(data, 'alignment.for.codeml.phylip')), code, leaf_name_pairs)
    patterns, _, counts = io.compress_patterns(states)
    weights = counts.astype(np.float64)

    model = TreeModel(T, root, len(code))
    model.set_root_distn(distn)
    N = model.tree.nnodes
    rng = np.random.RandomState(0)
    t = model.tree.branch_lengths() * np.exp(rng.uniform(-1.0, 1.0, N))      # perturbed start
    t[0] = 0.0
    model.set_rates(Q=Q, t=t)
    batch = model.upload_sites(leaves, patterns, kind='state')
    batch.set_weights(weights)

    def total():
        ll, status = model.log_likelihoods(batch)
        return float(np.dot(weights, ll)) if not (status & 1).any() else -np.inf

    calls, brute = 1, 0
    best = total()
    print('%d taxa, %d patterns of %d columns, %d branches; start %.6f'
          % (len(leaves), len(patterns), len(states), N - 1, best))
    span = np.log(4.0)
    for r in range(rounds):
        x = np.linspace(-span, span, GRID)
        prof = model.branch_profiles(batch, factors=np.exp(x))      # one call: every branch
        calls += 1
        brute += (N - 1) * GRID
        move = np.zeros(N)
        for v in range(1, N):
            if t[v] > 0 and np.isfinite(prof.sums[v]).any():
                move[v] = parabola_argmax(x, prof.sums[v], int(np.nanargmax(prof.sums[v])))
        scale, accepted = 1.0, False
        for _ in range(6):
            trial = t * np.exp(scale * move)
            model.set_rates(Q=Q, t=trial)
            calls += 1
            now = total()
            if now > best:
                t, best, accepted = trial, now, True
                break
            scale *= 0.5
        if not accepted:
            model.set_rates(Q=Q, t=t)
            calls += 1
        # the profiles are per branch: a joint move overshoots where neighbours trade length, so
        # the grid narrows only once the full move is taken
        if accepted and scale == 1.0:
            span = max(0.5 * span, 0.02)
        print('round %d: total %.6f (move x %.3g, largest |log factor| %.3f); %d device calls so '
              'far, the brute-force loop %d set_rates + step pairs'
              % (r + 1, best, scale if accepted else 0.0, np.abs(move).max(), calls, brute))
        if not accepted or np.abs(move).max() < 1e-4:
            break
    print('final total %.6f; branch lengths from %.4g to %.4g' % (best, t[1:].min(), t[1:].max()))


if __name__ == '__main__':
    main(sys.argv)
