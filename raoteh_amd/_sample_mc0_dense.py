"""
Joint draws of a state for every node of a tree from ready subtree likelihoods: the mirror of
raoteh/sampler/_sample_mc0_dense.py (``resample_states`` :20-98), same arguments, same error
protocol, same result (dict node -> state).  The node_to_pmap comes from the caller, so the
draw itself is a few n-term products per node: it is taken on the host, with the device's
counter-based generator (_philox) and the device's rule (rt_sites_sample_states), root ~
root_distn * pmap[root], then child ~ P_edge[parent's state] * pmap[child].
"""
from __future__ import annotations

import networkx as nx
import numpy as np

from . import _mc0_dense
from ._philox import philox_uniform
from ._util import NumericalZeroProb

__all__ = ['resample_states', 'draw_seed', 'pick_state']


def draw_seed(seed=None):
    """The Philox key of a call: `seed`, or 63 bits from numpy's global generator (so
    np.random.seed governs a call without a seed as it governs the reference's)."""
    if seed is None:
        return int(np.random.randint(0, 1 << 63, dtype=np.int64))
    return int(seed)


def pick_state(weights, u):
    """The first state in index order with w > 0 whose cumulative weight exceeds u * total (the
    last state with w > 0 if rounding leaves none); negative weights count as 0.  None when no
    weight is positive."""
    w = np.asarray(weights, dtype=np.float64).clip(min=0)
    pos = np.nonzero(w > 0)[0]
    if not len(pos):
        return None
    cdf = np.cumsum(w)
    k = int(np.searchsorted(cdf[pos], u * cdf[-1], side='right'))
    return int(pos[min(k, len(pos) - 1)])


def resample_states(T, root, node_to_pmap, nstates, root_distn=None, P_default=None, seed=None):
    root_pmap = node_to_pmap[root]
    likelihood = _mc0_dense.get_likelihood(root_pmap, root_distn=root_distn)
    if likelihood <= 0:
        raise NumericalZeroProb('numerically intractably small likelihood: %s' % likelihood)
    key = draw_seed(seed)
    predecessors = nx.dfs_predecessors(T, root)
    node_to_sampled_state = {}
    for index, node in enumerate(nx.dfs_preorder_nodes(T, root)):
        pmap = np.asarray(node_to_pmap[node], dtype=np.float64)
        if node == root:
            prior = root_distn
        else:
            parent_node = predecessors[node]
            P = T[parent_node][node].get('P', P_default)
            prior = np.asarray(P)[node_to_sampled_state[parent_node]]
        dpost = pmap if prior is None else np.asarray(prior, dtype=np.float64) * pmap
        state = pick_state(dpost, float(philox_uniform(key, 0, index)))
        if state is None:
            raise NumericalZeroProb('no state of positive weight at node %r' % (node,))
        node_to_sampled_state[node] = state
    return node_to_sampled_state
