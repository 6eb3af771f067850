"""
Joint draws of a state for every node of a tree given allowed-state sets: the mirror of
raoteh/sampler/_sample_mcy_dense.py (``resample_states`` :23-69), same arguments and result
(dict node -> state).  The upward pass and the draw run on the device
(rt_sites_sample_states): the edges' P as the model's transitions, the allowed sets as one
RT_OBS_MASK site, one draw.  Outside 2..128 states the draw falls to _sample_mc0_dense over
_mcy_dense.get_node_to_pmap.
"""
from __future__ import annotations

import numpy as np

from . import _lib, _mcy_dense, _sample_mc0_dense
from ._util import NumericalZeroProb, StructuralZeroProb

__all__ = ['resample_states']


def resample_states(T, root, nstates, node_to_allowed_states=None, root_distn=None,
                    P_default=None, seed=None):
    if root not in T:
        raise ValueError('unrecognized root')
    key = _sample_mc0_dense.draw_seed(seed)
    if not 2 <= nstates <= 128:
        node_to_pmap = _mcy_dense.get_node_to_pmap(
            T, root, nstates, node_to_allowed_states=node_to_allowed_states, P_default=P_default)
        return _sample_mc0_dense.resample_states(T, root, node_to_pmap, nstates,
                                                 root_distn=root_distn, P_default=P_default,
                                                 seed=key)
    from .device import TreeModel, states_to_mask
    model = TreeModel(T, root, nstates)
    try:
        ta = model.tree
        if ta.nnodes > 1:
            model.set_transitions(ta.esd_transitions(nstates, P_default=P_default))
        if root_distn is not None:
            model.set_root_distn(root_distn)
        every = set(range(nstates))
        allowed = {root: every}
        for v in ta.preorder_nodes:
            if node_to_allowed_states is not None:
                S = set(s for s in node_to_allowed_states.get(v, every) if 0 <= s < nstates)
                if S != every or v == root:
                    allowed[v] = S
        obs_nodes = list(allowed)
        words = np.array([[states_to_mask(sorted(allowed[v]), nstates) for v in obs_nodes]],
                         dtype=np.uint64)
        data = words[:, :, 0].copy() if nstates <= 64 else words
        batch = model.upload_sites(obs_nodes, data, kind='mask')
        got = model.sample_states(batch, ndraws=1, seed=key)
        if got.status[0] & _lib.RT_SITE_ZERO_PROB:
            raise StructuralZeroProb('all root states have either zero prior likelihood '
                                     'or give a subtree likelihood of zero')
        if got.status[0]:
            raise NumericalZeroProb('a node has no state of positive weight')
        return dict((v, int(s)) for v, s in zip(got.nodes, got.states[0, 0]))
    finally:
        model.close()
