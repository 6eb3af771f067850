"""Host side of rt_model_nni_moves / rt_sites_nni_scores: the order and count of the moves
against a brute-force enumeration, raoteh_amd._tree.nni_apply against the hand-built arrays of the
host reference (tests/_nni_cases.py), the reference against itself (a move and its inverse, the
two-child root under a stationary reversible model), and the declared surface."""
import re

import networkx as nx
import numpy as np
import pytest
import scipy.linalg

from conftest import ROOT
from oracle import oracle_numpy as orc
from _nni_cases import (brute_moves, moved_arrays, moved_log_likelihoods, nni_from_transitions,
                        parents_of)
from _resident_cases import make_case


def arrays(T, root):
    from raoteh_amd._tree import TreeArrays
    return TreeArrays(T, root)


def balanced(nleaves):
    T = nx.Graph()
    T.add_node(0)
    for child in range(1, 2 * nleaves - 1):
        T.add_edge((child - 1) // 2, child, weight=0.1 + 0.01 * child)
    return T


def star(nleaves):
    T = nx.Graph()
    for child in range(1, nleaves + 1):
        T.add_edge(0, child, weight=0.1 * child)
    return T


def path(nnodes):
    T = nx.Graph()
    T.add_node(0)
    for child in range(1, nnodes):
        T.add_edge(child - 1, child, weight=0.1 * child)
    return T


# ---- the move list -------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 1, 2, 3, 4, 11])
def test_moves_of_random_trees_match_the_brute_force(seed):
    from raoteh_amd import device, synth
    T, root, _ = synth.random_tree(12, seed, max_children=3)
    ta = arrays(T, root)
    got = device.tree_nni_moves(ta)
    want = brute_moves(ta.indices, ta.indptr)
    assert got.dtype == np.int32 and got.shape == want.shape and len(want) > 0
    assert np.array_equal(got, want)
    # the count by the formula: sum over v of #children(v) * #siblings(v)
    kids = np.diff(ta.indptr)
    assert len(got) == sum(int(kids[v]) * (int(kids[ta.parent[v]]) - 1) for v in range(1, ta.nnodes))
    # v ascending; every triple is a move
    assert np.all(np.diff(got[:, 0]) >= 0)
    for v, c, s in got:
        assert ta.parent[c] == v and ta.parent[s] == ta.parent[v] and s != v and v != 0


def test_moves_of_a_balanced_tree_a_star_and_a_path():
    from raoteh_amd import device
    ta = arrays(balanced(8), 0)
    got = device.tree_nni_moves(ta)
    assert len(got) == 12                        # 6 internal non-root nodes, 2 children, 1 sibling
    assert np.array_equal(got, brute_moves(ta.indices, ta.indptr))
    for T, root in ((star(7), 0), (path(6), 0), (path(1), 0)):
        ta = arrays(T, root)
        got = device.tree_nni_moves(ta)
        assert got.shape == (0, 3) and got.dtype == np.int32
        assert brute_moves(ta.indices, ta.indptr).shape == (0, 3)


def test_moves_capacity_and_bad_trees():
    import ctypes
    from raoteh_amd import _lib
    ta = arrays(balanced(4), 0)
    p64, p32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    count = ctypes.c_int64(-1)
    moves = np.full((4, 3), -7, dtype=np.int32)
    call = _lib.lib().rt_tree_nni_moves
    idx, ptr = ta.indices.ctypes.data_as(p64), ta.indptr.ctypes.data_as(p64)
    assert call(ta.nnodes, idx, ptr, None, 0, ctypes.byref(count)) == _lib.RT_OK
    assert count.value == 4
    # too small an array: refused, the count still returned, nothing written
    count.value = -1
    assert call(ta.nnodes, idx, ptr, moves.ctypes.data_as(p32), 3,
                ctypes.byref(count)) == _lib.RT_ERR_INVALID
    assert count.value == 4 and (moves == -7).all()
    assert call(ta.nnodes, idx, ptr, moves.ctypes.data_as(p32), 4, ctypes.byref(count)) == _lib.RT_OK
    assert np.array_equal(moves, brute_moves(ta.indices, ta.indptr))
    bad = ta.indices.copy()
    bad[0] = 0                                   # a child that is not after its parent
    assert call(ta.nnodes, bad.ctypes.data_as(p64), ptr, None, 0,
                ctypes.byref(count)) == _lib.RT_ERR_INVALID
    # a child listed twice leaves another node without a parent: refused before the moves are
    # counted through the parents
    twice = ta.indices.copy()
    twice[1] = twice[0]
    assert call(ta.nnodes, twice.ctypes.data_as(p64), ptr, None, 0,
                ctypes.byref(count)) == _lib.RT_ERR_INVALID
    assert 'twice' in _lib.last_error()


# ---- nni_apply ------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 3, 11])
def test_nni_apply_agrees_with_the_hand_built_arrays(seed):
    """For every move: TreeArrays of the rearranged networkx tree has the CSR of the reference's
    moved_arrays, node for node, and every edge's attributes are those of the node below it."""
    from raoteh_amd import synth
    from raoteh_amd._tree import nni_apply
    T, root, _ = synth.random_tree(12, seed, max_children=3)
    for a, b, d in T.edges(data=True):
        d['tag'] = ('edge', a, b)
    ta = arrays(T, root)
    below = dict((ta.preorder_nodes[i], ta.edge_data[i]) for i in range(1, ta.nnodes))
    before = nx.to_dict_of_dicts(T)
    for v, c, s in brute_moves(ta.indices, ta.indptr):
        labels = [ta.preorder_nodes[int(x)] for x in (v, c, s)]
        moved = nni_apply(T, root, *labels)
        assert moved is not T and nx.to_dict_of_dicts(T) == before       # T is as it was
        tm = arrays(moved, root)
        ni, npt, old_of_new = moved_arrays(ta.indices, ta.indptr, int(v), int(c), int(s))
        assert np.array_equal(tm.indices, ni) and np.array_equal(tm.indptr, npt)
        assert tm.preorder_nodes == [ta.preorder_nodes[int(k)] for k in old_of_new]
        for i in range(1, tm.nnodes):
            assert tm.edge_data[i] == below[tm.preorder_nodes[i]]
            assert tm.edge_data[i] is not below[tm.preorder_nodes[i]]    # (a copy)
        # the parents: c below p, s below v, every other node where it was
        want = dict((ta.preorder_nodes[i], ta.preorder_nodes[int(ta.parent[i])])
                    for i in range(1, ta.nnodes))
        want[labels[1]], want[labels[2]] = want[labels[0]], labels[0]
        got = dict((tm.preorder_nodes[i], tm.preorder_nodes[int(tm.parent[i])])
                   for i in range(1, tm.nnodes))
        assert got == want


def test_nni_apply_rejects_what_is_not_a_move():
    from raoteh_amd._tree import nni_apply
    T = balanced(4)                              # 0 -> (1 -> 3, 4), (2 -> 5, 6)
    assert arrays(nni_apply(T, 0, 1, 3, 2), 0).nnodes == 7
    for triple in ((0, 1, 2),                    # v is the root
                   (1, 5, 2),                    # c is not a child of v
                   (1, 3, 1),                    # s is v itself
                   (1, 3, 4),                    # s is a child of v, not a sibling
                   (3, 1, 4),                    # v has no children
                   (1, 3, 99),                   # not a node
                   (1, 2, 2)):
        with pytest.raises(ValueError):
            nni_apply(T, 0, *triple)
    with pytest.raises(ValueError):
        nni_apply(T, 42, 1, 3, 2)


# ---- the reference against itself ----------------------------------------------------------

def reference_case(n, seed):
    case = make_case(n, 12, 9, 'mask', seed, internal=True, per_edge=True)
    ta = arrays(case.T, case.root)
    t = ta.branch_lengths()
    esd = np.zeros((ta.nnodes, n, n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * case.Qs[case.node_q[v]])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return case, ta, esd, cols


def test_a_move_and_its_inverse_restore_the_likelihoods():
    """After (v, c, s) the node s is a child of v and c a sibling of v: the move (v, s, c) of the
    moved tree, in its own numbering, gives the first tree back -- the same log-likelihoods to
    the last bit but the order of the factors (<= 1e-13 of |log L|)."""
    case, ta, esd, cols = reference_case(5, 9100)
    base, bstat = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                            case.root_distn)
    assert (bstat == 0).sum() >= 4
    changed = 0
    for v, c, s in brute_moves(ta.indices, ta.indptr):
        ni, npt, old_of_new = moved_arrays(ta.indices, ta.indptr, int(v), int(c), int(s))
        new_of_old = np.empty_like(old_of_new)
        new_of_old[old_of_new] = np.arange(ta.nnodes)
        esd1 = esd[old_of_new]
        cols1 = [int(new_of_old[k]) for k in cols]
        ll1, st1 = orc.batch_log_likelihoods(ni, npt, esd1, cols1, case.obs_lik, case.root_distn)
        again, _ = moved_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                         case.root_distn, (v, c, s))
        assert np.array_equal(again, ll1)
        changed += int(np.any(np.abs(ll1[bstat == 0] - base[bstat == 0]) > 1e-6))
        inverse = (int(new_of_old[v]), int(new_of_old[s]), int(new_of_old[c]))
        assert inverse in [tuple(m) for m in brute_moves(ni, npt)]
        ll2, st2 = moved_log_likelihoods(ni, npt, esd1, cols1, case.obs_lik, case.root_distn, inverse)
        assert np.array_equal(st2, bstat)
        ok = bstat == 0
        assert np.abs(ll2[ok] - base[ok]).max() <= 1e-13 * np.abs(base[ok]).max()
        # ... and the arrays themselves are the first tree's, up to the numbering
        mi, mpt, back = moved_arrays(ni, npt, *inverse)
        parent0 = parents_of(ta.indices, ta.indptr)
        parent2 = parents_of(mi, mpt)
        old = old_of_new[back]
        assert all(parent2[j] < 0 and parent0[old[j]] < 0 or old[parent2[j]] == parent0[old[j]]
                   for j in range(ta.nnodes))
    assert changed > 0                           # (the moves do change the likelihood)


def jc_matrix(t, alpha=0.3):
    same = 0.25 + 0.75 * np.exp(-4.0 * alpha * t)
    diff = 0.25 - 0.25 * np.exp(-4.0 * alpha * t)
    return diff + (same - diff) * np.eye(4)


def test_a_two_child_root_under_a_reversible_model_keeps_the_unrooted_tree():
    """Four leaves, root -> (v -> a, b), (s -> c, d), Jukes-Cantor with the uniform root
    distribution.  The move (v, a, s) gives root -> (v -> s, b), a: the same unrooted tree ab|cd
    with the lengths along the root's edge redistributed -- a now t_a + t_v from v, and v t_s from
    s.  So its log-likelihood is that of the UNMOVED arrays with those lengths (1e-13), and where
    t_v = 0 the moves about v at the resident length leave log L unchanged."""
    T = nx.Graph()
    T.add_edge('r', 'v', weight=0.21)
    T.add_edge('v', 'a', weight=0.13)
    T.add_edge('v', 'b', weight=0.34)
    T.add_edge('r', 's', weight=0.08)
    T.add_edge('s', 'c', weight=0.27)
    T.add_edge('s', 'd', weight=0.19)
    ta = arrays(T, 'r')
    ix = ta.node_to_index
    leaves = [ix[x] for x in 'abcd']
    rng = np.random.RandomState(5)
    states = rng.randint(0, 4, size=(40, 4))
    obs = np.eye(4)[states]
    pi = np.full(4, 0.25)
    Q = 0.3 * (np.ones((4, 4)) - 4.0 * np.eye(4))
    for tv in (0.21, 0.0):
        t = ta.branch_lengths()
        t[ix['v']] = tv
        esd = np.stack([jc_matrix(x) for x in t])
        esd[0] = 0.0
        moves, values, status, base = nni_from_transitions(ta.indices, ta.indptr, esd, leaves, obs, pi)
        assert not status.any() and len(moves) == 4
        for k, (v, c, s) in enumerate(moves):
            # the unmoved tree with c's edge longer by t_v, the edge above v of length t_s and
            # s drawn into the root (length 0)
            t2 = t.copy()
            t2[c] = t[c] + t[v]
            t2[v], t2[s] = t[s], 0.0
            esd2 = np.stack([jc_matrix(x) for x in t2])
            same, _ = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd2, leaves, obs, pi)
            assert np.abs(values[:, k, 0] - (same - base)).max() <= 1e-13 * np.abs(base).max()
            if t[v] == 0.0:
                assert np.abs(values[:, k, 0]).max() <= 1e-13 * np.abs(base).max()
            else:
                assert np.abs(values[:, k, 0]).max() > 1e-3
        # a trial length in the place of the resident one: the grid column at t_v is the swap
        grid = np.zeros((ta.nnodes, 2))
        grid[:, 0] = t
        grid[:, 1] = 0.5 * t + 0.05
        _, gv, _, _ = nni_from_transitions(ta.indices, ta.indptr, esd, leaves, obs, pi, Q[None],
                                           np.zeros(ta.nnodes, dtype=np.int64), grid)
        assert np.abs(gv[:, :, 0] - values[:, :, 0]).max() <= 1e-13 * np.abs(base).max()
        assert np.abs(gv[:, :, 1] - values[:, :, 0]).max() > 1e-4


def test_reference_gives_minus_infinity_and_zero_sites():
    """root -> (v -> x, y), s with v observed; no state enters state 0.  Site 0: v = 1, s = 0:
    once s hangs below v its state 0 cannot be reached from 1 -- -inf for the two moves, at a
    live site.  Site 1 has likelihood 0 as it stands (x = 0 below v = 1): status 1 and zeros."""
    T = nx.Graph()
    T.add_edge(0, 1, weight=0.3)
    T.add_edge(1, 2, weight=0.2)
    T.add_edge(1, 3, weight=0.4)
    T.add_edge(0, 4, weight=0.5)
    ta = arrays(T, 0)
    assert list(ta.preorder_nodes) == [0, 1, 2, 3, 4]
    Q = np.array([[-1.0, 0.6, 0.4], [0.0, -1.0, 1.0], [0.0, 0.7, -0.7]])
    esd = np.stack([scipy.linalg.expm(Q * x) for x in ta.branch_lengths()])
    eye, one = np.eye(3), np.ones(3)
    obs = np.array([[eye[1], eye[1], eye[2], eye[0]],        # nodes 1 (v), 2, 3, 4 (s)
                    [eye[1], eye[0], one, one]])
    moves, values, status, base = nni_from_transitions(ta.indices, ta.indptr, esd, [1, 2, 3, 4], obs,
                                                       np.full(3, 1.0 / 3))
    assert moves.tolist() == [[1, 2, 4], [1, 3, 4]]
    assert status.tolist() == [0, 1] and np.isfinite(base[0]) and base[1] == 0.0
    assert np.isneginf(values[0]).all() and not values[1].any()


# ---- the surface ----------------------------------------------------------------------------

def test_entry_points_are_declared_bound_and_surfaced():
    from raoteh_amd import _lib, _tree, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    assert re.search(r'\bint rt_model_nni_moves\(', header)
    assert re.search(r'\bint rt_tree_nni_moves\(', header)
    assert re.search(r'\bint rt_sites_nni_scores\(', header)
    assert 'UNROOTED' in header                  # the two-child root is documented
    assert len(_lib.SIGNATURES['rt_model_nni_moves'][1]) == 4
    assert len(_lib.SIGNATURES['rt_sites_nni_scores'][1]) == 8
    for name in ('rt_model_nni_moves', 'rt_tree_nni_moves', 'rt_sites_nni_scores'):
        assert getattr(_lib.lib(), name) is not None
    assert callable(device.TreeModel.nni_moves) and callable(device.TreeModel.nni_scores)
    assert callable(_tree.nni_apply)
    assert device.NniScores._fields == ('moves', 'lengths', 'sums', 'values', 'status')
