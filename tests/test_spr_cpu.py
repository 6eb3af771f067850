"""Host side of rt_model_spr_moves / rt_tree_spr_moves / rt_sites_spr_scores: the order and count
of the moves against a brute-force enumeration at radius 0, 1, 2 and without a limit,
raoteh_amd._tree.spr_apply against the hand-built arrays of the host reference
(tests/_spr_cases.py), a move out and back under the oracle, the reference's own invariants (the
two families of moves that leave the tree unchanged) and the formula of the header evaluated in
numpy against the brute force."""
import ctypes

import networkx as nx
import numpy as np
import pytest
import scipy.linalg

from oracle import oracle_numpy as orc
from _nni_cases import children_of, parents_of
from _spr_cases import (brute_moves, moved_arrays, moved_log_likelihoods, spr_formula,
                        spr_from_transitions, unlimited_count)
from _resident_cases import make_case


def arrays(T, root):
    from raoteh_amd._tree import TreeArrays
    return TreeArrays(T, root)


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
    """12-node trees with multifurcations (and, at some seeds, a single-child node)."""
    from raoteh_amd import device, synth
    T, root, _ = synth.random_tree(12, seed, max_children=3)
    ta = arrays(T, root)
    counts = []
    for radius in (0, 1, 2, None):
        got = device.tree_spr_moves(ta, radius)
        want = brute_moves(ta.indices, ta.indptr, radius)
        assert got.dtype == np.int32 and got.shape == want.shape and len(want) > 0
        assert np.array_equal(got, want)
        assert got.tolist() == sorted(got.tolist())              # c ascending, then y
        counts.append(len(got))
    assert counts == sorted(counts) and counts[0] < counts[-1]
    assert counts[-1] == unlimited_count(ta.indices, ta.indptr)
    assert np.array_equal(device.tree_spr_moves(ta), device.tree_spr_moves(ta, 99))
    # radius 0: the edge above v and the edges above the siblings of c
    kids = children_of(ta.indices, ta.indptr)
    want0 = []
    for c in range(1, ta.nnodes):
        v = int(ta.parent[c])
        want0 += [(c, y) for y in sorted(([v] if v else []) + [w for w in kids[v] if w != c])]
    assert device.tree_spr_moves(ta, 0).tolist() == [list(x) for x in want0]


def test_single_child_nodes_and_multifurcations_are_covered():
    from raoteh_amd import synth
    shapes = set()
    for seed in (0, 1, 2, 3, 4, 11):
        T, root, _ = synth.random_tree(12, seed, max_children=3)
        shapes |= set(np.diff(arrays(T, root).indptr).tolist())
    assert {1, 3} <= shapes


def test_moves_of_a_star_a_path_and_small_trees():
    from raoteh_amd import device
    ta = arrays(star(5), 0)
    for radius in (0, 1, None):
        got = device.tree_spr_moves(ta, radius)
        assert len(got) == 20                    # every leaf onto the edge above every other
        assert np.array_equal(got, brute_moves(ta.indices, ta.indptr, radius))
    ta = arrays(path(6), 0)
    for radius, count in ((0, 4), (1, 7), (2, 9), (None, 10)):
        # c = 2 .. 5 onto the edges above its ancestors but the root: 1 + 2 + 3 + 4 without a limit
        got = device.tree_spr_moves(ta, radius)
        assert len(got) == count
        assert np.array_equal(got, brute_moves(ta.indices, ta.indptr, radius))
    for T in (path(2), path(1)):
        ta = arrays(T, 0)
        for radius in (0, None):
            got = device.tree_spr_moves(ta, radius)
            assert got.shape == (0, 2) and got.dtype == np.int32
            assert brute_moves(ta.indices, ta.indptr, radius).shape == (0, 2)
    with pytest.raises(ValueError):
        device.tree_spr_moves(arrays(star(3), 0), -1)
    with pytest.raises(ValueError):
        device.tree_spr_moves(arrays(star(3), 0), 1.5)


def test_moves_capacity_and_bad_trees():
    from raoteh_amd import _lib
    ta = arrays(star(3), 0)
    p64, p32 = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    count = ctypes.c_int64(-1)
    moves = np.full((6, 2), -7, dtype=np.int32)
    call = _lib.lib().rt_tree_spr_moves
    idx, ptr = ta.indices.ctypes.data_as(p64), ta.indptr.ctypes.data_as(p64)
    assert call(ta.nnodes, idx, ptr, -1, None, 0, ctypes.byref(count)) == _lib.RT_OK
    assert count.value == 6
    # too small an array: refused, the count still returned, nothing written
    count.value = -1
    assert call(ta.nnodes, idx, ptr, -1, moves.ctypes.data_as(p32), 5,
                ctypes.byref(count)) == _lib.RT_ERR_INVALID
    assert count.value == 6 and (moves == -7).all()
    assert call(ta.nnodes, idx, ptr, -1, moves.ctypes.data_as(p32), 6,
                ctypes.byref(count)) == _lib.RT_OK
    assert np.array_equal(moves, brute_moves(ta.indices, ta.indptr))
    bad = ta.indices.copy()
    bad[0] = 0                                   # a child that is not after its parent
    assert call(ta.nnodes, bad.ctypes.data_as(p64), ptr, -1, None, 0,
                ctypes.byref(count)) == _lib.RT_ERR_INVALID
    # a child listed twice leaves another node without a parent: refused at every radius, before
    # anything walks up through the parents
    twice = ta.indices.copy()
    twice[1] = twice[0]
    for radius in (-1, 0, 2):
        assert call(ta.nnodes, twice.ctypes.data_as(p64), ptr, radius, None, 0,
                    ctypes.byref(count)) == _lib.RT_ERR_INVALID
        assert 'twice' in _lib.last_error()
    tb = arrays(path(5), 0)
    deep = tb.indices.copy()
    deep[3] = deep[2]                            # ... and so does one deeper in the tree
    assert call(tb.nnodes, deep.ctypes.data_as(p64), tb.indptr.ctypes.data_as(p64), -1, None, 0,
                ctypes.byref(count)) == _lib.RT_ERR_INVALID


# ---- spr_apply ------------------------------------------------------------------------------

@pytest.mark.parametrize('seed', [0, 3, 11])
def test_spr_apply_agrees_with_the_hand_built_arrays(seed):
    """For every move: TreeArrays of the rearranged networkx tree has the CSR of the reference's
    moved_arrays, node for node; the pruned edge and every other edge keep their attributes, the
    two halves of the cut edge carry its attributes with the split length."""
    from raoteh_amd import synth
    from raoteh_amd._tree import spr_apply
    T, root, _ = synth.random_tree(12, seed, max_children=3)
    for a, b, d in T.edges(data=True):
        d['tag'] = ('edge', a, b)
    ta = arrays(T, root)
    below = dict((ta.preorder_nodes[i], ta.edge_data[i]) for i in range(1, ta.nnodes))
    before = nx.to_dict_of_dicts(T)
    rho = 0.3
    for c, y in brute_moves(ta.indices, ta.indptr):
        lc, ly = ta.preorder_nodes[int(c)], ta.preorder_nodes[int(y)]
        moved = spr_apply(T, root, lc, ly, rho, cut_label='new')
        assert moved is not T and nx.to_dict_of_dicts(T) == before       # T is as it was
        tm = arrays(moved, root)
        ni, npt, old_of_new = moved_arrays(ta.indices, ta.indptr, int(c), int(y))
        assert np.array_equal(tm.indices, ni) and np.array_equal(tm.indptr, npt)
        labels = list(ta.preorder_nodes) + ['new']
        assert tm.preorder_nodes == [labels[int(k)] for k in old_of_new]
        t = below[ly]['weight']
        for i in range(1, tm.nnodes):
            label = tm.preorder_nodes[i]
            if label == 'new':
                assert tm.edge_data[i] == dict(below[ly], weight=rho * t)
            elif label == ly:
                assert tm.edge_data[i] == dict(below[ly], weight=(1.0 - rho) * t)
            else:
                assert tm.edge_data[i] == below[label]
                assert tm.edge_data[i] is not below[label]               # (a copy)
        i_new = tm.node_to_index['new']
        assert [tm.preorder_nodes[int(k)] for k in
                tm.indices[tm.indptr[i_new]:tm.indptr[i_new + 1]]] == [ly, lc]
    assert spr_apply(T, root, lc, ly, 0.5).has_node(('cut', lc))


def test_spr_apply_rejects_what_is_not_a_move():
    from raoteh_amd._tree import spr_apply
    T = nx.Graph()                               # 0 -> (1 -> 3, 4), (2 -> 5, 6)
    for child in range(1, 7):
        T.add_edge((child - 1) // 2, child, weight=0.1 * child)
    assert arrays(spr_apply(T, 0, 3, 2, 0.5), 0).nnodes == 8
    for c, y, rho, label in ((0, 1, 0.5, None),  # the root pruned
                             (1, 0, 0.5, None),  # no edge above the root
                             (1, 3, 0.5, None),  # y inside the subtree of c
                             (1, 1, 0.5, None),  # y is c itself
                             (3, 99, 0.5, None),  # not a node
                             (3, 2, 1.5, None),  # not a fraction
                             (3, 2, 0.5, 4)):    # a label in use
        with pytest.raises(ValueError):
            spr_apply(T, 0, c, y, rho, cut_label=label)


def _oracle_total(T, root, case, q_of):
    """Sum of the oracle's log-likelihoods of the case's live sites on the tree T, every edge
    under scipy expm of the rate matrix q_of[node below it] at the edge's weight."""
    ta = arrays(T, root)
    t = ta.branch_lengths()
    esd = np.zeros((ta.nnodes, case.n, case.n))
    for i in range(1, ta.nnodes):
        esd[i] = scipy.linalg.expm(case.Qs[q_of[ta.preorder_nodes[i]]] * t[i])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    ll, st = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                       case.root_distn)
    return ll, st


@pytest.mark.parametrize('seed', [0, 3])
def test_spr_apply_out_and_back_restores_the_likelihood(seed):
    """c to a far edge at rho = 0.3, then back onto the edge above its old parent at rho = 1 (or
    above an old sibling at rho = 0 where that parent is the root): the cut nodes that stay are
    single-child nodes whose halves multiply to the matrix of the whole edge, and the one that
    carries c again sits on v across an identity."""
    from raoteh_amd._tree import spr_apply
    case = make_case(5, 12, 9, 'dense', 7700 + seed, internal=True, per_edge=True)
    ta = arrays(case.T, case.root)
    q_of = dict((ta.preorder_nodes[i], int(case.node_q[i])) for i in range(ta.nnodes))
    ll0, st0 = _oracle_total(case.T, case.root, case, q_of)
    moves = brute_moves(ta.indices, ta.indptr)
    kids = children_of(ta.indices, ta.indptr)
    done = 0
    for c, y in moves[::7]:
        c, y = int(c), int(y)
        v = int(ta.parent[c])
        lc, ly, lv = (ta.preorder_nodes[k] for k in (c, y, v))
        out = spr_apply(case.T, case.root, lc, ly, 0.3, cut_label='x1')
        q1 = dict(q_of, x1=q_of[ly])
        ll1, st1 = _oracle_total(out, case.root, case, q1)
        if v:
            back = spr_apply(out, case.root, lc, lv, 1.0, cut_label='x2')
            q2 = dict(q1, x2=q_of[lv])
        else:
            sib = ta.preorder_nodes[[w for w in kids[0] if w != c][0]]
            # (the sibling may be y: the edge below the root is then the one above the cut node)
            back = spr_apply(out, case.root, lc, 'x1' if sib == ly else sib, 0.0, cut_label='x2')
            q2 = dict(q1, x2=q_of[sib])
        ll2, st2 = _oracle_total(back, case.root, case, q2)
        assert np.array_equal(st2, st0)
        live = st0 == 0
        assert np.abs(ll2[live] - ll0[live]).max() <= 1e-12 * np.maximum(1, np.abs(ll0[live])).max()
        done += bool(np.abs(ll1[live & (st1 == 0)] - ll0[live & (st1 == 0)]).max() > 1e-6)
    assert done >= 3                             # (the moves out did change something)


# ---- the reference against itself and against the formula ------------------------------------

def _host_case(n, seed, nsites=9, zero_edge=True):
    case = make_case(n, 12, nsites, 'dense' if n > 4 else 'mask', seed, internal=True, per_edge=True)
    ta = arrays(case.T, case.root)
    t = ta.branch_lengths().copy()
    if zero_edge:
        t[3] = 0.0                               # a resident length of 0
    esd = np.zeros((ta.nnodes, n, n))
    for i in range(1, ta.nnodes):
        esd[i] = scipy.linalg.expm(case.Qs[case.node_q[i]] * t[i])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return case, ta, t, esd, cols


@pytest.mark.parametrize('n,seed', [(4, 0), (5, 3)])
def test_moves_that_leave_the_tree_unchanged_score_zero(n, seed):
    """(c, v) at rho = 1 and (c, sibling of c) at rho = 0: the cut node coincides with v across an
    identity matrix, so the reference's value is 0 to rounding at every live site."""
    case, ta, t, esd, cols = _host_case(n, 7800 + seed)
    moves, values, status, ll = spr_from_transitions(
        ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, t, (0.0, 1.0), 0,
        case.Qs, case.node_q)
    assert np.array_equal(moves, brute_moves(ta.indices, ta.indptr, 0))
    live = status == 0
    assert live.sum() >= len(live) - 1
    up = seen = 0
    for k, (c, y) in enumerate(moves):
        if y == ta.parent[c]:
            assert np.abs(values[live, k, 1]).max() <= 1e-12
            up += 1
        else:
            assert ta.parent[y] == ta.parent[c]
            assert np.abs(values[live, k, 0]).max() <= 1e-12
            seen += 1
    assert up >= 5 and seen >= 5
    assert np.abs(values[live]).max() > 1e-3     # (the other fraction is a real move)


@pytest.mark.parametrize('n,seed', [(4, 0), (5, 3), (5, 11)])
def test_the_formula_agrees_with_the_brute_force(n, seed):
    """Every move without a limit at rho in {0, 0.3, 1}: the ratio of the header's formula,
    evaluated in numpy from _nni_cases.up_pass, against the oracle on the hand-built moved tree,
    to 1e-10 absolute; rate matrices with structural zeros, observed internal nodes, a resident
    length of 0, a zero-likelihood site."""
    case, ta, t, esd, cols = _host_case(n, 7900 + seed)
    fractions = (0.0, 0.3, 1.0)
    base, status = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                             case.root_distn)
    live = status == 0
    moves = brute_moves(ta.indices, ta.indptr)
    assert len(moves) == unlimited_count(ta.indices, ta.indptr)
    worst = 0.0
    for c, y in moves:
        Q = case.Qs[case.node_q[y]]
        for rho in fractions:
            Pa, Pb = scipy.linalg.expm(Q * rho * t[y]), scipy.linalg.expm(Q * (1 - rho) * t[y])
            ratio, lik, _, _ = spr_formula(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                           case.root_distn, int(c), int(y), Pa, Pb)
            ll, st = moved_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                           case.root_distn, c, y, Pa, Pb)
            want = np.where(st == 0, np.exp(ll - np.where(live, base, 0.0)), 0.0)
            assert np.allclose(lik[live], np.exp(base[live]), rtol=1e-12, atol=0)
            worst = max(worst, np.abs(ratio[live] - want[live]).max())
            assert not ratio[~live].any()
    print('n=%d: %d moves x 3 fractions, worst |ratio - brute force| %.2e (bound 1e-10)'
          % (n, len(moves), worst))
    assert worst <= 1e-10


def test_the_declared_surface():
    from raoteh_amd import _lib, device, _tree
    for name in ('rt_model_spr_moves', 'rt_tree_spr_moves', 'rt_sites_spr_scores'):
        assert name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name)
    assert device.SprScores._fields == ('moves', 'fractions', 'sums', 'values', 'status', 'best')
    assert 'spr_apply' in _tree.__all__
    for name in ('spr_moves', 'spr_scores'):
        assert callable(getattr(device.TreeModel, name))
