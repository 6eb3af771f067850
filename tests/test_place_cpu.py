"""Host side of rt_sites_placements: raoteh_amd._tree.place_apply (the shape of the new tree, its
edges, its refusals), the host reference (tests/_place_cases.py) against its own invariants --
an all-ones query changes nothing, the attachment points that coincide agree, place_apply and the
oracle give what the hand-built arrays give --, device.check_placement_grid and the declared
surface."""
import re

import networkx as nx
import numpy as np
import pytest
import scipy.linalg

from conftest import ROOT
from oracle import oracle_numpy as orc
from _nni_cases import children_of
from _place_cases import (place_from_transitions, placed_arrays, placed_log_likelihoods,
                          query_likelihoods)
from _resident_cases import make_case


def arrays(T, root):
    from raoteh_amd._tree import TreeArrays
    return TreeArrays(T, root)


def small_tree():
    T = nx.Graph()                               # 0 -> (1 -> 3, 4), 2
    T.add_edge(0, 1, weight=0.4, tag='a', Q='Qa')
    T.add_edge(0, 2, weight=0.3, tag='b')
    T.add_edge(1, 3, weight=0.2, tag='c')
    T.add_edge(1, 4, weight=0.1, tag='d')
    return T


# ---- place_apply ------------------------------------------------------------------------------

def test_place_apply_shape_edges_and_child_order():
    from raoteh_amd._tree import place_apply
    T = small_tree()
    before = nx.to_dict_of_dicts(T)
    out = place_apply(T, 0, 1, 0.25, 0.7, 'q')
    assert out is not T and nx.to_dict_of_dicts(T) == before and type(out) is type(T)
    ta = arrays(out, 0)
    cut = ('cut', 'q')
    assert ta.preorder_nodes == [0, cut, 1, 3, 4, 'q', 2]      # the cut node in the place of 1
    assert children_of(ta.indices, ta.indptr) == [[1, 6], [2, 5], [3, 4], [], [], [], []]
    assert out[0][cut] == {'weight': 0.25 * 0.4, 'tag': 'a', 'Q': 'Qa'}
    assert out[cut][1] == {'weight': 0.75 * 0.4, 'tag': 'a', 'Q': 'Qa'}
    assert out[cut]['q'] == {'weight': 0.7, 'tag': 'a', 'Q': 'Qa'}
    assert out[1][3] == T[1][3] and out[1][3] is not T[1][3]
    assert not out.has_edge(0, 1) and out.number_of_nodes() == 7 and out.number_of_edges() == 6
    t = ta.branch_lengths()
    assert t[1] + t[2] == pytest.approx(0.4, abs=1e-16) and t[5] == 0.7
    # a leaf's edge, the ends of the edge, a label of the caller's for the cut node
    for fraction in (0.0, 1.0):
        leaf = place_apply(T, 0, 4, fraction, 0.0, 'q', cut_label='x')
        tl = arrays(leaf, 0)
        assert tl.preorder_nodes == [0, 1, 3, 'x', 4, 'q', 2]
        assert leaf[1]['x']['weight'] == fraction * 0.1
        assert leaf['x'][4]['weight'] == (1.0 - fraction) * 0.1 and leaf['x']['q']['weight'] == 0.0
    # the same arrays as the reference builds by hand
    ta0 = arrays(T, 0)
    for v in range(1, ta0.nnodes):
        ni, npt, old_of_new = placed_arrays(ta0.indices, ta0.indptr, v)
        tp = arrays(place_apply(T, 0, ta0.preorder_nodes[v], 0.5, 0.1, 'q'), 0)
        assert np.array_equal(tp.indices, ni) and np.array_equal(tp.indptr, npt)
        labels = ta0.preorder_nodes + [cut, 'q']
        assert tp.preorder_nodes == [labels[int(k)] for k in old_of_new]


def test_place_apply_refusals():
    from raoteh_amd._tree import place_apply
    T = small_tree()
    for args in ((0, 0.5, 0.1, 'q'),             # the root
                 (99, 0.5, 0.1, 'q'),            # not a node
                 (1, 0.5, 0.1, 3),               # a label already in the tree
                 (1, -0.01, 0.1, 'q'), (1, 1.01, 0.1, 'q'), (1, float('nan'), 0.1, 'q')):
        with pytest.raises(ValueError):
            place_apply(T, 0, *args)
    with pytest.raises(ValueError):
        place_apply(T, 0, 1, 0.5, 0.1, 'q', cut_label=2)
    with pytest.raises(ValueError):
        place_apply(T, 42, 1, 0.5, 0.1, 'q')


# ---- the reference against itself ------------------------------------------------------------

def reference_case(n, seed, per_edge):
    case = make_case(n, 9, 7, 'mask', seed, internal=True, per_edge=per_edge)
    ta = arrays(case.T, case.root)
    t = ta.branch_lengths()
    esd = np.zeros((ta.nnodes, n, n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * case.Qs[case.node_q[v]])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return case, ta, t, esd, cols


def some_queries(n, nsites, seed):
    rng = np.random.RandomState(seed)
    dense = rng.uniform(0.0, 1.0, size=(2, nsites, n))
    dense[:, :, 0] = 0.0
    return dense


@pytest.mark.parametrize('n', [3, 5])
def test_an_all_ones_query_changes_nothing(n):
    case, ta, t, esd, cols = reference_case(n, 9010 + n, per_edge=True)
    qlik = np.ones((1, 7, n))
    values, status, base = place_from_transitions(
        ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, t, qlik,
        [0.0, 0.3, 1.0], [0.0, 0.4], case.Qs, case.node_q)
    assert (status == 0).sum() >= 4 and status[-1] == 1
    assert np.abs(values[status == 0]).max() <= 1e-12
    assert not values[status != 0].any() and not values[:, :, 0].any()


@pytest.mark.parametrize('n', [3, 5])
def test_coinciding_attachment_points_agree(n):
    """One shared Q.  rho = 0 on every child edge of one p is the same tree (the pendant edge
    hangs at p); rho = 1 on v is rho = 0 on each child edge of v (it hangs at v)."""
    case, ta, t, esd, cols = reference_case(n, 9020 + n, per_edge=False)
    qlik = some_queries(n, 7, n)
    values, status, base = place_from_transitions(
        ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, t, qlik, [0.0, 1.0],
        [0.0, 0.25], case.Qs, case.node_q)
    live = status == 0
    assert live.sum() >= 4
    tol = 1e-12 * np.maximum(1.0, np.abs(base[live]))[:, None, None]
    kids = children_of(ta.indices, ta.indptr)
    seen = 0
    for p, ch in enumerate(kids):
        for w in ch[1:]:
            a, b = values[live][:, :, ch[0], 0], values[live][:, :, w, 0]
            assert np.array_equal(np.isneginf(a), np.isneginf(b))
            fin = np.isfinite(a)
            assert (np.abs(np.where(fin, a - b, 0.0)) <= tol).all()
            seen += 1
        if p:
            for w in ch:
                a, b = values[live][:, :, p, 1], values[live][:, :, w, 0]
                assert np.array_equal(np.isneginf(a), np.isneginf(b))
                fin = np.isfinite(a)
                assert (np.abs(np.where(fin, a - b, 0.0)) <= tol).all()
                seen += 1
    assert seen >= 6
    assert np.abs(values[live][np.isfinite(values[live])]).max() > 1e-3     # (not all zero)


@pytest.mark.parametrize('n', [3, 5])
def test_place_apply_and_the_oracle_give_the_hand_built_reference(n):
    from raoteh_amd._tree import place_apply
    case, ta, t, esd, cols = reference_case(n, 9030 + n, per_edge=True)
    qlik = some_queries(n, 7, n)
    base, bstat = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                            case.root_distn)
    for v, rho, tau in ((1, 0.3, 0.2), (ta.nnodes - 1, 1.0, 0.0), (ta.nnodes // 2, 0.0, 0.5)):
        Qv = case.Qs[case.node_q[v]]
        Pa, Pb = scipy.linalg.expm(Qv * rho * t[v]), scipy.linalg.expm(Qv * (1.0 - rho) * t[v])
        Pt = scipy.linalg.expm(Qv * tau)
        want, wst = placed_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                           case.root_distn, v, Pa, Pb, Pt, qlik)
        T2 = place_apply(case.T, case.root, ta.preorder_nodes[v], rho, tau, 'query')
        t2 = arrays(T2, case.root)
        q_of = dict((ta.preorder_nodes[i], case.node_q[i]) for i in range(ta.nnodes))
        q_of['query'] = q_of[('cut', 'query')] = case.node_q[v]
        len2 = t2.branch_lengths()
        esd2 = np.zeros((t2.nnodes, n, n))
        for i in range(1, t2.nnodes):
            esd2[i] = scipy.linalg.expm(len2[i] * case.Qs[q_of[t2.preorder_nodes[i]]])
        cols2 = [t2.node_to_index[x] for x in case.obs_nodes] + [t2.node_to_index['query']]
        for q in range(qlik.shape[0]):
            obs = np.concatenate([case.obs_lik, qlik[q][:, None, :]], axis=1)
            got, gst = orc.batch_log_likelihoods(t2.indices, t2.indptr, esd2, cols2, obs,
                                                 case.root_distn)
            assert np.array_equal(gst, wst[q])
            ok = gst == 0
            assert ok.sum() >= 3
            assert np.abs(got[ok] - want[q][ok]).max() <= 1e-12 * np.abs(base[bstat == 0]).max()


def test_state_queries_as_likelihoods():
    lik = query_likelihoods(np.array([[0, 2, 3, 255]], dtype=np.uint8), 'state', 3)
    assert lik.tolist() == [[[1, 0, 0], [0, 0, 1], [1, 1, 1], [1, 1, 1]]]


# ---- the grid's checks, the surface ----------------------------------------------------------

def test_check_placement_grid():
    from raoteh_amd import device
    f, t = device.check_placement_grid((0, 0.5, 1), [0.0, 2.5])
    assert f.dtype == np.float64 and f.tolist() == [0.0, 0.5, 1.0] and t.tolist() == [0.0, 2.5]
    assert f.flags.c_contiguous and t.flags.c_contiguous
    device.check_placement_grid([0.5] * 8, [0.1] * 16)
    for fractions, pendant in (([], [0.1]), ([0.5], []), ([0.5] * 9, [0.1]), ([0.5], [0.1] * 17),
                               ([-0.1], [0.1]), ([1.5], [0.1]), ([np.nan], [0.1]),
                               ([0.5], [-1e-9]), ([0.5], [np.inf]), ([0.5], [np.nan]),
                               ([[0.5]], [0.1]), ([0.5], [[0.1]]), ('ab', [0.1]), (None, [0.1]),
                               ([0.5], None)):
        with pytest.raises(ValueError):
            device.check_placement_grid(fractions, pendant)


def test_entry_point_is_declared_bound_and_surfaced():
    import ctypes
    from raoteh_amd import _lib, _tree, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    decl = re.search(r'\bint rt_sites_placements\(([^;]*)\);', header)
    assert decl and len(decl.group(1).split(',')) == 13
    assert re.search(r'#define RT_MAX_PLACE_FRACTIONS\s+8\b', header)
    assert re.search(r'#define RT_MAX_PLACE_PENDANT\s+16\b', header)
    assert (_lib.RT_MAX_PLACE_FRACTIONS, _lib.RT_MAX_PLACE_PENDANT) == (8, 16)
    restype, argtypes = _lib.SIGNATURES['rt_sites_placements']
    assert restype is ctypes.c_int and len(argtypes) == 13
    assert argtypes[4] is ctypes.c_int and argtypes[5] is ctypes.c_void_p
    assert getattr(_lib.lib(), 'rt_sites_placements') is not None
    assert callable(device.TreeModel.place_queries) and callable(_tree.place_apply)
    assert callable(device.check_placement_grid)
    assert device.Placements._fields == ('fractions', 'pendant', 'sums', 'values', 'status', 'best')
    with open(f'{ROOT}/raoteh_amd/csrc/Makefile') as f:
        assert 'place.hip' in f.read()
