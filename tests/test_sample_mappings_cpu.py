"""Host side of rt_sites_sample_mappings: the numpy mirror of the branch rule
(tests/_mapping_cases.py) follows the law it is meant to sample -- its means converge to the
exact conditional expectations -- and every case of the GPU parity tests keeps its pick targets
away from the cell boundaries, which is what makes exact event counts a fair demand there; the
entry point, its binding and the Python argument checks exist."""
import re

import numpy as np
import pytest

from conftest import ROOT
from _posterior_cases import oracle_site
import _mapping_cases as mc
import _sample_cases as sc


def test_the_mirror_follows_the_law():
    """n = 4, a 14-node tree, 2 sites, 2048 draws: the mean of every statistic on every branch
    against sum_ab J[a][b] G[a][b] / P[a][b] (scipy's expm of the block matrix), within 5 sample
    standard errors + 1e-9 per cell; the dwell times of a path sum to the branch length."""
    n, ndraws = 4, 2048
    T, root, leaves, Q0, rd, data, lik = sc.law_case(n)
    ta, Q, node_q, t, esd = mc.host_model(T, root, n, Q0)
    assert ta.nnodes == 14 and lik.shape[0] == 2
    states, status, L = mc.host_states(ta, esd, rd, leaves, lik, sc.LAW_SEED, 0, ndraws)
    assert not status.any()
    coefs = mc.parity_coefs(n, seed=1)
    got = mc.numpy_mappings(Q, t, node_q, ta.parent, states, coefs, sc.LAW_SEED, 0)
    assert not got['status'].any()
    vals = got['values']
    for i in range(2):
        _, J = oracle_site(ta.indices, ta.indptr, esd, rd, L[i])
        want = mc.exact_expectations(Q, t, node_q, esd, J, coefs)
        mean = vals[:, i].mean(axis=0)
        se = vals[:, i].std(axis=0, ddof=1) / np.sqrt(ndraws)
        assert (np.abs(mean - want) <= 5 * se + 1e-9).all(), np.abs(mean - want).max()
        assert np.abs(mean - want)[1:, :2].max() > 0      # (a sample, not the expectation itself)
    np.testing.assert_allclose(vals[:, :, 1:, 2], np.broadcast_to(t[1:], vals.shape[:2] + (13,)),
                               rtol=1e-12)
    cnt = got['counts']
    a = states[:, :, ta.parent[1:]]
    b = states[:, :, 1:]
    assert (cnt[:, :, 1:, 1][a != b] >= 1).all() and (cnt[:, :, 1:, 1][a == b] != 1).all()
    assert (cnt[..., 1] <= cnt[..., 0]).all() and (cnt[:, :, 0] == 0).all()
    # a draw depends on (seed, first_draw + d, site, node) alone
    tail = mc.numpy_mappings(Q, t, node_q, ta.parent, states[5:9], coefs, sc.LAW_SEED, 5)
    assert np.array_equal(tail['values'], vals[5:9]) and np.array_equal(tail['counts'], cnt[5:9])


def margin_of(T, root, n, Q0, rd, leaves, lik, seed, first_draw, ndraws, t=None, Q=None,
              dead_sites=False):
    ta, Qs, node_q, tt, esd = mc.host_model(T, root, n, Q0)
    if t is not None or Q is not None:
        import scipy.linalg
        tt = tt if t is None else t
        Qs = Qs if Q is None else Q
        for v in range(1, ta.nnodes):
            esd[v] = scipy.linalg.expm(tt[v] * Qs[node_q[v]])
    states, status, _ = mc.host_states(ta, esd, rd, leaves, lik, seed, first_draw, ndraws)
    assert dead_sites or not status.any()
    got = mc.numpy_mappings(Qs, tt, node_q, ta.parent, states, mc.parity_coefs(n, seed), seed,
                            first_draw)
    live = lik.shape[0] - int((status != 0).sum())
    assert not got['status'].any() and got['picks'] >= ndraws * live * (ta.nnodes - 1)
    return got['margin']


@pytest.mark.parametrize('n', mc.PARITY_NS)
def test_margins_of_the_parity_cases(n):
    T, root, leaves, Q, rd, data, lik, seed = mc.parity_case(n)
    m = margin_of(T, root, n, Q, rd, leaves, lik, seed, mc.PARITY_FIRST, mc.PARITY_DRAWS)
    assert m > mc.MARGIN, m


@pytest.mark.parametrize('n', [4, 20, 61])
def test_margins_of_the_per_edge_cases(n):
    T, root, leaves, Q, rd, data, lik, seed = mc.per_edge_case(n)
    m = margin_of(T, root, n, Q, rd, leaves, lik, seed, 0, 3)
    assert m > mc.MARGIN, m
    ta, Qs, node_q, _, _ = mc.host_model(T, root, n, Q)
    assert Qs.shape[0] > 1
    m = margin_of(T, root, n, Q, rd, leaves, lik, seed + 1, 0, 3, Q=mc.second_rates(Qs, seed))
    assert m > mc.MARGIN, m


@pytest.mark.parametrize('n', [7, 20])
def test_margins_of_the_branch_length_cases(n):
    T, root, leaves, Q, rd, data, lik, t, seed = mc.length_case(n)
    lam = (-np.diag(Q)).max() * t
    assert abs(lam.max() - 40.0) < 1e-9 and mc.edge_constants(Q[None], t, np.zeros(14, int),
                                                              int(lam.argmax()))[3] == 124
    m = margin_of(T, root, n, Q, rd, leaves, lik, seed, 0, 3, t=t)
    assert m > mc.MARGIN, m


@pytest.mark.parametrize('n', [4, 20, 70])
@pytest.mark.parametrize('kind', ['state', 'mask', 'dense'])
def test_margins_of_the_observation_kind_cases(kind, n):
    T, root, obs_nodes, Q, rd, data, lik = mc.kinds_case(kind, n)
    m = margin_of(T, root, n, Q, rd, obs_nodes, lik, 9, 0, 3, dead_sites=kind == 'dense')
    assert m > mc.MARGIN, m


def test_margins_of_the_split_case():
    T, root, leaves, Q, rd, data, lik = mc.split_case(14)
    m = margin_of(T, root, 7, Q, rd, leaves, lik, 3, 7, 17)
    assert m > mc.MARGIN, m


def test_the_pick_margin_sees_a_close_call():
    """Negative control of the margin: a target moved onto a boundary is reported."""
    w = np.array([[0.25, 0.0, 0.5, 0.25]])
    idx, m = mc.pick(w, np.array([0.5]))
    assert idx[0] == 2 and abs(m[0] - 0.25) < 1e-15
    idx, m = mc.pick(w, np.array([0.25 + 1e-12]))
    assert idx[0] == 2 and m[0] < 1e-11
    idx, m = mc.pick(w, np.array([1e-14]))                 # nothing below the first cell
    assert idx[0] == 0 and abs(m[0] - 0.25) < 1e-12
    idx, m = mc.pick(np.zeros((1, 3)), np.array([0.3]))
    assert idx[0] == -1


def test_entry_point_is_declared_bound_and_surfaced():
    from raoteh_amd import _lib, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    assert re.search(r'\bint rt_sites_sample_mappings\(', header)
    m = re.search(r'#define RT_MAX_MAPPING_EVENTS (\d+)\b', header)
    assert m and int(m.group(1)) == _lib.RT_MAX_MAPPING_EVENTS == mc.MAX_EVENTS
    restype, argtypes = _lib.SIGNATURES['rt_sites_sample_mappings']
    assert len(argtypes) == 13
    assert getattr(_lib.lib(), 'rt_sites_sample_mappings') is not None
    assert device.SampledMappings._fields == ('states', 'values', 'counts', 'means', 'status',
                                              'nodes')


class FakeTree(object):
    nnodes = 3
    preorder_nodes = [0, 1, 2]


class FakeBatch(object):
    nsites = 2
    _h = None


def test_python_argument_checks():
    """The checks made before the library is called (no device needed to fail them)."""
    from raoteh_amd import device
    model = object.__new__(device.TreeModel)
    model.nstates, model.tree, model._h = 4, FakeTree(), None
    batch = FakeBatch()
    E = np.zeros((4, 4))
    for kwargs in (dict(ndraws=0), dict(ndraws=-3), dict(seed=-1), dict(seed=1 << 64),
                   dict(first_draw=-1), dict(first_draw=(1 << 64) - 1, ndraws=2)):
        with pytest.raises(ValueError):
            model.sample_mappings(batch, E, **kwargs)
    for coefs in (np.zeros((3, 3)), np.zeros((9, 4, 4)), np.zeros((0, 4, 4)), 'x',
                  np.full((4, 4), np.nan)):
        with pytest.raises(ValueError):
            model.sample_mappings(batch, coefs)
