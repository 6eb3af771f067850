"""Host reference of rt_sites_branch_expectations (test_branch_expect_cpu.py,
test_branch_expect_gpu.py): per site and per edge
    value = sum_{a, b : J[a][b] != 0} J[a][b] G[a][b] / P[a][b],   G = expm_frechet(t Q, t C)
with D, J from the oracle (oracle/oracle_numpy.py), P = scipy expm(t Q) and scipy's
expm_frechet, as examples/code2x3/extras.get_expected_ntransitions forms it -- never from a
device path.  C = E * Q off the diagonal, E on it (the meaning of include/raoteh_hip.h)."""
import json
import os

import networkx as nx
import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
from _posterior_cases import oracle_pmaps, oracle_site
from _resident_cases import down_pass

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden',
                      'branch_expectations.json')


def direction(E, Q):
    C = np.asarray(E, dtype=float) * Q
    np.fill_diagonal(C, np.diag(E))
    return C


def edge_value(J, P, G):
    """The reference's sum over the endpoint states, entries with J == 0 skipped."""
    live = J != 0
    return float((J[live] * G[live] / P[live]).sum())


def one_site_reference(T, root, nstates, allowed, root_distn, Q, E):
    """dict edge -> expectation for one site, edges as nx.bfs_edges directs them."""
    if E is None:
        E = np.ones((nstates, nstates))
        np.fill_diagonal(E, 0)
    pre, idx, ptr, esd = orc.get_expm_augmented_transitions(T, root, nstates, Q_default=Q)
    mask = orc.define_state_mask(allowed, pre, nstates)
    _, pmap = orc.esd_get_node_to_pmap(idx, ptr, esd, mask)
    D = orc.mc0_esd_get_node_to_distn(idx, ptr, esd, root_distn, pmap)
    J = orc.mc0_esd_get_joint_endpoint_distn(idx, ptr, esd, pmap, D)
    C = direction(E, Q)
    out = {}
    for na, nb in nx.bfs_edges(T, root):
        t = T[na][nb]['weight']
        v = pre.index(nb)
        G = scipy.linalg.expm_frechet(t * Q, t * C, compute_expm=False)
        out[na, nb] = edge_value(J[v], esd[v], G)
    return out


def load_golden():
    """The recorded calls of the reference's worked example: dicts with T, root, nstates,
    allowed, root_distn, Q, E (dense or None) and expectations {(na, nb): float}."""
    with open(GOLDEN) as f:
        fix = json.load(f)
    mats = [np.array(Q) for Q in fix['Q']]
    calls = []
    for row in fix['calls']:
        n = row['nstates']
        T = nx.Graph()
        for a, b, w in row['edges']:
            T.add_edge(a, b, weight=w)
        E = None
        if row['E'] is not None:
            E = np.zeros((n, n))
            for i, j, x in row['E']:
                E[i, j] = x
        calls.append(dict(
            T=T, root=row['root'], nstates=n, Q=mats[row['q']], E=E,
            root_distn=None if row['root_distn'] is None else np.array(row['root_distn']),
            allowed=dict((int(v), set(ss)) for v, ss in row['allowed'].items()),
            expectations=dict(((a, b), x) for a, b, x in row['expectations'])))
    return fix, calls


def branch_reference(model, case, coefs, check_sites=()):
    """(values f64[S, N, K], status int32[S]) of a _resident_cases.Case for the coefficient
    matrices `coefs` [K, n, n]: zero-likelihood sites give zeros.  The site-axis restatement
    of J is checked against the oracle's own per-site passes on `check_sites`."""
    ta = model.tree
    n = case.n
    t = ta.branch_lengths()
    coefs = np.asarray(coefs, dtype=float).reshape(-1, n, n)
    esd = np.zeros((ta.nnodes, n, n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * case.Qs[case.node_q[v]])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    L = oracle_pmaps(ta.indices, ta.indptr, esd, cols, case.obs_lik)
    D, U = down_pass(ta, esd, case.root_distn, L)
    S = L.shape[0]
    status = (~((L[:, 0] * case.root_distn).sum(axis=1) > 0)).astype(np.int32)
    values = np.zeros((S, ta.nnodes, len(coefs)))
    Gs = {}
    for v in range(1, ta.nnodes):
        P, Q = esd[v], case.Qs[case.node_q[v]]
        J = U[:, v][:, :, None] * P[None] * L[:, v][:, None, :]
        for k, E in enumerate(coefs):
            G = Gs[v, k] = scipy.linalg.expm_frechet(t[v] * Q, t[v] * direction(E, Q),
                                                     compute_expm=False)
            # (J != 0 implies P != 0; the entries with J == 0 add nothing)
            R = np.where(P != 0, G / np.where(P != 0, P, 1.0), 0.0)
            values[:, v, k] = (J * R[None]).sum(axis=(1, 2))
    for i in check_sites:
        got = oracle_site(ta.indices, ta.indptr, esd, case.root_distn, L[i])
        if got is None:
            assert status[i] == 1 and not values[i].any()
            continue
        Jo = got[1]
        for v in range(1, ta.nnodes):
            for k in range(len(coefs)):
                G = Gs[v, k]
                want = edge_value(Jo[v], esd[v], G)
                assert abs(values[i, v, k] - want) <= 1e-12 * max(abs(want), np.abs(G).max())
    return values, status


def make_coefs(n, count, seed):
    """`count` coefficient matrices: indicator-like 0/1 off the diagonal first, then one with a
    non-zero diagonal, one with negative entries, one all zero, the rest random."""
    rng = np.random.RandomState(seed)
    out = []
    for k in range(count):
        E = (rng.uniform(size=(n, n)) < 0.5).astype(float)
        np.fill_diagonal(E, 0.0)
        if k == 1:
            E = rng.uniform(0.0, 2.0, (n, n))            # weights of time on the diagonal
        elif k == 2:
            E = rng.uniform(-1.0, 1.0, (n, n))
            np.fill_diagonal(E, 0.0)
        elif k == 3:
            E = np.zeros((n, n))
        elif k > 3:
            E *= rng.uniform(0.5, 1.5, (n, n))
        out.append(E)
    return np.array(out)
