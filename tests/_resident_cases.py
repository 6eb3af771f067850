"""Host references for every read of a resident batch (test_resident_reads_gpu.py,
test_gpu_parity.py): random trees whose transition matrices have exact zeros, observations of
every kind at the leaves and at internal nodes, and what the log-likelihoods, totals, posterior
set sums and expected history statistics of such a batch must be -- computed from the oracle
(oracle/oracle_numpy.py) and scipy, never from another device path."""
import collections
import math

import networkx as nx
import numpy as np

from oracle import oracle_numpy as orc
from _posterior_cases import oracle_pmaps, oracle_site, sums_over_sets


def _extended_log_likelihoods(tree, esd, leaf_idx, states, n, root_w):
    """Felsenstein pruning in np.longdouble (x87 extended: exponent range 2^-16445) on the
    device's own transition matrices -- what the f64 recursion would give without underflow."""
    ld = np.longdouble
    nsites = states.shape[0]
    L = [None] * tree.nnodes
    col = dict((v, k) for k, v in enumerate(leaf_idx))
    for v in range(tree.nnodes - 1, -1, -1):
        x = np.ones((nsites, n), dtype=ld)
        if v in col:
            s = states[:, col[v]]
            obs = s != 255
            x[obs] = 0
            x[np.nonzero(obs)[0], s[obs]] = 1
        for c in tree.indices[tree.indptr[v]:tree.indptr[v + 1]]:
            x = x * (L[c] @ esd[c].astype(ld).T)
            L[c] = None
        L[v] = x
    lik = L[0] @ np.asarray(root_w, dtype=ld)
    return np.log(lik).astype(np.float64)


def rate_matrix(n, rng):
    """A random rate matrix that never enters state 0 (column 0 is zero off the diagonal): every
    P = expm(Q t) then has P[a][0] = 0 exactly for a != 0 -- zeros the expectation step must mask
    -- and state 0 observed below an observed state a != 0 has likelihood 0."""
    R = rng.uniform(0.1, 1.0, (n, n)) * (rng.uniform(size=(n, n)) < 0.7)
    R[np.arange(n), (np.arange(n) + 1) % n] += 0.3
    R[np.arange(2, n), np.arange(1, n - 1)] += 0.2         # states 1 .. n-1 communicate
    R[:, 0] = 0.0
    np.fill_diagonal(R, 0.0)
    return R - np.diag(R.sum(axis=1))


Case = collections.namedtuple(
    'Case', 'T root n obs_nodes kind data obs_lik Qs node_q root_distn zero_site')


def _encode(kind, n, lik):
    """0/1 allowed-set likelihoods f64[S, K, n] -> upload data of `kind`."""
    if kind == 'mask':
        words = np.zeros(lik.shape[:2] + ((n + 63) // 64,), dtype=np.uint64)
        for s in range(n):
            words[:, :, s >> 6] |= (lik[:, :, s] != 0).astype(np.uint64) << np.uint64(s & 63)
        return words[:, :, 0].copy() if n <= 64 else words
    return lik


def make_case(n, nnodes, nsites, kind, seed, internal=True, per_edge=False, every_leaf=False,
              pairs=False):
    """A tree, per-edge rate matrices (model.set_rates(Q=Qs, node_q=...) order) and observations.
    kind 'state' / 'mask' / 'dense' (0/1 for n <= 4, values above); `internal`: every second
    internal node observed too; `every_leaf`: leaves only, every leaf observed as one state
    (pairs: one or two states) -- what the gathered-column kernels take.  State 0 appears only
    at the last site, which has likelihood 0 (a leaf in state 0 below an observed state 1)
    wherever an internal node is observed."""
    from raoteh_amd import synth, _tree
    rng = np.random.RandomState(seed)
    T, root, leaves = synth.random_tree(nnodes, seed=seed, max_children=3)
    inner = [v for v in T if v not in leaves]
    obs_nodes = list(leaves) + (inner[::2] if internal else [])
    ta = _tree.TreeArrays(T, root)
    mats = [rate_matrix(n, rng)]
    node_q = np.zeros(ta.nnodes, dtype=np.int64)
    if per_edge:
        mats.append(rate_matrix(n, rng))
        node_q[1::3] = 1
    node_q[0] = 0
    root_distn = rng.uniform(0.1, 1.0, n)
    root_distn /= root_distn.sum()
    K = len(obs_nodes)
    S = nsites
    if kind == 'state' or every_leaf:
        st = rng.randint(1, n, size=(S, K)) if n > 1 else np.zeros((S, K), dtype=np.int64)
        if not every_leaf:
            st[rng.uniform(size=st.shape) < 0.1] = 255
        lik = np.ones((S, K, n))
        seen = st != 255
        lik[seen] = 0.0
        ii, kk = np.nonzero(seen)
        lik[ii, kk, st[ii, kk]] = 1.0
        if pairs:
            second = rng.randint(1, n, size=(S, K))
            lik[np.arange(S)[:, None], np.arange(K)[None, :], second] = 1.0
    elif kind == 'mask' or n <= 4:
        lik = (rng.uniform(size=(S, K, n)) < 0.4).astype(np.float64)
        lik[:, :, 0] = 0.0
        lik[:, :, 1 % n] = 1.0
    else:
        lik = rng.uniform(0.0, 1.0, size=(S, K, n))
        lik[rng.uniform(size=lik.shape) < 0.2] = 0.0
        lik[:, :, 0] = 0.0
        lik[:, :, 1] += 0.05
    zero_site = None
    if internal and n >= 2 and S > 1:
        # an observed internal node in state 1, a leaf below it in state 0: P[1][0] = 0 on
        # every edge of the path, likelihood 0 -- in the last (padded) block
        v = inner[0]
        D = nx.bfs_tree(T, root)
        c = sorted(u for u in nx.descendants(D, v) if u in leaves)[0]
        kv, kc = obs_nodes.index(v), obs_nodes.index(c)
        lik[-1, kv] = 0.0
        lik[-1, kv, 1] = 1.0
        lik[-1, kc] = 0.0
        lik[-1, kc, 0] = 1.0
        zero_site = S - 1
        if kind == 'state':
            st[-1, kv], st[-1, kc] = 1, 0
    if kind == 'state':
        data = st.astype(np.uint8)
    else:
        data = _encode(kind, n, lik) if kind == 'mask' else lik
    return Case(T, root, n, obs_nodes, kind, data, lik, np.stack(mats), node_q, root_distn,
                zero_site)


def set_rates(model, case, Qs=None):
    model.set_rates(Q=case.Qs if Qs is None else Qs, node_q=case.node_q)


def loglik_reference(model, case):
    """(log-likelihoods, statuses) of the oracle on the device's own transition matrices."""
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return orc.batch_log_likelihoods(ta.indices, ta.indptr, model.get_transitions(), cols,
                                     case.obs_lik, case.root_distn)


def totals_reference(ll, status):
    ok = (status & 1) == 0
    return np.array([math.fsum(ll[ok]), float((~ok).sum()), float(len(ll))])


def down_pass(ta, esd, root_distn, L):
    """Posterior marginals D [S, N, n] and u = D_p / M_v [S, N, n] of every site at once (the
    oracle's mc0_esd_get_node_to_distn, restated over the site axis); zero where the site's
    likelihood is zero."""
    S, N, n = L.shape
    D = np.zeros_like(L)
    U = np.zeros_like(L)
    w = L[:, 0] * root_distn
    tot = w.sum(axis=1)
    ok = tot > 0
    D[ok, 0] = w[ok] / tot[ok][:, None]
    for v in range(1, N):
        p = ta.parent[v]
        M = L[:, v] @ esd[v].T
        dp = D[:, p]
        assert not np.any((dp != 0) & ~(M > 0)), 'a zero denominator under a live parent state'
        U[:, v] = np.where(dp != 0, dp / np.where(M > 0, M, 1.0), 0.0)
        D[:, v] = (U[:, v] @ esd[v]) * L[:, v]
    return D, U


def set_sums(ta, esd, D, U, L, node_sets, edge_sets):
    """node_values [S, N, len(node_sets)], edge_values [S, N, len(edge_sets)] (root slot 0)."""
    S, N, n = D.shape
    nv = np.stack([D[:, :, sorted(A)].sum(axis=2) for A in node_sets], axis=2)
    ev = np.zeros((S, N, len(edge_sets)))
    for v in range(1, N):
        for k, (A, B) in enumerate(edge_sets):
            A, B = sorted(A), sorted(B)
            ev[:, v, k] = ((U[:, v][:, A] @ esd[v][np.ix_(A, B)]) * L[:, v][:, B]).sum(axis=1)
    return nv, ev


def posterior_reference(model, case, node_sets, edge_sets, check_sites):
    """(node_values, edge_values, marginals of every node, status) for every site, from the
    device's transition matrices; on `check_sites` the site-axis restatement is checked against
    the oracle's own per-site passes (oracle_site, sums_over_sets)."""
    ta = model.tree
    esd = model.get_transitions()
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    L = oracle_pmaps(ta.indices, ta.indptr, esd, cols, case.obs_lik)
    D, U = down_pass(ta, esd, case.root_distn, L)
    nv, ev = set_sums(ta, esd, D, U, L, node_sets, edge_sets)
    status = (~((L[:, 0] * case.root_distn).sum(axis=1) > 0)).astype(np.int32)
    for i in check_sites:
        got = oracle_site(ta.indices, ta.indptr, esd, case.root_distn, L[i])
        if got is None:
            assert status[i] == 1 and not D[i].any()
            continue
        Do, Jo = got
        nvo, evo = sums_over_sets(Do, Jo, node_sets, edge_sets)
        np.testing.assert_allclose(D[i], Do, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(nv[i], nvo, rtol=1e-12, atol=1e-300)
        np.testing.assert_allclose(ev[i], evo, rtol=1e-12, atol=1e-300)
    return nv, ev, D, status


def expectation_reference(model, case, Qs=None, check_sites=()):
    """(dwell, root posterior sums, transitions) independent of the device: P = scipy expm(t Q)
    per edge, W = sum over sites of J / P over the live entries (J from the oracle's joint
    endpoint distribution, restated over the site axis and checked against
    orc.mc0_esd_get_joint_endpoint_distn on `check_sites`), then one expm of the 2n block
    [[t Q^T, W], [0, t Q^T]] per edge."""
    import scipy.linalg
    Qs = case.Qs if Qs is None else Qs
    ta = model.tree
    n = case.n
    t = ta.branch_lengths()
    esd = np.zeros((ta.nnodes, n, n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * Qs[case.node_q[v]])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    L = oracle_pmaps(ta.indices, ta.indptr, esd, cols, case.obs_lik)
    D, U = down_pass(ta, esd, case.root_distn, L)
    for i in check_sites:
        got = oracle_site(ta.indices, ta.indptr, esd, case.root_distn, L[i])
        if got is None:
            continue
        Jo = got[1]
        for v in range(1, ta.nnodes):
            J = U[i, v][:, None] * esd[v] * L[i, v][None, :]
            np.testing.assert_allclose(J, Jo[v], rtol=1e-12, atol=1e-300)
    dwell, trans = np.zeros(n), np.zeros((n, n))
    rootp = D[:, 0].sum(axis=0)
    for v in range(1, ta.nnodes):
        P, Q = esd[v], Qs[case.node_q[v]]
        W = np.where(P != 0, U[:, v].T @ L[:, v], 0.0)         # sum_i J_i / P, live entries
        B = np.zeros((2 * n, 2 * n))
        B[:n, :n] = B[n:, n:] = t[v] * Q.T
        B[:n, n:] = W
        M = scipy.linalg.expm(B)[:n, n:]
        dwell += t[v] * np.diag(M)
        trans += np.where(Q != 0, t[v] * Q * M, 0.0)
    return dwell, rootp, trans
