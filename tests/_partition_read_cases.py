"""Host reference of rt_sites_branch_expectations_partitioned (test_partition_reads_cpu.py,
test_partition_reads_gpu.py): per rate set k, _branch_cases.branch_reference over that set's
sites with t[k] and Q[k][node_q] -- scipy expm and expm_frechet, the oracle's upward and downward
passes, the site-axis restatement checked against oracle_site on a few sites of every set --
never from a device path.  The cases are _partition_cases.make_case's."""
import types

import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
from _branch_cases import branch_reference, direction, make_coefs  # noqa: F401 (re-exported)
import _partition_cases as pc


class _TreeWithLengths(object):
    """model.tree with the branch lengths of one rate set (what branch_reference reads)."""

    def __init__(self, ta, t):
        self._ta, self._t = ta, np.asarray(t, dtype=float)

    def branch_lengths(self):
        return self._t.copy()

    def __getattr__(self, name):
        return getattr(self._ta, name)


def set_case(ta, case, k, sites):
    """(model, case) as branch_reference takes them: rate set k of a _partition_cases.Case on
    the sites `sites`."""
    model = types.SimpleNamespace(tree=_TreeWithLengths(ta, case.t[k]))
    sub = types.SimpleNamespace(n=case.n, Qs=case.Q[k], node_q=case.node_q, obs_nodes=case.leaves,
                                obs_lik=case.obs_lik[sites], root_distn=case.root_distn)
    return model, sub


def coefs_of_set(coefs, n, k):
    """The coefficient matrices set k uses: (n, n) and (C, n, n) are shared, (nsets, C, n, n)
    holds set k's at [k]."""
    E = np.asarray(coefs, dtype=float)
    return E[k] if E.ndim == 4 else E.reshape(-1, n, n)


def partition_reference(ta, case, coefs, weights=None, check=2):
    """(values f64[S, N, C] in caller order, status int32[S], set_edge_sums f64[nsets, N, C],
    edge_sums f64[N, C]) for a _partition_cases.Case: a site of zero likelihood under its set
    has zero values, an empty set zero rows.  `check`: sites per set on which branch_reference
    checks its site-axis restatement against the oracle's own passes."""
    n, S = case.n, len(case.site_sets)
    C = coefs_of_set(coefs, n, 0).shape[0]
    w = np.ones(S) if weights is None else np.asarray(weights, dtype=float)
    values = np.zeros((S, ta.nnodes, C))
    status = np.zeros(S, dtype=np.int32)
    set_sums = np.zeros((case.nsets, ta.nnodes, C))
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        model, sub = set_case(ta, case, k, mine)
        picks = sorted(set(np.linspace(0, len(mine) - 1, check).astype(int))) if check else ()
        values[mine], status[mine] = branch_reference(model, sub, coefs_of_set(coefs, n, k),
                                                      check_sites=picks)
        set_sums[k] = np.einsum('i,ivc->vc', w[mine], values[mine])
    return values, status, set_sums, set_sums.sum(axis=0)


def gradient_coefs(Q):
    """The per-set coefficients of branch_length_gradient_partitioned for Q [nsets, 1, n, n]:
    ones off the diagonal, diag(Q[k]) on it."""
    K, n = Q.shape[0], Q.shape[-1]
    E = np.ones((K, 1, n, n))
    for k in range(K):
        np.fill_diagonal(E[k, 0], np.diag(Q[k, 0]))
    return E


def gradient_reference(ta, case, weights=None):
    """g[k, v] = d (sum_{i in set k} w_i log L_i) / d t[k][v] from the host reference (0 at the
    root), for a case with one rate matrix per set."""
    _, status, set_sums, _ = partition_reference(ta, case, gradient_coefs(case.Q), weights, check=0)
    assert not status.any()
    g = np.zeros((case.nsets, ta.nnodes))
    g[:, 1:] = set_sums[:, 1:, 0] / case.t[:, 1:]
    return g


def oracle_set_total(ta, case, k, t):
    """sum of the oracle's log-likelihoods (scipy expm, oracle pruning) over set k's sites with
    the branch lengths t [nnodes] in the place of t[k]."""
    esd = np.zeros((ta.nnodes, case.n, case.n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * case.Q[k, case.node_q[v]])
    cols = [ta.node_to_index[v] for v in case.leaves]
    mine = np.flatnonzero(case.site_sets == k)
    ll, st = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik[mine],
                                       case.root_distn)
    assert not st.any()
    return float(np.sum(ll))


def gradient_gap(ta, case, h):
    """(analytic g [nsets, nnodes] of the host reference, max over sets and branches of the gap
    between the oracle's central difference with step h and that value)."""
    analytic = gradient_reference(ta, case)
    fd = np.zeros_like(analytic)
    for k in range(case.nsets):
        if not (case.site_sets == k).any():
            continue
        for v in range(1, ta.nnodes):
            tp, tm = case.t[k].copy(), case.t[k].copy()
            tp[v] += h
            tm[v] -= h
            fd[k, v] = (oracle_set_total(ta, case, k, tp) - oracle_set_total(ta, case, k, tm)) / (2 * h)
    return analytic, float(np.abs(fd - analytic).max())


def gradient_case(n, seed, nsites):
    """'state' data, one rate matrix per set, no site of zero likelihood, three non-empty sets
    in a random order (set 3 empty)."""
    rng = np.random.RandomState(seed)
    case = pc.make_case(n, 'state', seed, nsites=nsites, site_sets=rng.randint(0, 3, size=nsites))
    return case._replace(Q=case.Q[:, :1].copy(), node_q=np.zeros_like(case.node_q))
