"""Host reference of rt_sites_branch_profiles_mixture and rt_sites_nni_scores_mixture
(test_mixture_search_cpu.py, test_mixture_search_gpu.py) -- never a device path.  Per rate set k
the transition matrices come from _mixture_cases.set_transitions, the trial edge gets
scipy.linalg.expm(factor * t[k][v] * Q[k][node_q[v]]), the site likelihoods L_ik come from
oracle_numpy.batch_log_likelihoods (for a move: on _nni_cases.moved_arrays through
moved_log_likelihoods), and the definitions of include/raoteh_hip.h section 2d are combined in
numpy:  value = log sum_k c_k L_ik(trial) - log sum_k c_k L_ik,  sums in set order."""
import collections
import functools

import networkx as nx
import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
import _mixture_cases as mc
import _nni_cases as nc
from _profile_cases import _one_blas_thread

NSITES = mc.NSITES           # 83: six tiles of 16 sites, the last one partial; two lane blocks

Reference = collections.namedtuple('Reference', 'values sums loglik status moves')


def make_factors(nnodes, npoints, seed, per_branch=True):
    """[nnodes, npoints] factors (row 0 zero): 1 (the resident length), one below and one above,
    the rest log-uniform in [1/4, 4], shuffled (from nine points on one of them is 0); per_branch: every branch's row scaled by a draw
    of its own in [0.8, 1.25], so that the rows differ."""
    rng = np.random.RandomState(seed)
    head = [1.0, 0.5, 1.75] if npoints >= 3 else [0.5, 1.75]
    f = np.concatenate([head, np.exp(rng.uniform(-np.log(4), np.log(4), 64))])
    f = f[:npoints][rng.permutation(npoints)]
    if npoints >= 9:
        f[3] = 0.0                               # (the edge collapsed: P = I)
    grid = np.repeat(f[None, :], nnodes, axis=0)
    if per_branch:
        grid = grid * np.exp(rng.uniform(-np.log(1.25), np.log(1.25), nnodes))[:, None]
    grid[0] = 0.0
    return np.ascontiguousarray(grid)


def class_weights(K, seed):
    c = np.random.RandomState(seed).uniform(0.2, 1.0, K)
    return c / c.sum()


def site_weights(nsites, seed):
    w = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(float)
    w[2] = 0.0
    w[nsites // 2] = 0.0
    return w


def _likelihoods(ll, st):
    return np.where(st == 0, np.exp(np.where(st == 0, ll, 0.0)), 0.0)


def _cols(ta, case):
    nodes = case.leaves if hasattr(case, 'leaves') else case.obs_nodes
    return [ta.node_to_index[v] for v in nodes]


def _trial(case, k, v, factor):
    return scipy.linalg.expm(factor * case.t[k][v] * case.Q[k][case.node_q[v]])


def _finish(case, c, L, trial, weights, nan_rows, moves):
    """The definitions: L [K, S] resident, trial [K, S, R, G] the likelihoods at the trial
    points (zeros for the sets that do not run), nan_rows [R] bool."""
    K, S = L.shape
    c = np.asarray(c, dtype=float)
    _, loglik, dead = mc.combine(L, c)
    mix = np.zeros(trial.shape[1:])
    for k in range(K):
        if c[k] > 0:
            mix = mix + c[k] * trial[k]
    with np.errstate(divide='ignore'):
        values = np.log(mix) - np.where(dead, 0.0, loglik)[:, None, None]
    values[:, nan_rows, :] = np.nan
    values[dead] = 0.0
    w = np.ones(S) if weights is None else np.asarray(weights, dtype=float)
    use = (w != 0) & ~dead
    sums = np.einsum('i,irg->rg', w[use], values[use]) if use.any() else np.zeros(values.shape[1:])
    sums[nan_rows, :] = np.nan
    return Reference(values, sums, loglik, np.where(dead, 1, 0).astype(np.int32), moves)


def profile_reference(ta, case, c, factors, weights=None):
    """Reference of rt_sites_branch_profiles_mixture: values [S, N, G] (the root's row 0)."""
    case = mc.normalised(case)
    K, N = case.t.shape
    G = factors.shape[1]
    cols = _cols(ta, case)
    S = case.obs_lik.shape[0]
    L = np.zeros((K, S))
    trial = np.zeros((K, S, N, G))
    nan_rows = np.zeros(N, dtype=bool)
    for k in range(K):
        if not c[k] > 0:
            continue
        esd = mc.set_transitions(ta, case, k)
        L[k] = _likelihoods(*orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols,
                                                       case.obs_lik, case.root_distn))
        nan_rows[1:] |= case.t[k][1:] == 0
        with _one_blas_thread():
            mats = [[_trial(case, k, v, factors[v, g]) for g in range(G)] for v in range(1, N)]
        for v in range(1, N):
            for g in range(G):
                e = esd.copy()
                e[v] = mats[v - 1][g]
                trial[k, :, v, g] = _likelihoods(*orc.batch_log_likelihoods(
                    ta.indices, ta.indptr, e, cols, case.obs_lik, case.root_distn))
    ref = _finish(case, c, L, trial, weights, nan_rows, None)
    ref.values[:, 0, :] = 0.0                   # (the root's row)
    ref.sums[0] = 0.0
    return ref


def nni_reference(ta, case, c, factors=None, weights=None):
    """Reference of rt_sites_nni_scores_mixture: values [S, M, G]; factors None: the plain swap."""
    case = mc.normalised(case)
    K, N = case.t.shape
    G = 1 if factors is None else factors.shape[1]
    cols = _cols(ta, case)
    S = case.obs_lik.shape[0]
    moves = nc.brute_moves(ta.indices, ta.indptr)
    L = np.zeros((K, S))
    trial = np.zeros((K, S, len(moves), G))
    for k in range(K):
        if not c[k] > 0:
            continue
        esd = mc.set_transitions(ta, case, k)
        L[k] = _likelihoods(*orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols,
                                                       case.obs_lik, case.root_distn))
        mats = {}
        if factors is not None:
            with _one_blas_thread():
                for v in sorted(set(int(x) for x in moves[:, 0])):
                    mats[v] = [_trial(case, k, v, factors[v, g]) for g in range(G)]
        for j, (v, cc, s) in enumerate(moves):
            for g in range(G):
                e = esd
                if factors is not None:
                    e = esd.copy()
                    e[v] = mats[int(v)][g]
                trial[k, :, j, g] = _likelihoods(*nc.moved_log_likelihoods(
                    ta.indices, ta.indptr, e, cols, case.obs_lik, case.root_distn, (v, cc, s)))
    return _finish(case, c, L, trial, weights, np.zeros(len(moves), dtype=bool), moves)


@functools.lru_cache(maxsize=None)
def cached_case(n, tree, kind, K, seed, nsites=NSITES):
    """(case, tree arrays); dense data: site 4 observes nothing at its first leaf -- dead under
    every set."""
    case = mc.make_case(n, tree, kind, K, seed, nsites=nsites,
                        dead_site=4 if kind == 'dense' else None)
    return case, mc.tree_arrays(case)


@functools.lru_cache(maxsize=None)
def cached_reference(call, n, tree, kind, K, seed, npoints, weighted, nsites=NSITES):
    """The shared reference of a parity case (computed once; callers must not write to it):
    (case, ta, c, factors or None, site weights or None, Reference)."""
    case, ta = cached_case(n, tree, kind, K, seed, nsites)
    c = class_weights(K, seed + 1)
    w = site_weights(nsites, seed + 2) if weighted else None
    if call == 'profile':
        f = make_factors(ta.nnodes, npoints, seed + 3)
        ref = profile_reference(ta, case, c, f, w)
    else:
        f = None if npoints == 0 else make_factors(ta.nnodes, npoints, seed + 3)
        ref = nni_reference(ta, case, c, f, w)
    for a in ref[:4]:
        a.setflags(write=False)
    return case, ta, c, f, w, ref


# ---- the revival case -----------------------------------------------------------------------

RevivalCase = collections.namedtuple(
    'RevivalCase', 'T root n obs_nodes leaves kind data obs_lik root_distn Q node_q t site move')


def revival_case(n=3):
    """A set with L_ik == 0 on the resident tree and L_ik > 0 after a move, c_k > 0, Lambda_i > 0.
    Set 0 is one-way: its rate matrix allows a -> a + 1 only (0 -> 1 -> 2 ...).  The tree:
    root p with the children v and s; v with the children c and c2.  v is OBSERVED in state 1;
    the leaves are c = 0, c2 = 2, s = 2.  Under set 0 the resident tree is impossible
    (v = 1 cannot reach c = 0); after the move (v, c, s) it is possible: p = 0 reaches c = 0, and
    p = 0 -> v = 1 -> s, c2 = 2.  Set 1 has a full rate matrix and keeps the site alive.
    Site 0 is that site; site 1 is an ordinary one (every leaf 2, v unobserved)."""
    T = nx.Graph()
    p, v, s, c, c2 = 0, 1, 2, 3, 4
    T.add_edge(p, v, weight=0.3)
    T.add_edge(p, s, weight=0.2)
    T.add_edge(v, c, weight=0.25)
    T.add_edge(v, c2, weight=0.15)
    obs_nodes = [c, c2, s, v]
    top = 2
    st = np.array([[0, top, top, 1], [top, top, top, 255]], dtype=np.uint8)
    lik = np.ones((2, 4, n))
    for i in range(2):
        for k in range(4):
            if st[i, k] != 255:
                lik[i, k] = 0.0
                lik[i, k, st[i, k]] = 1.0
    one_way = np.zeros((n, n))
    for a in range(n - 1):
        one_way[a, a + 1] = 1.0 + 0.25 * a
        one_way[a, a] = -one_way[a, a + 1]
    rng = np.random.RandomState(4242 + n)
    full = rng.uniform(0.2, 1.0, (n, n))
    np.fill_diagonal(full, 0.0)
    full -= np.diag(full.sum(axis=1))
    Q = np.stack([one_way, full])[:, None]
    from raoteh_amd import _tree
    ta = _tree.TreeArrays(T, p)
    t = np.stack([ta.branch_lengths(), 0.8 * ta.branch_lengths()])
    t[:, 0] = 0.0
    root_distn = np.full(n, 1.0 / n)
    move = tuple(ta.node_to_index[x] for x in (v, c, s))
    return RevivalCase(T, p, n, obs_nodes, obs_nodes, 'state', st, lik, root_distn, Q,
                       np.zeros(ta.nnodes, dtype=np.int64), t, 0, move), ta


def revival_likelihoods(case, ta):
    """(L [K, S] on the resident tree, L' [K, S] after the case's move) from the oracle."""
    cols = _cols(ta, case)
    K = case.Q.shape[0]
    L = np.zeros((K, case.obs_lik.shape[0]))
    moved = np.zeros_like(L)
    for k in range(K):
        esd = mc.set_transitions(ta, case, k)
        L[k] = _likelihoods(*orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols,
                                                       case.obs_lik, case.root_distn))
        moved[k] = _likelihoods(*nc.moved_log_likelihoods(ta.indices, ta.indptr, esd, cols,
                                                          case.obs_lik, case.root_distn, case.move))
    return L, moved


def lost_case(n=3):
    """The converse on the same tree: a live site whose mixture likelihood is 0 after the move --
    the value is -inf.  Both sets are one-way (set 1 at 1.5 times the rates of set 0); v is
    observed in state 1, the leaves are c = 1, c2 = 2, s = 0: the resident tree is possible
    (p = 0 -> s = 0, p = 0 -> v = 1 -> c = 1, c2 = 2), after the move (v, c, s) the leaf s = 0
    hangs below v = 1, which cannot reach it under either set."""
    case, ta = revival_case(n)
    st = case.data.copy()
    st[0] = [1, 2, 0, 1]
    lik = case.obs_lik.copy()
    lik[0] = 0.0
    lik[0, np.arange(4), st[0]] = 1.0
    Q = np.stack([case.Q[0], 1.5 * case.Q[0]])
    return case._replace(data=st, obs_lik=lik, Q=Q), ta
