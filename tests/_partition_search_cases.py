"""Host reference of rt_sites_branch_profiles_partitioned and rt_sites_nni_scores_partitioned
(test_partition_search_cpu.py, test_partition_search_gpu.py) -- never a device path.  Per rate set
k, over that set's sites: the resident matrices are scipy.linalg.expm(t[k][v] Q[k][node_q[v]]),
the trial grid is factors * t[k], and _profile_cases.profile_from_transitions /
_nni_cases.nni_from_transitions (the oracle's pruning, whole-tree evaluations) give the values; they
are scattered to caller order, set_sums and sums are taken in numpy.  The cases are
_partition_cases.make_case's; brute_* evaluate a likelihood by summing over every assignment of
states to the internal nodes, for the CPU test of this reference."""
import collections
import functools
import itertools

import numpy as np
import scipy.linalg

import _nni_cases as nc
import _partition_cases as pc
import _profile_cases as pfc

Reference = collections.namedtuple('Reference', 'values status set_sums sums loglik moves')


def tree_arrays(case):
    from raoteh_amd import _tree
    return _tree.TreeArrays(case.T, case.root)


def make_factors(nnodes, npoints, seed):
    """[nnodes, npoints] factors, row 0 zero: 1 (the resident length) from two points on, 0 (the
    edge collapsed, P = I) from three points on, the rest log-uniform in [1/4, 4]; every branch's
    row scaled by a draw of its own in [0.8, 1.25] except at the factors 0 and 1."""
    rng = np.random.RandomState(seed)
    f = np.exp(rng.uniform(-np.log(4), np.log(4), npoints))
    grid = np.repeat(f[None, :], nnodes, axis=0)
    grid = grid * np.exp(rng.uniform(-np.log(1.25), np.log(1.25), nnodes))[:, None]
    if npoints >= 2:
        grid[:, npoints - 1] = 1.0
    if npoints >= 3:
        grid[:, 1] = 0.0
    grid[0] = 0.0
    return np.ascontiguousarray(grid)


def device_factors(factors, nnodes):
    """A 1-D sequence of factors as the [nnodes, G] array the call evaluates (row 0 zero)."""
    grid = np.repeat(np.asarray(factors, dtype=float)[None, :], nnodes, axis=0)
    grid[0] = 0.0
    return np.ascontiguousarray(grid)


def site_weights(nsites, seed):
    """Small integer weights with zeros in them."""
    w = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(float)
    w[[1, 2, nsites // 2, nsites - 1]] = 0.0
    return w


def set_transitions(ta, case, k):
    esd = np.zeros((ta.nnodes, case.n, case.n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(case.t[k, v] * case.Q[k, case.node_q[v]])
    return esd


def _cols(ta, case):
    return [ta.node_to_index[v] for v in case.leaves]


def _sums(case, values, status, weights, nan_rows):
    """set_sums [nsets, R, G] and sums [R, G]: w_i values over the live sites of non-zero weight of
    every set; nan_rows [nsets, R]: rows that are NaN for a set with a site."""
    S = len(case.site_sets)
    w = np.ones(S) if weights is None else np.asarray(weights, dtype=float)
    set_sums = np.zeros((case.nsets,) + values.shape[1:])
    for k in range(case.nsets):
        mine = case.site_sets == k
        use = mine & (w != 0) & (status == 0)
        if use.any():
            set_sums[k] = np.einsum('i,irg->rg', w[use], values[use])
        if mine.any():
            set_sums[k][nan_rows[k]] = np.nan
    return set_sums, set_sums.sum(axis=0)


def profile_reference(ta, case, factors, weights=None):
    """Reference of rt_sites_branch_profiles_partitioned: values [S, N, G] in caller order."""
    S, N, G = len(case.site_sets), ta.nnodes, factors.shape[1]
    values = np.zeros((S, N, G))
    status = np.zeros(S, dtype=np.int32)
    loglik = np.zeros(S)
    nan_rows = np.zeros((case.nsets, N), dtype=bool)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        nan_rows[k, 1:] = case.t[k, 1:] == 0
        if not len(mine):
            continue
        v, st, ll = pfc.profile_from_transitions(
            ta.indices, ta.indptr, set_transitions(ta, case, k), _cols(ta, case),
            case.obs_lik[mine], case.root_distn, case.Q[k], case.node_q,
            factors * case.t[k][:, None])
        v[np.ix_(st == 0, nan_rows[k])] = np.nan
        values[mine], status[mine], loglik[mine] = v, st, ll
    set_sums, sums = _sums(case, values, status, weights, nan_rows)
    return Reference(values, status, set_sums, sums, loglik, None)


def nni_reference(ta, case, factors=None, weights=None):
    """Reference of rt_sites_nni_scores_partitioned: values [S, M, G]; factors None: the plain
    swap."""
    S = len(case.site_sets)
    moves = nc.brute_moves(ta.indices, ta.indptr)
    G = 1 if factors is None else factors.shape[1]
    values = np.zeros((S, len(moves), G))
    status = np.zeros(S, dtype=np.int32)
    loglik = np.zeros(S)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        _, v, st, ll = nc.nni_from_transitions(
            ta.indices, ta.indptr, set_transitions(ta, case, k), _cols(ta, case),
            case.obs_lik[mine], case.root_distn, case.Q[k], case.node_q,
            None if factors is None else factors * case.t[k][:, None])
        values[mine], status[mine], loglik[mine] = v, st, ll
    nan_rows = np.zeros((case.nsets, len(moves)), dtype=bool)
    set_sums, sums = _sums(case, values, status, weights, nan_rows)
    return Reference(values, status, set_sums, sums, loglik, moves)


# ---- the cases of the parity tests ----------------------------------------------------------

def runs_site_sets(n, seed):
    """A random order of runs that do not end on a granule (set 3: two sites)."""
    G = pc.granule(n)
    return np.random.RandomState(seed).permutation(np.repeat([0, 1, 2, 3], [G + 6, G - 4, G + 3, 2]))


LOST_SET = 2


def plant_lost_sites(case, ta, k=LOST_SET):
    """-> (case, lost0, lost1, v): set k gets Q[k][0] = 0, so that its edges with node_q == 0 have
    P = I at every length while those with node_q == 1 keep a full rate matrix; nodes joined by
    identity edges share one state.  v is a full-rate edge with a leaf on either side among the
    nodes so joined to its ends; the two sites lost0 and lost1 of set k have state 1 at the leaves
    joined to v and state 0 at every other leaf: alive on the resident tree, and of likelihood
    exactly 0 once the edge above v is collapsed (factor 0: its ends must agree) -- -inf there,
    resting only on expm(0) = I.  Most other 'state' and 'mask' sites of set k are dead under it
    (leaves joined by identity edges disagree); the sites with one state at every leaf live."""
    import _step_multi_cases as smc
    Q = case.Q.copy()
    Q[k, 0] = 0.0
    parent = nc.parents_of(ta.indices, ta.indptr)
    comp = list(range(ta.nnodes))

    def find(x):
        while comp[x] != x:
            x = comp[x]
        return x
    for v in range(1, ta.nnodes):
        if case.node_q[v] == 0:
            comp[find(v)] = find(int(parent[v]))
    cols = _cols(ta, case)
    leaf_comps = set(find(c) for c in cols)
    edge = [v for v in range(1, ta.nnodes) if case.node_q[v] == 1 and find(v) in leaf_comps
            and find(int(parent[v])) in leaf_comps]
    assert edge, 'no full-rate edge with leaves joined to both ends: another seed'
    v = edge[0]
    states = np.array([1 if find(c) == find(v) else 0 for c in cols])
    mine = np.flatnonzero(case.site_sets == k)
    lost0, lost1 = int(mine[1]), int(mine[2])
    lik = case.obs_lik.copy()
    for i in (lost0, lost1):
        lik[i] = 0.0
        lik[i, np.arange(len(cols)), states] = 1.0
    if case.kind == 'dense':
        data = lik.copy()
    elif case.kind == 'state':
        data = case.data.copy()
        data[[lost0, lost1]] = states
    else:
        data = smc._encode_mask(case.n, lik)
        keep = np.ones(len(data), dtype=bool)
        keep[[lost0, lost1]] = False
        assert np.array_equal(data[keep], case.data[keep])
    return case._replace(Q=Q, obs_lik=lik, data=data), lost0, lost1, v


@functools.lru_cache(maxsize=None)
def cached_case(n, kind, sets, seed):
    """(case, tree arrays, (lost0, lost1, v, k) of plant_lost_sites in set k).  sets: 'empty' =
    site i in set i % 3 of 4 (set 3 empty), 'runs' = runs_site_sets, 'zero' = 'empty' with Q = 0 in
    set 1, 'two' = two sets, site i in set i % 2."""
    k = LOST_SET
    if sets == 'two':
        nsites = 3 * pc.granule(n) + 5
        case = pc.make_case(n, kind, seed, nsets=2, nsites=nsites, site_sets=np.arange(nsites) % 2)
        k = 1
    elif sets == 'runs':
        ss = runs_site_sets(n, seed)
        case = pc.make_case(n, kind, seed, nsites=len(ss), site_sets=ss)
    else:
        case = pc.make_case(n, kind, seed, zero_set=1 if sets == 'zero' else None)
    ta = tree_arrays(case)
    case, lost0, lost1, v = plant_lost_sites(case, ta, k)
    return case, ta, (lost0, lost1, v, k)


@functools.lru_cache(maxsize=None)
def cached_reference(call, n, kind, sets, seed, npoints, weighted):
    """The shared reference of a parity case (computed once; callers must not write to it):
    (case, ta, (lost0, lost1, v, k), factors or None, weights or None, Reference).  npoints 0: the
    plain swap.  With weights, lost0 has weight 0 and lost1 weight 1."""
    case, ta, special = cached_case(n, kind, sets, seed)
    w = None
    if weighted:
        w = site_weights(len(case.site_sets), seed + 2)
        w[special[0]], w[special[1]] = 0.0, 1.0
    f = None if npoints == 0 else make_factors(ta.nnodes, npoints, seed + 3)
    ref = profile_reference(ta, case, f, w) if call == 'profile' else nni_reference(ta, case, f, w)
    for a in ref[:5]:
        a.setflags(write=False)
    return case, ta, special, f, w, ref


# ---- brute force -----------------------------------------------------------------------------

def brute_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn):
    """L_i = sum over the states of every internal node of root[s_0] prod_edges P_v[s_p][s_v]
    prod_leaves obs: one term per assignment, no pruning.  obs_lik [S, leaves, n] -> [S]."""
    kids = nc.children_of(indices, indptr)
    parent = nc.parents_of(indices, indptr)
    N, n = len(kids), esd.shape[1]
    obs_of = {v: j for j, v in enumerate(cols)}
    internal = [v for v in range(N) if kids[v]]
    assert all(v not in obs_of for v in internal)
    total = np.zeros(obs_lik.shape[0])
    for states in itertools.product(range(n), repeat=len(internal)):
        s = dict(zip(internal, states))
        term = np.full(obs_lik.shape[0], root_distn[s[0]])
        for v in range(1, N):
            row = esd[v][s[parent[v]]]
            if v in s:
                term = term * row[s[v]]
            else:
                term = term * (obs_lik[:, obs_of[v]] @ row)
        total += term
    return total


def brute_profile(ta, case, k, sites, factors):
    """values [len(sites), N, G] of set k's sites `sites` by brute force."""
    esd = set_transitions(ta, case, k)
    cols = _cols(ta, case)
    obs = case.obs_lik[sites]
    base = brute_likelihoods(ta.indices, ta.indptr, esd, cols, obs, case.root_distn)
    out = np.zeros((len(sites), ta.nnodes, factors.shape[1]))
    for v in range(1, ta.nnodes):
        for g in range(factors.shape[1]):
            e = esd.copy()
            e[v] = scipy.linalg.expm(factors[v, g] * case.t[k, v] * case.Q[k, case.node_q[v]])
            with np.errstate(divide='ignore'):
                out[:, v, g] = np.log(brute_likelihoods(ta.indices, ta.indptr, e, cols, obs,
                                                        case.root_distn)) - np.log(base)
    return out


def brute_nni(ta, case, k, sites, factors=None):
    """values [len(sites), M, G] of set k's sites by brute force on every moved tree."""
    esd = set_transitions(ta, case, k)
    cols = _cols(ta, case)
    obs = case.obs_lik[sites]
    base = brute_likelihoods(ta.indices, ta.indptr, esd, cols, obs, case.root_distn)
    moves = nc.brute_moves(ta.indices, ta.indptr)
    G = 1 if factors is None else factors.shape[1]
    out = np.zeros((len(sites), len(moves), G))
    for j, (v, c, s) in enumerate(moves):
        ni, npt, old_of_new = nc.moved_arrays(ta.indices, ta.indptr, int(v), int(c), int(s))
        new_of_old = np.empty_like(old_of_new)
        new_of_old[old_of_new] = np.arange(len(old_of_new))
        for g in range(G):
            e = esd.copy()
            if factors is not None:
                e[v] = scipy.linalg.expm(factors[v, g] * case.t[k, v] * case.Q[k, case.node_q[v]])
            with np.errstate(divide='ignore'):
                out[:, j, g] = np.log(brute_likelihoods(
                    ni, npt, e[old_of_new], [int(new_of_old[x]) for x in cols], obs,
                    case.root_distn)) - np.log(base)
    return out
