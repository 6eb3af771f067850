"""What the tests of rt_sites_map_states share (test_map_states_cpu.py, test_map_states_gpu.py):
the max-times recursion pinned in include/raoteh_hip.h in numpy, the log-probability of a given
assignment, an enumeration of every assignment of a small tree, and the cases.  numpy only.

Arrays: P f64[N, n, n] keyed by the child's preorder index (P[0] unused), obs f64[nsites, N, n]
the observation vector of every node (ones where unobserved), w f64[n] the root weights or None,
parent int[N] in preorder (-1 at the root)."""
import itertools

import numpy as np

from raoteh_amd import synth
from raoteh_amd._tree import TreeArrays
import _sample_cases as sc

NO_STATE = 255
# the state counts of the exact cases on the device: both lane sizes' ends, one and several row
# tiles, the 64/65 and 128 edges
EXACT_N = [2, 3, 4, 5, 16, 17, 20, 61, 64, 65, 122, 128]
EXACT_SITES = 33                               # two full tiles and one lane of a third


def _factor(x):
    """Negative or NaN factors count as 0."""
    x = np.asarray(x, dtype=np.float64)
    return np.where(x > 0, x, 0.0)


def map_reference(P, obs, w, parent, scale=True):
    """(states uint8[nsites, N], log_joint f64[nsites], tied int[nsites]): the recursion
    L_v(b) = o_v(b) prod_c M_c(b), M_c(a) = max_b P_c(a, b) L_c(b) in f64, every L_v scaled per
    site by a power of two (np.frexp / np.ldexp; scale=False: not at all), then the walk in
    preorder with np.argmax, which picks the first maximum: the tie rule.  tied counts the
    decisions of a site at which more than one state attains the maximum.  A site whose maximum
    is not positive and finite: states 255, log_joint -inf."""
    obs = _factor(obs)
    P = _factor(P)
    nsites, N, n = obs.shape
    L = obs.copy()
    E = np.zeros(nsites, dtype=np.int64)
    with np.errstate(under='ignore', over='ignore', invalid='ignore'):
        for v in range(N - 1, -1, -1):
            if scale:
                mx = L[:, v].max(axis=1)
                ok = (mx > 0) & np.isfinite(mx)
                e = np.where(ok, np.frexp(np.where(ok, mx, 1.0))[1], 0).astype(np.int64)
                L[:, v] = np.ldexp(L[:, v], (-e)[:, None].astype(np.int32))
                E += e
            if v == 0:
                break
            M = (P[v][None, :, :] * L[:, v][:, None, :]).max(axis=2)
            L[:, parent[v]] *= M
        wv = np.ones(n) if w is None else _factor(w)
        r = wv[None, :] * L[:, 0]
        best = r.max(axis=1)
        live = (best > 0) & np.isfinite(best)
        states = np.full((nsites, N), NO_STATE, dtype=np.uint8)
        tied = np.zeros(nsites, dtype=np.int64)
        log_joint = np.full(nsites, -np.inf)
        log_joint[live] = np.log(best[live]) + E[live] * np.log(2.0)
        states[live, 0] = np.argmax(r[live], axis=1)
        tied[live] += (r[live] == best[live, None]).sum(axis=1) > 1
        idx = np.nonzero(live)[0]
        for v in range(1, N):
            a = states[idx, parent[v]].astype(np.int64)
            r = P[v][a] * L[idx, v]
            top = r.max(axis=1)
            states[idx, v] = np.argmax(r, axis=1)
            tied[idx] += (r == top[:, None]).sum(axis=1) > 1
    return states, log_joint, tied


def joint_log(P, obs, w, parent, states):
    """f64[nsites]: the sum of the logs of the factors of J(states); a zero factor (or a node
    without a state) gives -inf."""
    obs = _factor(obs)
    P = _factor(P)
    states = np.asarray(states)
    nsites, N, n = obs.shape
    wv = np.ones(n) if w is None else _factor(w)
    x = states.astype(np.int64)
    none = (x >= n).any(axis=1)
    x = np.where(x >= n, 0, x)
    rows = np.arange(nsites)
    with np.errstate(divide='ignore'):
        total = np.log(wv[x[:, 0]])
        for v in range(N):
            total = total + np.log(obs[rows, v, x[:, v]])
            if v:
                total = total + np.log(P[v][x[:, parent[v]], x[:, v]])
    total[none] = -np.inf
    return total


def brute_force(P, obs, w, parent):
    """Every assignment of a small tree: (log of the maximum f64[nsites], the first assignment in
    lexicographic order that attains it uint8[nsites, N], unique bool[nsites])."""
    obs = _factor(obs)
    P = _factor(P)
    nsites, N, n = obs.shape
    wv = np.ones(n) if w is None else _factor(w)
    x = np.array(list(itertools.product(range(n), repeat=N)), dtype=np.int64)      # [n^N, N]
    edge = np.ones(len(x))
    for v in range(1, N):
        edge = edge * P[v][x[:, parent[v]], x[:, v]]
    edge = edge * wv[x[:, 0]]
    best = np.zeros(nsites)
    states = np.full((nsites, N), NO_STATE, dtype=np.uint8)
    unique = np.zeros(nsites, dtype=bool)
    for i in range(nsites):
        J = edge.copy()
        for v in range(N):
            J = J * obs[i, v, x[:, v]]
        k = int(np.argmax(J))
        best[i] = J[k]
        if J[k] > 0:
            states[i] = x[k]
            unique[i] = (J == J[k]).sum() == 1
    with np.errstate(divide='ignore'):
        return np.log(best), states, unique


def full_observations(ta, obs_nodes, lik, n):
    """f64[nsites, N, n]: lik f64[nsites, len(obs_nodes), n] at the observed nodes' preorder
    columns, ones elsewhere."""
    lik = np.asarray(lik, dtype=np.float64)
    obs = np.ones((lik.shape[0], ta.nnodes, n))
    for k, v in enumerate(obs_nodes):
        obs[:, ta.node_to_index[v]] = lik[:, k]
    return obs


class Case(object):
    pass


# seeds of dyadic_case, per state count: test_map_states_cpu.py holds each to "no dead site, at
# least 5 of the 33 sites with a tied decision"
DYADIC_SEED = dict((n, 500 + n) for n in EXACT_N)


def dyadic_case(n, seed=None):
    """An exact case: a 14-node tree, every entry of every P_v a power of two 2^-k, k in 0..6
    (for n > 4 each entry zeroed with probability 0.2), root weights 2^-k, k in 0..3, 33 dense
    sites whose leaf vectors hold 2^-k, k in 0..4, each entry kept with probability 0.6 and one
    random entry per leaf always.  Every product of such numbers is exact in f64, so the
    reference's states are the only correct answer, ties included, whatever the order of the
    multiplications."""
    seed = DYADIC_SEED[n] if seed is None else seed
    rng = np.random.RandomState(seed)
    c = Case()
    c.n = n
    c.T, c.root, c.leaves = synth.random_tree(14, seed, max_children=3)
    c.ta = TreeArrays(c.T, c.root)
    N = c.ta.nnodes
    c.parent = c.ta.parent
    c.P = np.ldexp(1.0, -rng.randint(0, 7, size=(N, n, n)))
    if n > 4:
        c.P[rng.uniform(size=c.P.shape) < 0.2] = 0.0
    c.P[0] = 0.0
    c.w = np.ldexp(1.0, -rng.randint(0, 4, size=n))
    nl = len(c.leaves)
    lik = np.ldexp(1.0, -rng.randint(0, 5, size=(EXACT_SITES, nl, n)))
    keep = rng.uniform(size=lik.shape) < 0.6
    one = rng.randint(0, n, size=(EXACT_SITES, nl))
    keep[np.arange(EXACT_SITES)[:, None], np.arange(nl)[None, :], one] = True
    c.dense = np.where(keep, lik, 0.0)
    c.obs = full_observations(c.ta, c.leaves, c.dense, n)
    return c


def small_case(n, seed):
    """The enumeration case: a 7-node tree, 20 dense sites with zeros (T, root, leaves, Q,
    root_distn, dense)."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=seed, nnodes=7)
    lik = rng.uniform(0.0, 1.0, size=(20, len(leaves), n))
    lik[rng.uniform(size=lik.shape) < 0.3] = 0.0
    lik[np.arange(20)[:, None], np.arange(len(leaves))[None, :],
        rng.randint(0, n, size=(20, len(leaves)))] += 0.1
    return T, root, leaves, Q, rd, lik


def long_case(n):
    """The scaling case: broom_tree(1500, nleaves=4) with every edge weight redrawn uniformly
    from 0.5..1.0, 17 sites of state observations at the tips (T, root, tips, Q, root_distn,
    data uint8, lik)."""
    T, root, tips = sc.broom_tree(1500, nleaves=4)
    rng = np.random.RandomState(1500 + n)
    for a, b in sorted(T.edges()):
        T[a][b]['weight'] = rng.uniform(0.5, 1.0)
    Q = sc.rate_matrix(n, rng)
    rd = rng.uniform(0.1, 1.0, n)
    data, lik = sc.state_observations(n, 17, len(tips), rng, unobserved=0.0)
    return T, root, tips, Q, rd, data, lik


def tolerance(nnodes, value):
    """The rounding of F = 2 nnodes multiplications on each side: 8 F 2^-53 max(1, |value|)."""
    return 8.0 * (2 * nnodes) * 2.0 ** -53 * np.maximum(1.0, np.abs(value))
