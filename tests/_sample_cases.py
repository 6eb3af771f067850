"""What the tests of rt_sites_sample_states share (test_sample_states_cpu.py,
test_sample_states_gpu.py): the replay check, a numpy sampler that follows the rule pinned in
include/raoteh_hip.h, the law check against the oracle's posteriors and the cases."""
import networkx as nx
import numpy as np

from oracle import oracle_numpy as orc
from raoteh_amd import synth
from raoteh_amd._philox import philox_uniform

# the relative tolerance at which the device's posterior passes are held to the oracle
# (RTOL of test_posteriors_gpu.py)
EPS = 1e-10
NO_STATE = 255

# the law case: shapes and seed shared by the CPU test (numpy sampler) and the GPU test
LAW_NNODES, LAW_SITES, LAW_DRAWS, LAW_SEED = 14, 2, 8192, 20240


class ReplayError(AssertionError):
    pass


def weights_of(v, parent_state, P, L, root_w, n):
    """w f64[..., n] of node v (preorder) for the sites' L[..., v, :] given the parents' states."""
    if v == 0:
        w = L[..., 0, :] * (np.ones(n) if root_w is None else root_w)
    else:
        w = P[v][parent_state] * L[..., v, :]
    return np.where(w > 0, w, 0.0)


def replay_check(states, status, P, L, root_w, parent, seed, first_draw=0, eps=EPS):
    """Every node of every draw of every site, conditional on the pick at the parent: the picked
    state b has w[b] > 0 and cdf[b-1] - eps total <= u total <= cdf[b] + eps total, with
    P f64[N, n, n], L f64[nsites, N, n] (the oracle's), u from _philox.  Zero-likelihood sites:
    status 1 and every byte 255.  Returns the number of picks checked."""
    states = np.asarray(states)
    ndraws, nsites, N = states.shape
    n = P.shape[1]
    if L.shape != (nsites, N, n):
        raise ReplayError('shape of L')
    w0 = weights_of(0, None, P, L, root_w, n)
    tot0 = w0.sum(axis=1)
    live = (tot0 > 0) & np.isfinite(tot0)
    want_status = np.where(live, 0, 1)
    if not np.array_equal(np.asarray(status), want_status):
        raise ReplayError('status %r, expected %r' % (np.asarray(status).tolist(),
                                                      want_status.tolist()))
    if not (states[:, ~live, :] == NO_STATE).all():
        raise ReplayError('a zero-likelihood site has a state')
    sites = np.nonzero(live)[0]
    if not len(sites):
        return 0
    st = states[:, sites, :].astype(np.int64)                      # [ndraws, live, N]
    Ls = L[sites]
    draws = np.arange(first_draw, first_draw + ndraws, dtype=np.uint64)
    checked = 0
    for v in range(N):
        b = st[:, :, v]
        if (b >= n).any():
            raise ReplayError('node %d: state out of range' % v)
        w = weights_of(v, None if v == 0 else st[:, :, parent[v]], P, Ls[None], root_w, n)
        w = np.broadcast_to(w, (ndraws, len(sites), n))
        cdf = np.cumsum(w, axis=2)
        total = cdf[:, :, -1]
        wb = np.take_along_axis(w, b[:, :, None], axis=2)[:, :, 0]
        hi = np.take_along_axis(cdf, b[:, :, None], axis=2)[:, :, 0]
        lo = hi - wb
        index = sites.astype(np.uint64)[None, :] * np.uint64(N) + np.uint64(v)
        target = philox_uniform(seed, draws[:, None], index) * total
        bad = ~(wb > 0) | (target < lo - eps * total) | (target > hi + eps * total)
        if bad.any():
            d, i = np.argwhere(bad)[0]
            raise ReplayError('node %d, draw %d, site %d: state %d with w = %r, target %r outside '
                              '[%r, %r] (%d of %d picks of the node fail)'
                              % (v, d, sites[i], b[d, i], wb[d, i], target[d, i], lo[d, i],
                                 hi[d, i], bad.sum(), bad.size))
        checked += bad.size
    return checked


def numpy_sample(P, L, root_w, parent, seed, first_draw, ndraws):
    """The rule of rt_sites_sample_states in numpy: (states uint8[ndraws, nsites, N], status)."""
    nsites, N, n = L.shape
    states = np.full((ndraws, nsites, N), NO_STATE, dtype=np.uint8)
    status = np.zeros(nsites, dtype=np.int32)
    draws = np.arange(first_draw, first_draw + ndraws, dtype=np.uint64)
    for i in range(nsites):
        for v in range(N):
            if v == 0:
                w = np.broadcast_to(weights_of(0, None, P, L[i], root_w, n), (ndraws, n))
                ok = np.ones(ndraws, dtype=bool)
            else:
                a = states[:, i, parent[v]].astype(np.int64)
                ok = a != NO_STATE
                w = weights_of(v, np.where(ok, a, 0), P, L[i], root_w, n)
            cdf = np.cumsum(w, axis=1)
            total = cdf[:, -1]
            if v == 0 and not (total[0] > 0 and np.isfinite(total[0])):
                status[i] |= 1
                break
            u = philox_uniform(seed, draws, np.uint64(i * N + v))
            target = u * total
            positive = w > 0
            hit = positive & (cdf > target[:, None])
            first = np.argmax(hit, axis=1)
            last = n - 1 - np.argmax(positive[:, ::-1], axis=1)
            pick = np.where(hit.any(axis=1), first, last)
            none = ok & ~positive.any(axis=1)
            if none.any():
                status[i] |= 2
            states[:, i, v] = np.where(ok & positive.any(axis=1), pick, NO_STATE)
    return states, status


def law_deviation(states, D, J, parent):
    """Of one site: the largest (|frequency - probability| - 5 sigma - 1e-9) over the cells of
    the node marginals D [N, n] and the joint endpoint laws J [N, n, n] (negative: inside)."""
    states = np.asarray(states).astype(np.int64)                   # [ndraws, N]
    ndraws, N = states.shape
    n = D.shape[1]
    worst = -np.inf
    for v in range(N):
        f = np.bincount(states[:, v], minlength=n)[:n] / ndraws
        sig = np.sqrt(np.clip(D[v] * (1 - D[v]), 0, None) / ndraws)
        worst = max(worst, (np.abs(f - D[v]) - 5 * sig - 1e-9).max())
        if v:
            pair = states[:, parent[v]] * n + states[:, v]
            f = (np.bincount(pair, minlength=n * n)[:n * n] / ndraws).reshape(n, n)
            sig = np.sqrt(np.clip(J[v] * (1 - J[v]), 0, None) / ndraws)
            worst = max(worst, (np.abs(f - J[v]) - 5 * sig - 1e-9).max())
    return worst


def law_edge_sets(n):
    """Eight (A, B) joint endpoint sets: the halves against each other, a few single cells."""
    h = n // 2
    lo, hi, every = list(range(h)), list(range(h, n)), list(range(n))
    return [(lo, lo), (lo, hi), (hi, lo), (hi, hi), ([0], [0]), ([0], [1]), ([1], [0]),
            ([n - 1], every)]


def law_set_deviation(states, marginals, edge_values, esets, parent):
    """As law_deviation, over the node marginals [N, n] and the sums edge_values [N, len(esets)]
    of the joint endpoint law over the sets (what TreeModel.posteriors returns for a site)."""
    states = np.asarray(states).astype(np.int64)
    ndraws, N = states.shape
    n = marginals.shape[1]
    worst = -np.inf
    for v in range(N):
        p = marginals[v]
        f = np.bincount(states[:, v], minlength=n)[:n] / ndraws
        sig = np.sqrt(np.clip(p * (1 - p), 0, None) / ndraws)
        worst = max(worst, (np.abs(f - p) - 5 * sig - 1e-9).max())
        if v:
            a, b = states[:, parent[v]], states[:, v]
            for k, (A, B) in enumerate(esets):
                p = edge_values[v, k]
                f = (np.isin(a, A) & np.isin(b, B)).mean()
                worst = max(worst, abs(f - p) - 5 * np.sqrt(max(p * (1 - p), 0) / ndraws) - 1e-9)
    return worst


def rate_matrix(n, rng):
    R = rng.uniform(0.1, 1.0, (n, n)) * (rng.uniform(size=(n, n)) < 0.7)
    np.fill_diagonal(R, 0.0)
    R[np.arange(n), (np.arange(n) + 1) % n] += 0.3                 # irreducible
    return R - np.diag(R.sum(axis=1))


def random_case(n, seed, nnodes=14, per_edge=False):
    """(T, root, leaves, Q, root_distn, rng): random_model of test_posteriors_gpu.py."""
    rng = np.random.RandomState(seed)
    T, root, leaves = synth.random_tree(nnodes, seed=seed, max_children=3)
    Q = rate_matrix(n, rng)
    if per_edge:
        for na, nb in nx.bfs_edges(T, root):
            if rng.uniform() < 0.5:
                T[na][nb]['Q'] = rate_matrix(n, rng)
    root_distn = rng.uniform(0.1, 1.0, n)
    root_distn /= root_distn.sum()
    return T, root, leaves, Q, root_distn, rng


def state_observations(n, nsites, nobs, rng, unobserved=0.1):
    """(uint8[nsites, nobs] with some 255, the same as likelihoods f64[nsites, nobs, n])."""
    st = rng.randint(0, n, size=(nsites, nobs))
    st[rng.uniform(size=st.shape) < unobserved] = NO_STATE
    lik = np.ones((nsites, nobs, n))
    obs = st != NO_STATE
    lik[obs] = np.eye(n)[st[obs]]
    return st.astype(np.uint8), lik


def mask_observations(n, nsites, nobs, rng):
    bits = rng.uniform(size=(nsites, nobs, n)) < 0.4
    bits[:, :, 0] |= ~bits.any(axis=2)
    words = np.zeros((nsites, nobs, 2), dtype=np.uint64)
    for s in range(n):
        words[:, :, s >> 6] |= bits[:, :, s].astype(np.uint64) << np.uint64(s & 63)
    data = words[:, :, 0].copy() if n <= 64 else words
    return data, bits.astype(np.float64)


def dense_observations(n, nsites, nobs, rng):
    lik = rng.uniform(0.0, 1.0, size=(nsites, nobs, n))
    lik[rng.uniform(size=lik.shape) < 0.2] = 0.0
    lik[-1, 0] = 0.0                           # a site of likelihood zero
    return lik, lik


def tree_arrays(T, root, n, Q):
    """(preorder, indices, indptr, esd of the oracle's expm, parent int[N])."""
    pre, idx, ptr, esd = orc.get_expm_augmented_transitions(T, root, n, Q_default=Q)
    parent = np.full(len(pre), -1, dtype=np.int64)
    for v in range(len(pre)):
        parent[idx[ptr[v]:ptr[v + 1]]] = v
    return pre, idx, ptr, esd, parent


def law_case(n):
    """The case of the law tests: a 14-node random tree, state observations at its leaves."""
    T, root, leaves, Q, rd, rng = random_case(n, seed=900 + n, nnodes=LAW_NNODES)
    data, lik = state_observations(n, LAW_SITES, len(leaves), rng, unobserved=0.0)
    return T, root, leaves, Q, rd, data, lik


def broom_tree(nnodes, nleaves=64, seed=0):
    """A balanced binary crown of `nleaves` leaves whose leaves are drawn out into unary chains
    until the tree has `nnodes` nodes: many nodes, few leaves, so the likelihood of observed
    leaf states stays far above the smallest f64 (64 factors instead of 2048)."""
    T, root, tips = synth.balanced_tree(nleaves, seed=seed)
    rng = np.random.RandomState(seed + 1)
    tips = list(tips)
    nxt = max(T) + 1
    k = 0
    while len(T) < nnodes:
        T.add_edge(tips[k], nxt, weight=0.02 + 0.05 * rng.uniform())
        tips[k] = nxt
        nxt += 1
        k = (k + 1) % len(tips)
    return T, root, tips
