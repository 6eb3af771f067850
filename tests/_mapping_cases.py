"""What the tests of rt_sites_sample_mappings share (test_sample_mappings_cpu.py,
test_sample_mappings_gpu.py): a numpy mirror of the branch rule pinned in include/raoteh_hip.h,
conditional on given node states and vectorised over draws and sites, the exact expectation the
law tests aim at, and the cases (shapes and seeds) of the GPU parity tests, so that the CPU test
can hold every one of them to the margin condition."""
import numpy as np
import scipy.linalg

from _posterior_cases import oracle_pmaps
import _sample_cases as sc
from raoteh_amd._philox import philox_uniform
from raoteh_amd._tree import TreeArrays

NO_STATE = 255
MAX_EVENTS = 512
BRANCH_STREAM = 1 << 63
# a pick may differ between two correct evaluations of the rule only if its target lies within
# rounding of a cell boundary; the parity tests demand exact counts where every target keeps this
# relative distance (the sums differ by a few hundred ulps at most: K * n terms of 1.1e-16)
MARGIN = 1e-9

# the state counts of the GPU parity tests: the lane kernel (2..4), every tile count's edge
PARITY_NS = [2, 3, 4, 5, 16, 17, 20, 61, 64, 65, 122, 128]
PARITY_SITES, PARITY_DRAWS, PARITY_FIRST = 33, 3, 2 ** 40 + 5


def edge_constants(Q, t, node_q, v):
    """(mu, R, lam, K_v, pois f64[K_v + 1]) of the edge above node v."""
    Qv = Q[node_q[v]]
    mu = float(max((-np.diag(Qv)).max(), 0.0))
    n = Qv.shape[0]
    R = np.eye(n) + Qv / mu if mu > 0 else np.eye(n)
    lam = mu * float(t[v])
    if not lam > 0:
        lam = 0.0
    K = int(np.ceil(lam + 10.0 * np.sqrt(lam) + 20.0))
    pois = np.zeros(K + 1)
    pois[0] = np.exp(-lam) if lam > 0 else 1.0
    for k in range(1, K + 1):
        pois[k] = pois[k - 1] * lam / k if lam > 0 else 0.0
    return mu, R, lam, K, pois


def powers(R, K):
    out = np.empty((K + 1,) + R.shape)
    out[0] = np.eye(R.shape[0])
    for m in range(1, K + 1):
        out[m] = out[m - 1] @ R
    return out


def pick(w, u):
    """The pick rule over the last axis of w (not negative): (index, or -1 where no weight is
    positive; relative distance of the target u * total to the nearer boundary of the picked cell
    that it shares with another cell of positive weight, inf without such a boundary)."""
    positive = w > 0
    cum = np.cumsum(w, axis=-1)
    total = cum[..., -1]
    target = u * total
    hit = positive & (cum > target[..., None])
    first = np.argmax(hit, axis=-1)
    last = w.shape[-1] - 1 - np.argmax(positive[..., ::-1], axis=-1)
    some = positive.any(axis=-1)
    idx = np.where(hit.any(axis=-1), first, last)
    hi = np.take_along_axis(cum, idx[..., None], axis=-1)[..., 0]
    lo = hi - np.take_along_axis(w, idx[..., None], axis=-1)[..., 0]
    safe = np.where(total > 0, total, 1.0)
    below = (np.cumsum(positive, axis=-1) - positive)                 # positive cells before
    has_below = np.take_along_axis(below, idx[..., None], axis=-1)[..., 0] > 0
    has_above = idx < last
    margin = np.minimum(np.where(has_below, (target - lo) / safe, np.inf),
                        np.where(has_above, (hi - target) / safe, np.inf))
    margin = np.where(some, np.abs(margin), np.inf)
    return np.where(some, idx, -1), margin


def numpy_mappings(Q, t, node_q, parent, states, coefs, seed, first_draw):
    """The branch rule of rt_sites_sample_mappings for the node states uint8[ndraws, nsites, N]:
    dict(values f64[ndraws, nsites, N, K], counts int32[ndraws, nsites, N, 2], status int32[nsites]
    (bit 4 only), margin: the smallest pick margin, picks: how many picks it is over)."""
    states = np.asarray(states)
    D, S, N = states.shape
    E = np.asarray(coefs, dtype=float)
    E = E[None] if E.ndim == 2 else E
    nk, n = E.shape[0], E.shape[1]
    Ediag = np.einsum('kcc->kc', E)
    values = np.zeros((D, S, N, nk))
    counts = np.zeros((D, S, N, 2), dtype=np.int32)
    status = np.zeros(S, dtype=np.int32)
    draws = (np.arange(D, dtype=np.uint64) + np.uint64(first_draw % (1 << 64)))[:, None]
    margin, picks = np.inf, 0
    pw_cache = {}
    need_K = {}
    for v in range(1, N):
        K = edge_constants(Q, t, node_q, v)[3]
        need_K[node_q[v]] = max(need_K.get(node_q[v], 1), K)
    for v in range(1, N):
        mu, R, lam, K, pois = edge_constants(Q, t, node_q, v)
        if K > MAX_EVENTS:
            raise ValueError('K_v = %d' % K)
        q = node_q[v]
        if q not in pw_cache:
            pw_cache[q] = powers(R, need_K[q])
        PW = pw_cache[q]
        a = states[:, :, parent[v]].astype(np.int64)
        b = states[:, :, v].astype(np.int64)
        live = (a != NO_STATE) & (b != NO_STATE)
        a, b = np.where(live, a, 0), np.where(live, b, 0)
        base = np.uint64(BRANCH_STREAM) + (np.arange(S, dtype=np.uint64) * np.uint64(N)
                                           + np.uint64(v)) * np.uint64(2048)

        def ub(j, base=base):
            return philox_uniform(seed, draws, (base + np.uint64(j))[None, :])

        # 1. the event count
        w = pois[None, None, :] * np.moveaxis(PW[:K + 1, a, b], 0, -1)
        w = np.where(w > 0, w, 0.0)
        total = w.sum(axis=-1)
        bad = live & ~((total > 0) & np.isfinite(total))
        status[bad.any(axis=0)] |= 4
        live = live & ~bad
        kev, mg = pick(w, ub(0))
        kev = np.where(live, kev, 0)
        if live.any():
            margin = min(margin, mg[live].min())
            picks += int(live.sum())
        # 2., 3. the path and the dwell times
        x = a.copy()
        sum_e = np.zeros((D, S))
        dw = np.zeros((D, S, nk))
        jm = np.zeros((D, S, nk))
        changes = np.zeros((D, S), dtype=np.int64)
        kmax = int(kev.max())
        for l in range(kmax + 1):
            act = live & (l <= kev)
            e = -np.log1p(-ub(1024 + l))
            sum_e += np.where(act, e, 0.0)
            dw += np.where(act[..., None], Ediag.T[x] * e[..., None], 0.0)
            if l == kmax:
                break
            nx = b.copy()
            need = act & (l + 1 < kev)
            if need.any():
                xs, bs, ms = x[need], b[need], kev[need] - (l + 1)
                ww = R[xs, :] * PW[ms, :, bs]
                ww = np.where(ww > 0, ww, 0.0)
                pk, mg = pick(ww, ub(l + 1)[need])
                margin = min(margin, mg.min())
                picks += len(pk)
                nx[need] = np.where(pk >= 0, pk, bs)
            step = act & (l < kev)
            jump = step & (nx != x)
            jm += np.where(jump[..., None], np.moveaxis(E[:, x, nx], 0, -1), 0.0)
            changes += jump
            x = np.where(step, nx, x)
        ok = sum_e > 0
        sc_ = np.where(ok, float(t[v]) / np.where(ok, sum_e, 1.0), 0.0)
        val = np.where(ok[..., None], dw * sc_[..., None], Ediag.T[a] * float(t[v])) + jm
        values[:, :, v] = np.where(live[..., None], val, 0.0)
        counts[:, :, v, 0] = np.where(live, kev, 0)
        counts[:, :, v, 1] = np.where(live, changes, 0)
    return dict(values=values, counts=counts, status=status, margin=margin, picks=picks)


def exact_expectations(Q, t, node_q, esd, J, coefs):
    """sum_ab J_v[a][b] G_v[a][b] / P_v[a][b] per node and coefficient matrix, f64[N, K], with
    G_v the upper right block of expm([[t Q, t C], [0, t Q]]), C = E * Q off the diagonal and E on
    it; J f64[N, n, n] the joint endpoint law of one site, esd the transition matrices."""
    E = np.asarray(coefs, dtype=float)
    N, n = esd.shape[0], esd.shape[1]
    out = np.zeros((N, len(E)))
    for v in range(1, N):
        Qv, tv = Q[node_q[v]], float(t[v])
        for k in range(len(E)):
            C = E[k] * Qv
            np.fill_diagonal(C, np.diag(E[k]))
            B = np.zeros((2 * n, 2 * n))
            B[:n, :n] = B[n:, n:] = tv * Qv
            B[:n, n:] = tv * C
            G = scipy.linalg.expm(B)[:n, n:]
            livecells = J[v] != 0
            out[v, k] = (J[v][livecells] * G[livecells] / esd[v][livecells]).sum()
    return out


def host_model(T, root, n, Q_default):
    """(TreeArrays, Q f64[nq, n, n], node_q, t, esd of scipy's expm) of a tree on the host."""
    ta = TreeArrays(T, root)
    Q, node_q = ta.rate_matrices(n, Q_default)
    t = ta.branch_lengths()
    esd = np.zeros((ta.nnodes, n, n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * Q[node_q[v]])
    return ta, Q, node_q, t, esd


def host_states(ta, esd, rd, leaves, lik, seed, first_draw, ndraws):
    """Node states of the numpy sampler of _sample_cases on the oracle's L."""
    L = oracle_pmaps(ta.indices, ta.indptr, esd, [ta.node_to_index[v] for v in leaves], lik)
    states, status = sc.numpy_sample(esd, L, rd, ta.parent, seed, first_draw, ndraws)
    return states, status, L


def parity_coefs(n, seed):
    """Two random matrices in [-1, 1] and the identity."""
    rng = np.random.RandomState(seed)
    return np.array([rng.uniform(-1, 1, (n, n)), rng.uniform(-1, 1, (n, n)), np.eye(n)])


def parity_case(n):
    """The mirror-parity case at n states: (T, root, leaves, Q, rd, data, lik, seed)."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=40 + n, nnodes=14)
    data, lik = sc.state_observations(n, PARITY_SITES, len(leaves), rng)
    return T, root, leaves, Q, rd, data, lik, 1000 + n


def per_edge_case(n):
    """Per-edge rate matrices on a 16-node tree, and the matrices of the second set_rates."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=7 + n, nnodes=16, per_edge=True)
    data, lik = sc.state_observations(n, 21, len(leaves), rng)
    return T, root, leaves, Q, rd, data, lik, 300 + n


def second_rates(Q, seed):
    """Other rate matrices of the same shapes (the stale-table check)."""
    rng = np.random.RandomState(seed)
    return np.array([sc.rate_matrix(Q.shape[1], rng) * 1.7 for _ in range(Q.shape[0])])


def length_case(n):
    """One branch with lam near 40, one of length 0 in a 14-node tree: (.., t, seed) with t the
    branch lengths to hand to set_rates."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=500 + n, nnodes=14)
    data, lik = sc.state_observations(n, 21, len(leaves), rng)
    ta = TreeArrays(T, root)
    t = ta.branch_lengths()
    mu = (-np.diag(Q)).max()
    internal = [v for v in range(1, ta.nnodes) if ta.indptr[v + 1] > ta.indptr[v]]
    t[internal[0]] = 40.0 / mu
    t[internal[-1] if len(internal) > 1 else ta.nnodes - 1] = 0.0
    assert (t == 0).sum() == 2 and internal[0] != internal[-1]
    return T, root, leaves, Q, rd, data, lik, t, 700 + n


def kinds_case(kind, n):
    """Unobserved leaves, an observed internal node and (dense) a site of likelihood zero:
    (T, root, obs_nodes, Q, rd, data, lik); 3 draws with seed 9."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=7 * n + len(kind), nnodes=14)
    internal = [v for v in T if v != root and v not in leaves][0]
    obs_nodes = list(leaves) + [internal]
    make = dict(state=sc.state_observations, mask=sc.mask_observations,
                dense=sc.dense_observations)[kind]
    data, lik = make(n, 21, len(obs_nodes), rng)
    return T, root, obs_nodes, Q, rd, data, lik


def split_case(nnodes):
    """The tree of the draw-block test, n = 7: seed 3, first draw 7."""
    n = 7
    T, root, leaves = sc.broom_tree(nnodes, nleaves=4, seed=nnodes)
    rng = np.random.RandomState(nnodes)
    Q = sc.rate_matrix(n, rng)
    rd = rng.uniform(0.1, 1.0, n)
    data, lik = sc.state_observations(n, 17, len(leaves), rng)
    return T, root, leaves, Q, rd, data, lik
