"""Host reference of rt_model_nni_moves / rt_sites_nni_scores (test_nni_cpu.py, test_nni_gpu.py):
the moves by brute force, and for every move the rearranged CSR arrays and the permuted per-node
transition matrices built by hand (never through raoteh_amd._tree.nni_apply, never a device
path), the matrix of the edge above v replaced by scipy.linalg.expm(Q_v tau) for a trial length,
the per-site likelihoods recomputed with the oracle's pruning (oracle/oracle_numpy.py) and
    value = log L(moved tree, tau) - log L
taken: nmoves * G whole-tree evaluations."""
import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
from _profile_cases import _one_blas_thread


def children_of(indices, indptr):
    return [[int(c) for c in indices[indptr[v]:indptr[v + 1]]] for v in range(len(indptr) - 1)]


def parents_of(indices, indptr):
    parent = np.full(len(indptr) - 1, -1, dtype=np.int64)
    for v, kids in enumerate(children_of(indices, indptr)):
        parent[kids] = v
    return parent


def brute_moves(indices, indptr):
    """Every (v, c, s) with v not the root, c a child of v and s another child of parent(v),
    sorted by v, then by the position of c among the children of v, then by that of s among the
    children of parent(v) -- from all triples of nodes, not from a walk of the tree."""
    kids = children_of(indices, indptr)
    parent = parents_of(indices, indptr)
    N = len(kids)
    found = []
    for v in range(N):
        for c in range(N):
            for s in range(N):
                p = parent[v]
                if p >= 0 and parent[c] == v and parent[s] == p and s != v:
                    found.append((v, kids[v].index(c), kids[p].index(s), c, s))
    found.sort()
    return np.array([(v, c, s) for v, _, _, c, s in found], dtype=np.int32).reshape(-1, 3)


def moved_arrays(indices, indptr, v, c, s):
    """(indices, indptr, old_of_new) of the tree after the move: s takes the place of c among the
    children of v, c that of s among the children of parent(v); the nodes are numbered again in
    the preorder of the moved tree, old_of_new[j] the old index of its node j."""
    kids = [list(k) for k in children_of(indices, indptr)]
    p = int(parents_of(indices, indptr)[v])
    kids[v][kids[v].index(c)] = s
    kids[p][kids[p].index(s)] = c
    old_of_new, stack = [], [0]
    while stack:
        a = stack.pop()
        old_of_new.append(a)
        stack.extend(reversed(kids[a]))
    old_of_new = np.array(old_of_new, dtype=np.int64)
    assert sorted(old_of_new) == list(range(len(kids)))
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(len(kids))
    new_indices, new_indptr = [], [0]
    for a in old_of_new:
        new_indices.extend(int(new_of_old[b]) for b in kids[a])
        new_indptr.append(len(new_indices))
    return (np.array(new_indices, dtype=np.int64), np.array(new_indptr, dtype=np.int64),
            old_of_new)


def moved_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn, move):
    """(log-likelihoods, status) of the oracle on the moved tree: every node keeps the matrix of
    the edge above it and its observation."""
    ni, npt, old_of_new = moved_arrays(indices, indptr, *[int(x) for x in move])
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(len(old_of_new))
    return orc.batch_log_likelihoods(ni, npt, np.asarray(esd)[old_of_new],
                                     [int(new_of_old[k]) for k in cols], obs_lik, root_distn)


def nni_from_transitions(indices, indptr, esd, cols, obs_lik, root_distn, Qs=None, node_q=None,
                         grid=None, trial_matrix=None):
    """(moves int32[M, 3], values f64[S, M, G], status int32[S], log-likelihoods f64[S]) from the
    transition matrices `esd` [N, n, n] of the resident lengths; grid None: the plain swap
    (G = 1, no exponential).  Zero-likelihood sites give zeros, a move after which a live site
    has likelihood 0 gives -inf.  trial_matrix(v, tau), where given, stands in for
    scipy.linalg.expm(Qs[node_q[v]] tau) (a model with spectral rates: the oracle's own
    reconstruction)."""
    esd = np.asarray(esd, dtype=float)
    if trial_matrix is None:
        def trial_matrix(v, tau):
            return scipy.linalg.expm(Qs[node_q[v]] * tau)
    moves = brute_moves(indices, indptr)
    G = 1 if grid is None else np.asarray(grid).shape[1]
    base, status = orc.batch_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn)
    live = status == 0
    values = np.zeros((len(base), len(moves), G))
    trials = {}
    if grid is not None:
        with _one_blas_thread():
            for v in sorted(set(int(x) for x in moves[:, 0])):
                trials[v] = [trial_matrix(v, grid[v, g]) for g in range(G)]
    for k, (v, c, s) in enumerate(moves):
        for g in range(G):
            trial = esd
            if grid is not None:
                trial = esd.copy()
                trial[v] = trials[int(v)][g]
            ll, st = moved_log_likelihoods(indices, indptr, trial, cols, obs_lik, root_distn,
                                           (v, c, s))
            values[live, k, g] = np.where(st[live] == 0, ll[live], -np.inf) - base[live]
    return moves, values, status.astype(np.int32), np.where(live, base, 0.0)


def nni_reference(model, case, grid=None, Qs=None, node_q=None, trial_matrix=None):
    """nni_from_transitions of a _resident_cases.Case on model.get_transitions() (Qs, node_q: the
    case's unless given)."""
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return nni_from_transitions(
        ta.indices, ta.indptr, model.get_transitions(), cols, case.obs_lik, case.root_distn,
        case.Qs if Qs is None else Qs, case.node_q if node_q is None else node_q, grid,
        trial_matrix)


def up_pass(indices, indptr, esd, cols, obs_lik, root_distn):
    """The vectors of the issue's formula for every site, on the host and without a division by a
    message: (obs, L, M, up) each [S, N, n] -- obs the observation of a node (ones where it has
    none), L_v = obs_v prod_children M_w, M_v = P_v L_v, and up_v the message into v from above,
    root_distn at the root, NOT normalised by the likelihood."""
    esd = np.asarray(esd, dtype=float)
    kids = children_of(indices, indptr)
    parent = parents_of(indices, indptr)
    N, S, n = len(kids), obs_lik.shape[0], esd.shape[1]
    obs = np.ones((S, N, n))
    for k, v in enumerate(cols):
        obs[:, v] = obs_lik[:, k]
    L, M, up = obs.copy(), np.zeros((S, N, n)), np.zeros((S, N, n))
    for v in range(N - 1, 0, -1):
        M[:, v] = L[:, v] @ esd[v].T
        L[:, parent[v]] *= M[:, v]
    up[:, 0] = np.asarray(root_distn, dtype=float)
    for v in range(1, N):
        p = parent[v]
        x = up[:, p] * obs[:, p]
        for w in kids[p]:
            if w != v:
                x = x * M[:, w]
        up[:, v] = x @ esd[v]
    return obs, L, M, up


def move_terms(indices, indptr, obs, M, up, move):
    """(W o M_c [S, n], L'_v [S, n], the states' mask [S, n] where M_v M_s = 0) of one move."""
    kids = children_of(indices, indptr)
    v, c, s = (int(x) for x in move)
    p = int(parents_of(indices, indptr)[v])
    x = up[:, p] * obs[:, p] * M[:, c]
    for w in kids[p]:
        if w not in (v, s):
            x = x * M[:, w]
    lp = obs[:, v] * M[:, s]
    for w in kids[v]:
        if w != c:
            lp = lp * M[:, w]
    return x, lp, (M[:, v] * M[:, s]) == 0
