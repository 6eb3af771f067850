"""Host reference of rt_model_spr_moves / rt_sites_spr_scores (test_spr_cpu.py, test_spr_gpu.py):
the moves by brute force -- all pairs (c, y) filtered by the definition and by path distances
taken from the parents, not by the walk the planner uses --, and for every move and fraction the
rearranged CSR arrays built by hand (never through raoteh_amd._tree.spr_apply, never a device
path): the subtree of c taken from its parent, a new node that cuts the edge above y with y and c
below it, the two halves under scipy.linalg.expm(Q_y rho t_y) and expm(Q_y (1 - rho) t_y), the
per-site likelihoods recomputed with the oracle's pruning (oracle/oracle_numpy.py) and
    value = log L(moved tree) - log L
taken: nmoves * R whole-tree evaluations."""
import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
from _nni_cases import children_of, parents_of, up_pass
from _profile_cases import _one_blas_thread


def _ancestors(parent, v):
    """v, parent(v), ..., the root."""
    out = []
    while v >= 0:
        out.append(int(v))
        v = parent[v]
    return out


def tree_distance(parent, a, b):
    """Edges on the path between a and b."""
    up_a, up_b = _ancestors(parent, a), _ancestors(parent, b)
    common = set(up_a) & set(up_b)
    return min(i for i, x in enumerate(up_a) if x in common) + \
        min(i for i, x in enumerate(up_b) if x in common)


def brute_moves(indices, indptr, radius=None):
    """Every (c, y) with c and y not the root, y outside the subtree of c and
    min(dist(v, y), dist(v, parent(y))) <= radius for v = parent(c) (radius None: no limit),
    sorted by c, then y."""
    parent = parents_of(indices, indptr)
    N = len(parent)
    found = []
    for c in range(1, N):
        v = int(parent[c])
        for y in range(1, N):
            if c in _ancestors(parent, y):
                continue
            d = min(tree_distance(parent, v, y), tree_distance(parent, v, int(parent[y])))
            if radius is None or d <= radius:
                found.append((c, y))
    return np.array(sorted(found), dtype=np.int32).reshape(-1, 2)


def unlimited_count(indices, indptr):
    """sum over c != root of nnodes - 1 - |subtree(c)|."""
    parent = parents_of(indices, indptr)
    N = len(parent)
    size = np.ones(N, dtype=np.int64)
    for v in range(N - 1, 0, -1):
        size[parent[v]] += size[v]
    return int(sum(N - 1 - size[c] for c in range(1, N)))


def moved_arrays(indices, indptr, c, y):
    """(indices, indptr, old_of_new) of the tree after the move: c leaves the children of its
    parent, the cut node (old index N) takes the place of y among the children of parent(y),
    its children are y and c; the nodes are numbered again in the preorder of the new tree."""
    kids = [list(k) for k in children_of(indices, indptr)]
    parent = parents_of(indices, indptr)
    N = len(kids)
    v, q = int(parent[c]), int(parent[y])
    assert v >= 0 and q >= 0 and c not in _ancestors(parent, y)
    kids[v].remove(c)
    kids[q][kids[q].index(y)] = N
    kids.append([y, c])
    old_of_new, stack = [], [0]
    while stack:
        a = stack.pop()
        old_of_new.append(a)
        stack.extend(reversed(kids[a]))
    old_of_new = np.array(old_of_new, dtype=np.int64)
    assert sorted(old_of_new) == list(range(N + 1))
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(N + 1)
    new_indices, new_indptr = [], [0]
    for a in old_of_new:
        new_indices.extend(int(new_of_old[b]) for b in kids[a])
        new_indptr.append(len(new_indices))
    return (np.array(new_indices, dtype=np.int64), np.array(new_indptr, dtype=np.int64),
            old_of_new)


def moved_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn, c, y, Pa, Pb):
    """(log-likelihoods, status) of the oracle on the moved tree: Pa above the cut node, Pb
    between it and y; every other node keeps the matrix of the edge above it and its
    observation, the cut node has none."""
    esd = np.asarray(esd, dtype=float)
    N = esd.shape[0]
    ni, npt, old_of_new = moved_arrays(indices, indptr, int(c), int(y))
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(N + 1)
    ext = np.concatenate([esd, Pa[None]])
    ext[y] = Pb
    return orc.batch_log_likelihoods(ni, npt, ext[old_of_new], [int(new_of_old[k]) for k in cols],
                                     obs_lik, root_distn)


def spr_from_transitions(indices, indptr, esd, cols, obs_lik, root_distn, t, fractions,
                         radius=None, Qs=None, node_q=None, trial_matrix=None, moves=None):
    """(moves int32[M, 2], values f64[S, M, R], status int32[S], log-likelihoods f64[S]) from
    the transition matrices `esd` [N, n, n] of the resident lengths t.  Zero-likelihood sites
    give zeros, a move after which a live site has likelihood 0 gives -inf.
    trial_matrix(y, tau), where given, stands in for scipy.linalg.expm(Qs[node_q[y]] tau);
    moves, where given, are scored in place of brute_moves(radius)."""
    esd = np.asarray(esd, dtype=float)
    if trial_matrix is None:
        def trial_matrix(y, tau):
            return scipy.linalg.expm(Qs[node_q[y]] * tau)
    if moves is None:
        moves = brute_moves(indices, indptr, radius)
    R = len(fractions)
    base, status = orc.batch_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn)
    live = status == 0
    values = np.zeros((len(base), len(moves), R))
    halves = {}
    with _one_blas_thread():
        for y in sorted(set(int(x) for x in moves[:, 1])):
            halves[y] = [(trial_matrix(y, rho * t[y]), trial_matrix(y, (1.0 - rho) * t[y]))
                         for rho in fractions]
    for k, (c, y) in enumerate(moves):
        for r in range(R):
            Pa, Pb = halves[int(y)][r]
            ll, st = moved_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn, c, y,
                                           Pa, Pb)
            values[live, k, r] = np.where(st[live] == 0, ll[live], -np.inf) - base[live]
    return moves, values, status.astype(np.int32), np.where(live, base, 0.0)


def spr_reference(model, case, fractions, radius=None, Qs=None, node_q=None, trial_matrix=None,
                  moves=None):
    """spr_from_transitions of a _resident_cases.Case on model.get_transitions() and
    model.branch_lengths() (Qs, node_q: the case's unless given)."""
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return spr_from_transitions(
        ta.indices, ta.indptr, model.get_transitions(), cols, case.obs_lik, case.root_distn,
        model.branch_lengths(), fractions, radius, case.Qs if Qs is None else Qs,
        case.node_q if node_q is None else node_q, trial_matrix, moves)


def spr_formula(indices, indptr, esd, cols, obs_lik, root_distn, c, y, Pa, Pb):
    """(ratio L'/L [S], the likelihood L [S], A-_y [S, n], M_v [S, n]) of one move by the
    formula of rt_sites_spr_scores, in numpy from _nni_cases.up_pass (up NOT normalised, so the
    ratio divides by L at the end): the path quantities L-, M- up from v = parent(c), then A-
    and up- down from the highest path node the target needs."""
    esd = np.asarray(esd, dtype=float)
    obs, L, M, up = up_pass(indices, indptr, esd, cols, obs_lik, root_distn)
    kids = children_of(indices, indptr)
    parent = parents_of(indices, indptr)
    lik = (L[:, 0] * up[:, 0]).sum(axis=1)
    v = int(parent[c])
    path = _ancestors(parent, v)
    Lm, Mm = {}, {}
    for j, a in enumerate(path):
        x = obs[:, a].copy()
        for w in kids[a]:
            if w == c:
                continue
            x = x * (Mm[w] if j and w == path[j - 1] else M[:, w])
        Lm[a] = x
        if a:
            Mm[a] = x @ esd[a].T

    def message(w):
        return Mm[w] if w in Mm else M[:, w]

    def up_minus(x):
        if x in Lm:                              # an ancestor's message from above holds no c
            return up[:, x]
        return A_minus(x) @ esd[x]

    def A_minus(x):
        q = int(parent[x])
        out = up_minus(q) * obs[:, q]
        for w in kids[q]:
            if w not in (x, c):
                out = out * message(w)
        return out

    A = A_minus(int(y))
    Ly = Lm[int(y)] if int(y) in Lm else L[:, int(y)]
    F = (A @ Pa) * (Ly @ Pb.T)
    ratio = (F * M[:, c]).sum(axis=1)
    with np.errstate(divide='ignore', invalid='ignore'):
        return np.where(lik > 0, ratio / np.where(lik > 0, lik, 1.0), 0.0), lik, A, M[:, v]
