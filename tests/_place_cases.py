"""Host reference of rt_sites_placements (test_place_cpu.py, test_place_gpu.py): for every
placement (v, rho, tau) the extended CSR arrays built by hand (never through
raoteh_amd._tree.place_apply, never a device path) -- a new node that cuts the edge above v and a
new leaf below it --, the three new edges under scipy.linalg.expm(Q_v rho t_v),
expm(Q_v (1 - rho) t_v) and expm(Q_v tau), the observation columns extended by the query, the
per-site likelihoods recomputed with the oracle's pruning (oracle/oracle_numpy.py) and
    value = log L(tree with the query placed) - log L
taken: (nnodes - 1) R K whole-tree evaluations, the queries side by side along the site axis."""
import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
from _nni_cases import children_of, parents_of, up_pass
from _profile_cases import _one_blas_thread


def placed_arrays(indices, indptr, v):
    """(indices, indptr, old_of_new) of the tree with the edge above v cut: the cut node (old
    index N) takes the place of v among the children of parent(v), its children are v and the new
    leaf (old index N + 1); the nodes are numbered again in the preorder of the new tree."""
    kids = [list(k) for k in children_of(indices, indptr)]
    N = len(kids)
    p = int(parents_of(indices, indptr)[v])
    assert p >= 0
    kids[p][kids[p].index(v)] = N
    kids.append([v, N + 1])
    kids.append([])
    old_of_new, stack = [], [0]
    while stack:
        a = stack.pop()
        old_of_new.append(a)
        stack.extend(reversed(kids[a]))
    old_of_new = np.array(old_of_new, dtype=np.int64)
    assert sorted(old_of_new) == list(range(N + 2))
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(N + 2)
    new_indices, new_indptr = [], [0]
    for a in old_of_new:
        new_indices.extend(int(new_of_old[b]) for b in kids[a])
        new_indptr.append(len(new_indices))
    return (np.array(new_indices, dtype=np.int64), np.array(new_indptr, dtype=np.int64),
            old_of_new)


def query_likelihoods(queries, kind, n):
    """f64[Q, S, n] of dense queries, or of uint8[Q, S] state queries (a value >= n: ones)."""
    if kind == 'dense':
        return np.asarray(queries, dtype=float)
    st = np.asarray(queries)
    lik = np.ones(st.shape + (n,))
    seen = st < n
    lik[seen] = 0.0
    qq, ii = np.nonzero(seen)
    lik[qq, ii, st[qq, ii]] = 1.0
    return lik


def placed_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn, v, Pa, Pb, Pt, qlik):
    """(log-likelihoods [Q, S], status [Q, S]) of the oracle on the tree with the edge above v cut
    (Pa above the cut, Pb below it) and a leaf with the observations qlik [Q, S, n] below the cut
    on an edge with matrix Pt."""
    esd = np.asarray(esd, dtype=float)
    N = esd.shape[0]
    Q, S = qlik.shape[:2]
    ni, npt, old_of_new = placed_arrays(indices, indptr, v)
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(N + 2)
    ext = np.concatenate([esd, Pa[None], Pt[None]])
    ext[v] = Pb
    obs = np.concatenate([np.tile(obs_lik, (Q, 1, 1)), qlik.reshape(Q * S, 1, -1)], axis=1)
    ll, st = orc.batch_log_likelihoods(ni, npt, ext[old_of_new],
                                       [int(new_of_old[k]) for k in cols] + [int(new_of_old[N + 1])],
                                       obs, root_distn)
    return ll.reshape(Q, S), st.reshape(Q, S)


def place_from_transitions(indices, indptr, esd, cols, obs_lik, root_distn, t, qlik, fractions,
                           pendant, Qs=None, node_q=None, trial_matrix=None):
    """(values f64[S, Q, N, R, K], status int32[S], log-likelihoods f64[S]) from the transition
    matrices `esd` [N, n, n] of the resident lengths t.  Zero-likelihood sites give zeros, a
    placement at which a live site has likelihood 0 gives -inf, the root's row is 0.
    trial_matrix(v, tau), where given, stands in for scipy.linalg.expm(Qs[node_q[v]] tau)."""
    esd = np.asarray(esd, dtype=float)
    if trial_matrix is None:
        def trial_matrix(v, tau):
            return scipy.linalg.expm(Qs[node_q[v]] * tau)
    N = esd.shape[0]
    Q, S = qlik.shape[:2]
    R, K = len(fractions), len(pendant)
    base, status = orc.batch_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn)
    live = status == 0
    values = np.zeros((S, Q, N, R, K))
    for v in range(1, N):
        with _one_blas_thread():
            Pa = [trial_matrix(v, rho * t[v]) for rho in fractions]
            Pb = [trial_matrix(v, (1.0 - rho) * t[v]) for rho in fractions]
            Pt = [trial_matrix(v, tau) for tau in pendant]
        for r in range(R):
            for k in range(K):
                ll, st = placed_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn, v,
                                                Pa[r], Pb[r], Pt[k], qlik)
                got = np.where(st == 0, ll, -np.inf)[:, live] - base[None, live]
                values[live, :, v, r, k] = got.T
    return values, status.astype(np.int32), np.where(live, base, 0.0)


def place_reference(model, case, queries, kind, fractions, pendant, Qs=None, node_q=None,
                    trial_matrix=None):
    """place_from_transitions of a _resident_cases.Case on model.get_transitions() and
    model.branch_lengths() (Qs, node_q: the case's unless given)."""
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return place_from_transitions(
        ta.indices, ta.indptr, model.get_transitions(), cols, case.obs_lik, case.root_distn,
        model.branch_lengths(), query_likelihoods(queries, kind, case.n), fractions, pendant,
        case.Qs if Qs is None else Qs, case.node_q if node_q is None else node_q, trial_matrix)


def field_terms(indices, indptr, esd, cols, obs_lik, root_distn, v, Pa, Pb, Pt, qlik):
    """(A_v [S, n], F [S, n], h [Q, S, n], M_v [S, n]) of the formula for one placement, from
    _nni_cases.up_pass (up NOT normalised by the likelihood): A_v = up_p obs_p prod_{w != v} M_w,
    F = (Pa^T A_v) (Pb L_v), h = Pt o_q."""
    obs, L, M, up = up_pass(indices, indptr, esd, cols, obs_lik, root_distn)
    kids = children_of(indices, indptr)
    p = int(parents_of(indices, indptr)[v])
    A = up[:, p] * obs[:, p]
    for w in kids[p]:
        if w != v:
            A = A * M[:, w]
    F = (A @ Pa) * (L[:, v] @ Pb.T)
    h = qlik @ Pt.T
    return A, F, h, M[:, v]
