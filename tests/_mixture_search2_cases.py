"""Host reference of rt_sites_spr_scores_mixture and rt_sites_placements_mixture
(test_mixture_search2_cpu.py, test_mixture_search2_gpu.py) -- never a device path.  Per rate set k
of positive class weight the transition matrices come from _mixture_cases.set_transitions, the
halves of the cut edge from scipy.linalg.expm(rho t[k][y] Q[k][node_q[y]]) and
expm((1 - rho) t[k][y] Q[k][node_q[y]]), the pendant edge from expm(pendant_scale[k] tau
Q[k][node_q[v]]), and the site LIKELIHOODS L_ik -- not per-set log ratios, which do not exist where
L_ik == 0 on the resident tree -- from the oracle on the rearranged arrays
(_spr_cases.moved_log_likelihoods, _place_cases.placed_log_likelihoods).  The definitions of
include/raoteh_hip.h section 2d are combined in numpy in set order
(_mixture_search_cases._finish):  value = log sum_k c_k L_ik(changed tree) - log sum_k c_k L_ik."""
import functools

import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
import _mixture_cases as mc
import _mixture_search_cases as msc
import _place_cases as plc
import _spr_cases as sc
from _mixture_search_cases import (NSITES, Reference, cached_case, class_weights,  # noqa: F401
                                   site_weights, _likelihoods)
from _profile_cases import _one_blas_thread


def _halves(case, k, y, fractions):
    Qy = case.Q[k][case.node_q[y]]
    t = case.t[k][y]
    return [(scipy.linalg.expm(rho * t * Qy), scipy.linalg.expm((1.0 - rho) * t * Qy))
            for rho in fractions]


def _resident(ta, case, k, cols):
    esd = mc.set_transitions(ta, case, k)
    return esd, _likelihoods(*orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols,
                                                        case.obs_lik, case.root_distn))


def spr_reference(ta, case, c, fractions, radius=None, weights=None, moves=None):
    """Reference of rt_sites_spr_scores_mixture: values [S, M, R], sums [M, R], loglik, status,
    moves (the brute-force list of _spr_cases within the radius unless given)."""
    case = mc.normalised(case)
    K = case.t.shape[0]
    cols = msc._cols(ta, case)
    S, R = case.obs_lik.shape[0], len(fractions)
    if moves is None:
        moves = sc.brute_moves(ta.indices, ta.indptr, radius)
    L = np.zeros((K, S))
    trial = np.zeros((K, S, len(moves), R))
    for k in range(K):
        if not c[k] > 0:
            continue
        esd, L[k] = _resident(ta, case, k, cols)
        with _one_blas_thread():
            halves = dict((y, _halves(case, k, y, fractions))
                          for y in sorted(set(int(x) for x in moves[:, 1])))
        for j, (cc, y) in enumerate(moves):
            for r in range(R):
                Pa, Pb = halves[int(y)][r]
                trial[k, :, j, r] = _likelihoods(*sc.moved_log_likelihoods(
                    ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, cc, y, Pa, Pb))
    return msc._finish(case, c, L, trial, weights, np.zeros(len(moves), dtype=bool), moves)


def check_scale(pendant_scale, K):
    return np.ones(K) if pendant_scale is None else np.asarray(pendant_scale, dtype=float)


def place_reference(ta, case, c, queries, kind, fractions, pendant, pendant_scale=None,
                    weights=None):
    """Reference of rt_sites_placements_mixture: values [S, Q, N, R, Kp] (the root's rows 0), sums
    [Q, N, R, Kp], loglik, status."""
    case = mc.normalised(case)
    K, N = case.t.shape
    cols = msc._cols(ta, case)
    S, R, Kp = case.obs_lik.shape[0], len(fractions), len(pendant)
    qlik = plc.query_likelihoods(queries, kind, case.n)
    nq = qlik.shape[0]
    scale = check_scale(pendant_scale, K)
    L = np.zeros((K, S))
    trial = np.zeros((K, S, nq, N, R, Kp))
    for k in range(K):
        if not c[k] > 0:
            continue
        esd, L[k] = _resident(ta, case, k, cols)
        for v in range(1, N):
            with _one_blas_thread():
                halves = _halves(case, k, v, fractions)
                Pt = [scipy.linalg.expm(scale[k] * tau * case.Q[k][case.node_q[v]])
                      for tau in pendant]
            for r in range(R):
                for j in range(Kp):
                    ll, st = plc.placed_log_likelihoods(
                        ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, v,
                        halves[r][0], halves[r][1], Pt[j], qlik)
                    trial[k, :, :, v, r, j] = _likelihoods(ll, st).T
    rows = nq * N * R
    ref = msc._finish(case, c, L, trial.reshape(K, S, rows, Kp), weights,
                      np.zeros(rows, dtype=bool), None)
    values = ref.values.reshape(S, nq, N, R, Kp)
    sums = ref.sums.reshape(nq, N, R, Kp)
    values[:, :, 0] = 0.0                       # (the root's rows)
    sums[:, 0] = 0.0
    return Reference(values, sums, ref.loglik, ref.status, None)


def make_queries(case, nq, kind, seed):
    """nq queries over the case's sites: dense f64[nq, S, n] positive likelihood vectors (site 1 of
    query 0 a point mass), or state uint8[nq, S] with an unobserved 255 at site 3 of query 0."""
    rng = np.random.RandomState(seed)
    S, n = case.obs_lik.shape[0], case.n
    if kind == 'dense':
        q = rng.uniform(0.05, 1.0, (nq, S, n))
        q[0, 1] = 0.0
        q[0, 1, n - 1] = 1.0
        return q
    q = rng.randint(0, n, size=(nq, S)).astype(np.uint8)
    q[0, 3] = 255
    return q


FRACTIONS = {1: (0.5,), 3: (0.0, 0.35, 1.0), 8: (0.0, 0.1, 0.25, 0.4, 0.5, 0.7, 0.9, 1.0)}
PENDANT = {1: (0.13,), 3: (0.0, 0.07, 0.4)}


@functools.lru_cache(maxsize=None)
def cached_spr_reference(n, tree, kind, K, seed, radius, nfractions, weighted, nsites=NSITES):
    """(case, ta, c, fractions, site weights or None, Reference), computed once; callers must not
    write to it."""
    case, ta = cached_case(n, tree, kind, K, seed, nsites)
    c = class_weights(K, seed + 1)
    w = site_weights(nsites, seed + 2) if weighted else None
    f = FRACTIONS[nfractions]
    ref = spr_reference(ta, case, c, f, radius, w)
    for a in ref[:5]:
        a.setflags(write=False)
    return case, ta, c, f, w, ref


@functools.lru_cache(maxsize=None)
def cached_place_reference(n, tree, kind, K, seed, qkind, nq, nfractions, npendant, scaled,
                           weighted, nsites=NSITES):
    """(case, ta, c, queries, fractions, pendant, pendant_scale or None, site weights or None,
    Reference), computed once; callers must not write to it."""
    case, ta = cached_case(n, tree, kind, K, seed, nsites)
    c = class_weights(K, seed + 1)
    w = site_weights(nsites, seed + 2) if weighted else None
    f, tau = FRACTIONS[nfractions], PENDANT[npendant]
    scale = np.linspace(0.5, 2.0, K) if scaled else None
    q = make_queries(case, nq, qkind, seed + 4)
    ref = place_reference(ta, case, c, q, qkind, f, tau, scale, w)
    for a in ref[:4]:
        a.setflags(write=False)
    q.setflags(write=False)
    return case, ta, c, q, f, tau, scale, w, ref


# ---- the revival and the lost case under SPR and under a placement -------------------------

def revival_move(ta):
    """On the tree of _mixture_search_cases.revival_case (root p, children v and s; v observed in
    state 1 with the children c = 0 and c2 = 2): prune c and regraft it above s.  Under the
    one-way set the resident tree is impossible (v = 1 cannot reach c = 0); after the move c hangs
    below a new node between p and s, which p = 0 reaches."""
    p, v, s, c, c2 = (ta.node_to_index[x] for x in (0, 1, 2, 3, 4))
    return (c, s)


def spr_move_likelihoods(case, ta, move, fraction=0.5):
    """(L [K, S] on the resident tree, L' [K, S] after the SPR move at the fraction) from the
    oracle."""
    case = mc.normalised(case)
    cols = msc._cols(ta, case)
    K = case.Q.shape[0]
    L = np.zeros((K, case.obs_lik.shape[0]))
    moved = np.zeros_like(L)
    for k in range(K):
        esd, L[k] = _resident(ta, case, k, cols)
        Pa, Pb = _halves(case, k, move[1], [fraction])[0]
        moved[k] = _likelihoods(*sc.moved_log_likelihoods(
            ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, move[0], move[1], Pa, Pb))
    return L, moved


def lost_move(ta):
    """The SPR form of _mixture_search_cases.lost_case's move (v, c, s), which hangs s below v:
    prune s and regraft it above c.  At any fraction the new node lies below v = 1, and under a
    one-way set nothing below state 1 reaches the leaf s = 0."""
    p, v, s, c, c2 = (ta.node_to_index[x] for x in (0, 1, 2, 3, 4))
    return (s, c)
