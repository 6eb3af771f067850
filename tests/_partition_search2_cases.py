"""Host reference of rt_sites_spr_scores_partitioned and rt_sites_placements_partitioned
(test_partition_search2_cpu.py, test_partition_search2_gpu.py) -- never a device path.  Per rate
set k, over that set's sites, the single-set references are fed the set's own matrices
(_partition_search_cases.set_transitions: scipy.linalg.expm(t[k][v] Q[k][node_q[v]])), lengths t[k]
and rate matrices Q[k]: _spr_cases.spr_from_transitions, and _place_cases.place_from_transitions
with the pendant lengths pendant_scale[k] * tau and the set's slice of the queries (the oracle's
pruning on every moved or placed tree).  The values are scattered to caller order, set_sums and
sums are taken in numpy as _partition_search_cases._sums does.  The cases are
_partition_search_cases.cached_case's; brute_* evaluate a likelihood by summing over every
assignment of states to the internal nodes, for the CPU test of this reference."""
import functools

import numpy as np
import scipy.linalg

import _partition_search_cases as psc
import _place_cases as plc
import _spr_cases as sc
from _mixture_search2_cases import FRACTIONS, PENDANT, make_queries  # noqa: F401
from _partition_search_cases import Reference, cached_case, site_weights  # noqa: F401

SEED = 11


def _set_sums(case, values, status, weights):
    """_partition_search_cases._sums over values [S, ...]: (set_sums [nsets, ...], sums [...])."""
    S = values.shape[0]
    flat = values.reshape(S, -1, 1)
    nan_rows = np.zeros((case.nsets, flat.shape[1]), dtype=bool)
    set_sums, sums = psc._sums(case, flat, status, weights, nan_rows)
    return set_sums.reshape((case.nsets,) + values.shape[1:]), sums.reshape(values.shape[1:])


def spr_reference(ta, case, fractions, radius=None, weights=None):
    """Reference of rt_sites_spr_scores_partitioned: values [S, M, R] in caller order."""
    S = len(case.site_sets)
    moves = sc.brute_moves(ta.indices, ta.indptr, radius)
    values = np.zeros((S, len(moves), len(fractions)))
    status = np.zeros(S, dtype=np.int32)
    loglik = np.zeros(S)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        _, v, st, ll = sc.spr_from_transitions(
            ta.indices, ta.indptr, psc.set_transitions(ta, case, k), psc._cols(ta, case),
            case.obs_lik[mine], case.root_distn, case.t[k], fractions, radius, case.Q[k],
            case.node_q, moves=moves)
        values[mine], status[mine], loglik[mine] = v, st, ll
    set_sums, sums = _set_sums(case, values, status, weights)
    return Reference(values, status, set_sums, sums, loglik, moves)


def pendant_scales(pendant_scale, nsets):
    return np.ones(nsets) if pendant_scale is None else np.asarray(pendant_scale, dtype=float)


def place_reference(ta, case, queries, kind, fractions, pendant, pendant_scale=None, weights=None):
    """Reference of rt_sites_placements_partitioned: values [S, Q, N, R, K] in caller order (the
    root's rows 0); pendant_scale [nsets] or None (ones)."""
    S = len(case.site_sets)
    qlik = plc.query_likelihoods(queries, kind, case.n)
    scale = pendant_scales(pendant_scale, case.nsets)
    values = np.zeros((S, qlik.shape[0], ta.nnodes, len(fractions), len(pendant)))
    status = np.zeros(S, dtype=np.int32)
    loglik = np.zeros(S)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        v, st, ll = plc.place_from_transitions(
            ta.indices, ta.indptr, psc.set_transitions(ta, case, k), psc._cols(ta, case),
            case.obs_lik[mine], case.root_distn, case.t[k], qlik[:, mine], fractions,
            scale[k] * np.asarray(pendant, dtype=float), case.Q[k], case.node_q)
        values[mine], status[mine], loglik[mine] = v, st, ll
    set_sums, sums = _set_sums(case, values, status, weights)
    return Reference(values, status, set_sums, sums, loglik, None)


# ---- the cases of the parity tests ----------------------------------------------------------

# n, upload kind, sets, query kind (the rows the reference was composed for with SEED: no NaN,
# every set with a site keeps at least 3 live sites), then what the calls are given: the SPR
# radius (None: no limit), the numbers of fractions and pendant lengths (FRACTIONS, PENDANT),
# pendant_scale distinct per set or None, site weights or none
PARITY = [
    (2, 'state', 'empty', 'state', 1, 3, 3, True, True),
    (4, 'state', 'empty', 'dense', None, 3, 1, False, True),
    (5, 'dense', 'runs', 'state', None, 1, 3, True, False),
    (20, 'mask', 'zero', 'dense', 1, 3, 3, True, True),
    (61, 'dense', 'two', 'state', None, 3, 1, False, True),
    (122, 'state', 'two', 'state', 1, 1, 3, True, False),
]
PARITY_IDS = ['n%d-%s-%s-q%s-r%s-f%d-p%d%s%s' % (c[0], c[1], c[2], c[3], c[4], c[5], c[6],
                                                 '-scaled' if c[7] else '', '-w' if c[8] else '')
              for c in PARITY]
NQ = 2


def case_weights(case, special, seed, weighted):
    """Site weights with zeros in them, lost0 at weight 0 and lost1 at weight 1; or None."""
    if not weighted:
        return None
    w = site_weights(len(case.site_sets), seed + 2)
    w[special[0]], w[special[1]] = 0.0, 1.0
    return w


def case_scale(nsets, scaled):
    """pendant_scale of the model's sets, distinct per set; or None."""
    return np.linspace(0.5, 2.0, nsets) if scaled else None


@functools.lru_cache(maxsize=None)
def cached_spr_reference(n, kind, sets, radius, nfractions, weighted, seed=SEED):
    """(case, ta, (lost0, lost1, v, k), fractions, weights or None, Reference), computed once;
    callers must not write to it."""
    case, ta, special = cached_case(n, kind, sets, seed)
    w = case_weights(case, special, seed, weighted)
    f = FRACTIONS[nfractions]
    ref = spr_reference(ta, case, f, radius, w)
    for a in ref[:5]:
        a.setflags(write=False)
    return case, ta, special, f, w, ref


@functools.lru_cache(maxsize=None)
def cached_place_reference(n, kind, sets, qkind, nfractions, npendant, scaled, weighted, seed=SEED):
    """(case, ta, special, queries, fractions, pendant, pendant_scale or None, weights or None,
    Reference), computed once; callers must not write to it."""
    case, ta, special = cached_case(n, kind, sets, seed)
    w = case_weights(case, special, seed, weighted)
    f, tau = FRACTIONS[nfractions], PENDANT[npendant]
    scale = case_scale(case.nsets, scaled)
    q = make_queries(case, NQ, qkind, seed + 4)
    ref = place_reference(ta, case, q, qkind, f, tau, scale, w)
    for a in ref[:5]:
        a.setflags(write=False)
    q.setflags(write=False)
    return case, ta, special, q, f, tau, scale, w, ref


def check_reference(case, ref):
    """What a parity case asks of its reference before anything is compared with it: no NaN, at
    least 2 live sites in every set with a site.  -> whether a live site has a -inf."""
    assert not np.isnan(ref.values).any()
    live = ref.status == 0
    for k in range(case.nsets):
        mine = case.site_sets == k
        assert not mine.any() or (mine & live).sum() >= 2, 'set %d: another seed' % k
    return bool(np.isneginf(ref.values[live]).any())


# ---- brute force -----------------------------------------------------------------------------

def brute_spr(ta, case, k, sites, moves, fractions):
    """values [len(sites), len(moves), R] of set k's sites by brute force on every moved tree."""
    esd = psc.set_transitions(ta, case, k)
    cols = psc._cols(ta, case)
    obs = case.obs_lik[sites]
    N = ta.nnodes
    base = psc.brute_likelihoods(ta.indices, ta.indptr, esd, cols, obs, case.root_distn)
    out = np.zeros((len(sites), len(moves), len(fractions)))
    for j, (c, y) in enumerate(moves):
        ni, npt, old_of_new = sc.moved_arrays(ta.indices, ta.indptr, int(c), int(y))
        new_of_old = np.empty_like(old_of_new)
        new_of_old[old_of_new] = np.arange(N + 1)
        Qy = case.Q[k, case.node_q[y]]
        for r, rho in enumerate(fractions):
            ext = np.concatenate([esd, scipy.linalg.expm(rho * case.t[k, y] * Qy)[None]])
            ext[y] = scipy.linalg.expm((1.0 - rho) * case.t[k, y] * Qy)
            with np.errstate(divide='ignore'):
                out[:, j, r] = np.log(psc.brute_likelihoods(
                    ni, npt, ext[old_of_new], [int(new_of_old[x]) for x in cols], obs,
                    case.root_distn)) - np.log(base)
    return out


def brute_place(ta, case, k, sites, qlik, nodes, fractions, pendant):
    """values [len(sites), Q, len(nodes), R, K] of set k's sites by brute force on every placed
    tree; qlik [Q, len(sites), n], pendant the lengths as the set sees them."""
    esd = psc.set_transitions(ta, case, k)
    cols = psc._cols(ta, case)
    obs = case.obs_lik[sites]
    N = ta.nnodes
    base = psc.brute_likelihoods(ta.indices, ta.indptr, esd, cols, obs, case.root_distn)
    out = np.zeros((len(sites), qlik.shape[0], len(nodes), len(fractions), len(pendant)))
    for j, v in enumerate(nodes):
        ni, npt, old_of_new = plc.placed_arrays(ta.indices, ta.indptr, int(v))
        new_of_old = np.empty_like(old_of_new)
        new_of_old[old_of_new] = np.arange(N + 2)
        new_cols = [int(new_of_old[x]) for x in cols] + [int(new_of_old[N + 1])]
        Qv = case.Q[k, case.node_q[v]]
        for r, rho in enumerate(fractions):
            for p, tau in enumerate(pendant):
                ext = np.concatenate([esd, scipy.linalg.expm(rho * case.t[k, v] * Qv)[None],
                                      scipy.linalg.expm(tau * Qv)[None]])
                ext[v] = scipy.linalg.expm((1.0 - rho) * case.t[k, v] * Qv)
                for q in range(qlik.shape[0]):
                    both = np.concatenate([obs, qlik[q][:, None, :]], axis=1)
                    with np.errstate(divide='ignore'):
                        out[:, q, j, r, p] = np.log(psc.brute_likelihoods(
                            ni, npt, ext[old_of_new], new_cols, both, case.root_distn)) - np.log(base)
    return out
