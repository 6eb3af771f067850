"""
Device-resident objects of the batched hot path (thin wrappers over the C ABI):

    ctx   = get_context()                      one per process / GPU
    model = TreeModel(T, root, nstates)        tree + schedule on the device
    model.set_rates(Q_default=Q)               per-edge expm(Q*t) on the device
    batch = model.upload_sites(obs_nodes, data, kind='dense')
    loglik, status = model.log_likelihoods(batch)
    total, nzero = model.total_log_likelihood(batch)

Reference path being replaced: raoteh/sampler/_mjp_dense.py:362-407 called once
per site (examples/p53/p53.py:88-100).
"""
from __future__ import annotations

import atexit
import collections
import ctypes
import weakref
from ctypes import byref, c_char_p, c_double, c_int, c_int32, c_int64, c_void_p

import numpy as np

from . import _lib
from ._tree import TreeArrays

__all__ = ['check_rate_sets', 'check_site_sets', 'Context', 'get_context', 'TreeModel', 'SiteBatch', 'device_count', 'Posteriors',
           'states_to_mask', 'BranchExpectations', 'check_branch_coefs', 'SampledStates', 'SampledMappings',
           'MapStates']

# At interpreter shutdown objects are finalised in arbitrary order (a model
# after its context, say); the process is going away, so skip the native
# destructors then instead of handing the library dangling handles.
_shutting_down = []
atexit.register(_shutting_down.append, True)

_KINDS = {'dense': _lib.RT_OBS_DENSE, 'state': _lib.RT_OBS_STATE,
          'mask': _lib.RT_OBS_MASK}


def _f64(a):
    return np.ascontiguousarray(a, dtype=np.float64)


def _i64(a):
    return np.ascontiguousarray(a, dtype=np.int64)


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype))


def _as_uint8_states(data, nstates):
    """Observed states -> uint8 (255 = unobserved).  A plain cast would wrap a state
    >= 256 (or a negative one) onto another state silently; anything that is neither a
    state in [0, nstates) nor the 255 / -1 'unobserved' marker is an error."""
    a = np.asarray(data)
    if a.dtype == np.uint8:
        bad = (a >= nstates) & (a != 255)
    else:
        if not np.issubdtype(a.dtype, np.integer):
            raise ValueError('observed states must be integers')
        bad = ((a < 0) | (a >= nstates)) & (a != 255) & (a != -1)
        a = np.where(a == -1, 255, a)
    if nstates > 255 or bad.any():
        raise ValueError('observed state outside [0, %d) (255 or -1 = unobserved)'
                         % nstates)
    return np.ascontiguousarray(a, dtype=np.uint8)


def states_to_mask(states, nstates):
    """An iterable of state indices -> the two-word bit mask of rt_sites_posteriors (bit s % 64
    of word s // 64, the RT_OBS_MASK encoding), uint64[2].  ValueError for a state outside
    0 .. nstates - 1."""
    words = [0, 0]
    for s in states:
        si = int(s)
        if si != s or not 0 <= si < nstates:
            raise ValueError('state %r is not in 0..%d' % (s, nstates - 1))
        words[si >> 6] |= 1 << (si & 63)
    return np.array(words, dtype=np.uint64)


# TreeModel.posteriors: per-site arrays indexed by the preorder `nodes` (node_values
# [nsites, nnodes, len(node_sets)], edge_values [nsites, nnodes, len(edge_sets)] keyed by the
# edge's child, 0 at the root), marginals [nsites, len(marginal_nodes), nstates] or None,
# status int32[nsites] (0 ok, 1 zero likelihood, 2 zero denominator)
Posteriors = collections.namedtuple(
    'Posteriors', 'node_values edge_values marginals status nodes marginal_nodes')


# TreeModel.branch_expectations: values [nsites, nnodes, ncoefs] (or None), edge_sums
# [nnodes, ncoefs], both keyed by the edge's child in the preorder `nodes` (0 at the root),
# status int32[nsites] as Posteriors
BranchExpectations = collections.namedtuple('BranchExpectations', 'values edge_sums status nodes')


# TreeModel.sample_states: states uint8[ndraws, nsites, nnodes] indexed by the preorder `nodes`
# (255 = no state), status int32[nsites] (0 ok, 1 zero likelihood: the site's draws are all 255,
# 2 a node without a state of positive weight)
SampledStates = collections.namedtuple('SampledStates', 'states status nodes')


# TreeModel.map_states: the joint maximum-likelihood reconstruction, states uint8[nsites, nnodes]
# indexed by the preorder `nodes` (255 = no state), log_joint f64[nsites] the log-probability of
# the reconstruction with the observations, status int32[nsites] (0 ok, 1 zero likelihood: the
# site's states are all 255 and log_joint is -inf)
MapStates = collections.namedtuple('MapStates', 'states log_joint status nodes')


# TreeModel.sample_mappings: states as SampledStates; values f64[ndraws, nsites, nnodes, ncoefs]
# and counts int32[ndraws, nsites, nnodes, 2] = (uniformized events, real changes) of the sampled
# path on the edge above each preorder node (None with per_draw=False), means
# f64[nsites, nnodes, ncoefs] over the draws; status as SampledStates, 4: an edge whose
# event-count weights have no positive total
SampledMappings = collections.namedtuple('SampledMappings',
                                         'states values counts means status nodes')


def check_branch_coefs(coefs, nstates):
    """One (n, n) coefficient matrix or a sequence of them -> f64[ncoefs, n, n] for
    rt_sites_branch_expectations.  ValueError for another shape, no matrix or more than
    RT_MAX_BRANCH_COEFS of them, or a coefficient that is not finite."""
    try:
        E = np.array(coefs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('coefs must be one (%d, %d) array or a sequence of them'
                         % (nstates, nstates))
    if E.ndim == 2:
        E = E[None]
    if E.ndim != 3 or E.shape[1:] != (nstates, nstates):
        raise ValueError('coefs must be one (%d, %d) array or a sequence of them, not %s'
                         % (nstates, nstates, E.shape))
    if not 1 <= E.shape[0] <= _lib.RT_MAX_BRANCH_COEFS:
        raise ValueError('between 1 and %d coefficient matrices per call (%d here)'
                         % (_lib.RT_MAX_BRANCH_COEFS, E.shape[0]))
    if not np.isfinite(E).all():
        raise ValueError('the coefficients must be finite')
    return np.ascontiguousarray(E)


# TreeModel.branch_expectations_partitioned: BranchExpectations of a partitioned batch (values in
# caller order, real sites only) plus set_edge_sums [nsets, nnodes, ncoefs], the weighted sums over
# each rate set's sites (zeros for an empty set; edge_sums is their sum in set order)
PartitionedBranchExpectations = collections.namedtuple(
    'PartitionedBranchExpectations', 'values edge_sums set_edge_sums status nodes')


def check_branch_coefs_partitioned(coefs, nstates, nsets):
    """The coefficients of TreeModel.branch_expectations_partitioned -> (f64[ncoefs, n, n], False)
    for one (n, n) matrix or a (C, n, n) sequence shared by all rate sets (check_branch_coefs), or
    (f64[nsets, ncoefs, n, n], True) for an (nsets, C, n, n) array with set k's matrices at [k].
    ValueError as check_branch_coefs, and for a four-dimensional array whose leading dimension is
    not nsets."""
    try:
        E = np.array(coefs, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('coefs must be (%d, %d), (C, %d, %d) or (nsets, C, %d, %d)'
                         % ((nstates,) * 6))
    if E.ndim != 4:
        return check_branch_coefs(coefs, nstates), False
    if E.shape[0] != nsets:
        raise ValueError('per-set coefs must have nsets=%d leading entries, not %d (shape %s)'
                         % (nsets, E.shape[0], E.shape))
    if E.shape[2:] != (nstates, nstates):
        raise ValueError('coefs must be (%d, %d), (C, %d, %d) or (nsets, C, %d, %d), not %s'
                         % ((nstates,) * 6 + (E.shape,)))
    if not 1 <= E.shape[1] <= _lib.RT_MAX_BRANCH_COEFS:
        raise ValueError('between 1 and %d coefficient matrices per call (%d here)'
                         % (_lib.RT_MAX_BRANCH_COEFS, E.shape[1]))
    if not np.isfinite(E).all():
        raise ValueError('the coefficients must be finite')
    return np.ascontiguousarray(E), True


# TreeModel.branch_expectations_mixture: values [nsites, nnodes, ncoefs] (or None) and edge_sums
# [nnodes, ncoefs] as BranchExpectations, under the site-class mixture over the K rate sets;
# set_edge_sums [K, nnodes, ncoefs] the posterior- and site-weighted sums per class (edge_sums is
# their sum in set order), class_posteriors [nsites, K], class_sums [K] = sum_i w_i posterior,
# log_likelihoods [nsites] (-inf where no class is live), status int32[nsites]
MixtureBranchExpectations = collections.namedtuple(
    'MixtureBranchExpectations',
    'values edge_sums set_edge_sums class_posteriors class_sums log_likelihoods status')


def rate_parameter_coefs(Q, dQ):
    """The coefficient matrix E for which branch_expectations (and its partitioned and mixture
    forms) return d log L_i / d theta on each branch, given the rate matrix Q and dQ = dQ / d
    theta: the direction C = E * Q off the diagonal, E on it, must be dQ, so E[c][d] =
    dQ[c][d] / Q[c][d] where Q[c][d] != 0 (0 elsewhere) and E[c][c] = dQ[c][c].  ValueError where
    dQ is non-zero off the diagonal at an entry where Q is zero: no E gives that direction."""
    Q = np.asarray(Q, dtype=np.float64)
    dQ = np.asarray(dQ, dtype=np.float64)
    if Q.ndim != 2 or Q.shape[0] != Q.shape[1] or dQ.shape != Q.shape:
        raise ValueError('Q and dQ must be square matrices of one shape, not %s and %s'
                         % (Q.shape, dQ.shape))
    off = ~np.eye(Q.shape[0], dtype=bool)
    if ((dQ != 0) & (Q == 0) & off).any():
        raise ValueError('dQ is non-zero where Q is zero: the direction is not E * Q for any E')
    E = np.zeros_like(Q)
    live = off & (Q != 0)
    E[live] = dQ[live] / Q[live]
    np.fill_diagonal(E, np.diag(dQ))
    return E


def partition_chain_rule(grad, rates, tau):
    """The gradient of TreeModel.branch_length_gradient_partitioned, grad[k, v] = d/d t[k][v],
    under the usual parametrisation t[k][v] = rates[k] * tau[v] -> (d/d tau f64[nnodes],
    d/d rates f64[nsets]): d/d tau_v = sum_k r_k g[k, v], d/d r_k = sum_v tau_v g[k, v]."""
    g = np.asarray(grad, dtype=np.float64)
    r = np.asarray(rates, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    if g.ndim != 2 or r.shape != (g.shape[0],) or tau.shape != (g.shape[1],):
        raise ValueError('grad [nsets, nnodes], rates [nsets] and tau [nnodes] expected, not %s, '
                         '%s and %s' % (g.shape, r.shape, tau.shape))
    return r @ g, g @ tau


# TreeModel.branch_profiles: lengths and sums [nnodes, G], values [nsites, nnodes, G] (or None),
# all keyed by the edge's child in the preorder `nodes` (the root's row: lengths 0, values 0);
# values[i, v, g] = log L_i(t_v -> lengths[v, g]) - log L_i, NaN in the row of an edge whose
# resident length is 0; status as Posteriors
BranchProfiles = collections.namedtuple('BranchProfiles', 'nodes lengths sums values status')


def check_profile_lengths(lengths, nnodes, factors=None, resident=None, tree=None):
    """The grid of TreeModel.branch_profiles -> f64[nnodes, G], C-contiguous, for
    rt_sites_branch_profiles.  Exactly one of `lengths` and `factors`:
    lengths  an absolute [nnodes, G] array in preorder (row 0, the root's, is ignored and comes
             back as zeros), or a dict edge -> sequence of G lengths, an edge being the preorder
             index of its child, or with `tree` (a TreeArrays) a pair of tree nodes in either
             direction; edges the dict leaves out stay at their `resident` length;
    factors  a 1-D sequence of G multipliers of every branch's `resident` length f64[nnodes].
    ValueError for both or neither, another shape, G outside 1..RT_MAX_PROFILE_POINTS, or a
    length that is negative or not finite."""
    if (lengths is None) == (factors is None):
        raise ValueError('exactly one of lengths and factors must be given')
    if resident is not None:
        resident = np.asarray(resident, dtype=np.float64)
        if resident.shape != (nnodes,):
            raise ValueError('the resident lengths must have one entry per node')
    if factors is not None:
        if resident is None:
            raise ValueError('factors multiply the resident branch lengths, which are not known')
        try:
            f = np.array(factors, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('factors must be a 1-D sequence of numbers')
        if f.ndim != 1:
            raise ValueError('factors must be 1-D, not %s' % (f.shape,))
        grid = resident[:, None] * f[None, :]
    elif isinstance(lengths, dict):
        rows = {}
        for edge, seq in lengths.items():
            if isinstance(edge, tuple):
                if tree is None or len(edge) != 2:
                    raise ValueError('an edge given as a pair of nodes needs the tree')
                try:
                    a, b = (tree.node_to_index[x] for x in edge)
                except KeyError:
                    raise ValueError('%r is not an edge of the tree' % (edge,))
                if tree.parent[b] == a:
                    v = b
                elif tree.parent[a] == b:
                    v = a
                else:
                    raise ValueError('%r is not an edge of the tree' % (edge,))
            else:
                v = int(edge)
                if v != edge or not 1 <= v < nnodes:
                    raise ValueError('edge %r: the preorder index of a non-root node' % (edge,))
            try:
                row = np.array(seq, dtype=np.float64)
            except (TypeError, ValueError):
                raise ValueError('the lengths of edge %r must be a sequence of numbers' % (edge,))
            if row.ndim != 1 or v in rows:
                raise ValueError('edge %r: one 1-D sequence of lengths per edge' % (edge,))
            rows[v] = row
        sizes = set(len(r) for r in rows.values())
        if len(sizes) != 1:
            raise ValueError('every edge needs the same number of lengths (at least one edge)')
        if len(rows) < nnodes - 1 and resident is None:
            raise ValueError('edges left out stay at their resident length, which is not known')
        grid = np.zeros((nnodes, sizes.pop()))
        if resident is not None:
            grid[:] = resident[:, None]
        for v, row in rows.items():
            grid[v] = row
    else:
        try:
            grid = np.array(lengths, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('lengths must be a [%d, G] array or a dict edge -> sequence' % nnodes)
        if grid.ndim != 2 or grid.shape[0] != nnodes:
            raise ValueError('lengths must be [%d, G], not %s' % (nnodes, grid.shape))
    if not 1 <= grid.shape[1] <= _lib.RT_MAX_PROFILE_POINTS:
        raise ValueError('between 1 and %d lengths per branch (%d here)'
                         % (_lib.RT_MAX_PROFILE_POINTS, grid.shape[1]))
    grid = np.ascontiguousarray(grid, dtype=np.float64)
    grid[0] = 0.0
    if not (np.isfinite(grid).all() and (grid >= 0).all()):
        raise ValueError('the lengths must be finite and not negative')
    return grid


# TreeModel.nni_scores: moves int32[nmoves, 3] (TreeModel.nni_moves), lengths [nnodes, G] as
# evaluated (the resident lengths [nnodes, 1] for the plain swap; None where the model has none),
# sums [nmoves, G], values [nsites, nmoves, G] (or None) with values[i, mv, g] = log L_i(tree after
# move mv, t_v -> lengths[v, g]) - log L_i; status as Posteriors
NniScores = collections.namedtuple('NniScores', 'moves lengths sums values status')


# TreeModel.branch_profiles_mixture: factors and sums [nnodes, G], values [nsites, nnodes, G] (or
# None) keyed by the edge's child in preorder; values[i, v, g] = log sum_k c_k L_ik(t[k][v] ->
# factors[v, g] t[k][v]) - log_likelihoods[i] under the site-class mixture over the K rate sets;
# loglik [nsites] = log sum_k c_k L_ik (-inf where dead); status as MixtureBranchExpectations
MixtureBranchProfiles = collections.namedtuple('MixtureBranchProfiles',
                                               'factors sums values loglik status')

# TreeModel.nni_scores_mixture: moves as NniScores, factors [nnodes, G] as evaluated (None for the
# plain swap), sums [nmoves, G], values [nsites, nmoves, G] (or None), loglik, status
MixtureNniScores = collections.namedtuple('MixtureNniScores',
                                          'moves factors sums values loglik status')


# TreeModel.branch_profiles_partitioned: factors [nnodes, G] as evaluated, values [nsites, nnodes,
# G] in caller order (or None), sums [nnodes, G], set_sums [nsets, nnodes, G] the weighted sums over
# each rate set's sites (zeros for an empty set; sums is their sum in set order), status, nodes
PartitionedBranchProfiles = collections.namedtuple(
    'PartitionedBranchProfiles', 'factors values sums set_sums status nodes')

# TreeModel.nni_scores_partitioned: moves as NniScores, factors [nnodes, G] as evaluated (None for
# the plain swap), values [nsites, nmoves, G] in caller order (or None), sums [nmoves, G], set_sums
# [nsets, nmoves, G], status
PartitionedNniScores = collections.namedtuple(
    'PartitionedNniScores', 'moves factors values sums set_sums status')

# TreeModel.spr_scores_partitioned: moves, fractions and best as SprScores, values [nsites, nmoves,
# R] in caller order (or None), sums [nmoves, R], set_sums [nsets, nmoves, R], status
PartitionedSprScores = collections.namedtuple(
    'PartitionedSprScores', 'moves fractions values sums set_sums status best')

# TreeModel.place_queries_partitioned: fractions, pendant and best as Placements, pendant_scale
# [the model's sets] as evaluated, values [nsites, Q, nnodes, R, K] in caller order (or None), sums
# [Q, nnodes, R, K], set_sums [nsets, Q, nnodes, R, K], status
PartitionedPlacements = collections.namedtuple(
    'PartitionedPlacements', 'fractions pendant pendant_scale values sums set_sums status best')


def check_profile_factors(factors, nnodes):
    """The trial lengths of TreeModel.branch_profiles_mixture / nni_scores_mixture, as factors of
    every class's own resident branch lengths -> f64[nnodes, G], C-contiguous, row 0 (the
    root's) zero.  `factors` is a 1-D sequence of G multipliers, one row for every branch, or a
    [nnodes, G] array in preorder.  ValueError for another shape, G outside
    1..RT_MAX_PROFILE_POINTS, or a factor that is negative or not finite."""
    try:
        f = np.array(factors, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('factors must be a 1-D sequence of numbers or a [%d, G] array' % nnodes)
    if f.ndim == 1:
        f = np.repeat(f[None, :], nnodes, axis=0)
    elif f.ndim != 2 or f.shape[0] != nnodes:
        raise ValueError('factors must be 1-D or [%d, G], not %s' % (nnodes, f.shape))
    if not 1 <= f.shape[1] <= _lib.RT_MAX_PROFILE_POINTS:
        raise ValueError('between 1 and %d factors per branch (%d here)'
                         % (_lib.RT_MAX_PROFILE_POINTS, f.shape[1]))
    f = np.ascontiguousarray(f, dtype=np.float64)
    f[0] = 0.0
    if not (np.isfinite(f).all() and (f >= 0).all()):
        raise ValueError('the factors must be finite and not negative')
    return f


def tree_nni_moves(tree):
    """rt_tree_nni_moves: the moves TreeModel.nni_moves lists, int32[nmoves, 3], from a
    TreeArrays alone (host only: no context, no model)."""
    idx = np.ascontiguousarray(tree.indices, dtype=np.int64)
    ptr = np.ascontiguousarray(tree.indptr, dtype=np.int64)
    count = c_int64(0)
    _lib.check(_lib.lib().rt_tree_nni_moves(tree.nnodes, _ptr(idx, c_int64), _ptr(ptr, c_int64),
                                            None, 0, byref(count)))
    moves = np.zeros((count.value, 3), dtype=np.int32)
    if count.value:
        _lib.check(_lib.lib().rt_tree_nni_moves(tree.nnodes, _ptr(idx, c_int64), _ptr(ptr, c_int64),
                                                _ptr(moves, c_int32), count.value, byref(count)))
    return moves


# TreeModel.spr_scores: moves int32[nmoves, 2] (TreeModel.spr_moves: the pruned node c and the
# node y below the target edge), fractions [R] as evaluated, sums [nmoves, R], values
# [nsites, nmoves, R] (or None) with values[i, mv, r] = log L_i(tree after move mv at fractions[r])
# - log L_i, status as Posteriors, best (move, r): the arg-max of sums, ties to the lowest index
# (None without moves)
SprScores = collections.namedtuple('SprScores', 'moves fractions sums values status best')


# TreeModel.spr_scores_mixture: as SprScores under the site-class mixture over the K rate sets,
# values[i, mv, r] = log sum_k c_k L_ik(tree after move mv at fractions[r]) - loglik[i]; loglik and
# status as MixtureNniScores
MixtureSprScores = collections.namedtuple('MixtureSprScores',
                                          'moves fractions sums values loglik status best')


def _spr_radius(radius):
    """radius=None (no limit) or an int >= 0 -> the radius of the C ABI (-1: no limit)."""
    if radius is None:
        return -1
    if isinstance(radius, bool) or int(radius) != radius or radius < 0:
        raise ValueError('the radius is None (no limit) or an integer >= 0, not %r' % (radius,))
    return int(radius)


def tree_spr_moves(tree, radius=None):
    """rt_tree_spr_moves: the moves TreeModel.spr_moves lists, int32[nmoves, 2], from a
    TreeArrays alone (host only: no context, no model)."""
    rad = _spr_radius(radius)
    idx = np.ascontiguousarray(tree.indices, dtype=np.int64)
    ptr = np.ascontiguousarray(tree.indptr, dtype=np.int64)
    count = c_int64(0)
    _lib.check(_lib.lib().rt_tree_spr_moves(tree.nnodes, _ptr(idx, c_int64), _ptr(ptr, c_int64),
                                            rad, None, 0, byref(count)))
    moves = np.zeros((count.value, 2), dtype=np.int32)
    if count.value:
        _lib.check(_lib.lib().rt_tree_spr_moves(tree.nnodes, _ptr(idx, c_int64), _ptr(ptr, c_int64),
                                                rad, _ptr(moves, c_int32), count.value,
                                                byref(count)))
    return moves


# TreeModel.place_queries: fractions [R] and pendant [K] as evaluated, sums [Q, nnodes, R, K],
# values [nsites, Q, nnodes, R, K] (or None) with values[i, q, v, r, k] = log L_i(tree with query q
# placed at (v, fractions[r], pendant[k])) - log L_i (the root's row: 0), status as Posteriors,
# best int[Q, 3]: the arg-max (v, r, k) of sums per query, ties to the lowest index
Placements = collections.namedtuple('Placements', 'fractions pendant sums values status best')


# TreeModel.place_queries_mixture: as Placements under the site-class mixture over the K rate sets,
# pendant_scale [K] as evaluated, values[i, q, v, r, j] = log sum_k c_k L_ik(tree with query q placed
# at (v, fractions[r], pendant_scale[k] pendant[j])) - loglik[i]; loglik and status as
# MixtureNniScores
MixturePlacements = collections.namedtuple(
    'MixturePlacements', 'fractions pendant pendant_scale sums values loglik status best')


def check_placement_grid(fractions, pendant):
    """The attachment grid of TreeModel.place_queries -> (fractions f64[R], pendant f64[K]),
    C-contiguous, for rt_sites_placements.  ValueError unless both are 1-D sequences of numbers,
    1 <= R <= RT_MAX_PLACE_FRACTIONS, 1 <= K <= RT_MAX_PLACE_PENDANT, 2 R + K <= 32, every
    fraction finite and in [0, 1], every pendant length finite and not negative."""
    out = []
    for name, seq in (('fractions', fractions), ('pendant', pendant)):
        if seq is None:
            raise ValueError('%s is None' % name)
        try:
            x = np.array(seq, dtype=np.float64)
        except (TypeError, ValueError):
            raise ValueError('%s must be a 1-D sequence of numbers' % name)
        if x.ndim != 1:
            raise ValueError('%s must be 1-D, not %s' % (name, x.shape))
        out.append(np.ascontiguousarray(x))
    f, t = out
    if not 1 <= len(f) <= _lib.RT_MAX_PLACE_FRACTIONS:
        raise ValueError('between 1 and %d fractions (%d here)'
                         % (_lib.RT_MAX_PLACE_FRACTIONS, len(f)))
    if not 1 <= len(t) <= _lib.RT_MAX_PLACE_PENDANT:
        raise ValueError('between 1 and %d pendant lengths (%d here)'
                         % (_lib.RT_MAX_PLACE_PENDANT, len(t)))
    if 2 * len(f) + len(t) > 32:
        raise ValueError('2 * fractions + pendant lengths is at most 32 (%d here)'
                         % (2 * len(f) + len(t)))
    if not (np.isfinite(f).all() and (f >= 0).all() and (f <= 1).all()):
        raise ValueError('the fractions must be finite and in [0, 1]')
    if not (np.isfinite(t).all() and (t >= 0).all()):
        raise ValueError('the pendant lengths must be finite and not negative')
    return f, t


def check_draws(ndraws, seed, first_draw):
    """The draw arguments of sample_states / sample_mappings as ints; ValueError unless there is
    at least one draw and the seed and every draw number fit an unsigned 64-bit integer."""
    ndraws, seed, first_draw = int(ndraws), int(seed), int(first_draw)
    if ndraws < 1:
        raise ValueError('ndraws must be at least 1')
    if not (0 <= seed < 1 << 64 and 0 <= first_draw and first_draw + ndraws <= 1 << 64):
        raise ValueError('seed and draw numbers are unsigned 64-bit integers')
    return ndraws, seed, first_draw


def check_rate_sets(Q, t, node_q, nstates, nnodes):
    """The arguments of TreeModel.set_rate_sets -> (Q f64[K, nq, n, n], t f64[K, nnodes],
    node_q int64[nnodes] or None).  Q is [K, n, n] or [K, nq, n, n]; t is [K, nnodes], or
    [nnodes] (broadcast to every set).  ValueError for another shape, no set or more than
    RT_MAX_RATE_SETS of them, several matrices per set without a node_q, or a node_q that is
    not one index in [0, nq) per node."""
    Q = np.asarray(Q, dtype=np.float64)
    if Q.ndim == 3:
        Q = Q[:, None]
    if Q.ndim != 4 or Q.shape[2:] != (nstates, nstates) or Q.shape[1] < 1:
        raise ValueError('Q must be [K, %d, %d] or [K, nq, %d, %d], not %s'
                         % (nstates, nstates, nstates, nstates, Q.shape))
    K, nq = Q.shape[:2]
    if not 1 <= K <= _lib.RT_MAX_RATE_SETS:
        raise ValueError('between 1 and %d rate sets per call (%d here)'
                         % (_lib.RT_MAX_RATE_SETS, K))
    t = np.asarray(t, dtype=np.float64)
    if t.shape == (nnodes,):
        t = np.broadcast_to(t, (K, nnodes))
    if t.shape != (K, nnodes):
        raise ValueError('t must be [%d, %d] or [%d], not %s' % (K, nnodes, nnodes, t.shape))
    if node_q is None:
        if nq != 1:
            raise ValueError('%d rate matrices per set need a node_q' % nq)
    else:
        node_q = np.ascontiguousarray(node_q, dtype=np.int64)
        if node_q.shape != (nnodes,):
            raise ValueError('node_q must have one entry per node')
        if ((node_q[1:] < 0) | (node_q[1:] >= nq)).any():
            raise ValueError('node_q out of range')
    return np.ascontiguousarray(Q), np.ascontiguousarray(t), node_q


def check_site_sets(site_sets, nsites, nsets=None):
    """The site_sets argument of TreeModel.upload_sites -> (int32[nsites], nsets).  One rate-set
    index per site, integers in [0, nsets); nsets None: one more than the largest index.
    ValueError for another shape, non-integers, an index out of range, or nsets outside
    1..RT_MAX_RATE_SETS."""
    a = np.asarray(site_sets)
    if a.shape != (nsites,):
        raise ValueError('site_sets must have one entry per site (%d), not %s' % (nsites, a.shape))
    if a.dtype == np.bool_ or not np.issubdtype(a.dtype, np.integer):
        raise ValueError('site_sets must be integers, not %s' % a.dtype)
    if nsites < 1:
        raise ValueError('a partitioned batch needs at least one site')
    if nsets is None:
        nsets = int(a.max()) + 1
    if int(nsets) != nsets or not 1 <= nsets <= _lib.RT_MAX_RATE_SETS:
        raise ValueError('between 1 and %d rate sets (%r here)' % (_lib.RT_MAX_RATE_SETS, nsets))
    if (a < 0).any() or (a >= nsets).any():
        raise ValueError('site_sets must lie in [0, %d)' % nsets)
    return np.ascontiguousarray(a, dtype=np.int32), int(nsets)


def check_class_weights(class_weights, nsets):
    """f64[K] mixture weights: finite, >= 0, not all zero (ValueError otherwise)."""
    c = np.ascontiguousarray(class_weights, dtype=np.float64)
    if c.shape != (nsets,):
        raise ValueError('one class weight per rate set expected (%d), not %s' % (nsets, c.shape))
    if not np.isfinite(c).all() or (c < 0).any() or not (c > 0).any():
        raise ValueError('the class weights must be finite, >= 0 and not all zero')
    return c


def check_pendant_scale(pendant_scale, nsets):
    """The per-class scale of the pendant lengths of TreeModel.place_queries_mixture -> f64[K]:
    under class k the query hangs on an edge of length pendant_scale[k] * pendant[j].  None gives
    ones (right where the classes differ in Q, Q_k = r_k Q, over shared lengths; with a shared Q
    and t_k = r_k t pass r_k).  ValueError for another shape or an entry that is negative or not
    finite."""
    if pendant_scale is None:
        return np.ones(nsets)
    try:
        s = np.ascontiguousarray(pendant_scale, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError('pendant_scale must be a sequence of %d numbers' % nsets)
    if s.shape != (nsets,):
        raise ValueError('one pendant scale per rate set expected (%d), not %s' % (nsets, s.shape))
    if not (np.isfinite(s).all() and (s >= 0).all()):
        raise ValueError('the pendant scales must be finite and not negative')
    return s


def _placement_queries(queries, kind, nsites, nstates):
    """The queries of TreeModel.place_queries and its _mixture and _partitioned forms as the C ABI
    takes them, (array, observation kind): 'dense' f64 [Q, nsites, n] or 'state' uint8 [Q, nsites]
    (255 or -1: unobserved), Q >= 1; ValueError otherwise ('mask' queries are not taken)."""
    S, n = nsites, nstates
    if kind == 'dense':
        q = np.ascontiguousarray(queries, dtype=np.float64)
        if q.ndim != 3 or q.shape[1:] != (S, n):
            raise ValueError('dense queries must be [Q, %d, %d], not %s' % (S, n, q.shape))
        code = _lib.RT_OBS_DENSE
    elif kind == 'state':
        q = np.asarray(queries)
        if q.ndim != 2 or q.shape[1] != S:
            raise ValueError('state queries must be [Q, %d], not %s' % (S, q.shape))
        q = _as_uint8_states(q, n)
        code = _lib.RT_OBS_STATE
    else:
        raise ValueError("queries of kind 'dense' or 'state', not %r" % (kind,))
    if q.shape[0] < 1:
        raise ValueError('at least one query')
    return q, code


def _mask_states(mask, nstates):
    return [s for s in range(nstates) if (int(mask[s >> 6]) >> (s & 63)) & 1]


def device_count():
    n = c_int(0)
    _lib.check(_lib.lib().rt_device_count(byref(n)))
    return n.value


class Context(object):
    """One HIP stream on one GPU.  Fails loudly without the library or a GPU."""

    def __init__(self, device=0):
        self._h = c_void_p()
        # models and chain batches of this context: the C objects refer to it, and
        # rt_ctx_destroy refuses while one of them lives, so close() closes them first
        # (objects that die in one garbage-collection cycle are finalised in any order)
        self._children = weakref.WeakSet()
        _lib.check(_lib.lib().rt_ctx_create(int(device), byref(self._h)))
        self.device = int(device)

    def close(self):
        if self._h and not _shutting_down:
            for child in list(self._children):
                child.close()
            _lib.check(_lib.lib().rt_ctx_destroy(self._h))
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def sync(self):
        _lib.check(_lib.lib().rt_ctx_sync(self._h))

    def set_option(self, key, value):
        """Per-context option (rt_ctx_set_option): 'jit' (-1 automatic / 0 / 1),
        'force_generic', 'jit_block_sites', 'jit_async', 'leaf_state_kernels', 'rescale' (power-of-two rescaling
        of the messages of batches uploaded from now on: trees whose likelihood underflows
        f64); value None = back to the process default."""
        _lib.check(_lib.lib().rt_ctx_set_option(
            self._h, key.encode(), -2 if value is None else int(value)))

    def set_timing(self, enabled):
        """False/0: off; True/1: every launch; N > 1: every N-th launch of each
        kernel (each HIP event pair costs a few microseconds of stream time)."""
        _lib.check(_lib.lib().rt_ctx_set_timing(self._h, int(enabled)))

    def reset_timing(self):
        _lib.check(_lib.lib().rt_ctx_reset_timing(self._h))

    def kernel_time(self, kernel):
        """(total_ms, launches, kernel name) accumulated since the last reset."""
        ms = c_double(0.0)
        cnt = c_int64(0)
        name = c_char_p()
        _lib.check(_lib.lib().rt_ctx_kernel_time(self._h, int(kernel), byref(ms),
                                                 byref(cnt), byref(name)))
        return ms.value, cnt.value, (name.value or b'').decode()

    # ---- reference-shaped, host-pointer entry points ----------------------

    def expm(self, Q, t, q_index=None, return_info=False):
        """P[b] = expm(Q[q_index[b]] * t[b]); Q is [n,n] or [nq,n,n]."""
        Q = _f64(Q)
        if Q.ndim == 2:
            Q = Q[None]
        if Q.ndim != 3 or Q.shape[1] != Q.shape[2]:
            raise ValueError('expected the array to be square')
        t = np.atleast_1d(_f64(t))
        n, nq, count = Q.shape[1], Q.shape[0], t.shape[0]
        P = np.empty((count, n, n), dtype=np.float64)
        info = np.zeros((count, 2), dtype=np.int32)
        qi = None if q_index is None else _i64(q_index)
        _lib.check(_lib.lib().rt_expm(
            self._h, n, count, _ptr(Q, c_double), nq,
            None if qi is None else _ptr(qi, c_int64), _ptr(t, c_double),
            _ptr(P, c_double), _ptr(info, c_int32)))
        return (P, info) if return_info else P

    def expm_spectral(self, A, lam, B, t, D=None):
        """P[b] = A diag(exp(lam t[b])) B, diagonal 1 where D == 0: the reference's
        getp_spectral_v2 (examples/p53/qtop.py:76-88) at all branch lengths in one launch."""
        A, lam, B = _f64(A), _f64(lam), _f64(B)
        n = lam.shape[0]
        if A.shape != (n, n) or B.shape != (n, n):
            raise ValueError('expected the array to be square')
        t = np.atleast_1d(_f64(t))
        D = None if D is None else _f64(D)
        if D is not None and D.shape != (n,):
            raise ValueError('D must have one entry per state')
        P = np.empty((t.shape[0], n, n), dtype=np.float64)
        _lib.check(_lib.lib().rt_expm_spectral(
            self._h, n, t.shape[0], _ptr(A, c_double), _ptr(lam, c_double), _ptr(B, c_double),
            None if D is None else _ptr(D, c_double), _ptr(t, c_double), _ptr(P, c_double)))
        return P

    def _pass_args(self, indices, indptr, esd, arr):
        indices, indptr, esd = _i64(indices), _i64(indptr), _f64(esd)
        nnodes, n = esd.shape[0], esd.shape[1]
        if arr.ndim == 2:
            nsites = 1
        elif arr.ndim == 3:
            nsites = arr.shape[0]
        else:
            raise ValueError('expected [nnodes,n] or [nsites,nnodes,n]')
        if arr.shape[-2:] != (nnodes, n):
            raise ValueError('array shape %s does not match (%d, %d)' % (
                arr.shape, nnodes, n))
        return indices, indptr, esd, nnodes, n, nsites

    def node_to_pset(self, indices, indptr, esd, state_mask):
        """In place on state_mask (int64, C-contiguous)."""
        self._mask_pass('rt_mcy_esd_get_node_to_pset', indices, indptr, esd,
                        state_mask)

    def node_to_set(self, indices, indptr, esd, state_mask):
        self._mask_pass('rt_esd_get_node_to_set', indices, indptr, esd,
                        state_mask)

    def _mask_pass(self, fn, indices, indptr, esd, state_mask):
        if (state_mask.dtype != np.int64 or
                not state_mask.flags['C_CONTIGUOUS']):
            raise ValueError('state_mask must be a C-contiguous int64 array')
        indices, indptr, esd, nnodes, n, nsites = self._pass_args(
            indices, indptr, esd, state_mask)
        _lib.check(getattr(_lib.lib(), fn)(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64),
            _ptr(indptr, c_int64), _ptr(esd, c_double),
            _ptr(state_mask, c_int64)))

    def node_to_pmap(self, indices, indptr, esd, state_mask, out,
                     obs_likelihood=None):
        if out.dtype != np.float64 or not out.flags['C_CONTIGUOUS']:
            raise ValueError('subtree_probability must be C-contiguous f64')
        state_mask = _i64(state_mask)
        indices, indptr, esd, nnodes, n, nsites = self._pass_args(
            indices, indptr, esd, state_mask)
        if out.shape != state_mask.shape:
            raise ValueError('shape mismatch')
        obs = None if obs_likelihood is None else _f64(obs_likelihood)
        if obs is not None and obs.shape != state_mask.shape:
            raise ValueError('shape mismatch')
        _lib.check(_lib.lib().rt_mcy_esd_get_node_to_pmap(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64),
            _ptr(indptr, c_int64), _ptr(esd, c_double),
            _ptr(state_mask, c_int64),
            None if obs is None else _ptr(obs, c_double), _ptr(out, c_double)))

    def passes(self, indices, indptr, esd, state_mask, out, obs_likelihood=None):
        """pset + set + pmap in one call (rt_mcy_esd_passes): state_mask (int64,
        C-contiguous) is updated in place, ``out`` receives the pmaps."""
        if (state_mask.dtype != np.int64 or not state_mask.flags['C_CONTIGUOUS']):
            raise ValueError('state_mask must be a C-contiguous int64 array')
        if out.dtype != np.float64 or not out.flags['C_CONTIGUOUS']:
            raise ValueError('subtree_probability must be C-contiguous f64')
        indices, indptr, esd, nnodes, n, nsites = self._pass_args(
            indices, indptr, esd, state_mask)
        if out.shape != state_mask.shape:
            raise ValueError('shape mismatch')
        obs = None
        if obs_likelihood is not None:
            obs = _f64(obs_likelihood)
            if obs.shape != state_mask.shape:
                raise ValueError('obs_likelihood shape mismatch')
        _lib.check(_lib.lib().rt_mcy_esd_passes(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64), _ptr(indptr, c_int64),
            _ptr(esd, c_double), _ptr(state_mask, c_int64),
            None if obs is None else _ptr(obs, c_double), _ptr(out, c_double)))

    def node_to_distn(self, indices, indptr, esd, root_distn, pmap):
        """Downward pass (mc0_esd_get_node_to_distn): returns (distn, status)."""
        pmap = _f64(pmap)
        indices, indptr, esd, nnodes, n, nsites = self._pass_args(
            indices, indptr, esd, pmap)
        out = np.empty(pmap.shape, dtype=np.float64)
        status = np.zeros(nsites, dtype=np.int32)
        rd = None if root_distn is None else _f64(root_distn)
        if rd is not None and rd.shape != (n,):
            raise ValueError('inconsistent root distribution')
        _lib.check(_lib.lib().rt_mc0_esd_get_node_to_distn(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64), _ptr(indptr, c_int64),
            _ptr(esd, c_double), None if rd is None else _ptr(rd, c_double),
            _ptr(pmap, c_double), _ptr(out, c_double), _ptr(status, c_int32)))
        return out, status

    def joint_endpoint_distn(self, indices, indptr, esd, pmap, distn):
        """mc0_esd_get_joint_endpoint_distn: f64[..., nnodes, n, n] keyed by
        the child index."""
        pmap, distn = _f64(pmap), _f64(distn)
        indices, indptr, esd, nnodes, n, nsites = self._pass_args(
            indices, indptr, esd, pmap)
        if distn.shape != pmap.shape:
            raise ValueError('shape mismatch')
        out = np.empty(pmap.shape + (n,), dtype=np.float64)
        _lib.check(_lib.lib().rt_mc0_esd_get_joint_endpoint_distn(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64), _ptr(indptr, c_int64),
            _ptr(esd, c_double), _ptr(pmap, c_double), _ptr(distn, c_double),
            _ptr(out, c_double)))
        return out

    def expectation_weights(self, indices, indptr, esd, root_distn, state_mask,
                            site_weights=None):
        """rt_mjp_esd_expectation_weights: upward passes + downward pass + per-edge
        site sums of J / P on the device.  Returns (W f64[nnodes, n, n] keyed by the
        child index, summed root posteriors f64[n], status int32[nsites])."""
        state_mask = _i64(state_mask)
        indices, indptr, esd, nnodes, n, nsites = self._pass_args(
            indices, indptr, esd, state_mask)
        rd = None if root_distn is None else _f64(root_distn)
        if rd is not None and rd.shape != (n,):
            raise ValueError('inconsistent root distribution')
        w = None if site_weights is None else _f64(site_weights)
        if w is not None and w.shape != (nsites,):
            raise ValueError('one weight per site expected')
        W = np.empty((nnodes, n, n), dtype=np.float64)
        status = np.zeros(nsites, dtype=np.int32)
        _lib.check(_lib.lib().rt_mjp_esd_expectation_weights(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64), _ptr(indptr, c_int64),
            _ptr(esd, c_double), None if rd is None else _ptr(rd, c_double),
            _ptr(state_mask, c_int64), None if w is None else _ptr(w, c_double),
            _ptr(W, c_double), _ptr(status, c_int32)))
        root_post = W[0, :, 0].copy()
        W[0] = 0.0
        return W, root_post, status

    def expectation_weights_obs(self, indices, indptr, esd, root_distn, obs_nodes, data,
                                kind, site_weights=None):
        """rt_mjp_esd_expectation_weights_obs: as expectation_weights, from compact
        observations -- ``data`` [nsites, len(obs_nodes)] uint8 states (kind='state')
        or uint64 allowed-set masks (kind='mask'); obs_nodes are preorder indices."""
        indices, indptr, esd = _i64(indices), _i64(indptr), _f64(esd)
        nnodes, n = esd.shape[0], esd.shape[1]
        obs_nodes = _i64(obs_nodes)
        if kind == 'state':
            data = _as_uint8_states(data, n)
            code = _lib.RT_OBS_STATE
        elif kind == 'mask':
            data = np.ascontiguousarray(data, dtype=np.uint64)
            code = _lib.RT_OBS_MASK
        else:
            raise ValueError("kind must be 'state' or 'mask'")
        if data.ndim != 2 or data.shape[1] != obs_nodes.shape[0]:
            raise ValueError('data must be [nsites, len(obs_nodes)]')
        nsites = data.shape[0]
        rd = None if root_distn is None else _f64(root_distn)
        if rd is not None and rd.shape != (n,):
            raise ValueError('inconsistent root distribution')
        w = None if site_weights is None else _f64(site_weights)
        if w is not None and w.shape != (nsites,):
            raise ValueError('one weight per site expected')
        W = np.empty((nnodes, n, n), dtype=np.float64)
        status = np.zeros(nsites, dtype=np.int32)
        _lib.check(_lib.lib().rt_mjp_esd_expectation_weights_obs(
            self._h, nnodes, n, nsites, _ptr(indices, c_int64), _ptr(indptr, c_int64),
            _ptr(esd, c_double), None if rd is None else _ptr(rd, c_double),
            obs_nodes.shape[0], _ptr(obs_nodes, c_int64), code,
            data.ctypes.data_as(c_void_p), None if w is None else _ptr(w, c_double),
            _ptr(W, c_double), _ptr(status, c_int32)))
        root_post = W[0, :, 0].copy()
        W[0] = 0.0
        return W, root_post, status

    def frechet_statistics(self, Qs, q_index, t, W):
        """rt_mjp_frechet_statistics: per edge e the Frechet derivative
        M_e = L(t[e] Q[q_index[e]]^T, W[e]) on the device, contracted over the edges:
        returns (dwell f64[n], trans f64[n, n])."""
        Qs = _f64(Qs)
        if Qs.ndim == 2:
            Qs = Qs[None]
        W = _f64(W)
        t = np.atleast_1d(_f64(t))
        nq, n = Qs.shape[0], Qs.shape[1]
        nedges = t.shape[0]
        if Qs.shape[1:] != (n, n) or W.shape != (nedges, n, n):
            raise ValueError('expected Q [nq, n, n], W [nedges, n, n], t [nedges]')
        qi = _i64(q_index)
        if qi.shape != (nedges,):
            raise ValueError('one rate-matrix index per edge expected')
        dwell = np.zeros(n, dtype=np.float64)
        trans = np.zeros((n, n), dtype=np.float64)
        _lib.check(_lib.lib().rt_mjp_frechet_statistics(
            self._h, n, nedges, _ptr(Qs, c_double), nq, _ptr(qi, c_int64), _ptr(t, c_double),
            _ptr(W, c_double), _ptr(dwell, c_double), _ptr(trans, c_double)))
        return dwell, trans

    # ---- multi-GPU ---------------------------------------------------------

    @staticmethod
    def comm_available():
        """True iff librccl can be loaded (no GPU / network touched)."""
        return _lib.lib().rt_comm_available() == _lib.RT_OK

    @staticmethod
    def comm_unique_id():
        buf = (ctypes.c_ubyte * 128)()
        _lib.check(_lib.lib().rt_comm_unique_id(buf))
        return bytes(buf)

    def comm_init(self, nranks, rank, uid):
        buf = (ctypes.c_ubyte * 128).from_buffer_copy(uid)
        _lib.check(_lib.lib().rt_comm_init(self._h, int(nranks), int(rank), buf))

    def comm_destroy(self):
        _lib.check(_lib.lib().rt_comm_destroy(self._h))


_contexts = {}


def get_context(device=0):
    ctx = _contexts.get(device)
    if ctx is None:
        ctx = _contexts[device] = Context(device)
    return ctx


class SiteBatch(object):
    def __init__(self, model, handle, nsites, site_sets=None, nsets=0):
        self.model = model
        self._h = handle
        self.nsites = nsites
        # a partitioned batch (upload_sites(..., site_sets=...)): the rate set of every site,
        # int32[nsites], and the number of sets; None / 0 for an ordinary batch
        self.site_sets = site_sets
        self.nsets = nsets
        self._weights = None      # what set_weights gave last (None: every site counts once)
        # the C object refers to its model: when both die in one garbage-collection cycle
        # (a traceback kept them alive) the model may be finalised first, so the model closes
        # its batches before it goes
        model._batches.add(self)

    def clone(self):
        h = c_void_p()
        _lib.check(_lib.lib().rt_sites_clone(self._h, byref(h)))
        return SiteBatch(self.model, h, self.nsites)

    @property
    def device_bytes(self):
        return _lib.lib().rt_sites_device_bytes(self._h)

    @property
    def jit_compile_seconds(self):
        """hiprtc seconds spent for this batch's tree-specialised kernel (0: none
        compiled, or it came from the cache)."""
        return _lib.lib().rt_sites_jit_compile_seconds(self._h)

    @property
    def kernel_name(self):
        return (_lib.lib().rt_sites_kernel_name(self._h) or b'').decode()

    @property
    def multi_kernel_name(self):
        """The batch's kernel of the last step_multi plus ',loop' (one launch per rate set) or
        ',multi' (one launch for all sets); '' before the first step_multi."""
        return (_lib.lib().rt_sites_multi_kernel_name(self._h) or b'').decode()

    def set_weights(self, weights=None):
        """Per-site multiplicities for expected_history_statistics (site patterns);
        None = every site counts once."""
        if weights is None:
            _lib.check(_lib.lib().rt_sites_set_weights(self._h, None))
            self._weights = None
            return self
        w = _f64(weights)
        if w.shape != (self.nsites,):
            raise ValueError('one weight per site expected')
        _lib.check(_lib.lib().rt_sites_set_weights(self._h, _ptr(w, c_double)))
        self._weights = w.copy()
        return self

    def _root_likelihoods(self, nstates):
        """One-node tree: the root's observation per site as likelihoods f64[nsites, n]
        (ones where the root is unobserved)."""
        L = np.ones((self.nsites, nstates))
        kind, idx, data = getattr(self, '_host_obs', ('dense', [], None))
        for j, v in enumerate(idx):
            if v != 0:
                continue
            if kind == 'dense':
                L *= data[:, j, :]
            elif kind == 'state':
                col = data[:, j].astype(np.int64)
                obs = col < nstates
                onehot = np.zeros((self.nsites, nstates))
                onehot[np.nonzero(obs)[0], col[obs]] = 1.0
                onehot[~obs] = 1.0
                L *= onehot
            else:
                words = data[:, j] if data.ndim == 2 else data[:, j, :]
                words = words.reshape(self.nsites, -1)
                for s in range(nstates):
                    bit = (words[:, s >> 6] >> np.uint64(s & 63)) & np.uint64(1)
                    L[:, s] *= bit.astype(np.float64)
        return L

    def wait_for_kernel(self):
        """Block until the background compile of this batch's tree-specialised kernel (if
        one is pending: rt_set_option 'jit_async') has finished and the batch has switched
        to it; until then it runs the interpreter kernel, with the same results."""
        _lib.check(_lib.lib().rt_sites_jit_wait(self._h))
        return self

    def close(self):
        if self._h and not _shutting_down:
            _lib.lib().rt_sites_destroy(self._h)
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class TreeModel(object):
    """Tree + per-edge transition matrices resident on one GPU."""

    def __init__(self, T, root, nstates, ctx=None):
        self.ctx = ctx if ctx is not None else get_context()
        self.tree = T if isinstance(T, TreeArrays) else TreeArrays(T, root)
        self.nstates = int(nstates)
        self._h = c_void_p()
        self._batches = weakref.WeakSet()
        self._root_w = None             # what set_root_distn sent (the one-node posteriors)
        ta = self.tree
        _lib.check(_lib.lib().rt_model_create(
            self.ctx._h, ta.nnodes, self.nstates, _ptr(ta.indices, c_int64),
            _ptr(ta.indptr, c_int64), byref(self._h)))
        self.ctx._children.add(self)

    def close(self):
        for batch in list(getattr(self, '_batches', ())):
            batch.close()
        if self._h and not _shutting_down:
            _lib.check(_lib.lib().rt_model_destroy(self._h))
            self._h = c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def schedule_depth(self):
        return _lib.lib().rt_model_schedule_depth(self._h)

    def set_rates(self, Q_default=None, Q=None, node_q=None, t=None):
        """expm(Q*t) for every edge on the device.  Either pass nothing but
        Q_default (edge 'Q' attributes override it, _mjp_dense.py:355) or the
        explicit arrays Q [nq,n,n], node_q [nnodes], t [nnodes]."""
        if Q is None:
            Q, node_q = self.tree.rate_matrices(self.nstates, Q_default)
        else:
            Q = _f64(Q)
            if Q.ndim == 2:
                Q = Q[None]
            if Q.shape[1:] != (self.nstates, self.nstates):
                raise ValueError('expected the array to be square')
        if t is None:
            t = self.tree.branch_lengths()
        t = _f64(t)
        nq = _i64(node_q) if node_q is not None else None
        if t.shape != (self.tree.nnodes,):
            raise ValueError('t must have one entry per node')
        _lib.check(_lib.lib().rt_model_set_rates(
            self._h, _ptr(Q, c_double), Q.shape[0],
            None if nq is None else _ptr(nq, c_int64), _ptr(t, c_double)))
        self._rates = (Q.copy(), t.copy())      # (branch_length_gradient builds its E from Q)

    def set_rates_spectral(self, A, lam, B, D=None, t=None):
        """One time-reversible rate matrix given by its spectral decomposition
        (raoteh_amd._spectral.decompose_spectral_v2, examples/p53/qtop.py:128-152): every
        edge's P = A diag(exp(lam t)) B on the device, now and at every later step()."""
        A, lam, B = _f64(A), _f64(lam), _f64(B)
        n = self.nstates
        if A.shape != (n, n) or B.shape != (n, n) or lam.shape != (n,):
            raise ValueError('expected the array to be square')
        D = None if D is None else _f64(D)
        if D is not None and D.shape != (n,):
            raise ValueError('D must have one entry per state')
        if t is None:
            t = self.tree.branch_lengths()
        t = _f64(t)
        if t.shape != (self.tree.nnodes,):
            raise ValueError('t must have one entry per node')
        _lib.check(_lib.lib().rt_model_set_rates_spectral(
            self._h, _ptr(A, c_double), _ptr(lam, c_double), _ptr(B, c_double),
            None if D is None else _ptr(D, c_double), _ptr(t, c_double)))
        self._rates = None

    def recompute_transitions(self):
        _lib.check(_lib.lib().rt_model_recompute_transitions(self._h))

    def set_transitions(self, esd):
        esd = _f64(esd)
        if esd.shape != (self.tree.nnodes, self.nstates, self.nstates):
            raise ValueError('esd_transitions has the wrong shape')
        _lib.check(_lib.lib().rt_model_set_transitions(self._h,
                                                       _ptr(esd, c_double)))

    def get_transitions(self):
        esd = np.empty((self.tree.nnodes, self.nstates, self.nstates))
        _lib.check(_lib.lib().rt_model_get_transitions(self._h,
                                                       _ptr(esd, c_double)))
        return esd

    def expm_info(self):
        info = np.zeros((self.tree.nnodes, 2), dtype=np.int32)
        _lib.check(_lib.lib().rt_model_get_expm_info(self._h,
                                                     _ptr(info, c_int32)))
        return info

    def set_root_distn(self, root_distn=None):
        if root_distn is None:
            _lib.check(_lib.lib().rt_model_set_root_distn(self._h, None))
            self._root_w = None
            return
        w = _f64(root_distn)
        if w.shape != (self.nstates,):
            raise ValueError('root shape mismatch: %s %s' % (
                (self.nstates,), w.shape))
        _lib.check(_lib.lib().rt_model_set_root_distn(self._h,
                                                      _ptr(w, c_double)))
        self._root_w = w.copy()

    def upload_sites(self, obs_nodes, data, kind='dense', site_sets=None, nsets=None):
        """obs_nodes: tree nodes (nx ids) carrying per-site data, in the order
        of the data's second axis.  data: dense f64[nsites,nobs,n] | state
        uint8[nsites,nobs] (255 = unobserved) | mask uint64[nsites,nobs] (nstates
        <= 64) or uint64[nsites,nobs,ceil(nstates/64)] (bit s % 64 of word s // 64).
        site_sets (int[nsites], with nsets or one more than its maximum): a PARTITIONED batch
        (rt_sites_create_partitioned) -- site i is evaluated under rate set site_sets[i] of
        set_rate_sets by step_partitioned and read by branch_expectations_partitioned /
        branch_length_gradient_partitioned, and by nothing else."""
        code = _KINDS[kind]
        idx = _i64([self.tree.node_to_index[v] for v in obs_nodes])
        if kind == 'dense':
            data = _f64(data)
            ok = data.ndim == 3 and data.shape[2] == self.nstates
        elif kind == 'state':
            data = _as_uint8_states(data, self.nstates)
            ok = data.ndim == 2
        else:
            # one 64-bit word per node for nstates <= 64, ceil(nstates / 64) words above
            data = np.ascontiguousarray(data, dtype=np.uint64)
            words = (self.nstates + 63) // 64
            ok = (data.ndim == 2 and words == 1) or (data.ndim == 3 and data.shape[2] == words)
        if not ok or data.shape[1] != len(idx):
            raise ValueError('observation array has the wrong shape')
        nsites = data.shape[0]
        h = c_void_p()
        if site_sets is not None:
            sets, nsets = check_site_sets(site_sets, nsites, nsets)
            _lib.check(_lib.lib().rt_sites_create_partitioned(
                self._h, nsites, code, len(idx), _ptr(idx, c_int64),
                data.ctypes.data_as(c_void_p), _ptr(sets, c_int32), nsets, byref(h)))
            return SiteBatch(self, h, nsites, sets, nsets)
        _lib.check(_lib.lib().rt_sites_create(
            self._h, nsites, code, len(idx), _ptr(idx, c_int64),
            data.ctypes.data_as(c_void_p), byref(h)))
        batch = SiteBatch(self, h, nsites)
        if self.tree.nnodes == 1:       # posteriors() answers a one-node tree on the host
            batch._host_obs = (kind, idx, data.copy())
        return batch

    def prune(self, batch):
        """Asynchronous: upward pass + root reduce + batch sum on the device."""
        _lib.check(_lib.lib().rt_prune(self._h, batch._h))

    def step(self, batch, recompute_transitions=True):
        """One iteration of a repeated-evaluation loop in one call (rt_step):
        per-edge expm from the resident rates (optional) + prune; asynchronous."""
        _lib.check(_lib.lib().rt_step(self._h, batch._h,
                                      1 if recompute_transitions else 0))

    def set_rate_sets(self, Q, t=None, node_q=None):
        """K rate sets next to the rates set_rates owns (rt_model_set_rate_sets): Q [K, n, n]
        or [K, nq, n, n] with node_q [nnodes] shared by all sets, t [K, nnodes], or [nnodes] /
        None (the tree's branch lengths) for every set.  expm(Q t) of every edge of every set
        in one launch; the model's own transitions do not change."""
        if t is None:
            t = self.tree.branch_lengths()
        Q, t, node_q = check_rate_sets(Q, t, node_q, self.nstates, self.tree.nnodes)
        _lib.check(_lib.lib().rt_model_set_rate_sets(
            self._h, Q.shape[0], _ptr(Q, c_double), Q.shape[1],
            None if node_q is None else _ptr(node_q, c_int64), _ptr(t, c_double)))
        self._nsets = Q.shape[0]
        # (branch_length_gradient_partitioned builds each set's E from its Q)
        self._rate_sets = (Q.copy(), t.copy())

    def step_multi(self, batch, recompute_transitions=True):
        """rt_step_multi: (the exponentials of every rate set again +) one pruning of the batch
        per rate set + K batch sums; asynchronous.  The batch's own results stay."""
        _lib.check(_lib.lib().rt_step_multi(self._h, batch._h,
                                            1 if recompute_transitions else 0))

    def fetch_multi_log_likelihoods(self, batch):
        """(loglik f64[K, nsites], status int32[K, nsites]) of the last step_multi."""
        K = getattr(self, '_nsets', 0)
        ll = np.empty((max(K, 1), batch.nsites), dtype=np.float64)
        st = np.empty((max(K, 1), batch.nsites), dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_get_multi_logliks(
            batch._h, _ptr(ll, c_double), _ptr(st, c_int32)))
        return ll, st

    def fetch_multi_totals(self, batch, weighted=False):
        """totals f64[K, 3] (per set: what fetch_totals gives after a separate step with that
        set); weighted=True: (totals, weighted_sums f64[K]) with the batch's site weights."""
        K = getattr(self, '_nsets', 0)
        tot = np.zeros((max(K, 1), 3), dtype=np.float64)
        ws = np.zeros(max(K, 1), dtype=np.float64)
        _lib.check(_lib.lib().rt_sites_get_multi_totals(
            batch._h, _ptr(tot, c_double), _ptr(ws, c_double) if weighted else None))
        return (tot, ws) if weighted else tot

    def step_partitioned(self, batch, recompute_transitions=True):
        """rt_step_partitioned on a batch uploaded with site_sets: (the exponentials of every
        rate set again +) ONE pruning launch in which every site reads the tables of its own
        set + the per-set sums; asynchronous.  fetch_log_likelihoods / fetch_totals /
        fetch_partition_totals read the results (caller order, real sites only)."""
        _lib.check(_lib.lib().rt_step_partitioned(self._h, batch._h,
                                                  1 if recompute_transitions else 0))

    def fetch_partition_totals(self, batch, weighted=False):
        """totals f64[nsets, 3] of the last step_partitioned (per set: what fetch_totals means,
        over that set's sites; zeros for an empty set); weighted=True: (totals, weighted_sums
        f64[nsets]) with the batch's site weights (caller order)."""
        K = max(int(getattr(batch, 'nsets', 0) or 0), 1)
        tot = np.zeros((K, 3), dtype=np.float64)
        ws = np.zeros(K, dtype=np.float64)
        _lib.check(_lib.lib().rt_sites_get_partition_totals(
            batch._h, _ptr(tot, c_double), _ptr(ws, c_double) if weighted else None))
        return (tot, ws) if weighted else tot

    def mixture_log_likelihoods(self, batch, class_weights):
        """Per site log sum_k c_k exp(loglik[k]) over the rate sets of the last step_multi
        (site-class models): (loglik f64[nsites], status int32[nsites], totals f64[3])."""
        c = check_class_weights(class_weights, getattr(self, '_nsets', 0))
        ll = np.empty(batch.nsites, dtype=np.float64)
        st = np.empty(batch.nsites, dtype=np.int32)
        tot = np.zeros(3, dtype=np.float64)
        _lib.check(_lib.lib().rt_sites_multi_mixture(
            batch._h, _ptr(c, c_double), _ptr(ll, c_double), _ptr(st, c_int32),
            _ptr(tot, c_double)))
        return ll, st, tot

    def expected_history_statistics(self, batch, recompute_transitions=True,
                                    return_status=False):
        """rt_expect_step: the reference's get_expected_history_statistics
        (_mjp_dense.py:410-539) summed over the resident batch -- (dwell f64[n], summed
        root posteriors f64[n], transitions f64[n, n]) -- with nothing but those numbers
        crossing PCIe.  Rates must have been set with set_rates; nstates <=
        RT_MAX_EXPECT_STEP_STATES (128: every batch of the matrix-pipe layout; for
        nstates <= 4 a dense batch is read as allowed sets: likelihood != 0)."""
        n = self.nstates
        dwell = np.empty(n)
        rootp = np.empty(n)
        trans = np.empty((n, n))
        status = np.zeros(batch.nsites, dtype=np.int32) if return_status else None
        _lib.check(_lib.lib().rt_expect_step(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(dwell, c_double),
            _ptr(rootp, c_double), _ptr(trans, c_double),
            None if status is None else _ptr(status, c_int32)))
        return (dwell, rootp, trans, status) if return_status else (dwell, rootp, trans)

    def _root_weights(self, batch):
        """One-node trees are answered on the host: the root's observation times the root
        weights, f64[nsites, n]."""
        n = self.nstates
        return batch._root_likelihoods(n) * (np.ones(n) if self._root_w is None else self._root_w)

    def posteriors(self, batch, node_sets=(), edge_sets=(), marginal_nodes=None, marginals=False,
                   recompute_transitions=False):
        """rt_sites_posteriors: _mcy_dense.kitchen_sink (_mcy_dense.py:57-230) for every site of
        the resident batch, reduced on the device.  node_sets: iterables of states S (the posterior
        probability of S at every node); edge_sets: pairs (A, B) (the joint posterior probability
        of A at the parent and B at the child, per edge); marginals=True or marginal_nodes (tree
        nodes): the full posterior marginals of those nodes (all nodes when marginal_nodes is
        None).  At most RT_MAX_POSTERIOR_SETS (8) sets of each kind.  Returns a Posteriors tuple;
        its arrays are indexed by `nodes` (the preorder)."""
        n = self.nstates
        ta = self.tree
        nsets = [states_to_mask(S, n) for S in node_sets]
        esets = []
        for pair in edge_sets:
            A, B = pair
            esets.append(np.concatenate([states_to_mask(A, n), states_to_mask(B, n)]))
        lim = _lib.RT_MAX_POSTERIOR_SETS
        if len(nsets) > lim or len(esets) > lim:
            raise ValueError('at most %d node sets and %d edge sets' % (lim, lim))
        want_marg = marginals or marginal_nodes is not None
        if marginal_nodes is None:
            mnodes = list(ta.preorder_nodes) if want_marg else []
        else:
            mnodes = list(marginal_nodes)
            for v in mnodes:
                if v not in ta.node_to_index:
                    raise ValueError('node %r is not in the tree' % (v,))
        N, S = ta.nnodes, batch.nsites
        node_values = np.zeros((S, N, len(nsets)))
        edge_values = np.zeros((S, N, len(esets)))
        marg = np.zeros((S, len(mnodes), n)) if want_marg else None
        status = np.zeros(S, dtype=np.int32)
        nodes = list(ta.preorder_nodes)
        if N == 1:
            # one node: the posterior is the normalised root weights times the root's
            # observation (kitchen_sink's len(T) == 1 case), no edges
            wl = self._root_weights(batch)
            tot = wl.sum(axis=1)
            ok = tot > 0
            status[~ok] = _lib.RT_SITE_ZERO_PROB
            D = np.zeros_like(wl)
            D[ok] = wl[ok] / tot[ok][:, None]
            for k, m in enumerate(nsets):
                node_values[:, 0, k] = D[:, _mask_states(m, n)].sum(axis=1)
            if want_marg:
                marg[:, :, :] = D[:, None, :]
            return Posteriors(node_values, edge_values, marg, status, nodes, mnodes)
        nmask = np.ascontiguousarray(np.array(nsets, dtype=np.uint64).reshape(-1, 2))
        emask = np.ascontiguousarray(np.array(esets, dtype=np.uint64).reshape(-1, 2, 2))
        # (the device writes each node once: a node listed twice is copied here)
        uniq = list(dict.fromkeys(mnodes))
        if len(uniq) != len(mnodes):
            marg = np.zeros((S, len(uniq), n))
        midx = _i64([ta.node_to_index[v] for v in uniq])
        _lib.check(_lib.lib().rt_sites_posteriors(
            self._h, batch._h, 1 if recompute_transitions else 0,
            len(nsets), nmask.ctypes.data_as(c_void_p) if len(nsets) else None,
            len(esets), emask.ctypes.data_as(c_void_p) if len(esets) else None,
            len(uniq), _ptr(midx, c_int64) if len(uniq) else None,
            _ptr(node_values, c_double) if len(nsets) else None,
            _ptr(edge_values, c_double) if len(esets) else None,
            _ptr(marg, c_double) if want_marg and len(mnodes) else None,
            _ptr(status, c_int32)))
        if len(uniq) != len(mnodes):
            marg = marg[:, [uniq.index(v) for v in mnodes]]
        return Posteriors(node_values, edge_values, marg, status, nodes, mnodes)

    def sample_states(self, batch, ndraws=1, seed=0, first_draw=0, recompute_transitions=False):
        """rt_sites_sample_states: _sample_mcy_dense.resample_states
        (_sample_mcy_dense.py:23-69) for every site of the resident batch, `ndraws` joint draws of
        a state for every node from the posterior.  The uniform of draw d, site i, preorder node
        v is _philox.philox_uniform(seed, first_draw + d, i * nnodes + v): draws [f, f + k) of one
        call are draws [0, k) of a call with first_draw = f.  Returns a SampledStates tuple."""
        ndraws, seed, first_draw = check_draws(ndraws, seed, first_draw)
        n = self.nstates
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        nodes = list(ta.preorder_nodes)
        states = np.full((ndraws, S, N), 255, dtype=np.uint8)
        status = np.zeros(S, dtype=np.int32)
        if N == 1:
            # one node: the root weights times the root's observation, on the host with the
            # device's uniform and rule (the first state whose cumulative weight exceeds u * total)
            from ._philox import philox_uniform
            w = self._root_weights(batch).clip(min=0)
            cdf = np.cumsum(w, axis=1)
            total = cdf[:, -1]
            ok = (total > 0) & np.isfinite(total)
            status[~ok] = _lib.RT_SITE_ZERO_PROB
            d = np.arange(first_draw, first_draw + ndraws, dtype=np.uint64)
            u = philox_uniform(seed, d[:, None], np.arange(S, dtype=np.uint64)[None, :])
            for i in np.nonzero(ok)[0]:
                pos = np.nonzero(w[i] > 0)[0]
                k = np.searchsorted(cdf[i, pos], u[:, i] * total[i], side='right')
                states[:, i, 0] = pos[np.minimum(k, len(pos) - 1)]
            return SampledStates(states, status, nodes)
        _lib.check(_lib.lib().rt_sites_sample_states(
            self._h, batch._h, 1 if recompute_transitions else 0, seed, first_draw, ndraws,
            _ptr(states, ctypes.c_ubyte), _ptr(status, c_int32)))
        return SampledStates(states, status, nodes)

    def map_states(self, batch, recompute_transitions=False):
        """rt_sites_map_states: the joint maximum-likelihood reconstruction (Pupko et al. 2000)
        of every site of the resident batch: the one assignment x of a state to every node that
        maximises J(x) = w[x_root] prod_v o_v[x_v] prod_{v != root} P_v[x_parent(v), x_v] (o_v the
        observation of v, w the root weights), ties always to the lowest state index, and
        log_joint = log J(x).  It is not the arg-max of the marginals of posteriors(...,
        marginals=True), which need not even be a possible history.  The posterior probability of
        the reconstruction of site i is exp(log_joint[i] - log-likelihood of site i), the second
        from log_likelihoods(batch).  Returns a MapStates tuple."""
        n = self.nstates
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        nodes = list(ta.preorder_nodes)
        states = np.full((S, N), 255, dtype=np.uint8)
        log_joint = np.full(S, -np.inf)
        status = np.zeros(S, dtype=np.int32)
        if N == 1:
            # one node: the lowest state that maximises the root weights times the observation
            w = self._root_weights(batch)
            w = np.where(w > 0, w, 0.0)
            best = w.max(axis=1)
            ok = (best > 0) & np.isfinite(best)
            status[~ok] = _lib.RT_SITE_ZERO_PROB
            states[ok, 0] = np.argmax(w[ok], axis=1)
            log_joint[ok] = np.log(best[ok])
            return MapStates(states, log_joint, status, nodes)
        _lib.check(_lib.lib().rt_sites_map_states(
            self._h, batch._h, 1 if recompute_transitions else 0,
            _ptr(states, ctypes.c_ubyte), _ptr(log_joint, c_double), _ptr(status, c_int32)))
        return MapStates(states, log_joint, status, nodes)

    def sample_mappings(self, batch, coefs, ndraws=1, seed=0, first_draw=0, per_draw=True,
                        recompute_transitions=False):
        """rt_sites_sample_mappings: `ndraws` stochastic mappings of every site of the resident
        batch: the node states of sample_states(batch, ndraws, seed, first_draw), then on every
        branch an endpoint-conditioned path by uniformization with that edge's Q and t, reduced
        to the statistics of branch_expectations: coefs is one (n, n) array E or up to 8 of them,
        E[c, d] the weight of a c -> d change, E[c, c] of a unit of time in c.  Returns a
        SampledMappings tuple; with per_draw=False values and counts are None (they never leave
        the device) and only the means over the draws come back.  The means converge to
        branch_expectations(batch, coefs).values.  The rates must have been set with set_rates."""
        ndraws, seed, first_draw = check_draws(ndraws, seed, first_draw)
        n = self.nstates
        E = check_branch_coefs(coefs, n)
        K = E.shape[0]
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        nodes = list(ta.preorder_nodes)
        values = np.zeros((ndraws, S, N, K)) if per_draw else None
        counts = np.zeros((ndraws, S, N, 2), dtype=np.int32) if per_draw else None
        means = np.zeros((S, N, K))
        if N == 1:
            # one node, no edges: the states as sample_states draws them, nothing else
            got = self.sample_states(batch, ndraws=ndraws, seed=seed, first_draw=first_draw)
            return SampledMappings(got.states, values, counts, means, got.status, nodes)
        states = np.full((ndraws, S, N), 255, dtype=np.uint8)
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_sample_mappings(
            self._h, batch._h, 1 if recompute_transitions else 0, seed, first_draw, ndraws, K,
            _ptr(E, c_double), _ptr(states, ctypes.c_ubyte),
            None if values is None else _ptr(values, c_double),
            None if counts is None else _ptr(counts, c_int32), _ptr(means, c_double),
            _ptr(status, c_int32)))
        return SampledMappings(states, values, counts, means, status, nodes)

    def branch_expectations(self, batch, coefs, per_site=True, recompute_transitions=False):
        """rt_sites_branch_expectations: the reference's branch-site map
        (examples/code2x3/extras.get_expected_ntransitions) for every site of the resident batch.
        coefs: one (n, n) array E or up to RT_MAX_BRANCH_COEFS (8) of them; E[c, d] weighs a
        c -> d transition, E[c, c] a unit of time spent in c.  Returns a BranchExpectations
        tuple: values[i, v, k] the conditional expectation at site i on the edge above preorder
        node v (None with per_site=False: the array never leaves the device), edge_sums[v, k]
        its site-weighted sum (SiteBatch.set_weights), status, nodes.  The rates must have
        been set with set_rates."""
        n = self.nstates
        E = check_branch_coefs(coefs, n)
        K = E.shape[0]
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        nodes = list(ta.preorder_nodes)
        values = np.zeros((S, N, K)) if per_site else None
        edge_sums = np.zeros((N, K))
        status = np.zeros(S, dtype=np.int32)
        if N == 1:
            # one node, no edges: only the status of the sites is to be had
            status[~(self._root_weights(batch).sum(axis=1) > 0)] = _lib.RT_SITE_ZERO_PROB
            return BranchExpectations(values, edge_sums, status, nodes)
        _lib.check(_lib.lib().rt_sites_branch_expectations(
            self._h, batch._h, 1 if recompute_transitions else 0, K, _ptr(E, c_double),
            None if values is None else _ptr(values, c_double), _ptr(edge_sums, c_double),
            _ptr(status, c_int32)))
        return BranchExpectations(values, edge_sums, status, nodes)

    def branch_expectations_partitioned(self, batch, coefs, per_site=True,
                                        recompute_transitions=False):
        """rt_sites_branch_expectations_partitioned: branch_expectations for a batch uploaded
        with site_sets -- on every edge site i uses Q, t, P and the derivative of its own rate
        set of set_rate_sets.  coefs: one (n, n) array, a (C, n, n) sequence shared by all sets,
        or (nsets, C, n, n) with set k's matrices at [k] (check_branch_coefs_partitioned).
        Returns a PartitionedBranchExpectations tuple: values[i, v, c] in caller order (None with
        per_site=False: the array never leaves the device), edge_sums[v, c] the site-weighted
        sum over the batch, set_edge_sums[k, v, c] the same over set k's sites (zeros for an
        empty set), status, nodes.  No earlier step_partitioned is needed; what the batch holds
        (log-likelihoods, totals, per-set totals) stays."""
        nsets = int(getattr(batch, 'nsets', 0) or 0)
        if batch.site_sets is None or nsets < 1:
            raise ValueError('branch_expectations_partitioned takes a batch uploaded with '
                             'site_sets (an ordinary batch: branch_expectations)')
        n = self.nstates
        E, per_set = check_branch_coefs_partitioned(coefs, n, nsets)
        C = E.shape[1] if per_set else E.shape[0]
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        values = np.zeros((S, N, C)) if per_site else None
        edge_sums = np.zeros((N, C))
        set_sums = np.zeros((nsets, N, C))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_branch_expectations_partitioned(
            self._h, batch._h, 1 if recompute_transitions else 0, C, 1 if per_set else 0,
            _ptr(E, c_double), None if values is None else _ptr(values, c_double),
            _ptr(edge_sums, c_double), _ptr(set_sums, c_double), _ptr(status, c_int32)))
        return PartitionedBranchExpectations(values, edge_sums, set_sums, status,
                                             list(ta.preorder_nodes))

    def branch_length_gradient_partitioned(self, batch, recompute_transitions=False):
        """g[k, v] = d (sum over the sites i of set k of w_i log L_i) / d t[k][v], f64[nsets,
        nnodes] in preorder (0 at the root and where t[k][v] == 0), analytically from one
        branch_expectations_partitioned call with per-set coefficients: ones off the diagonal
        and diag(Q[k]) on it, so that set k's direction is Q[k] itself and its edge sum is
        t[k][v] times the derivative.  For ONE rate matrix per set: the coefficient matrix of
        a set is shared by all its edges, so with per-edge rate matrices no single E has every
        edge's diag(Q) on its diagonal -- ValueError then.
        Chain rule for the usual parametrisation t[k][v] = r_k * tau_v (a tree shared by the
        partitions, one multiplier each): d/d tau_v = sum_k r_k g[k, v] and d/d r_k =
        sum_v tau_v g[k, v] (partition_chain_rule)."""
        rates = getattr(self, '_rate_sets', None)
        if rates is None:
            raise ValueError('set_rate_sets has not been called')
        Q, t = rates
        nsets = int(getattr(batch, 'nsets', 0) or 0)
        if Q.shape[1] != 1:
            raise ValueError('branch_length_gradient_partitioned needs one rate matrix per set '
                             'for all edges (%d here): the coefficient matrix of a set is '
                             'shared by all its edges' % Q.shape[1])
        if Q.shape[0] < nsets:
            raise ValueError('the batch uses nsets=%d rate sets, set_rate_sets gave %d'
                             % (nsets, Q.shape[0]))
        n = self.nstates
        E = np.ones((max(nsets, 1), 1, n, n))
        for k in range(nsets):
            np.fill_diagonal(E[k, 0], np.diag(Q[k, 0]))
        sums = self.branch_expectations_partitioned(
            batch, E, per_site=False, recompute_transitions=recompute_transitions).set_edge_sums
        tk = t[:nsets]
        grad = np.zeros((nsets, self.tree.nnodes))
        live = tk != 0
        live[:, 0] = False
        grad[live] = sums[:, :, 0][live] / tk[live]
        return grad

    def branch_expectations_mixture(self, batch, coefs, class_weights, per_site=True,
                                    recompute_transitions=False):
        """rt_sites_branch_expectations_mixture: branch_expectations of an ordinary batch under
        the site-class mixture over the K rate sets of set_rate_sets with the class weights c
        (check_class_weights): every site under every class, weighted by the class posteriors
        post[i, k] = c_k L_ik / sum_j c_j L_ij.  coefs: one (n, n) array, a (C, n, n) sequence
        shared by all classes, or (K, C, n, n) with class k's matrices at [k]
        (check_branch_coefs_partitioned).  Returns a MixtureBranchExpectations tuple: values[i,
        v, c] = sum_k post[i, k] x_k[i, v, c] with x_k what branch_expectations gives under set k
        (None with per_site=False: the array never leaves the device), edge_sums,
        set_edge_sums[k, v, c] = sum_i w_i post[i, k] x_k[i, v, c], class_posteriors,
        class_sums[k] = sum_i w_i post[i, k], log_likelihoods[i] = log sum_k c_k L_ik, status.
        A class with c_k = 0 or L_ik = 0 is skipped at that site.  No earlier step_multi is
        needed; nothing the batch or the model holds changes."""
        K = int(getattr(self, '_nsets', 0) or 0)
        if K < 1:
            raise ValueError('set_rate_sets has not been called')
        if batch.site_sets is not None:
            raise ValueError('branch_expectations_mixture takes an ordinary batch (a batch '
                             'uploaded with site_sets: branch_expectations_partitioned)')
        c = check_class_weights(class_weights, K)
        E, per_set = check_branch_coefs_partitioned(coefs, self.nstates, K)
        C = E.shape[1] if per_set else E.shape[0]
        N, S = self.tree.nnodes, batch.nsites
        values = np.zeros((S, N, C)) if per_site else None
        edge_sums = np.zeros((N, C))
        set_sums = np.zeros((K, N, C))
        post = np.zeros((S, K))
        class_sums = np.zeros(K)
        ll = np.zeros(S)
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_branch_expectations_mixture(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(c, c_double), C,
            1 if per_set else 0, _ptr(E, c_double),
            None if values is None else _ptr(values, c_double), _ptr(edge_sums, c_double),
            _ptr(set_sums, c_double), _ptr(post, c_double), _ptr(class_sums, c_double),
            _ptr(ll, c_double), _ptr(status, c_int32)))
        return MixtureBranchExpectations(values, edge_sums, set_sums, post, class_sums, ll, status)

    def class_posteriors(self, batch, class_weights, recompute_transitions=False):
        """(posteriors f64[nsites, K], log_likelihoods f64[nsites]) of the site-class mixture:
        post[i, k] = c_k L_ik / sum_j c_j L_ij, the empirical-Bayes classification of the sites
        (a row of zeros and -inf where no class is live).  This is branch_expectations_mixture
        with one identity coefficient matrix, the cheapest there is, and its sums left on the
        device: the call still costs a full expectation pass (K upward and downward passes and
        the derivative of every edge of every set)."""
        K = int(getattr(self, '_nsets', 0) or 0)
        if K < 1:
            raise ValueError('set_rate_sets has not been called')
        if batch.site_sets is not None:
            raise ValueError('class_posteriors takes an ordinary batch')
        c = check_class_weights(class_weights, K)
        E = np.ascontiguousarray(np.eye(self.nstates)[None])
        post = np.zeros((batch.nsites, K))
        ll = np.zeros(batch.nsites)
        _lib.check(_lib.lib().rt_sites_branch_expectations_mixture(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(c, c_double), 1, 0,
            _ptr(E, c_double), None, None, None, _ptr(post, c_double), None, _ptr(ll, c_double),
            None))
        return post, ll

    def branch_length_gradient_mixture(self, batch, class_weights, recompute_transitions=False):
        """The analytic gradient of f = sum_i w_i log sum_k c_k L_ik from ONE
        branch_expectations_mixture call with per-class coefficients (ones off the diagonal,
        diag(Q[k]) on it: class k's direction is Q[k] itself) -> (g_t f64[K, nnodes], g_c
        f64[K], total): g_t[k, v] = d f / d t[k][v] = set_edge_sums[k, v, 0] / t[k][v] (0 at
        the root), g_c[k] = d f / d c_k = class_sums[k] / c_k (0 where c_k == 0), total = f over
        the sites with a live class.  ValueError for several rate matrices per set (no single E
        has every edge's diag(Q)) and for a resident t[k][v] == 0 below the root (the sum is
        t times the derivative: it says nothing there)."""
        rates = getattr(self, '_rate_sets', None)
        if rates is None:
            raise ValueError('set_rate_sets has not been called')
        Q, t = rates
        if Q.shape[1] != 1:
            raise ValueError('branch_length_gradient_mixture needs one rate matrix per set for '
                             'all edges (%d here): the coefficient matrix of a set is shared '
                             'by all its edges' % Q.shape[1])
        if (t[:, 1:] == 0).any():
            raise ValueError('a resident branch length t[k][v] is 0: the edge sum is t[k][v] '
                             'times the derivative and gives no gradient there')
        K, n = Q.shape[0], self.nstates
        c = check_class_weights(class_weights, K)
        E = np.ones((K, 1, n, n))
        for k in range(K):
            np.fill_diagonal(E[k, 0], np.diag(Q[k, 0]))
        res = self.branch_expectations_mixture(batch, E, c, per_site=False,
                                               recompute_transitions=recompute_transitions)
        g_t = np.zeros((K, self.tree.nnodes))
        g_t[:, 1:] = res.set_edge_sums[:, 1:, 0] / t[:, 1:]
        g_c = np.zeros(K)
        g_c[c > 0] = res.class_sums[c > 0] / c[c > 0]
        w = np.ones(batch.nsites) if batch._weights is None else batch._weights
        live = np.isfinite(res.log_likelihoods)
        return g_t, g_c, float(np.sum(w[live] * res.log_likelihoods[live]))

    def branch_lengths(self):
        """The branch lengths of the last set_rates / set_rates_spectral as the device holds
        them (rt_model_get_branch_lengths), f64[nnodes] in preorder, 0 at the root."""
        t = np.zeros(self.tree.nnodes)
        _lib.check(_lib.lib().rt_model_get_branch_lengths(self._h, _ptr(t, c_double)))
        return t

    def branch_profiles(self, batch, lengths=None, factors=None, per_site=False,
                        recompute_transitions=False):
        """rt_sites_branch_profiles: for every branch v and every trial length of its grid, the
        change of the log-likelihood when that branch alone takes that length -- one upward and
        one downward pass for all of them instead of one set_rates + step per branch and length.
        Exactly one of `lengths` (absolute, [nnodes, G] in preorder or a dict edge -> sequence)
        and `factors` (G multipliers of every branch's resident length): check_profile_lengths.
        Returns a BranchProfiles tuple: nodes, lengths [nnodes, G] as evaluated, sums[v, g] the
        site-weighted sum (SiteBatch.set_weights) of values[i, v, g] = log L_i(t_v ->
        lengths[v, g]) - log L_i (None unless per_site: the array never leaves the device),
        status.  The root's row is 0; the row of a branch whose resident length is 0 is NaN.
        The rates come from set_rates (per-edge rate matrices included) or set_rates_spectral."""
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        resident = None
        if factors is not None or isinstance(lengths, dict):
            resident = self.branch_lengths()
        grid = check_profile_lengths(lengths, N, factors=factors, resident=resident, tree=ta)
        G = grid.shape[1]
        values = np.zeros((S, N, G)) if per_site else None
        sums = np.zeros((N, G))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_branch_profiles(
            self._h, batch._h, 1 if recompute_transitions else 0, G, _ptr(grid, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(status, c_int32)))
        return BranchProfiles(list(ta.preorder_nodes), grid, sums, values, status)

    def nni_moves(self):
        """rt_model_nni_moves: the nearest-neighbour interchanges of the tree, int32[nmoves, 3]
        of preorder indices (v, c, s) -- the subtrees of the child c of v and of the sibling s of
        v exchanged -- ordered by v, then c, then s in child order (_tree.nni_apply makes the
        moved tree).  Where parent(v) is a root with the two children v and s the move keeps
        the unrooted topology."""
        count = c_int64(0)
        _lib.check(_lib.lib().rt_model_nni_moves(self._h, None, 0, byref(count)))
        moves = np.zeros((count.value, 3), dtype=np.int32)
        if count.value:
            _lib.check(_lib.lib().rt_model_nni_moves(self._h, _ptr(moves, c_int32), count.value,
                                                     byref(count)))
        return moves

    def nni_scores(self, batch, lengths=None, factors=None, per_site=False,
                   recompute_transitions=False):
        """rt_sites_nni_scores: the change of the log-likelihood for every move of nni_moves()
        -- one upward and one downward pass for the whole neighbourhood instead of a model
        build, an upload and a step per candidate.  With neither `lengths` nor `factors` the
        edge above v keeps its transition matrix (the plain swap; no rates needed); else the
        moves about v are scored at every trial length of that edge, given as for
        branch_profiles (check_profile_lengths; rows of nodes without a move are ignored).
        Returns an NniScores tuple: moves, lengths [nnodes, G] as evaluated, sums[mv, g] the
        site-weighted sum (SiteBatch.set_weights) of values[i, mv, g] (None unless per_site),
        status.  -inf where a live site has likelihood 0 on the moved tree."""
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        moves = self.nni_moves()
        if lengths is None and factors is None:
            grid, G = None, 1
        else:
            resident = None
            if factors is not None or isinstance(lengths, dict):
                resident = self.branch_lengths()
            grid = check_profile_lengths(lengths, N, factors=factors, resident=resident, tree=ta)
            G = grid.shape[1]
        M = len(moves)
        values = np.zeros((S, M, G)) if per_site else None
        sums = np.zeros((M, G))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_nni_scores(
            self._h, batch._h, 1 if recompute_transitions else 0, G,
            None if grid is None else _ptr(grid, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(status, c_int32)))
        if grid is None:
            try:                                 # (a model with transitions set directly: none)
                grid = self.branch_lengths()[:, None].copy()
            except (ValueError, _lib.RaotehHipError):
                grid = None
        return NniScores(moves, grid, sums, values, status)

    def _mixture_search_args(self, batch, class_weights, who):
        K = int(getattr(self, '_nsets', 0) or 0)
        if K < 1:
            raise ValueError('set_rate_sets has not been called')
        if batch.site_sets is not None:
            raise ValueError('%s takes an ordinary batch' % who)
        return check_class_weights(class_weights, K)

    def branch_profiles_mixture(self, batch, class_weights, factors, per_site=False,
                                recompute_transitions=False):
        """rt_sites_branch_profiles_mixture: branch_profiles of an ordinary batch under the
        site-class mixture over the K rate sets of set_rate_sets with the class weights c
        (check_class_weights).  Trial lengths are `factors` of every class's own resident
        lengths (check_profile_factors): at point g the edge above v has length factors[v, g] *
        t[k][v] under class k.  Returns a MixtureBranchProfiles tuple: factors [nnodes, G] as
        evaluated, sums[v, g] the site-weighted sum of values[i, v, g] = log sum_k c_k L_ik(...)
        - loglik[i] (None unless per_site: the array never leaves the device), loglik[i] = log
        sum_k c_k L_ik, status.  The root's row is 0; the row of a branch with resident length 0
        under a class with c_k > 0 is NaN.  A class with c_k = 0 is not run.  No earlier
        step_multi is needed; nothing the batch or the model holds changes."""
        c = self._mixture_search_args(batch, class_weights, 'branch_profiles_mixture')
        N, S = self.tree.nnodes, batch.nsites
        grid = check_profile_factors(factors, N)
        G = grid.shape[1]
        values = np.zeros((S, N, G)) if per_site else None
        sums = np.zeros((N, G))
        ll = np.zeros(S)
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_branch_profiles_mixture(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(c, c_double), G,
            _ptr(grid, c_double), None if values is None else _ptr(values, c_double),
            _ptr(sums, c_double), _ptr(ll, c_double), _ptr(status, c_int32)))
        return MixtureBranchProfiles(grid, sums, values, ll, status)

    def nni_scores_mixture(self, batch, class_weights, factors=None, per_site=False,
                           recompute_transitions=False):
        """rt_sites_nni_scores_mixture: nni_scores of an ordinary batch under the site-class
        mixture over the K rate sets with the class weights c, for every move of nni_moves().
        Without `factors` every class keeps its resident matrix on the edge above v (the plain
        swap); else the moves about v are scored with that edge at factors[v, g] * t[k][v] under
        class k (check_profile_factors; rows of nodes without a move are ignored).  Returns a
        MixtureNniScores tuple: moves, factors [nnodes, G] as evaluated (None for the plain
        swap), sums[mv, g] the site-weighted sum of values[i, mv, g] = log sum_k c_k L_ik(tree
        after mv, ...) - loglik[i] (None unless per_site), loglik, status.  Exact in every term:
        a class under which the site is impossible on the current tree still adds what it gives
        on the moved one."""
        c = self._mixture_search_args(batch, class_weights, 'nni_scores_mixture')
        N, S = self.tree.nnodes, batch.nsites
        moves = self.nni_moves()
        grid = None if factors is None else check_profile_factors(factors, N)
        G = 1 if grid is None else grid.shape[1]
        M = len(moves)
        values = np.zeros((S, M, G)) if per_site else None
        sums = np.zeros((M, G))
        ll = np.zeros(S)
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_nni_scores_mixture(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(c, c_double), G,
            None if grid is None else _ptr(grid, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(ll, c_double), _ptr(status, c_int32)))
        return MixtureNniScores(moves, grid, sums, values, ll, status)

    def _partitioned_search_args(self, batch, who):
        nsets = int(getattr(batch, 'nsets', 0) or 0)
        if batch.site_sets is None or nsets < 1:
            raise ValueError('%s takes a batch uploaded with site_sets (an ordinary batch: %s)'
                             % (who, who[:-len('_partitioned')]))
        K = int(getattr(self, '_nsets', 0) or 0)
        if K < 1:
            raise ValueError('set_rate_sets has not been called')
        if K < nsets:
            raise ValueError('the batch uses nsets=%d rate sets, set_rate_sets gave %d'
                             % (nsets, K))
        return nsets

    def branch_profiles_partitioned(self, batch, factors, per_site=False,
                                    recompute_transitions=False):
        """rt_sites_branch_profiles_partitioned: branch_profiles for a batch uploaded with
        site_sets -- site i reads every edge under its own rate set of set_rate_sets.  Trial
        lengths are `factors` of every set's own resident lengths (check_profile_factors): at
        point g the edge above v has length factors[v, g] * t[k][v] under set k.  Returns a
        PartitionedBranchProfiles tuple: factors [nnodes, G] as evaluated, values[i, v, g] =
        log L_i(t[k][v] -> factors[v, g] t[k][v]) - log L_i in caller order (None unless
        per_site: the array never leaves the device), sums[v, g] the site-weighted sum over the
        batch, set_sums[k, v, g] the same over set k's sites (zeros for an empty set), status,
        nodes.  The root's row is 0; where t[k][v] == 0 row v is NaN for the live sites of set
        k, in set_sums[k] and in sums.  No earlier step_partitioned is needed; nothing the
        batch or the model holds changes."""
        nsets = self._partitioned_search_args(batch, 'branch_profiles_partitioned')
        ta = self.tree
        N, S = ta.nnodes, batch.nsites
        grid = check_profile_factors(factors, N)
        G = grid.shape[1]
        values = np.zeros((S, N, G)) if per_site else None
        sums = np.zeros((N, G))
        set_sums = np.zeros((nsets, N, G))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_branch_profiles_partitioned(
            self._h, batch._h, 1 if recompute_transitions else 0, G, _ptr(grid, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(set_sums, c_double), _ptr(status, c_int32)))
        return PartitionedBranchProfiles(grid, values, sums, set_sums, status,
                                         list(ta.preorder_nodes))

    def nni_scores_partitioned(self, batch, factors=None, per_site=False,
                               recompute_transitions=False):
        """rt_sites_nni_scores_partitioned: nni_scores for a batch uploaded with site_sets, for
        every move of nni_moves() -- under set k the moved tree keeps every moved subtree's own
        edge of set k.  Without `factors` every set keeps its resident matrix on the edge above
        v (the plain swap); else the moves about v are scored with that edge at factors[v, g] *
        t[k][v] under set k (check_profile_factors; rows of nodes without a move are ignored).
        Returns a PartitionedNniScores tuple: moves, factors [nnodes, G] as evaluated (None for
        the plain swap), values[i, mv, g] in caller order (None unless per_site), sums[mv, g],
        set_sums[k, mv, g] over set k's sites (zeros for an empty set), status.  -inf where a
        live site has likelihood 0 on the moved tree."""
        nsets = self._partitioned_search_args(batch, 'nni_scores_partitioned')
        N, S = self.tree.nnodes, batch.nsites
        moves = self.nni_moves()
        grid = None if factors is None else check_profile_factors(factors, N)
        G = 1 if grid is None else grid.shape[1]
        M = len(moves)
        values = np.zeros((S, M, G)) if per_site else None
        sums = np.zeros((M, G))
        set_sums = np.zeros((nsets, M, G))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_nni_scores_partitioned(
            self._h, batch._h, 1 if recompute_transitions else 0, G,
            None if grid is None else _ptr(grid, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(set_sums, c_double), _ptr(status, c_int32)))
        return PartitionedNniScores(moves, grid, values, sums, set_sums, status)

    def spr_moves(self, radius=None):
        """rt_model_spr_moves: the subtree pruning and regrafting moves of the tree within
        `radius` (None: no limit), int32[nmoves, 2] of preorder indices (c, y) -- the subtree of
        the non-root node c cut off its parent v and hung on the edge above y, a non-root node
        outside that subtree -- ordered by c, then y (_tree.spr_apply makes the moved tree).
        The radius of a move is min(dist(v, y), dist(v, parent(y))) in edges: 0 for the edge
        above v and those above the siblings of c.  (c, v) at fraction 1 and (c, sibling) at
        fraction 0 leave the tree as it is; they are listed."""
        rad = _spr_radius(radius)
        count = c_int64(0)
        _lib.check(_lib.lib().rt_model_spr_moves(self._h, rad, None, 0, byref(count)))
        moves = np.zeros((count.value, 2), dtype=np.int32)
        if count.value:
            _lib.check(_lib.lib().rt_model_spr_moves(self._h, rad, _ptr(moves, c_int32),
                                                     count.value, byref(count)))
        return moves

    def spr_scores(self, batch, radius=None, fractions=(0.5,), per_site=False,
                   recompute_transitions=False):
        """rt_sites_spr_scores: the change of the log-likelihood for every move of
        spr_moves(radius) at every fraction -- the subtree of c, with its own edge, hung on a new
        node that cuts the edge above y at fractions[r] of its length (from the parent), both
        halves under the rate matrix of the cut edge -- in one call instead of a model build, an
        upload and a step per candidate.  Returns an SprScores tuple: moves, fractions, sums
        [nmoves, R] the site-weighted sums (SiteBatch.set_weights), values [nsites, nmoves, R]
        (None unless per_site), status, best = (move, r) the arg-max of sums (ties to the lowest
        index; None where the tree has no move).  -inf where a live site has likelihood 0 on the
        moved tree."""
        S = batch.nsites
        rad = _spr_radius(radius)
        f, _ = check_placement_grid(fractions, (0.0,))
        moves = self.spr_moves(radius)
        M, R = len(moves), len(f)
        values = np.zeros((S, M, R)) if per_site else None
        sums = np.zeros((M, R))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_spr_scores(
            self._h, batch._h, 1 if recompute_transitions else 0, rad, R, _ptr(f, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(status, c_int32)))
        best = None
        if M:
            flat = np.where(np.isnan(sums), -np.inf, sums).reshape(-1)
            best = tuple(int(x) for x in np.unravel_index(int(np.argmax(flat)), (M, R)))
        return SprScores(moves, f, sums, values, status, best)

    def spr_scores_mixture(self, batch, class_weights, radius=None, fractions=(0.5,),
                           per_site=False, recompute_transitions=False):
        """rt_sites_spr_scores_mixture: spr_scores of an ordinary batch under the site-class
        mixture over the K rate sets of set_rate_sets with the class weights c
        (check_class_weights), for every move of spr_moves(radius) at every fraction: under class
        k the edge above y is cut at fractions[r] of its own resident length t[k][y], the pruned
        subtree keeps its edge.  Returns a MixtureSprScores tuple: moves, fractions, sums[mv, r]
        the site-weighted sum of values[i, mv, r] = log sum_k c_k L_ik(tree after mv at
        fractions[r]) - loglik[i] (None unless per_site), loglik, status, best as spr_scores.
        Exact in every term: a class under which the site is impossible on the current tree
        still adds what it gives on the moved one.  Nothing the batch or the model holds
        changes."""
        c = self._mixture_search_args(batch, class_weights, 'spr_scores_mixture')
        S = batch.nsites
        rad = _spr_radius(radius)
        f, _ = check_placement_grid(fractions, (0.0,))
        moves = self.spr_moves(radius)
        M, R = len(moves), len(f)
        values = np.zeros((S, M, R)) if per_site else None
        sums = np.zeros((M, R))
        ll = np.zeros(S)
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_spr_scores_mixture(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(c, c_double), rad, R,
            _ptr(f, c_double), None if values is None else _ptr(values, c_double),
            _ptr(sums, c_double), _ptr(ll, c_double), _ptr(status, c_int32)))
        best = None
        if M:
            flat = np.where(np.isnan(sums), -np.inf, sums).reshape(-1)
            best = tuple(int(x) for x in np.unravel_index(int(np.argmax(flat)), (M, R)))
        return MixtureSprScores(moves, f, sums, values, ll, status, best)

    def place_queries(self, batch, queries, kind='dense', fractions=(0.5,), pendant=None,
                      per_site=False, recompute_transitions=False):
        """rt_sites_placements: every query placed on every branch -- for query q, non-root
        node v, fraction r and pendant length k the change of the log-likelihood when a new
        node cuts the edge above v at fractions[r] of its length (from the parent) and the
        query hangs below it on an edge of length pendant[k], all under the rate matrix of the
        cut edge -- in one call instead of a model build, an upload and a step per candidate.
        queries: kind 'dense', f64 [Q, nsites, n] likelihood vectors, or 'state', uint8
        [Q, nsites] (255 or -1: unobserved, as for upload_sites); fractions and pendant as check_placement_grid
        takes them, pendant=None the one value mean(branch_lengths()[1:]).  Returns a Placements
        tuple: fractions, pendant, sums [Q, nnodes, R, K] the site-weighted sums
        (SiteBatch.set_weights), values [nsites, Q, nnodes, R, K] (None unless per_site),
        status, best [Q, 3] the arg-max (v, r, k) of sums per query (ties to the lowest index;
        _tree.place_apply adopts it).  The root's row is 0 and never the best; -inf where the
        query's column is impossible given the reference column."""
        ta = self.tree
        N, S, n = ta.nnodes, batch.nsites, self.nstates
        if pendant is None:
            pendant = [float(np.mean(self.branch_lengths()[1:]))] if N > 1 else [0.0]
        f, t = check_placement_grid(fractions, pendant)
        q, code = _placement_queries(queries, kind, S, n)
        Q, R, K = q.shape[0], len(f), len(t)
        values = np.zeros((S, Q, N, R, K)) if per_site else None
        sums = np.zeros((Q, N, R, K))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_placements(
            self._h, batch._h, 1 if recompute_transitions else 0, Q, code,
            q.ctypes.data_as(ctypes.c_void_p), R, _ptr(f, c_double), K, _ptr(t, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(status, c_int32)))
        best = np.zeros((Q, 3), dtype=np.int64)
        if N > 1:
            flat = sums[:, 1:].reshape(Q, -1)
            flat = np.where(np.isnan(flat), -np.inf, flat)
            v, r, k = np.unravel_index(np.argmax(flat, axis=1), (N - 1, R, K))
            best = np.stack([v + 1, r, k], axis=1).astype(np.int64)
        return Placements(f, t, sums, values, status, best)

    def place_queries_mixture(self, batch, class_weights, queries, kind='dense', fractions=(0.5,),
                              pendant=None, pendant_scale=None, per_site=False,
                              recompute_transitions=False):
        """rt_sites_placements_mixture: place_queries of an ordinary batch under the site-class
        mixture over the K rate sets of set_rate_sets with the class weights c
        (check_class_weights).  Under class k the edge above v is cut at fractions[r] of its own
        resident length t[k][v] and the query hangs on an edge of length pendant_scale[k] *
        pendant[j] (check_pendant_scale: None gives ones, right for classes Q_k = r_k Q over
        shared lengths; for a shared Q with t_k = r_k t pass r_k).  queries, kind, fractions and
        pendant as for place_queries (pendant=None: the one value mean(rate_set_lengths)).
        Returns a MixturePlacements tuple: fractions, pendant, pendant_scale, sums
        [Q, nnodes, R, K] the site-weighted sums of values[i, q, v, r, j] = log sum_k c_k
        L_ik(tree with q placed) - loglik[i] (None unless per_site), loglik, status, best as
        place_queries.  The root's row is 0.  Exact in every term; nothing the batch or the
        model holds changes."""
        c = self._mixture_search_args(batch, class_weights, 'place_queries_mixture')
        ta = self.tree
        N, S, n = ta.nnodes, batch.nsites, self.nstates
        scale = check_pendant_scale(pendant_scale, len(c))
        if pendant is None:
            sets = getattr(self, '_rate_sets', None)
            t = None if sets is None else np.asarray(sets[1])
            pendant = [float(np.mean(t[:, 1:]))] if t is not None and N > 1 else [0.0]
        f, t = check_placement_grid(fractions, pendant)
        q, code = _placement_queries(queries, kind, S, n)
        Q, R, K = q.shape[0], len(f), len(t)
        values = np.zeros((S, Q, N, R, K)) if per_site else None
        sums = np.zeros((Q, N, R, K))
        ll = np.zeros(S)
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_placements_mixture(
            self._h, batch._h, 1 if recompute_transitions else 0, _ptr(c, c_double), Q, code,
            q.ctypes.data_as(ctypes.c_void_p), R, _ptr(f, c_double), K, _ptr(t, c_double),
            _ptr(scale, c_double), None if values is None else _ptr(values, c_double),
            _ptr(sums, c_double), _ptr(ll, c_double), _ptr(status, c_int32)))
        best = np.zeros((Q, 3), dtype=np.int64)
        if N > 1:
            flat = sums[:, 1:].reshape(Q, -1)
            flat = np.where(np.isnan(flat), -np.inf, flat)
            v, r, k = np.unravel_index(np.argmax(flat, axis=1), (N - 1, R, K))
            best = np.stack([v + 1, r, k], axis=1).astype(np.int64)
        return MixturePlacements(f, t, scale, sums, values, ll, status, best)

    def spr_scores_partitioned(self, batch, radius=None, fractions=(0.5,), per_site=False,
                               recompute_transitions=False):
        """rt_sites_spr_scores_partitioned: spr_scores for a batch uploaded with site_sets, for
        every move of spr_moves(radius) at every fraction -- site i reads every edge under its own
        rate set k of set_rate_sets: the edge above y is cut at fractions[r] of the set's own
        resident length t[k][y], the pruned subtree keeps its own edge of set k.  Returns a
        PartitionedSprScores tuple: moves, fractions, values[i, mv, r] in caller order (None
        unless per_site), sums[mv, r], set_sums[k, mv, r] over set k's sites (zeros for an empty
        set), status, best as spr_scores.  -inf where a live site has likelihood 0 on the moved
        tree.  No earlier step_partitioned is needed; nothing the batch or the model holds
        changes."""
        nsets = self._partitioned_search_args(batch, 'spr_scores_partitioned')
        S = batch.nsites
        rad = _spr_radius(radius)
        f, _ = check_placement_grid(fractions, (0.0,))
        moves = self.spr_moves(radius)
        M, R = len(moves), len(f)
        values = np.zeros((S, M, R)) if per_site else None
        sums = np.zeros((M, R))
        set_sums = np.zeros((nsets, M, R))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_spr_scores_partitioned(
            self._h, batch._h, 1 if recompute_transitions else 0, rad, R, _ptr(f, c_double),
            None if values is None else _ptr(values, c_double), _ptr(sums, c_double),
            _ptr(set_sums, c_double), _ptr(status, c_int32)))
        best = None
        if M:
            flat = np.where(np.isnan(sums), -np.inf, sums).reshape(-1)
            best = tuple(int(x) for x in np.unravel_index(int(np.argmax(flat)), (M, R)))
        return PartitionedSprScores(moves, f, values, sums, set_sums, status, best)

    def place_queries_partitioned(self, batch, queries, kind='dense', fractions=(0.5,),
                                  pendant=None, pendant_scale=None, per_site=False,
                                  recompute_transitions=False):
        """rt_sites_placements_partitioned: place_queries for a batch uploaded with site_sets --
        site i under its own rate set k of set_rate_sets: the edge above v is cut at fractions[r]
        of the set's own resident length t[k][v] and the query hangs on an edge of length
        pendant_scale[k] * pendant[j] under the set's rate matrix of the cut edge
        (check_pendant_scale over the model's sets: None gives ones).  queries, kind and
        fractions as for place_queries, the queries in the caller's site order; pendant=None:
        the one value mean(t[:nsets, 1:]) of the resident rate sets.  Returns a
        PartitionedPlacements tuple: fractions, pendant, pendant_scale, values[i, q, v, r, j] in
        caller order (None unless per_site), sums [Q, nnodes, R, K], set_sums [nsets, Q, nnodes,
        R, K] over each set's sites (zeros for an empty set), status, best as place_queries.
        The root's row is 0.  Nothing the batch or the model holds changes."""
        nsets = self._partitioned_search_args(batch, 'place_queries_partitioned')
        ta = self.tree
        N, S, n = ta.nnodes, batch.nsites, self.nstates
        scale = check_pendant_scale(pendant_scale, int(self._nsets))
        if pendant is None:
            sets = getattr(self, '_rate_sets', None)
            t = None if sets is None else np.asarray(sets[1])
            pendant = [float(np.mean(t[:nsets, 1:]))] if t is not None and N > 1 else [0.0]
        f, t = check_placement_grid(fractions, pendant)
        q, code = _placement_queries(queries, kind, S, n)
        Q, R, K = q.shape[0], len(f), len(t)
        values = np.zeros((S, Q, N, R, K)) if per_site else None
        sums = np.zeros((Q, N, R, K))
        set_sums = np.zeros((nsets, Q, N, R, K))
        status = np.zeros(S, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_placements_partitioned(
            self._h, batch._h, 1 if recompute_transitions else 0, Q, code,
            q.ctypes.data_as(ctypes.c_void_p), R, _ptr(f, c_double), K, _ptr(t, c_double),
            _ptr(scale, c_double), None if values is None else _ptr(values, c_double),
            _ptr(sums, c_double), _ptr(set_sums, c_double), _ptr(status, c_int32)))
        best = np.zeros((Q, 3), dtype=np.int64)
        if N > 1:
            flat = sums[:, 1:].reshape(Q, -1)
            flat = np.where(np.isnan(flat), -np.inf, flat)
            v, r, k = np.unravel_index(np.argmax(flat, axis=1), (N - 1, R, K))
            best = np.stack([v + 1, r, k], axis=1).astype(np.int64)
        return PartitionedPlacements(f, t, scale, values, sums, set_sums, status, best)

    def branch_length_gradient(self, batch, recompute_transitions=False):
        """d (sum_i w_i log L_i) / d t_v for every branch, f64[nnodes] in preorder (0 at the
        root), analytically from one branch_expectations call: with E = ones off the diagonal
        and diag(Q) on it the direction is Q itself and the edge sum is t_v times the
        derivative.  For a model with ONE rate matrix: the coefficient matrix of a call is
        shared by all edges, so with per-edge rate matrices no single E has every edge's
        diag(Q) on its diagonal -- ValueError then (call branch_expectations once per rate
        matrix and pick the edges)."""
        rates = getattr(self, '_rates', None)
        if rates is None:
            raise ValueError('set_rates has not been called')
        Q, t = rates
        if Q.shape[0] != 1:
            raise ValueError('branch_length_gradient needs one rate matrix for all edges '
                             '(%d here): the coefficient matrix is shared by all edges'
                             % Q.shape[0])
        E = np.ones((self.nstates, self.nstates))
        np.fill_diagonal(E, np.diag(Q[0]))
        sums = self.branch_expectations(batch, E, per_site=False,
                                        recompute_transitions=recompute_transitions).edge_sums
        grad = np.zeros(self.tree.nnodes)
        live = t != 0
        live[0] = False
        grad[live] = sums[live, 0] / t[live]
        return grad

    def allreduce(self, batch):
        _lib.check(_lib.lib().rt_allreduce_totals(self.ctx._h, batch._h))

    def allreduce_group(self, batches):
        """The totals of several batches in one collective (rt_allreduce_totals_group)."""
        arr = (c_void_p * len(batches))(*[b._h for b in batches])
        _lib.check(_lib.lib().rt_allreduce_totals_group(self.ctx._h, arr, len(batches)))

    def fetch_log_likelihoods(self, batch):
        ll = np.empty(batch.nsites, dtype=np.float64)
        st = np.empty(batch.nsites, dtype=np.int32)
        _lib.check(_lib.lib().rt_sites_get_logliks(
            batch._h, _ptr(ll, c_double), _ptr(st, c_int32)))
        return ll, st

    def fetch_totals(self, batch):
        tot = np.zeros(3, dtype=np.float64)
        _lib.check(_lib.lib().rt_sites_get_totals(batch._h, _ptr(tot, c_double)))
        return tot

    def log_likelihoods(self, batch):
        self.prune(batch)
        return self.fetch_log_likelihoods(batch)

    def total_log_likelihood(self, batch):
        """(sum of log-likelihoods, number of zero-probability sites); the sum
        is -inf when any site has zero probability."""
        self.prune(batch)
        tot = self.fetch_totals(batch)
        nzero = int(tot[1])
        return (-np.inf if nzero else float(tot[0])), nzero
