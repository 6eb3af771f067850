"""History independence of the resident objects (test_history_cpu.py, test_history_gpu.py): after
any sequence of valid calls, every read of a long-lived TreeModel / SiteBatch returns what the same
read returns on a fresh pair that was given the current parameters alone.

This module is host only and imports no device code at module level.  It holds
  * the SHADOW STATE: a plain record of what the caller has told the library, as parameter tokens
    (small integers: a seeded generator turns (row, parameter, token) into the arrays, so a
    stale-parameter twin is a state with one token put back), in several snapshots -- "current" and
    "as of the last pruning launch" of each kind (prune / step, step_multi, step_partitioned);
  * the OPERATION CATALOGUE: mutators and reads, READS being the one explicit table of which
    snapshot a read answers from, what it needs, what it depends on and the line of
    include/raoteh_hip.h (or of the device.py docstring) that says so;
  * the WALK: an Euler circuit over the graph of all (operation, read) and (read, mutator) pairs --
    every ordered pair (operation, read) adjacent exactly once, which is the minimal length -- from a
    seeded Hierholzer construction, followed by repairs: a pair whose read was refused at its one
    occurrence because of state left by calls further back (not by the operation right before it)
    occurs once more behind the shortest mutator prefix that makes the read live.  What remains
    refused is DOCUMENTED_REFUSALS: the pairs whose second call the header refuses right after the
    first;
  * the FRESH TWIN built from a snapshot in the canonical shortest way, and the bitwise COMPARISON.

A read called with recompute_transitions=True is a mutator of its own, 'recompute:<read>': it is
compared with the twin like any read, and every read follows it once.
"""
import collections
import copy
import itertools
import zlib

import numpy as np

INVALID, UNSUPPORTED = -1, -3              # RT_ERR_INVALID (the wrapper's ValueError), RT_ERR_UNSUPPORTED


# ---- rows -------------------------------------------------------------------------------------

Row = collections.namedtuple('Row', 'name n kind nsites nnodes opts prefix need leaves_only '
                                    'partitioned wide background seed')


def _row(name, n, kind, nsites, nnodes, opts, prefix, need=(), leaves_only=False,
         partitioned=False, background=False):
    return Row(name, n, kind, nsites, nnodes, opts, prefix, tuple(need), leaves_only, partitioned,
               n > 64, background, zlib.crc32(name.encode()) & 0xffff)


# the kernel-name proof of a row is taken after wait_for_kernel and a pruning launch
ROWS = [
    _row('lane-interp-n3-state-65', 3, 'state', 65, 11, {'jit': 0}, 'prune_lane'),
    _row('lane-background-n4-mask-38', 4, 'mask', 38, 9,
         {'jit': 1, 'jit_async': 1, 'jit_block_sites': 37}, 'prune_tree_jit<4', need=(',masks',),
         background=True),
    _row('expect-lane-form-n8-dense-17', 8, 'dense', 17, 10, {'jit': 0}, 'prune_mfma'),
    _row('mfma-one-wave-n20-dense-33', 20, 'dense', 33, 12, {'jit': 1}, 'prune_tree_jit_mfma'),
    _row('split-m-leaf-states-n61-state-33', 61, 'state', 33, 13, {'jit': 1},
         'prune_tree_jit_mfma', need=('leaf-states',), leaves_only=True),
    _row('wide-n70-mask-17', 70, 'mask', 17, 9, {'jit': 0}, 'prune_mfma'),
    _row('partitioned-n20-dense-4sets', 20, 'dense', 41, 11, {'jit': 0}, 'prune_mfma',
         need=(',partitioned',), partitioned=True),
]
ROW = dict((r.name, r) for r in ROWS)
PART_SIZES = (17, 5, 16, 3)                # sites per rate set of the partitioned row: ragged granules
PART_NSETS = len(PART_SIZES)

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


# ---- the case of a row: tree, observations, call arguments (fixed over a walk) ----------------

Fixed = collections.namedtuple(
    'Fixed', 'T root leaves obs_nodes data obs_lik zero_site zero_weight_site site_sets coefs '
             'node_sets edge_sets marginal_nodes queries node_q')


def make_tree(nnodes, rng):
    """9..13 nodes: the root has three children (a multifurcation), node 1 has one child, every
    other internal node two.  Node labels are integers in preorder-unfriendly order."""
    import networkx as nx
    assert 9 <= nnodes <= 13
    T = nx.Graph()
    edges = [(0, 1), (0, 2), (0, 3), (1, 4), (4, 5), (4, 6), (2, 7), (2, 8)]
    grow = [3, 5, 7, 6]                            # leaves that get two children, in this order
    nxt = 9
    while nxt < nnodes:
        p = grow.pop(0)
        for _ in range(2):
            if nxt < nnodes:
                edges.append((p, nxt))
                nxt += 1
    label = lambda v: 100 + 7 * v                  # (not the preorder index)
    for a, b in edges:
        T.add_edge(label(a), label(b), weight=float(rng.uniform(0.05, 0.5)))
    assert T.number_of_nodes() == nnodes, (T.number_of_nodes(), nnodes)
    leaves = sorted(v for v in T if T.degree(v) == 1 and v != label(0))
    return T, label(0), leaves


def _encode_mask(n, lik):
    words = np.zeros(lik.shape[:2] + ((n + 63) // 64,), dtype=np.uint64)
    for s in range(n):
        words[:, :, s >> 6] |= (lik[:, :, s] != 0).astype(np.uint64) << np.uint64(s & 63)
    return words[:, :, 0].copy() if n <= 64 else words


_fixed_cache = {}


def fixed_of(row):
    """Tree, observations and the arguments of the reads.  State 0 is isolated under every rate
    matrix and transition matrix of a walk and allowed at no observed node -- but at site S // 2
    one leaf is observed in state 0 and another in state 1: likelihood 0 under every parameter
    set."""
    if row.name in _fixed_cache:
        return _fixed_cache[row.name]
    rng = np.random.RandomState(row.seed)
    n, S = row.n, row.nsites
    T, root, leaves = make_tree(row.nnodes, rng)
    inner = sorted(v for v in T if v not in leaves and v != root)
    obs_nodes = list(leaves) + ([] if row.leaves_only else [inner[1]])
    K = len(obs_nodes)
    z = S // 2
    st = None
    if row.kind == 'state':
        st = rng.randint(1, n, size=(S, K))
        if not row.leaves_only:
            st[rng.uniform(size=st.shape) < 0.1] = 255
        st[z, 0], st[z, 1] = 0, 1
        lik = np.ones((S, K, n))
        seen = st != 255
        lik[seen] = 0.0
        ii, kk = np.nonzero(seen)
        lik[ii, kk, st[ii, kk]] = 1.0
    else:
        if row.kind == 'mask' or n <= 4:
            lik = (rng.uniform(size=(S, K, n)) < 0.4).astype(np.float64)
            lik[:, :, 1] = 1.0
            if n > 64:
                lik[:, :, n - 1] = 1.0             # (both words of the mask in use)
        else:
            lik = rng.uniform(0.0, 1.0, size=(S, K, n))
            lik[rng.uniform(size=lik.shape) < 0.2] = 0.0
            lik[:, :, 1] += 0.05
        lik[:, :, 0] = 0.0
        lik[z, 0] = 0.0
        lik[z, 0, 0] = 1.0
        lik[z, 1] = 0.0
        lik[z, 1, 1] = 1.0
    if row.kind == 'state':
        data = st.astype(np.uint8)
    elif row.kind == 'mask':
        data = _encode_mask(n, lik)
    else:
        data = lik
    site_sets = None
    if row.partitioned:
        assert sum(PART_SIZES) == S
        site_sets = rng.permutation(np.repeat(np.arange(PART_NSETS), PART_SIZES)).astype(np.int64)
    coefs = rng.uniform(-0.5, 1.0, size=(2, n, n))
    h = max(1, n // 2)
    lo, hi = list(range(h)), list(range(h, n))
    sub = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    node_sets = [lo, sorted(set(sub + [n - 1]))]
    edge_sets = [(lo, hi), (sub, list(range(n)))]
    marginal_nodes = [inner[0], leaves[-1]]
    queries = rng.randint(1, n, size=(2, S)).astype(np.uint8)
    queries[0, 1] = 255
    node_q = np.zeros(row.nnodes, dtype=np.int64)
    node_q[1::3] = 1
    node_q[0] = 0
    fx = Fixed(T, root, leaves, obs_nodes, data, lik, z, (z + 3) % S, site_sets, coefs, node_sets,
               edge_sets, marginal_nodes, queries, node_q)
    _fixed_cache[row.name] = fx
    return fx


# ---- parameter tokens -> arrays -----------------------------------------------------------------

def _rng(row, what, token):
    return np.random.RandomState(zlib.crc32(('%s/%s/%d' % (row.name, what, token)).encode())
                                 & 0x7fffffff)


def iso_rate_matrix(n, rng):
    """A random rate matrix with exact zeros in which state 0 is isolated (row 0 and column 0 are
    zero) and the other states communicate; mean exit rate 1 over the states 1 .. n-1."""
    R = rng.uniform(0.1, 1.0, (n, n)) * (rng.uniform(size=(n, n)) < 0.7)
    R[np.arange(n), (np.arange(n) + 1) % n] += 0.3
    if n > 2:
        R[np.arange(2, n), np.arange(1, n - 1)] += 0.2
        R[n - 1, 1] += 0.3
    R[:, 0] = 0.0
    R[0, :] = 0.0
    np.fill_diagonal(R, 0.0)
    Q = R - np.diag(R.sum(axis=1))
    return Q / R.sum(axis=1)[1:].mean()


def gen_Q(row, token, nq):
    rng = _rng(row, 'Q', token)
    return np.stack([iso_rate_matrix(row.n, rng) for _ in range(nq)])


def gen_t(row, token, zero=True):
    """Branch lengths in [0.05, 0.5]; one edge of length 0."""
    rng = _rng(row, 't', token)
    t = rng.uniform(0.05, 0.5, size=row.nnodes)
    if zero:
        t[1 + token % (row.nnodes - 1)] = 0.0
    t[0] = 0.0
    return t


def gen_spectral(row, token):
    """(A, lam, B, D) of a reversible rate matrix with state 0 isolated."""
    from raoteh_amd import _spectral
    rng = _rng(row, 'spectral', token)
    n = row.n
    S = rng.uniform(0.1, 1.0, (n, n))
    S = 0.5 * (S + S.T)
    S[0, :] = 0.0
    S[:, 0] = 0.0
    pi = rng.dirichlet(np.ones(n) * 4.0)
    Q = S * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    Q -= np.diag(Q.sum(axis=1))
    Q /= -np.diag(Q)[1:].mean()
    return _spectral.decompose_rate_matrix(Q, pi), Q


def gen_esd(row, token):
    """Row-stochastic matrices with exact zeros, state 0 isolated; the root's slot zero."""
    rng = _rng(row, 'esd', token)
    n, N = row.n, row.nnodes
    P = rng.uniform(0.05, 1.0, (N, n, n)) * (rng.uniform(size=(N, n, n)) < 0.8)
    P[:, np.arange(n), np.arange(n)] += 0.5
    P[:, :, 0] = 0.0
    P[:, 0, :] = 0.0
    P[:, 0, 0] = 1.0
    P /= P.sum(axis=2, keepdims=True)
    P[0] = 0.0
    return P


def gen_root(row, token):
    w = _rng(row, 'root', token).uniform(0.1, 1.0, row.n)
    return w / w.sum()


def gen_weights(row, token):
    """Site multiplicities; one site (not the zero-probability one) has weight 0."""
    w = _rng(row, 'weights', token).randint(1, 5, size=row.nsites).astype(np.float64)
    w += 0.25 * (token % 3)
    w[fixed_of(row).zero_weight_site] = 0.0
    return w


def gen_sets(row, token, K, nq):
    """(Q f64[K, nq, n, n], node_q or None, t f64[K, nnodes]); a zero-length edge where nq == 2."""
    rng = _rng(row, 'sets', token)
    Q = np.stack([np.stack([iso_rate_matrix(row.n, rng) * rng.uniform(0.5, 2.0) for _ in range(nq)])
                  for _ in range(K)])
    t = rng.uniform(0.05, 0.5, size=(K, row.nnodes))
    if nq == 2:
        t[token % K, 1 + token % (row.nnodes - 1)] = 0.0
    t[:, 0] = 0.0
    return Q, (fixed_of(row).node_q if nq == 2 else None), t


def gen_class_weights(row, token, K):
    c = _rng(row, 'cw', token).uniform(0.1, 1.0, K)
    if K == 3:
        c[1] = 0.0                                 # (a class that is skipped)
    return c


# ---- shadow state ---------------------------------------------------------------------------------

class Params(object):
    """One snapshot of what the library was told.  mode: what the transition matrices are made of
    ('rates', 'spectral', 'direct'); rates_kind: what the resident rates are ('rates', 'spectral'):
    what recompute_transitions rebuilds the matrices from."""
    __slots__ = ('Q', 'nq', 't', 'mode', 'rates_kind', 'spec', 'esd', 'root', 'weights', 'sets',
                 'K', 'set_nq', 'cw')

    def __init__(self):
        self.Q, self.nq, self.t = 0, 1, 0
        self.mode = self.rates_kind = 'rates'
        self.spec = self.esd = None
        self.root = 0                              # token, or None: weights of one
        self.weights = None                        # token, or None: every site counts once
        self.sets, self.K, self.set_nq, self.cw = None, 0, 1, None

    def key(self):
        return tuple(getattr(self, k) for k in self.__slots__)


class Shadow(object):
    """cur, and the snapshots of the last launch of each kind (None before the first; `multi_ok` /
    `part_ok`: the rate-set epoch of that launch is still the model's)."""

    def __init__(self, row):
        self.row = row
        self.cur = Params()
        self.pruned = self.multi = self.part = None
        self.multi_ok = self.part_ok = False
        self.waited = not row.background          # the batch runs its final kernel
        # ... and did when the last launch of that kind ran (a background row only: before, the
        # long-lived batch and a twin may run either kernel)
        self.pruned_final = self.multi_final = True
        self.clock = 0                             # the next parameter token

    def copy(self):
        s = copy.copy(self)
        s.cur = copy.copy(self.cur)
        return s

    def tick(self):
        self.clock += 1
        return self.clock

    @property
    def rates_current(self):
        return self.cur.mode != 'direct'

    @property
    def epoch_ok(self):
        return self.part_ok if self.row.partitioned else self.multi_ok


# ---- the reads: ONE table ---------------------------------------------------------------------------
# snapshot: which snapshot the read answers from ('cur', 'pruned', 'multi', 'part');
# needs: '' nothing but transition matrices | 'rates' resident rates of either kind that describe the
#   matrices | 'rateq' resident rate MATRICES that describe them (no spectral rates) | 'rateq1' the
#   same, and ONE rate matrix for all edges | 'sets' rate sets | 'sets1' rate sets of ONE matrix each
#   (and, for the mixture gradient, no resident length of 0) | 'launch' the snapshot's launch with a
#   valid epoch;
# deps: the parameters the result depends on (Q, t, root, weights, sets, cw);
# flag: the read takes recompute_transitions; kinds: 'o' ordinary batch, 'p' partitioned batch;
# cite: the line of include/raoteh_hip.h (device.py where marked) this row is taken from.
Read = collections.namedtuple('Read', 'name snapshot needs deps flag kinds cite')

READS = [
    Read('loglik', 'pruned', 'launch', ('Q', 't', 'root'), False, 'o',
         'rt_sites_get_logliks: "What the last rt_prune / rt_step of the batch wrote (or its clone '
         'source\'s); RT_ERR_INVALID for a batch that no pruning kernel has written yet."'),
    Read('expected_history_statistics', 'cur', 'rateq', ('Q', 't', 'root', 'weights'), True, 'o',
         'rt_expect_step: "rates set by rt_model_set_rates ... RT_ERR_INVALID for spectral rates, '
         'and for transitions set directly after the rates with recompute_transitions == 0" '
         '(second half added by this suite: the header did not say)'),
    Read('posteriors', 'cur', '', ('Q', 't', 'root'), True, 'o',
         'rt_sites_posteriors: "models whose transitions came from any of the rt_model_set_* calls '
         '(recompute_transitions != 0 needs rates) ... the batch keeps its kernel, log-likelihoods, '
         'status and totals"'),
    Read('sample_states', 'cur', '', ('Q', 't', 'root'), True, 'o',
         'rt_sites_sample_states: "transitions from any of the rt_model_set_* calls '
         '(recompute_transitions != 0 needs rates)"'),
    Read('map_states', 'cur', '', ('Q', 't', 'root'), True, 'o',
         'rt_sites_map_states: "Batches and trees: those of rt_sites_sample_states ... nothing of '
         'the batch is written"'),
    Read('sample_mappings', 'cur', 'rateq', ('Q', 't', 'root'), True, 'o',
         'rt_sites_sample_mappings: "The rates must come from rt_model_set_rates: RT_ERR_INVALID '
         'for spectral rates or transitions set directly"'),
    Read('branch_expectations', 'cur', 'rateq', ('Q', 't', 'root', 'weights'), True, 'o',
         'rt_sites_branch_expectations: "The rates must come from rt_model_set_rates (the '
         'derivative needs Q): RT_ERR_INVALID for a model with spectral rates or with transitions '
         'set directly"'),
    Read('branch_length_gradient', 'cur', 'rateq1', ('Q', 't', 'root', 'weights'), True, 'o',
         'device.py TreeModel.branch_length_gradient: "For a model with ONE rate matrix ... with '
         'per-edge rate matrices ... ValueError then"; else rt_sites_branch_expectations'),
    Read('branch_profiles', 'cur', 'rates', ('Q', 't', 'root', 'weights'), True, 'o',
         'rt_sites_branch_profiles: "RT_ERR_INVALID: no rates (transitions set directly: on a model '
         'that never had rates, or after them with recompute_transitions == 0"'),
    Read('nni_scores', 'cur', 'rates', ('Q', 't', 'root', 'weights'), True, 'o',
         'rt_sites_nni_scores: "RT_ERR_INVALID: ... lengths on a model without rates (or whose '
         'transitions were set directly after them, with recompute_transitions == 0)"'),
    Read('spr_scores', 'cur', 'rates', ('Q', 't', 'root', 'weights'), True, 'o',
         'rt_sites_spr_scores: "RT_ERR_INVALID: ... a model without rates (or whose transitions '
         'were set directly after them, with recompute_transitions == 0)"'),
    Read('place_queries', 'cur', 'rates', ('Q', 't', 'root', 'weights'), True, 'o',
         'rt_sites_placements: "RT_ERR_INVALID: ... a model without rates (or whose transitions '
         'were set directly after them, with recompute_transitions == 0)"'),
    Read('multi', 'multi', 'launch', ('sets', 'root', 'weights'), False, 'o',
         'section 2b: "The getters and the mixture ... return RT_ERR_INVALID before any '
         'rt_step_multi of the batch and after the number of rate sets changed (until the next '
         'rt_step_multi)"; weighted_sums: "w from rt_sites_set_weights at the time of the step"'),
    Read('mixture_log_likelihoods', 'multi', 'launch', ('sets', 'root', 'weights', 'cw'), False, 'o',
         'rt_sites_multi_mixture: as the getters of section 2b; "with the site weights applied to '
         'totals[0]" (the weights of the time of the call: added to the header by this suite)'),
    Read('class_posteriors', 'cur', 'sets', ('sets', 'root', 'cw'), True, 'o',
         'rt_sites_branch_expectations_mixture: "no earlier rt_step_multi is needed ... '
         'RT_ERR_INVALID: no rate sets"'),
    Read('branch_expectations_mixture', 'cur', 'sets', ('sets', 'root', 'weights', 'cw'), True, 'o',
         'rt_sites_branch_expectations_mixture: "no earlier rt_step_multi is needed ... '
         'RT_ERR_INVALID: no rate sets"'),
    Read('branch_length_gradient_mixture', 'cur', 'sets1', ('sets', 'root', 'weights', 'cw'), True,
         'o', 'device.py TreeModel.branch_length_gradient_mixture: "ValueError for several rate '
              'matrices per set ... and for a resident t[k][v] == 0 below the root"'),
    Read('partition_loglik', 'part', 'launch', ('sets', 'root', 'weights'), False, 'p',
         'section 2c: "The getters synchronise; they return RT_ERR_INVALID before the first '
         'rt_step_partitioned ... and after the model\'s number of rate sets changed, until the next '
         'rt_step_partitioned"; weighted_sums: "at the time of the step"'),
    Read('branch_expectations_partitioned', 'cur', 'sets', ('sets', 'root', 'weights'), True, 'p',
         'rt_sites_branch_expectations_partitioned: "no earlier rt_step_partitioned is needed"'),
    Read('branch_length_gradient_partitioned', 'cur', 'sets1', ('sets', 'root', 'weights'), True,
         'p', 'device.py TreeModel.branch_length_gradient_partitioned: "For ONE rate matrix per set '
              '... ValueError then"'),
]
READ = dict((r.name, r) for r in READS)

# reads of an ordinary batch a partitioned batch refuses, with the check they fail first (section 2c:
# "Everything else refuses a partitioned batch with RT_ERR_UNSUPPORTED and leaves it untouched:
# ... rt_expect_step, rt_sites_posteriors, ... rt_sites_sample_states, rt_sites_map_states")
PART_REFUSED_READS = ('expected_history_statistics', 'posteriors', 'sample_states', 'map_states')
# launches and calls a partitioned batch refuses (the same sentence: rt_prune, rt_step_multi,
# rt_sites_clone)
PART_REFUSED_MUTATORS = ('prune', 'step_multi', 'clone')

MUTATORS_ORDINARY = (
    'set_rates_Q', 'set_rates_per_edge', 'set_rates_t', 'set_rates_spectral', 'set_transitions',
    'recompute_transitions', 'set_root_w', 'set_root_none', 'set_weights_w', 'set_weights_none',
    'set_rate_sets_same', 'set_rate_sets_other', 'set_rate_sets_per_edge', 'prune', 'step_true', 'step_false', 'step_multi',
    'clone', 'wait_for_kernel')
MUTATORS_PARTITIONED = (
    'set_rates_Q', 'set_root_w', 'set_root_none', 'set_weights_w', 'set_weights_none',
    'set_rate_sets_same', 'set_rate_sets_other', 'set_rate_sets_per_edge',
    'step_partitioned_true', 'step_partitioned_false') + PART_REFUSED_MUTATORS

# what the comparison may see differ in bits, with the sentence that allows it.  key: (row name,
# read name) -> (fields, citation, relative tolerance: the one the read's own parity test uses).
# An entry holds only while `tolerance` below says so: where the launch the read answers from ran
# before wait_for_kernel (or a clone, which waits), when the long-lived batch and its twin may run
# either kernel; after it both run the tree-specialised kernel and the bits must match.
EXCEPTIONS = {
    ('lane-background-n4-mask-38', 'loglik'): (
        ('totals',),
        'DESIGN.md section 4: "The lane family (n <= 4) too: its kernel\'s resident layout differs '
        'from the interpreter\'s (sites per wave balanced over the CUs ...) ... at the switch ... the '
        'per-site outputs and partial sums are re-allocated for the new block size": the batch sum is '
        'reduced in the block order of the kernel that ran.  Tolerance: the one of '
        'test_resident_reads_gpu.check_loglik for the totals against the sum of the per-site values '
        '("rel = ... 1e-12")', 1e-12),
    ('lane-background-n4-mask-38', 'multi'): (
        ('totals', 'weighted_sums'),
        'as (lane-background-n4-mask-38, loglik): section 2b gives totals[k] "the bits of '
        'rt_sites_get_totals after a separate step with set k", which go by the kernel that ran',
        1e-12),
}


def tolerance(state, read):
    """(fields, relative tolerance) of the EXCEPTIONS entry that holds for `read` in this state, or
    None: bit for bit."""
    exc = EXCEPTIONS.get((state.row.name, read))
    if exc is None:
        return None
    final = state.pruned_final if READ[read].snapshot == 'pruned' else state.multi_final
    return None if final else (exc[0], exc[2])


def reads_of(row):
    if row.partitioned:
        return [r.name for r in READS if 'p' in r.kinds] + list(PART_REFUSED_READS)
    return [r.name for r in READS if 'o' in r.kinds]


RECOMPUTE = 'recompute:'


def mutators_of(row):
    """The mutators of the catalogue, and every read that has the flag called with
    recompute_transitions=True."""
    return (list(MUTATORS_PARTITIONED if row.partitioned else MUTATORS_ORDINARY)
            + [RECOMPUTE + r for r in flagged_reads(row)])


def ops_of(row):
    return mutators_of(row) + reads_of(row)


def flagged_reads(row):
    """The reads that take recompute_transitions."""
    return [r for r in reads_of(row) if READ[r].flag and
            not (row.partitioned and r in PART_REFUSED_READS)]


# ---- expected outcome and state transition ------------------------------------------------------

def read_outcome(s, name, recompute=False):
    """'ok' or the error code the header documents for this read in state s.  Every refusal below
    is decided on the host before anything is launched (post_open, post_grid::check, the RT_REQUIRE
    lines at the head of each entry point, sites_multi_ready, the wrapper's own ValueErrors)."""
    row, c = s.row, s.cur
    r = READ[name]
    if row.partitioned and name in PART_REFUSED_READS:
        return UNSUPPORTED
    described = s.rates_current or recompute
    if r.needs == 'launch':
        snap = getattr(s, r.snapshot)
        ok = snap is not None and (r.snapshot == 'pruned' or s.epoch_ok)
        return 'ok' if ok else INVALID
    if r.needs == 'rates':
        return 'ok' if described else INVALID
    if r.needs in ('rateq', 'rateq1'):
        if c.rates_kind != 'rates' or not described:
            return INVALID
        if r.needs == 'rateq1' and c.nq != 1:
            return INVALID
        return 'ok'
    if r.needs in ('sets', 'sets1'):
        if c.sets is None:
            return INVALID
        if r.needs != 'sets' and c.set_nq != 1:
            return INVALID                         # (sets of two matrices have a zero-length edge too)
        return 'ok'
    return 'ok'


def mutator_outcome(s, name):
    row = s.row
    if row.partitioned and name in PART_REFUSED_MUTATORS:
        return UNSUPPORTED
    if name == 'set_rates_spectral' and row.n > 64:
        return UNSUPPORTED                         # rt_model_set_rates_spectral: "n <= 64"
    if name == 'step_multi' and s.cur.sets is None:
        return INVALID                             # "RT_ERR_INVALID without rate sets"
    if name.startswith('step_partitioned') and s.cur.sets is None:
        return INVALID
    if name.startswith(RECOMPUTE):
        return read_outcome(s, name[len(RECOMPUTE):], True)
    return 'ok'


def outcome(s, op):
    return read_outcome(s, op) if op in READ else mutator_outcome(s, op)


def _recomputed(c):
    c.mode = c.rates_kind


def other_K(row, K):
    if row.partitioned:
        return PART_NSETS + 1 if K == PART_NSETS else PART_NSETS
    return 2 if K == 3 else 3


def apply(s, op):
    """The state after a call that succeeded (a refused call leaves everything as it was: the
    caller does not apply it).  Returns the new state; s is not changed."""
    s = s.copy()
    c, row = s.cur, s.row
    if op in READ:
        return s
    if op in ('set_rates_Q', 'set_rates_per_edge'):
        c.Q, c.nq = s.tick(), (2 if op == 'set_rates_per_edge' else 1)
        c.mode = c.rates_kind = 'rates'
    elif op == 'set_rates_t':
        c.t = s.tick()
        c.mode = c.rates_kind = 'rates'            # (set_rates with the last Q and node_q again)
    elif op == 'set_rates_spectral':
        c.spec = c.t = s.tick()
        c.mode = c.rates_kind = 'spectral'
    elif op == 'set_transitions':
        c.esd = s.tick()
        c.mode = 'direct'
    elif op == 'recompute_transitions':
        _recomputed(c)
    elif op == 'set_root_w':
        c.root = s.tick()
    elif op == 'set_root_none':
        c.root = None
    elif op == 'set_weights_w':
        c.weights = s.tick()
    elif op == 'set_weights_none':
        c.weights = None
    elif op in ('set_rate_sets_same', 'set_rate_sets_other', 'set_rate_sets_per_edge'):
        # same: the K there is, one matrix per set; other: another K, one matrix per set;
        # per_edge: the K there is, two matrices per set and a node_q, one edge of length 0
        first = c.sets is None
        K = c.K if not first else (PART_NSETS if row.partitioned else 3)
        if op == 'set_rate_sets_other' and not first:
            K = other_K(row, K)
        c.set_nq = 2 if op == 'set_rate_sets_per_edge' else 1
        if K != c.K:                               # the epoch: results of another K are stale
            s.multi_ok = s.part_ok = False
            c.cw = s.tick()
        c.K = K
        c.sets = s.tick()
    elif op == 'prune' or op == 'step_false':
        s.pruned, s.pruned_final = copy.copy(c), s.waited
    elif op == 'step_true':
        _recomputed(c)
        s.pruned, s.pruned_final = copy.copy(c), s.waited
    elif op == 'step_multi':
        s.multi, s.multi_ok, s.multi_final = copy.copy(c), True, s.waited
    elif op.startswith('step_partitioned'):
        s.part, s.part_ok = copy.copy(c), True
    elif op == 'clone':
        # rt_sites_clone: "the same observations, pruning kernel, per-site log-likelihoods, statuses
        # and totals ... (Site weights are not copied.)" -- nor the rt_step_multi results (added to
        # the header by this suite); a clone of a lane-family batch waits for its kernel
        c.weights = None
        s.multi, s.multi_ok = None, False
        if row.n <= 4:
            s.waited = True
    elif op == 'wait_for_kernel':
        s.waited = True
    elif op.startswith(RECOMPUTE):
        name = op[len(RECOMPUTE):]
        if READ[name].snapshot == 'cur' and READ[name].needs not in ('sets', 'sets1'):
            _recomputed(c)                         # (the rate-set reads rebuild the sets' tables)
    else:
        raise KeyError(op)
    return s


def initial_state(row):
    """What setup_calls leave: rates, root weights, the upload; no weights, no rate sets, no launch."""
    return Shadow(row)


# ---- the refusals the header documents for the pair itself ------------------------------------------

def documented_refusals(row):
    """The pairs (operation, read) whose read the header refuses right after the operation, whatever
    came before.  Everything else must be live somewhere in the walk."""
    out = set()
    ops, reads = ops_of(row), reads_of(row)
    for r in reads:
        if row.partitioned and r in PART_REFUSED_READS:
            out.update((x, r) for x in ops)        # a read the batch kind does not support
            continue
        needs = READ[r].needs
        if needs in ('rates', 'rateq', 'rateq1'):
            out.add(('set_transitions', r))        # transitions set directly after the rates
        if needs in ('rateq', 'rateq1') and row.n <= 64:
            out.add(('set_rates_spectral', r))     # spectral rates have no rate matrix
        if needs == 'rateq1':
            out.add(('set_rates_per_edge', r))     # no single E has every edge's diag(Q)
        if needs == 'launch' and READ[r].snapshot in ('multi', 'part'):
            out.add(('set_rate_sets_other', r))    # the epoch: the number of rate sets changed
        if needs == 'launch' and READ[r].snapshot == 'multi':
            out.add(('clone', r))                  # a clone carries no rt_step_multi results
        if needs == 'sets1':
            out.add(('set_rate_sets_per_edge', r))  # several matrices per set / a zero length
    return set(p for p in out if p[0] in ops)


# ---- the walk ---------------------------------------------------------------------------------------

def euler_circuit(row, seed):
    """Hierholzer over the graph with an edge (x, r) for every operation x and read r and an edge
    (r, m) for every read r and mutator m: every node is balanced, so one closed walk takes every
    edge once.  Starts and ends at the first read."""
    rng = np.random.RandomState(seed)
    muts, reads = mutators_of(row), reads_of(row)
    out = {}
    for x in muts:
        out[x] = list(reads)
    for r in reads:
        out[r] = list(reads) + list(muts)
    for x in sorted(out):
        rng.shuffle(out[x])
    start = reads[0]
    stack, circuit = [start], []
    while stack:
        v = stack[-1]
        if out[v]:
            stack.append(out[v].pop())
        else:
            circuit.append(stack.pop())
    circuit.reverse()
    return circuit


FIXERS_ORDINARY = ('set_rates_Q', 'set_rate_sets_same', 'prune', 'step_multi')
FIXERS_PARTITIONED = ('set_rate_sets_same', 'step_partitioned_true')


def simulate(row, ops, state=None):
    """[(op, expected outcome, state after)] of a sequence of operations."""
    s = state if state is not None else initial_state(row)
    out = []
    for op in ops:
        res = outcome(s, op)
        if res == 'ok':
            s = apply(s, op)
        out.append((op, res, s))
    return out


def live_pairs(row, trace):
    reads = set(reads_of(row))
    return set((a[0], b[0]) for a, b in zip(trace, trace[1:]) if b[0] in reads and b[1] == 'ok')


def adjacent_pairs(row, ops):
    reads = set(reads_of(row))
    return set((a, b) for a, b in zip(ops, ops[1:]) if b in reads)


# pieces a row's walk is cut into, each a test case of its own that starts from a fresh long-lived
# pair (a few seconds per case on the device)
SEGMENTS = {}


def build_segments(row, nseg=None, seed=0):
    """The row's walk as nseg lists of operation names.  The Euler circuit is cut into pieces of
    about equal length, every cut repeating the operation before it so that no adjacent pair is
    lost; every piece starts from a fresh long-lived pair.  Then the repairs: a pair that is live in
    no piece -- its read was refused at its one occurrence for reasons older than the pair -- is
    appended to the last piece behind the shortest prefix of FIXERS that makes the read live."""
    nseg = SEGMENTS.get(row.name, 1) if nseg is None else nseg
    ops = euler_circuit(row, seed + row.seed)
    size = (len(ops) + nseg - 1) // nseg
    pieces = [list(ops[max(0, i * size - 1):(i + 1) * size]) for i in range(nseg)]
    live = set()
    for piece in pieces:
        trace = simulate(row, piece)
        live |= live_pairs(row, trace)
    missing = sorted(set(itertools.product(ops_of(row), reads_of(row))) - live
                     - documented_refusals(row))
    fixers = FIXERS_PARTITIONED if row.partitioned else FIXERS_ORDINARY
    state = trace[-1][2]
    for a, b in missing:
        found = None
        for k in range(len(fixers) + 1):
            for prefix in itertools.combinations(fixers, k):      # (in the order of `fixers`)
                t = simulate(row, list(prefix) + [a, b], state)
                if t[-1][1] == 'ok':
                    found = list(prefix)
                    break
            if found is not None:
                break
        if found is None:
            raise AssertionError('no prefix makes %s live after %s in row %s' % (b, a, row.name))
        pieces[-1].extend(found + [a, b])
        state = t[-1][2]
    return pieces


# ---- calls on real objects --------------------------------------------------------------------------

_arrays_cache = {}


def materialise(row, p):
    """The arrays of a snapshot: dict with Q, node_q, t, spec, esd, root, weights, sets, cw (shared
    between callers: never written)."""
    key = (row.name, p.key())
    if key not in _arrays_cache:
        if len(_arrays_cache) > 64:
            _arrays_cache.clear()
        _arrays_cache[key] = _materialise(row, p)
    return _arrays_cache[key]


def _materialise(row, p):
    fx = fixed_of(row)
    a = {}
    a['Q'] = gen_Q(row, p.Q, p.nq)
    a['node_q'] = fx.node_q if p.nq == 2 else None
    if p.rates_kind == 'spectral':
        a['spec'], a['Qspec'] = gen_spectral(row, p.spec)
    a['t'] = gen_t(row, p.t)
    a['esd'] = gen_esd(row, p.esd) if p.esd is not None else None
    a['root'] = gen_root(row, p.root) if p.root is not None else None
    a['weights'] = gen_weights(row, p.weights) if p.weights is not None else None
    a['sets'] = gen_sets(row, p.sets, p.K, p.set_nq) if p.sets is not None else None
    a['cw'] = gen_class_weights(row, p.cw, p.K) if p.cw is not None else None
    return a


def set_model_transitions(model, row, p, a):
    """ONE call that gives the model the transition matrices of snapshot p."""
    if p.mode == 'direct':
        model.set_transitions(a['esd'])
    elif p.mode == 'spectral':
        A, lam, B, D = a['spec']
        model.set_rates_spectral(A, lam, B, D=D, t=a['t'])
    else:
        model.set_rates(Q=a['Q'], node_q=a['node_q'], t=a['t'])


def upload(model, row):
    fx = fixed_of(row)
    if row.partitioned:
        return model.upload_sites(fx.obs_nodes, fx.data, kind=row.kind, site_sets=fx.site_sets,
                                  nsets=PART_NSETS)
    return model.upload_sites(fx.obs_nodes, fx.data, kind=row.kind)


def call_read(model, batch, row, name, a, recompute=False):
    """The read `name` with the row's fixed arguments -> the wrapper's return value."""
    fx = fixed_of(row)
    kw = {'recompute_transitions': True} if recompute else {}
    cw = a['cw'] if a['cw'] is not None else np.ones(max(1, getattr(model, '_nsets', 0) or 1))
    if name == 'loglik':
        ll, st = model.fetch_log_likelihoods(batch)
        return {'loglik': ll, 'status': st, 'totals': model.fetch_totals(batch)}
    if name == 'expected_history_statistics':
        return model.expected_history_statistics(batch, recompute_transitions=recompute,
                                                 return_status=True)
    if name == 'posteriors':
        return model.posteriors(batch, node_sets=fx.node_sets, edge_sets=fx.edge_sets,
                                marginal_nodes=fx.marginal_nodes, **kw)
    if name == 'sample_states':
        return model.sample_states(batch, ndraws=2, seed=row.seed, first_draw=3, **kw)
    if name == 'map_states':
        return model.map_states(batch, **kw)
    if name == 'sample_mappings':
        return model.sample_mappings(batch, fx.coefs[:1], ndraws=2, seed=row.seed, first_draw=1, **kw)
    if name == 'branch_expectations':
        return model.branch_expectations(batch, fx.coefs, **kw)
    if name == 'branch_length_gradient':
        return model.branch_length_gradient(batch, **kw)
    if name == 'branch_profiles':
        return model.branch_profiles(batch, factors=(0.5, 1.0, 1.75), per_site=True, **kw)
    if name == 'nni_scores':
        return model.nni_scores(batch, factors=(0.5, 1.5), per_site=True, **kw)
    if name == 'spr_scores':
        return model.spr_scores(batch, radius=2, fractions=(0.25, 0.75), per_site=True, **kw)
    if name == 'place_queries':
        return model.place_queries(batch, fx.queries, kind='state', fractions=(0.5,),
                                   pendant=(0.125,), per_site=True, **kw)
    if name == 'multi':
        ll, st = model.fetch_multi_log_likelihoods(batch)
        tot, ws = model.fetch_multi_totals(batch, weighted=True)
        return {'loglik': ll, 'status': st, 'totals': tot, 'weighted_sums': ws,
                'shape': np.array(ll.shape)}
    if name == 'mixture_log_likelihoods':
        return model.mixture_log_likelihoods(batch, cw)
    if name == 'class_posteriors':
        return model.class_posteriors(batch, cw, **kw)
    if name == 'branch_expectations_mixture':
        return model.branch_expectations_mixture(batch, fx.coefs, cw, **kw)
    if name == 'branch_length_gradient_mixture':
        return model.branch_length_gradient_mixture(batch, cw, **kw)
    if name == 'partition_loglik':
        ll, st = model.fetch_log_likelihoods(batch)
        tot, ws = model.fetch_partition_totals(batch, weighted=True)
        return {'loglik': ll, 'status': st, 'totals': model.fetch_totals(batch),
                'set_totals': tot, 'weighted_sums': ws}
    if name == 'branch_expectations_partitioned':
        return model.branch_expectations_partitioned(batch, fx.coefs, **kw)
    if name == 'branch_length_gradient_partitioned':
        return model.branch_length_gradient_partitioned(batch, **kw)
    raise KeyError(name)


def canonical(value):
    """A wrapper's return value -> [(field, dtype, shape, bytes)]: what the comparison sees."""
    if isinstance(value, dict):
        items = sorted(value.items())
    elif hasattr(value, '_fields'):
        items = list(zip(value._fields, value))
    elif isinstance(value, tuple):
        items = [('item%d' % i, v) for i, v in enumerate(value)]
    else:
        items = [('value', value)]
    out = []
    for k, v in items:
        if v is None:
            out.append((k, 'none', (), b''))
            continue
        arr = np.ascontiguousarray(v)
        out.append((k, str(arr.dtype), arr.shape, arr.tobytes()))
    return out


def attempt(lib, fn):
    """('ok', canonical value) or ('refused', error code); a refusal is the wrapper's ValueError
    (RT_ERR_INVALID and the wrapper's own argument checks) or a RaotehHipError -- but never
    RT_ERR_HIP: a failed HIP call is an error of the library, and it is raised."""
    try:
        value = fn()
    except ValueError:
        return ('refused', INVALID)
    except lib.RaotehHipError as e:
        if e.code == lib.RT_ERR_HIP:
            raise
        return ('refused', e.code)
    return ('ok', canonical(value))


def differences(got, want, tolerate=None):
    """The fields in which two attempts differ: [] when they are the same outcome with the same
    bits.  tolerate: (fields, relative tolerance) of an EXCEPTIONS entry."""
    if got[0] != want[0]:
        brief = lambda x: x if x[0] == 'refused' else ('ok',)
        return ['outcome %r against %r' % (brief(got), brief(want))]
    if got[0] == 'refused':
        return [] if got[1] == want[1] else ['error code %r against %r' % (got[1], want[1])]
    bad = []
    if [g[0] for g in got[1]] != [w[0] for w in want[1]]:
        return ['fields']
    for (k, dt, shape, raw), (_, wdt, wshape, wraw) in zip(got[1], want[1]):
        if (dt, shape) != (wdt, wshape):
            bad.append('%s: %s%s against %s%s' % (k, dt, shape, wdt, wshape))
        elif raw != wraw:
            if tolerate and k in tolerate[0] and dt == 'float64':
                x = np.frombuffer(raw, dtype=np.float64)
                y = np.frombuffer(wraw, dtype=np.float64)
                if np.all(np.abs(x - y) <= tolerate[1] * np.abs(y)):
                    continue
            bad.append(k)
    return bad


class Twin(object):
    """A fresh TreeModel and SiteBatch in `ctx` that were told the snapshot of `read` alone:
    one call for the transition matrices, (the rate sets if the read uses them,) the root weights,
    the upload, the site weights, the snapshot's pruning launch if it has one.  stale: (parameter,
    Params to take it from) for the stale-twin test."""

    def __init__(self, device, ctx, state, read, stale=None):
        row = state.row
        r = READ[read]
        snap = getattr(state, r.snapshot) if r.snapshot != 'cur' else state.cur
        launch = r.snapshot if r.snapshot != 'cur' else None
        if snap is None:                           # no such launch yet: nothing to replay
            snap, launch = state.cur, None
        elif launch in ('multi', 'part') and not state.epoch_ok:
            # the epoch is gone: a twin that steps with the current number of sets and then sees
            # the number change would be the same history again; an unstepped twin refuses alike
            snap, launch = state.cur, None
        cur = state.cur
        if stale is not None:
            snap, cur = copy.copy(snap), copy.copy(cur)
            for p in (snap, cur):
                stale_param(p, stale[0], stale[1])
        a = materialise(row, snap)
        self.arrays = a
        self.model = model = device.TreeModel(fixed_of(row).T, fixed_of(row).root, row.n, ctx=ctx)
        self.batch = None
        set_model_transitions(model, row, snap, a)
        if a['sets'] is not None and (r.needs in ('sets', 'sets1') or launch in ('multi', 'part')
                                      or r.snapshot in ('multi', 'part')):
            Q, node_q, t = a['sets']
            model.set_rate_sets(Q, t=t, node_q=node_q)
        if a['root'] is not None:
            model.set_root_distn(a['root'])
        self.batch = batch = upload(model, row)
        if a['weights'] is not None:
            batch.set_weights(a['weights'])
        if row.background and state.waited:
            batch.wait_for_kernel()
        if launch == 'pruned':
            model.prune(batch)
        elif launch == 'multi':
            model.step_multi(batch, recompute_transitions=False)
        elif launch == 'part':
            model.step_partitioned(batch, recompute_transitions=False)
        # the parameters a read takes at the time of the call, where they changed since the launch
        if launch is not None and cur.weights != snap.weights:
            batch.set_weights(gen_weights(row, cur.weights) if cur.weights is not None else None)
        self.call_arrays = dict(a, cw=gen_class_weights(row, cur.cw, cur.K)
                                if cur.cw is not None else None)

    def read(self, lib, row, name, recompute=False):
        return attempt(lib, lambda: call_read(self.model, self.batch, row, name, self.call_arrays,
                                              recompute))

    def close(self):
        self.model.close()


# which token of a snapshot a parameter of the dependency table is
PARAM_TOKENS = {'Q': ('Q',), 't': ('t',), 'root': ('root',), 'weights': ('weights',),
                'sets': ('sets',), 'cw': ('cw',)}
# the mutator that changes a parameter, and the launch kinds that take it into their snapshots
PARAM_MUTATOR = {'Q': 'set_rates_Q', 't': 'set_rates_t', 'root': 'set_root_w',
                 'weights': 'set_weights_w', 'sets': 'set_rate_sets_same', 'cw': None}


def stale_param(p, param, old):
    for k in PARAM_TOKENS[param]:
        setattr(p, k, getattr(old, k))


def stale_cases(row):
    """[(read, parameter)]: the dependency table of the row's reads."""
    return [(r, p) for r in reads_of(row) if not (row.partitioned and r in PART_REFUSED_READS)
            for p in READ[r].deps]


def stale_states(row, read, param):
    """(state, old): a state in which `read` is live and `param` was changed last -- and launched, so
    that every snapshot holds the change -- and the snapshot `old` from before that change."""
    base = ['set_root_w', 'set_weights_w', 'set_rate_sets_same']
    launches = (['step_partitioned_true'] if row.partitioned else ['prune', 'step_multi'])
    s = simulate(row, base + launches)[-1][2]
    old = copy.copy(s.cur)
    if PARAM_MUTATOR[param] is None:
        s = s.copy()
        s.cur.cw = s.tick()
        seq = launches
    else:
        seq = [PARAM_MUTATOR[param]] + launches
    for op, res, s in simulate(row, seq, s):
        assert res == 'ok', (op, res)
    assert read_outcome(s, read) == 'ok', (read, param)
    return s, old


class LongLived(object):
    """The long-lived model and batch of a walk, and the calls of the catalogue on them."""

    def __init__(self, device, lib, ctx, row):
        self.device, self.lib, self.ctx, self.row = device, lib, ctx, row
        s = initial_state(row)
        a = materialise(row, s.cur)
        self.model = device.TreeModel(fixed_of(row).T, fixed_of(row).root, row.n, ctx=ctx)
        set_model_transitions(self.model, row, s.cur, a)
        self.model.set_root_distn(a['root'])
        self.batch = upload(self.model, row)
        self.state = s

    def run(self, op):
        """Expected outcome from the shadow state, the call itself, the new shadow state.
        -> (expected, attempt, name of the read that ran or None, recompute flag)."""
        row, s = self.row, self.state
        expected = outcome(s, op)
        after = apply(s, op) if expected == 'ok' else s
        a = materialise(row, after.cur)
        model, batch = self.model, self.batch
        read, flag = (op, False) if op in READ else (None, False)
        if op.startswith(RECOMPUTE):
            read, flag = op[len(RECOMPUTE):], True
        if read is not None:
            got = attempt(self.lib, lambda: call_read(model, batch, row, read, a, flag))
        else:
            got = attempt(self.lib, lambda: self.mutate(op, a))
        self.state = after
        return expected, got, read, flag

    def mutate(self, op, a):
        model, batch = self.model, self.batch
        if op in ('set_rates_Q', 'set_rates_per_edge', 'set_rates_t'):
            model.set_rates(Q=a['Q'], node_q=a['node_q'], t=a['t'])
        elif op == 'set_rates_spectral':
            if self.row.n > 64:                    # (no decomposition is made for a call that is refused)
                n = self.row.n
                model.set_rates_spectral(np.eye(n), np.zeros(n), np.eye(n), t=a['t'])
            else:
                A, lam, B, D = a['spec']
                model.set_rates_spectral(A, lam, B, D=D, t=a['t'])
        elif op == 'set_transitions':
            model.set_transitions(a['esd'])
        elif op == 'recompute_transitions':
            model.recompute_transitions()
        elif op in ('set_root_w', 'set_root_none'):
            model.set_root_distn(a['root'])
        elif op in ('set_weights_w', 'set_weights_none'):
            batch.set_weights(a['weights'])
        elif op in ('set_rate_sets_same', 'set_rate_sets_other', 'set_rate_sets_per_edge'):
            Q, node_q, t = a['sets']
            model.set_rate_sets(Q, t=t, node_q=node_q)
        elif op == 'prune':
            model.prune(batch)
        elif op == 'step_true':
            model.step(batch, True)
        elif op == 'step_false':
            model.step(batch, False)
        elif op == 'step_multi':
            model.step_multi(batch)
        elif op == 'step_partitioned_true':
            model.step_partitioned(batch, True)
        elif op == 'step_partitioned_false':
            model.step_partitioned(batch, False)
        elif op == 'clone':
            twin = batch.clone()
            batch.close()
            self.batch = twin
        elif op == 'wait_for_kernel':
            batch.wait_for_kernel()
        else:
            raise KeyError(op)
        return None
