"""What the tests of the one-word Rao-Teh forest kernels share (test_forest_states_cpu.py,
test_forest_states_gpu.py; csrc/forest.hip up to 64 states): a ragged forest per state count with
its host reference from the oracle, a numpy sampler that follows the kernels' rule, and the three
checks the GPU test applies to what the device returns -- sets, pmap, and a replay of every pick
against its Philox uniform."""
import functools

import networkx as nx
import numpy as np

from _forest_wide_cases import sparse_uniformized
from _sample_cases import EPS
from oracle import oracle_numpy as orc
from raoteh_amd._philox import philox_uniform
from raoteh_amd._tree import TreeArrays

# the dispatch of csrc/forest.hip (launch_forest_*), restated: the largest state count of each
# form, in the order the launchers test them
GROUPED_LIMITS = (4, 8, 16)          # *_grouped_kernel<4>, <8>, <16>: 16, 8, 4 trees per wave
ONE_WORD_LIMIT = 64                  # forest_*_kernel: one wave per tree, one lane per state
FAMILY_LIMITS = GROUPED_LIMITS + (ONE_WORD_LIMIT,)
FOREST_CAP = 1024                    # nodes of a wave's LDS image

STATES = [2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 20, 31, 32, 33, 47, 61, 63, 64]
NTREES = 45                          # no multiple of 16, 8 or 4: every last wave partly filled
BIG_STATES = (4, 8, 16, 33, 61)      # these get a tree beyond FOREST_CAP at the end
BIG_NODES = 1100
# the seed of a state count's case; a count missing here uses 1000 + n (61: seed 1061 leaves 27
# feasible trees, test_forest_states_cpu.py asks for 30)
SEEDS = {61: 5061}


def family_of(n):
    """The largest state count of the kernel form that runs n states."""
    for limit in FAMILY_LIMITS:
        if n <= limit:
            return limit
    raise ValueError('%d states: not a one-word kernel' % n)


class ForestCheckError(AssertionError):
    pass


def _restriction(n, rng):
    """A single state, the pair {n - 1, random}, or a random set of up to n / 2 states."""
    u = rng.uniform()
    if u < 1.0 / 3:
        return {int(rng.randint(n))}
    if u < 2.0 / 3:
        return {n - 1, int(rng.randint(n))}
    size = int(rng.randint(1, max(1, n // 2) + 1))
    return set(int(x) for x in rng.choice(n, size=size, replace=False))


def _random_tree(nn, rng, reach=None):
    T = nx.Graph()
    T.add_node(0)
    for k in range(1, nn):
        T.add_edge(int(rng.randint(0 if reach is None else max(0, k - reach), k)), k)
    return T


class TreeRef(object):
    """One tree's host reference: `ta` (TreeArrays), `pset` and `sets` bool[N, n] after the
    backward and after both boolean passes, `L` f64[N, n] subtree likelihoods, `lik` = L[0] . root
    prior, `live` (lik positive and finite)."""

    def __init__(self, T, allowed, P, root):
        n = P.shape[0]
        self.ta = ta = TreeArrays(T, 0)
        self.N = ta.nnodes
        self.parent = ta.parent
        self.esd = esd = np.broadcast_to(P, (ta.nnodes, n, n))
        mask = np.ones((ta.nnodes, n), dtype=np.int64)
        for i, v in enumerate(ta.preorder_nodes):
            if v in allowed:
                mask[i] = 0
                mask[i, sorted(allowed[v])] = 1
        self.allowed = mask.astype(bool)
        orc.mcy_esd_get_node_to_pset(ta.indices, ta.indptr, esd, mask)
        self.pset = mask.astype(bool)
        orc.esd_get_node_to_set(ta.indices, ta.indptr, esd, mask)
        self.sets = mask.astype(bool)
        self.L = orc.mcy_esd_get_node_to_pmap(ta.indices, ta.indptr, esd, mask)
        self.lik = float(self.L[0].dot(root))
        self.live = bool(self.lik > 0 and np.isfinite(self.lik))

    def distn(self, root):
        """The exact node marginals f64[N, n] (mc0_esd_get_node_to_distn)."""
        return orc.mc0_esd_get_node_to_distn(self.ta.indices, self.ta.indptr, self.esd, root,
                                             self.L)


class Case(object):
    pass


@functools.lru_cache(maxsize=None)
def case(n):
    """The case of a state count, built once and shared: Q, P = I + Q / omega (sparse, support
    holds the cycle), `width` (most nonzeros in a row of P: the ELL width), `root` (a prior with
    one zero entry), `trees` [(T, 0)], `obs` [{node: allowed set}], `refs` [TreeRef]."""
    rng = np.random.RandomState(SEEDS.get(n, 1000 + n))
    c = Case()
    c.n = n
    c.Q, c.P = sparse_uniformized(rng, n)
    c.width = int((c.P != 0).sum(axis=1).max())
    c.root = rng.dirichlet(np.ones(n))
    c.root[int(rng.randint(n - 1))] = 0.0
    sizes = [1, 2, 3] + [int(x) for x in rng.randint(2, 14, size=NTREES - 3)]
    c.trees, c.obs = [], []
    for nn in sizes:
        c.trees.append((_random_tree(nn, rng), 0))
        c.obs.append(dict((v, _restriction(n, rng)) for v in range(nn) if rng.uniform() < 1.0 / 3))
    if n >= 34:
        # a set on both sides of lane 32, at the last node of the first tree of four nodes or more
        k = next(k for k, nn in enumerate(sizes) if nn >= 4)
        c.obs[k][sizes[k] - 1] = _restriction(n, rng) | {31, 32}
    if n in BIG_STATES:
        c.trees.append((_random_tree(BIG_NODES, rng, reach=12), 0))
        c.obs.append(dict((int(v), _restriction(n, rng))
                          for v in rng.choice(BIG_NODES, size=10, replace=False)))
    c.refs = [TreeRef(T, d, c.P, c.root) for (T, _), d in zip(c.trees, c.obs)]
    return c


def offsets_of(refs):
    return np.concatenate([[0], np.cumsum([r.N for r in refs])]).astype(np.int64)


def pmap_rtol(N, width, n):
    """The first-order rounding error of the device's and the host's upward pass together: each
    has one dot product of non-negative terms per node (width terms on the device, n on the host,
    each term one product and one sum: relative error (terms + 1) 2^-53 at most) and the product
    over the children runs over N nodes."""
    return max(1e-12, N * (width + n + 2) * 2.0 ** -53)


def check_sets(masks, refs, n):
    """uint64[total] from the device against the oracle's sets, bit for bit below n."""
    off = offsets_of(refs)
    masks = np.asarray(masks, dtype=np.uint64)
    if masks.shape != (off[-1],):
        raise ForestCheckError('shape of the sets')
    bits = ((masks[:, None] >> np.arange(n, dtype=np.uint64)[None, :]) & np.uint64(1)).astype(bool)
    for k, r in enumerate(refs):
        bad = bits[off[k]:off[k + 1]] != r.sets
        if bad.any():
            v = int(np.argwhere(bad)[0][0])
            raise ForestCheckError('tree %d node %d: set %r, expected %r' % (
                k, v, np.nonzero(bits[off[k] + v])[0].tolist(), np.nonzero(r.sets[v])[0].tolist()))


def check_pmap(L, refs, n, width):
    """f64[total, n] from the device against the oracle's pmap: atol 0, rtol pmap_rtol."""
    off = offsets_of(refs)
    L = np.asarray(L)
    if L.shape != (off[-1], n):
        raise ForestCheckError('shape of the pmap')
    for k, r in enumerate(refs):
        got = L[off[k]:off[k + 1]]
        rtol = pmap_rtol(r.N, width, n)
        bad = ~(np.abs(got - r.L) <= rtol * np.abs(r.L))
        if bad.any():
            v, s = np.argwhere(bad)[0]
            raise ForestCheckError('tree %d node %d state %d: pmap %r, expected %r (rtol %.3g)' % (
                k, v, s, got[v, s], r.L[v, s], rtol))


def _groups(refs):
    """Trees that share one TreeRef object, as (ref, tree numbers): one numpy pass each."""
    seen, out = {}, []
    for k, r in enumerate(refs):
        if id(r) not in seen:
            seen[id(r)] = len(out)
            out.append((r, []))
        out[seen[id(r)]][1].append(k)
    return [(r, np.array(ks)) for r, ks in out]


def _weights(r, v, parent_state, P, root, n, copies):
    if v == 0:
        w = np.broadcast_to(r.L[0] * (np.ones(n) if root is None else root), (copies, n))
    else:
        w = P[parent_state] * r.L[v]
    return np.maximum(w, 0.0)


def rule_pick(w, cdf, target):
    """The first positive state whose cumulative weight exceeds the target, else the last
    positive state (rounding at the top)."""
    positive = w > 0
    hit = positive & (cdf > target[:, None])
    first = np.argmax(hit, axis=1)
    last = w.shape[1] - 1 - np.argmax(positive[:, ::-1], axis=1)
    return np.where(hit.any(axis=1), first, last)


def numpy_forest_sample(P, refs, root, n, seed, sweep, pick=rule_pick, weights=None,
                        total_of=None, tree_counter=False):
    """The rule of forest_sample_kernel in numpy -> (states int32[total], status int32[ntrees]).
    Weight max(prior L, 0), cdf in state order, target = philox_uniform(seed, sweep, node's index
    in the whole forest) * total, pick as rule_pick; a tree whose root total is not positive and
    finite: status 1 and -1 at every node.  The keywords swap in the wrong parts of the
    sensitivity tests: another `pick`, `weights(w)`, `total_of(cdf)`, the counter within the
    tree."""
    off = offsets_of(refs)
    states = np.full(off[-1], -1, dtype=np.int32)
    status = np.zeros(len(refs), dtype=np.int32)
    for r, ks in _groups(refs):
        st = np.full((len(ks), r.N), -1, dtype=np.int64)
        for v in range(r.N):
            w = _weights(r, v, None if v == 0 else st[:, r.parent[v]], P, root, n, len(ks))
            if v == 0:
                t0 = w[0].sum()
                if not (t0 > 0 and np.isfinite(t0)):
                    status[ks] = 1
                    break
            if weights is not None:
                w = weights(w)
            cdf = np.cumsum(w, axis=1)
            total = cdf[:, -1] if total_of is None else total_of(cdf)
            index = (0 if tree_counter else off[ks]) + v
            target = philox_uniform(seed, np.uint64(sweep), np.asarray(index, dtype=np.uint64)) * total
            st[:, v] = pick(w, cdf, np.broadcast_to(target, (len(ks),)))
        for j, k in enumerate(ks):
            states[off[k]:off[k + 1]] = st[j]
    return states, status


def forest_replay_check(states, status, P, refs, root, n, seed, sweep, eps=EPS):
    """Every node of every tree, conditional on the pick at the parent: the picked state b has
    w[b] > 0 and cdf[b - 1] - eps total <= u total <= cdf[b] + eps total, with w from the
    oracle's L and u from _philox at the node's index in the whole forest.  Status 0 / 1 and the
    -1 states as the host likelihood says.  Nothing is left out.  Returns the picks checked."""
    off = offsets_of(refs)
    states = np.asarray(states)
    status = np.asarray(status)
    if states.shape != (off[-1],) or status.shape != (len(refs),):
        raise ForestCheckError('shapes of states and status')
    checked = 0
    for r, ks in _groups(refs):
        w0 = np.maximum(r.L[0] * (np.ones(n) if root is None else root), 0.0)
        t0 = w0.sum()
        live = bool(t0 > 0 and np.isfinite(t0))
        st = np.stack([states[off[k]:off[k + 1]] for k in ks]).astype(np.int64)
        if not (status[ks] == (0 if live else 1)).all():
            raise ForestCheckError('tree %d: status %r, likelihood %r' % (
                ks[0], status[ks][:8].tolist(), t0))
        if not live:
            if not (st == -1).all():
                raise ForestCheckError('tree %d: a zero-likelihood tree has a state' % ks[0])
            continue
        if ((st < 0) | (st >= n)).any():
            raise ForestCheckError('tree %d: a state outside [0, %d)' % (ks[0], n))
        for v in range(r.N):
            b = st[:, v]
            w = _weights(r, v, None if v == 0 else st[:, r.parent[v]], P, root, n, len(ks))
            cdf = np.cumsum(w, axis=1)
            total = cdf[:, -1]
            at = np.arange(len(ks))
            wb, hi = w[at, b], cdf[at, b]
            lo = np.where(b > 0, cdf[at, np.maximum(b - 1, 0)], 0.0)
            index = (off[ks] + v).astype(np.uint64)
            target = philox_uniform(seed, np.uint64(sweep), index) * total
            bad = ~(wb > 0) | (target < lo - eps * total) | (target > hi + eps * total)
            if bad.any():
                j = int(np.nonzero(bad)[0][0])
                raise ForestCheckError(
                    'tree %d node %d: state %d with w = %r, target %r outside [%r, %r] '
                    '(%d of %d picks of the node fail)' % (ks[j], v, b[j], wb[j], target[j], lo[j],
                                                           hi[j], bad.sum(), bad.size))
            checked += bad.size
    return checked
