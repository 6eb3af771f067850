"""Rao-Teh sampling for 65 to 128 states (csrc/forest.hip, the *_wide_kernel siblings and the
two-word instantiations of the sweep kernels): a lane owns the states `lane` and `lane + 64`, a
set is two uint64 words.  Against the reference's un-accelerated passes and exact marginals
(tests/golden/forest_wide.json), against the one-word kernels on an embedded 64-state problem,
against a closed-form stationary law and against the expectation path at 122 states.  The
tolerances are those of the sampler tests for up to 64 states in test_gpu_parity.py."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from _forest_wide_cases import (check_lumped_cycle_law, check_resident_histories, forest_wide_cases,
                                rows, sparse_uniformized)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ra():
    import raoteh_amd
    from raoteh_amd import device, _lib, synth, pyfelscore_compat

    class NS(object):
        pass
    ns = NS()
    ns.pkg, ns.device, ns.lib, ns.synth, ns.pyf = raoteh_amd, device, _lib, synth, pyfelscore_compat
    ns.ctx = device.get_context()
    return ns


# ---------------------------------------------------------------------------
# 4, 5, 6: the fixture from the reference
# ---------------------------------------------------------------------------

def test_wide_forest_passes_match_the_reference(ra):
    """pset / set / pmap of every chunk tree of forest_wide.json, each in a ragged batch with
    unrestricted trees of the same state count, against the reference's un-accelerated passes:
    sets equal, pmap within rtol 1e-12 (atol 0); the companions keep the full set and pmap 1."""
    from raoteh_amd import _forest
    cases = forest_wide_cases()
    done = 0
    for c, T in cases:
        n = c['nstates']
        allowed = dict((int(v), set(ss)) for v, ss in c['allowed'].items())
        other = [(T2, c2) for c2, T2 in cases if c2['nstates'] == n and c2 is not c][:3]
        assert other
        trees = [(T, c['root'])] + [(T2, c2['root']) for T2, c2 in other]
        obs = [allowed] + [None] * len(other)
        forest = _forest.Forest(trees)
        sets, pmaps = _forest.get_node_to_set_and_pmap(forest, c['P'], obs)
        if c.get('single'):
            # one chunk: nothing to pass along; the node keeps its allowed set
            assert sets[0][c['root']] == allowed[c['root']]
            np.testing.assert_array_equal(
                pmaps[0][c['root']], [1.0 if s in allowed[c['root']] else 0.0 for s in range(n)])
        else:
            for v in T:
                assert sets[0][v] == set(c['set'][str(v)]), (v, sets[0][v], c['set'][str(v)])
                np.testing.assert_allclose(pmaps[0][v], rows(c['pmap'], v, n), rtol=1e-12, atol=0)
        for k in range(1, len(trees)):
            for v in trees[k][0]:
                assert sets[k][v] == set(range(n))
                np.testing.assert_allclose(pmaps[k][v], 1.0, rtol=1e-12)
        done += 1
    assert done >= 10


def test_wide_pyfelscore_shared_matrix_passes(ra):
    """pyfelscore.mcy_get_node_to_pset / get_node_to_set with the reference's argument lists
    (_mcy.py:158,168,259) at 65..128 states reproduce pset and set exactly; the forward pass
    alone removes only what the root's set cannot reach."""
    from raoteh_amd._tree import TreeArrays
    pyf = ra.pyf
    done = 0
    for c, T in forest_wide_cases():
        if c.get('single'):
            continue
        n = c['nstates']
        P = c['P']
        ta = TreeArrays(T, c['root'])
        tptr = np.concatenate([[0], np.cumsum((P != 0).sum(axis=1))]).astype(np.int64)
        tidx = np.nonzero(P != 0)[1].astype(np.int64)
        mask = np.zeros((ta.nnodes, n), dtype=np.int64)
        for i, v in enumerate(ta.preorder_nodes):
            mask[i, sorted(c['allowed'][str(v)])] = 1
        pyf.mcy_get_node_to_pset(ta.indices, ta.indptr, tidx, tptr, mask)
        for i, v in enumerate(ta.preorder_nodes):
            assert set(np.nonzero(mask[i])[0]) == set(c['pset'][str(v)]), (v, mask[i])
        tmp = np.zeros(n, dtype=np.int64)
        pyf.get_node_to_set(ta.indices, ta.indptr, tidx, tptr, mask, tmp)
        for i, v in enumerate(ta.preorder_nodes):
            assert set(np.nonzero(mask[i])[0]) == set(c['set'][str(v)]), (v, mask[i])
        for start in (0, n - 1):                 # a root state in the low and in the high word
            raw = np.ones((ta.nnodes, n), dtype=np.int64)
            raw[0] = 0
            raw[0, start] = 1
            want = raw.copy()
            for i in range(ta.nnodes):
                for j in range(ta.indptr[i], ta.indptr[i + 1]):
                    k = ta.indices[j]
                    want[k] &= ((P != 0)[want[i] != 0].any(axis=0)).astype(np.int64)
            pyf.get_node_to_set(ta.indices, ta.indptr, tidx, tptr, raw, None)
            np.testing.assert_array_equal(raw, want)
        done += 1
    assert done >= 9


def test_wide_forest_sampling_follows_the_exact_posterior(ra):
    """4 000 replicates per case against the reference's exact node marginals
    (_mc0.get_node_to_distn): never a state outside the support, frequencies within
    5 sigma + 1e-9, every sampled parent -> child pair a transition of P; zero-likelihood
    trees are flagged and raise; (seed, sweep) fixes the draws."""
    from raoteh_amd import _forest
    reps = 4000
    for c, T in forest_wide_cases():
        if c.get('single'):
            continue
        n = c['nstates']
        P = c['P']
        allowed = dict((int(v), set(ss)) for v, ss in c['allowed'].items())
        distn = np.array(c['root_distn'])
        forest = _forest.Forest([(T, c['root'])] * reps)
        obs = [allowed] * reps
        states, status = _forest.resample_states(forest, P, obs, root_distn=distn,
                                                 seed=99, sweep=3, return_status=True)
        if c['zero']:
            assert (status == 1).all()
            assert all(s == -1 for d in states for s in d.values())
            with pytest.raises(ra.pkg.StructuralZeroProb):
                _forest.resample_states(forest, P, obs, root_distn=distn, seed=99, sweep=3)
            continue
        assert not status.any()
        for v in T:
            want = rows(c['distn'], v, n)
            got = np.bincount([d[v] for d in states], minlength=n) / float(reps)
            assert not got[want == 0].any(), (v, got, want)
            sigma = np.sqrt(np.maximum(want * (1 - want), 1e-12) / reps)
            assert np.all(np.abs(got - want) <= 5 * sigma + 1e-9), (v, got, want)
        for d in states[:200]:
            for a, b in nx.bfs_edges(T, c['root']):
                assert P[d[a], d[b]] > 0
        again, _ = _forest.resample_states(forest, P, obs, root_distn=distn, seed=99, sweep=3,
                                           return_status=True)
        assert again == states
        other, _ = _forest.resample_states(forest, P, obs, root_distn=distn, seed=99, sweep=4,
                                           return_status=True)
        if any(rows(c['distn'], v, n).max() < 0.9 for v in T):     # not a degenerate posterior
            assert other != states


# ---------------------------------------------------------------------------
# 7: a 64-state problem embedded into 65 states
# ---------------------------------------------------------------------------

def test_embedded_64_state_problem_gets_the_draws_of_the_one_word_kernels(ra):
    """A 64-state forest and the same forest in 65 states, the extra state unreachable,
    allowed nowhere and of root weight zero: the wide kernels (65) give the sets of the
    one-word kernels (64) on states 0..63, pmap within 1e-12 and IDENTICAL sampled states at
    the same seed and sweep -- the cumulative weights of states 0..63 are summed exactly as
    the one-word scan sums them, and the second scan starts from that total.  Trees on both
    sides of the wide kernel's LDS cap (512 nodes) and beyond the one-word cap (1 024)."""
    from raoteh_amd import _forest
    rng = np.random.RandomState(64)
    n = 64
    Q, P = sparse_uniformized(rng, n, extras=4.0)
    P65 = np.zeros((n + 1, n + 1))
    P65[:n, :n] = P
    P65[n, n] = 1.0
    trees, obs64 = [], []
    for nn in [1, 2, 3, 7, 20, 33, 64, 65, 130, 300, 511, 512, 513, 700, 1100] + \
            [int(x) for x in rng.randint(2, 90, size=25)]:
        T = nx.Graph()
        T.add_node(0)
        for k in range(1, nn):
            T.add_edge(int(rng.randint(max(0, k - 12), k)), k)
        d = {}
        for v in rng.choice(nn, size=max(1, min(nn // 8, 10)), replace=False):
            u = rng.uniform()
            if u < 0.2:
                d[int(v)] = {int(rng.randint(n))}
            else:
                d[int(v)] = set(int(x) for x in rng.choice(n, size=int(rng.randint(8, 40)),
                                                           replace=False))
        trees.append((T, 0))
        obs64.append(d)
    low = set(range(n))
    obs65 = [dict((v, d.get(v, low)) for v in T) for (T, _), d in zip(trees, obs64)]
    forest = _forest.Forest(trees)
    rd = rng.dirichlet(np.ones(n))
    rd[5] = 0.0
    rd65 = np.concatenate([rd, [0.0]])
    sets64, pmap64 = _forest.get_node_to_set_and_pmap(forest, P, obs64)
    sets65, pmap65 = _forest.get_node_to_set_and_pmap(forest, P65, obs65)
    feasible = 0
    for k, (T, _) in enumerate(trees):
        for v in T:
            assert sets65[k][v] == sets64[k][v], (k, v)
            assert pmap65[k][v][n] == 0.0
            np.testing.assert_allclose(pmap65[k][v][:n], pmap64[k][v], rtol=1e-12, atol=0)
        feasible += bool(pmap64[k][0].dot(rd) > 0)
    assert feasible >= len(trees) // 2
    for sweep in (0, 7):
        s64, st64 = _forest.resample_states(forest, P, obs64, root_distn=rd, seed=5, sweep=sweep,
                                            return_status=True)
        s65, st65 = _forest.resample_states(forest, P65, obs65, root_distn=rd65, seed=5,
                                            sweep=sweep, return_status=True)
        np.testing.assert_array_equal(st64, st65)
        assert s64 == s65
        assert (st64 == 0).sum() >= len(trees) // 2


# ---------------------------------------------------------------------------
# 8: exact stationary law
# ---------------------------------------------------------------------------

LUMPED_SETTINGS = [
    ('device', 128, (3.0, 2.0), 2.0, 400),
    ('device', 128, (0.9, 0.7), 2.0, 3000),
    ('device', 128, (0.9, 0.7), 16.0, 300),
    ('host', 128, (3.0, 2.0), 2.0, 400),
    ('device', 100, (3.0, 2.0), 2.0, 400),
]


@pytest.mark.parametrize('where,n,lengths,factor,sweeps', LUMPED_SETTINGS)
def test_wide_stationary_law_on_a_lumped_cycle_is_exact(ra, where, n, lengths, factor, sweeps):
    """n = 4 R states s = 4 r + c with rate 1 / R from (c, r) to (c + 1 mod 4, r') for every r':
    the class c = s % 4 is the unit-rate 4-cycle of
    test_rao_teh_stationary_law_on_a_pure_cycle_is_exact and every transition changes it.  On
    the 3-node tree with both leaves allowed {s : s % 4 == 0} (R states, in both words) and a
    uniform root, the law of (root class, total number of transitions) is that test's closed
    form; same chains, settings and criteria.  The number of transitions of a chain is its
    rows minus its two edges (the int64[C][n][n] count array would be 2.6 GB)."""
    check_lumped_cycle_law(ra.ctx, where, n, lengths, factor, sweeps)


# ---------------------------------------------------------------------------
# 9: posterior expectations at 122 states
# ---------------------------------------------------------------------------

def _switching_problem(ra):
    """The switching rate matrix of synth.make_config('c6') (122 states) on the tree of c1;
    the leaves carry the first codons of c6's first site in the default class, one of them
    (a benign codon) in either class."""
    c6 = ra.synth.make_config('c6', nsites=1)
    c1 = ra.synth.make_config('c1', nsites=1)
    T, root, leaves = c1['T'], c1['root'], c1['leaves']
    n, half = c6['nstates'], c6['nstates'] // 2
    Q, rd = c6['Q_default'], c6['root_distn']
    codons = [int(x) for x in c6['leaf_states'][0][:len(leaves)]]
    benign = np.nonzero(rd[:half] > 0)[0]
    amb = 2
    if codons[amb] not in benign:
        codons[amb] = int(benign[0])
    allowed = dict((v, set(range(n))) for v in T)
    for leaf, c in zip(leaves, codons):
        allowed[leaf] = {half + c}
    allowed[leaves[amb]] = {codons[amb], half + codons[amb]}
    return T, root, leaves, n, half, Q, rd, allowed


@pytest.mark.parametrize('where', ['device', 'host'])
def test_wide_sweeps_reproduce_the_posterior_expectations(ra, where):
    """The 122-state switching model on a 15-node tree, leaves observed as allowed sets (one
    across the two classes): dwell time per state, root posterior per state and the transition
    counts summed over the four blocks {< 61, >= 61}^2, averaged over replicate chains,
    against _mjp_dense.get_expected_history_statistics on the same inputs -- the 65..128-state
    expectation route, pinned by expectations_wide.json.
    Criterion of the 4-state test: |mean - expected| <= 5 se + 1e-3 max(|expected|, 1e-2).

    Chains and sweeps: the 4-state test runs 3 000 chains, 8 sweeps of burn-in and 24 kept.  With
    122 states the root posterior and the dwell times of most states are small numbers, and the
    criterion has an absolute floor of 1e-5 with the SAMPLE standard error beside it: a state
    whose expectation lies just above 1e-5 and which 72 000 draws never show (probability
    exp(-0.72) = 0.49 at 1e-5) has se = 0 and fails, whatever the sampler does (seen at 3 000 /
    8 / 24: root state 45, expected 1.06e-5, never drawn).  So the sample is sized for the floor:
    20 000 chains x 100 kept sweeps = 2e6 draws, 20 expected at 1e-5, which leaves room for the
    correlation between the sweeps of a chain.

    Burn-in: lengthened from 8 to 48 sweeps, for mixing.  The start-up history is far from the
    posterior here (the switch from the reference to the default class happens once per history
    and moves slowly along the tree); with 20 000 chains the means of the six largest dwell
    times, in windows of sweeps, were off by 85, 63, 48, 28, 11, 5 (device) and 84, 61, 48, 29,
    14, 8 (host) standard errors over sweeps 1, 2, 3-4, 5-8, 9-16, 17-32, and within 3.1 from
    sweep 33 and within 2.2 from sweep 49 on, the same decay on both routes; with 8 sweeps of
    burn-in the host batch was 5.9 se off on state 61 while the stationary-law tests passed."""
    from raoteh_amd import _mjp_dense, _sampler
    T, root, leaves, n, half, Q, rd, allowed = _switching_problem(ra)
    want_dwell, want_root, want_trans = _mjp_dense.get_expected_history_statistics(
        T, allowed, root, n, root_distn=rd, Q_default=Q)
    want_block = np.zeros(4)
    for a, b, d in want_trans.edges(data=True):
        if a != b:
            want_block[2 * (a >= half) + (b >= half)] += d['weight']
    B, burn, keep = 20000, 48, 100
    device = where == 'device'
    cls = _sampler.DeviceHistoryBatch if device else _sampler.HistoryBatch
    batch = cls(T, root, Q, node_to_allowed_states=allowed, nchains=B, root_distn=rd, seed=11,
                ctx=ra.ctx)
    total = sum(d['weight'] for _, _, d in T.edges(data=True))
    dwell = np.zeros((B, n))
    block = np.zeros((B, 4))
    roots = np.zeros((B, n))
    for it in range(burn + keep):
        batch.sweep()
        if it < burn:
            continue
        d = batch.dwell_times()
        np.testing.assert_allclose(d.sum(axis=1), total, rtol=1e-12)
        dwell += d
        chain, edge, length, state = batch.rows() if device else \
            (batch.chain, batch.edge, batch.length, batch.state)
        at = np.nonzero((chain[1:] == chain[:-1]) & (edge[1:] == edge[:-1]))[0] + 1
        key = chain[at] * 4 + 2 * (state[at - 1] >= half) + (state[at] >= half)
        block += np.bincount(key, minlength=B * 4).reshape(B, 4)
        roots[np.arange(B), batch.root_states()] += 1
        node_states = batch.node_states
        for leaf in leaves:
            st = node_states[:, batch.tree.node_to_index[leaf]]
            assert set(np.unique(st).tolist()) <= allowed[leaf]
    dwell /= keep
    block /= keep
    roots /= keep
    # the block sums of the rows are what the count kernel gives (a few chains: the array is
    # 119 KB per chain)
    if device:
        few = batch.transition_counts()[:1]
        got = [few[0][:half, :half].sum(), few[0][:half, half:].sum(), few[0][half:, :half].sum(),
               few[0][half:, half:].sum()]
        at0 = at[chain[at] == 0]
        key0 = 2 * (state[at0 - 1] >= half) + (state[at0] >= half)
        assert got == np.bincount(key0, minlength=4).tolist()
        assert few[0][np.arange(n), np.arange(n)].sum() == 0

    def close(sample, expected, what):
        mean = sample.mean(axis=0)
        se = sample.std(axis=0, ddof=1) / np.sqrt(B)
        assert abs(mean - expected) <= 5 * se + 1e-3 * max(abs(expected), 1e-2), \
            '%s: %.5f vs %.5f (se %.5f)' % (what, mean, expected, se)

    print('122 states %s: %d root states and %d dwell times expected in (1e-5, 1e-3)' % (
        where, ((want_root > 1e-5) & (want_root < 1e-3)).sum(),
        sum(1 for s in range(n) if 1e-5 < want_dwell[s] < 1e-3)))
    for s in range(n):
        close(dwell[:, s], want_dwell[s], 'dwell %d' % s)
        close(roots[:, s], want_root[s], 'root %d' % s)
    for k in range(4):
        close(block[:, k], want_block[k], 'transitions of block %d' % k)
    assert want_block[2] == 0.0 and not block[:, 2].any()      # no way back from the default class
    assert want_block[1] > 0.05 and want_block[3] > 0.05       # the test sees both classes
    assert batch.last_chunks >= B


# ---------------------------------------------------------------------------
# 10: device-resident histories at 122 states
# ---------------------------------------------------------------------------

def test_wide_device_resident_histories_are_consistent_and_reproducible(ra):
    """rt_chains_* at 122 states on the 127-node tree of c6: (seed, batch) fixes the rows; the
    rows are sorted by (edge, position), add up to the branch lengths, change state between
    neighbours of an edge through transitions Q allows; node states agree with the rows at the
    edge ends and with the two-word masks; the statistics kernels agree with numpy on the
    rows; snapshot / restore returns rejected chains to their snapshot."""
    from raoteh_amd import _forest, _sampler
    C = 150
    cfg = ra.synth.make_config('c6', nsites=C)
    T, root, n = cfg['T'], cfg['root'], cfg['nstates']
    Q = cfg['Q_default']
    index = _sampler.TreeArrays(T, root).node_to_index
    N = len(index)
    masks = np.empty((C, N, 2), dtype=np.uint64)
    masks[:] = _forest.full_mask(n)
    table = np.array([_forest.states_to_mask(ss, n) for ss in cfg['leaf_allowed']])
    cols = [index[v] for v in cfg['leaves']]
    masks[:, cols] = table[cfg['leaf_states']]
    masks[:, :, 1] |= np.uint64(1) << np.uint64(63)          # bits at or above n are ignored
    rows_a = check_resident_histories(ra.ctx, T, root, Q, cfg['root_distn'], masks)
    state = rows_a[3]
    assert (state >= 64).any() and (state < 64).any()
    # the shapes the constructor takes at 122 states
    with pytest.raises(ValueError):
        _sampler.DeviceHistoryBatch(T, root, Q, node_masks=masks[:, :, 0], ctx=ra.ctx)
    # a chain without a feasible history is an error at creation
    bad = masks.copy()
    bad[5, cols[0]] = 0
    with pytest.raises(ra.pkg.StructuralZeroProb):
        _sampler.DeviceHistoryBatch(T, root, Q, node_masks=bad, ctx=ra.ctx)


def test_wide_generators_inherit_the_range(ra):
    """gen_restricted_histories and gen_mh_histories at 122 states."""
    from raoteh_amd import _sampler
    T, root, leaves, n, half, Q, rd, allowed = _switching_problem(ra)
    total = sum(d['weight'] for _, _, d in T.edges(data=True))
    count = 0
    for h in _sampler.gen_restricted_histories(T, Q, allowed, root, root_distn=rd, nhistories=4,
                                               seed=3, ctx=ra.ctx):
        count += 1
        assert nx.is_tree(h) and set(T) <= set(h)
        assert sum(d['weight'] for _, _, d in h.edges(data=True)) == pytest.approx(total, rel=1e-12)
        for v in h:
            states = set(d['state'] for d in h[v].values())
            if v in T:
                assert len(states) == 1 and states <= allowed[v]
            else:
                assert h.degree(v) == 2 and len(states) == 2
                a, b = sorted(states)
                assert Q[a, b] > 0 or Q[b, a] > 0
    assert count == 4
    count = 0
    for h, ok in _sampler.gen_mh_histories(
            T, Q, allowed, lambda tree: -0.5 * sum(d['weight'] for _, _, d in tree.edges(data=True)
                                                   if d['state'] >= half),
            root, root_distn=rd, nhistories=5, seed=2, ctx=ra.ctx):
        count += 1
        assert isinstance(ok, bool)
        assert sum(d['weight'] for _, _, d in h.edges(data=True)) == pytest.approx(total, rel=1e-12)
    assert count == 5


# ---------------------------------------------------------------------------
# 11: limits
# ---------------------------------------------------------------------------

def test_wide_limits(ra):
    """128 states with the full set everywhere run; 129 states are a ValueError from Python
    and RT_ERR_INVALID from the C entry points, not a fault."""
    from raoteh_amd import _forest, _sampler
    rng = np.random.RandomState(128)
    n = 128
    Q, P = sparse_uniformized(rng, n)
    T = ra.synth.make_config('c1', nsites=1)['T']
    root = ra.synth.make_config('c1', nsites=1)['root']
    forest = _forest.Forest([(T, root), (nx.path_graph(3), 0)])
    sets, pmaps = _forest.get_node_to_set_and_pmap(forest, P)
    for k, d in enumerate(sets):
        for v, ss in d.items():
            assert ss == set(range(n))
            np.testing.assert_allclose(pmaps[k][v], 1.0, rtol=1e-12)
    states = _forest.resample_states(forest, P, seed=1, sweep=0)
    assert all(0 <= s < n for d in states for s in d.values())
    for cls in (_sampler.DeviceHistoryBatch, _sampler.HistoryBatch):
        b = cls(T, root, Q, nchains=40, seed=2, ctx=ra.ctx)
        for _ in range(3):
            b.sweep()
        total = sum(d['weight'] for _, _, d in T.edges(data=True))
        np.testing.assert_allclose(b.dwell_times().sum(axis=1), total, rtol=1e-12)
        assert b.node_states.max() >= 64 and b.node_states.min() >= 0
    # 129 states, Python
    Q129 = np.zeros((129, 129))
    Q129[np.arange(129), (np.arange(129) + 1) % 129] = 1.0
    Q129 -= np.diag(Q129.sum(axis=1))
    P129 = np.identity(129) + Q129 / 2.0
    for cls in (_sampler.DeviceHistoryBatch, _sampler.HistoryBatch):
        with pytest.raises(ValueError):
            cls(T, root, Q129, nchains=2, ctx=ra.ctx)
    with pytest.raises(ValueError):
        _forest.get_node_to_set_and_pmap(forest, P129)
    with pytest.raises(ValueError):
        _forest.resample_states(forest, P129)
    with pytest.raises(ValueError):
        next(_sampler.gen_restricted_histories(T, Q129, {}, root, ctx=ra.ctx))
    # 129 states, the C entry points
    lib = ra.lib.lib()
    h = ra.ctx._h
    i64, i32, f64, u64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64
    p = lambda a, t: a.ctypes.data_as(ctypes.POINTER(t))
    nn = 129
    off = np.array([0, 3], dtype=np.int64)
    idx = np.array([1, 2], dtype=np.int64)
    ptr = np.array([0, 1, 2, 2], dtype=np.int64)
    par = np.array([-1, 0, 1], dtype=np.int32)
    sets3 = np.full((3, 3), 2 ** 64 - 1, dtype=np.uint64)
    L = np.zeros((3, nn))
    st3, status = np.zeros(3, dtype=np.int32), np.zeros(1, dtype=np.int32)
    INVALID = ra.lib.RT_ERR_INVALID
    assert lib.rt_forest_passes(h, nn, 1, p(off, i64), p(idx, i64), p(ptr, i64), p(P129, f64),
                                p(sets3, u64), p(L, f64)) == INVALID
    assert lib.rt_forest_resample_states(h, nn, 1, p(off, i64), p(idx, i64), p(ptr, i64),
                                         p(P129, f64), None, p(sets3, u64), u64(1), u64(0),
                                         p(st3, i32), p(status, i32), None) == INVALID
    assert lib.rt_forest_resample_states_parents(h, nn, 1, p(off, i64), p(par, i32), p(P129, f64),
                                                 None, p(sets3, u64), u64(1), u64(0), p(st3, i32),
                                                 p(status, i32)) == INVALID
    mask = np.ones((3, nn), dtype=np.int64)
    tptr = np.concatenate([[0], np.cumsum((P129 != 0).sum(axis=1))]).astype(np.int64)
    tidx = np.nonzero(P129 != 0)[1].astype(np.int64)
    assert lib.rt_mcy_get_node_to_pset(h, 3, nn, p(idx, i64), p(ptr, i64), p(tidx, i64),
                                       p(tptr, i64), p(mask, i64)) == INVALID
    assert lib.rt_get_node_to_set(h, 3, nn, p(idx, i64), p(ptr, i64), p(tidx, i64), p(tptr, i64),
                                  p(mask, i64), None) == INVALID
    assert (mask == 1).all()
    branch = np.array([0.0, 0.3, 0.4])
    rates = np.ones(nn)
    handle = ctypes.c_void_p()
    assert lib.rt_chains_create(h, 3, p(par, i32), p(branch, f64), nn, p(P129, f64), p(rates, f64),
                                None, 1, p(sets3, u64), u64(1), ctypes.byref(handle)) == INVALID
    assert not handle.value


def test_wide_forest_trees_beyond_the_lds_image(ra):
    """Wide trees with more nodes than the set image of a wave holds (512 at two words; the
    sampled states 1 024) take the coherent global path: a long path of chunk nodes with side
    twigs at 70 states, against a plain numpy statement of the passes; and the same tree's
    lower part, cut out below the cap and run with the sets of the whole, gives the same sets
    and pmap there.  The draws stay inside the sets and follow the root's exact posterior."""
    from raoteh_amd import _forest
    rng = np.random.RandomState(70)
    n = 70
    Q, P = sparse_uniformized(rng, n, extras=6.0)
    nz = P > 0
    for nn in (513, 1500):
        big = nx.Graph()
        big.add_node(0)
        for k in range(1, nn):              # a spine with a twig leaf at every fifth node
            big.add_edge(k - 2 if k % 5 == 0 else k - 1, k)
        small = nx.path_graph(6)
        allowed = dict((int(v), set(int(x) for x in rng.choice(n, size=20, replace=False)))
                       for v in rng.choice(nn, size=nn // 12, replace=False))
        allowed[nn - 1] = {3, 66}
        allowed[0] = set(range(0, n, 2))
        reps = 200
        forest = _forest.Forest([(big, 0), (small, 0)] + [(big, 0)] * (reps - 1))
        obs = [allowed, {5: {69}}] + [allowed] * (reps - 1)
        sets, pmaps = _forest.get_node_to_set_and_pmap(forest, P, obs)
        order = list(nx.dfs_preorder_nodes(big, 0))
        par = dict((b, a) for a, b in nx.bfs_edges(big, 0))
        S = np.ones((nn, n), dtype=bool)
        for v, ss in allowed.items():
            S[v] = False
            S[v, sorted(ss)] = True
        for v in reversed(order[1:]):
            S[par[v]] &= nz[:, S[v]].any(axis=1)
        for v in order[1:]:
            S[v] &= nz[S[par[v]], :].any(axis=0)
        L = S.astype(float)
        for v in reversed(order[1:]):
            L[par[v]] = L[par[v]] * P.dot(L[v])
        assert S[0].any() and not S.all(axis=1).all()
        for v in big:
            assert sets[0][v] == set(np.nonzero(S[v])[0]), v
            np.testing.assert_allclose(pmaps[0][v], L[v], rtol=1e-11, atol=0)
        assert sets[1][5] == {69}
        # the lower part of the same tree as a tree of its own, below the cap
        top = nn - 402                      # a spine node: everything after it hangs below it
        sub_nodes = list(range(top, nn))
        sub = big.subgraph(sub_nodes).copy()
        part = _forest.Forest([(sub, top)])
        psets, ppmaps = _forest.get_node_to_set_and_pmap(
            part, P, [dict((v, sets[0][v]) for v in sub_nodes)])
        for v in sub_nodes:
            assert psets[0][v] == sets[0][v]
            np.testing.assert_allclose(ppmaps[0][v], pmaps[0][v], rtol=1e-12, atol=0)
        distn = rng.dirichlet(np.ones(n))
        states, status = _forest.resample_states(forest, P, obs, root_distn=distn, seed=4, sweep=1,
                                                 return_status=True)
        assert not status.any()
        post = distn * L[0]
        post /= post.sum()
        got = np.bincount([states[k][0] for k in range(len(states)) if k != 1],
                          minlength=n) / float(reps)
        assert not got[post == 0].any()
        assert np.all(np.abs(got - post) <=
                      5 * np.sqrt(np.maximum(post * (1 - post), 1e-12) / reps) + 1e-9)
        for k in (0, 2, 7):
            d = states[k]
            for v in big:
                assert S[v, d[v]]
            for a, b in nx.bfs_edges(big, 0):
                assert P[d[a], d[b]] > 0
        assert states[1][5] == 69
        again, _ = _forest.resample_states(forest, P, obs, root_distn=distn, seed=4, sweep=1,
                                           return_status=True)
        assert again == states
