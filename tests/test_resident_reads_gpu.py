"""Every read of a resident batch -- log-likelihoods, statuses, totals, posterior set sums and
expected history statistics -- against host references (tests/_resident_cases.py), in every
layout a batch can be resident in, and after everything that changes a batch under the caller:
the background switch to a tree-specialised kernel (which packs the lane family again), clone,
the posterior and expectation passes (twins and scratch of their own), new rates.

Each row of the layout table runs on a fresh context with its own options (nothing leaks into
other modules) and proves by its kernel name that the batch got there."""
import collections

import numpy as np
import pytest

from _resident_cases import (_extended_log_likelihoods, expectation_reference, make_case,
                             posterior_reference, rate_matrix, set_rates, totals_reference,
                             loglik_reference)

pytestmark = pytest.mark.gpu

RTOL = 1e-10


@pytest.fixture(scope='module')
def ra():
    from raoteh_amd import device, _lib, synth

    class NS(object):
        pass
    ns = NS()
    ns.device, ns.lib, ns.synth = device, _lib, synth
    return ns


# name, states, kind, sites, tree nodes, context options, kernel-name proof (prefix, required
# parts, forbidden parts), internal observations, per-edge rates, leaf-state upload (0 / 1 one
# state per leaf / 2 one or two states per leaf)
Row = collections.namedtuple('Row', 'name n kind nsites nnodes opts prefix need avoid internal '
                                    'per_edge leaf')


def row(name, n, kind, nsites, nnodes, opts, prefix, need=(), avoid=(), internal=True,
        per_edge=False, leaf=0):
    return Row(name, n, kind, nsites, nnodes, opts, prefix, tuple(need), tuple(avoid), internal,
               per_edge, leaf)


LANE_JIT = ('prune_tree_jit<',)
ROWS = [
    # lane interpreter: blocks of 64 sites, an even number of them
    row('lane-interp-n2-dense-1', 2, 'dense', 1, 12, {'jit': 0}, 'prune_lane'),
    row('lane-interp-n3-state-127', 3, 'state', 127, 15, {'jit': 0}, 'prune_lane', per_edge=True),
    row('lane-interp-n4-mask-129', 4, 'mask', 129, 17, {'jit': 0}, 'prune_lane'),
    row('lane-interp-n4-state-343', 4, 'state', 343, 21, {'jit': 0}, 'prune_lane'),
    # lane tree-specialised: dense f64, one byte per state, one byte per allowed-set mask
    row('lane-jit-n4-dense-65', 4, 'dense', 65, 19, {'jit': 1}, 'prune_tree_jit<4',
        avoid=(',states', ',masks')),
    row('lane-jit-n3-state-63', 3, 'state', 63, 13, {'jit': 1}, 'prune_tree_jit<3',
        need=(',states',)),
    row('lane-jit-n4-mask-201', 4, 'mask', 201, 16, {'jit': 1}, 'prune_tree_jit<4',
        need=(',masks',), per_edge=True),
    # ... with a ragged lane block of 37 sites
    row('lane-jit37-n3-dense-38', 3, 'dense', 38, 14, {'jit': 1, 'jit_block_sites': 37},
        'prune_tree_jit<3', avoid=(',states', ',masks')),
    row('lane-jit37-n2-state-116', 2, 'state', 116, 11, {'jit': 1, 'jit_block_sites': 37},
        'prune_tree_jit<2', need=(',states',)),
    row('lane-jit37-n4-mask-36', 4, 'mask', 36, 18, {'jit': 1, 'jit_block_sites': 37},
        'prune_tree_jit<4', need=(',masks',)),
    # MFMA interpreter: tiles of 16 sites
    row('mfma-interp-n5-state-1', 5, 'state', 1, 13, {'jit': 0}, 'prune_mfma'),
    row('mfma-interp-n16-dense-15', 16, 'dense', 15, 14, {'jit': 0}, 'prune_mfma', per_edge=True),
    row('mfma-interp-n17-mask-17', 17, 'mask', 17, 12, {'jit': 0}, 'prune_mfma'),
    row('mfma-interp-n33-state-71', 33, 'state', 71, 15, {'jit': 0}, 'prune_mfma'),
    row('mfma-interp-n61-dense-31', 61, 'dense', 31, 11, {'jit': 0}, 'prune_mfma'),
    row('mfma-interp-n64-mask-33', 64, 'mask', 33, 10, {'jit': 0}, 'prune_mfma', per_edge=True),
    row('mfma-interp-n65-state-17', 65, 'state', 17, 9, {'jit': 0}, 'prune_mfma'),
    row('mfma-interp-n122-mask-15', 122, 'mask', 15, 9, {'jit': 0}, 'prune_mfma'),
    row('mfma-interp-n128-dense-19', 128, 'dense', 19, 8, {'jit': 0}, 'prune_mfma'),
    # MFMA tree-specialised, dense
    row('mfma-jit-n13-dense-53', 13, 'dense', 53, 15, {'jit': 1}, 'prune_tree_jit_mfma',
        avoid=('leaf-states',)),
    row('mfma-jit-n40-dense-17', 40, 'dense', 17, 13, {'jit': 1}, 'prune_tree_jit_mfma',
        avoid=('leaf-states',), per_edge=True),
    # gathered columns: observed states / sets of one or two at every leaf, leaves only
    row('leaf-states-n33-state-40', 33, 'state', 40, 15, {'jit': 1}, 'prune_tree_jit_mfma',
        need=('leaf-states',), internal=False, leaf=1),
    row('leaf-states-n20-mask-47', 20, 'mask', 47, 14, {'jit': 1}, 'prune_tree_jit_mfma',
        need=('leaf-states',), internal=False, leaf=2),
    row('leaf-states-off-n33-state-40', 33, 'state', 40, 15, {'jit': 1, 'leaf_state_kernels': 0},
        'prune_tree_jit_mfma', avoid=('leaf-states',), internal=False, leaf=1),
    # the generic kernel (no posterior / expectation passes)
    row('generic-n4-state-70', 4, 'state', 70, 16, {'force_generic': 1}, 'prune_generic'),
    row('generic-n20-dense-40', 20, 'dense', 40, 13, {'force_generic': 1}, 'prune_generic'),
]

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


def open_context(ra, opts):
    ctx = ra.device.Context(0)
    for k, v in dict(DEFAULTS, **opts).items():
        ctx.set_option(k, v)
    return ctx


def case_of(r, seed):
    return make_case(r.n, r.nnodes, r.nsites, r.kind, seed, internal=r.internal,
                     per_edge=r.per_edge, every_leaf=r.leaf > 0, pairs=r.leaf == 2)


def check_name(r, name):
    assert name.startswith(r.prefix), (r.name, name)
    for part in r.need:
        assert part in name, (r.name, name)
    for part in r.avoid:
        assert part not in name, (r.name, name)


def sets_of(n, rng):
    """Node sets and edge sets; above 64 states they span both words of the masks."""
    def sub():
        return sorted(rng.choice(n, size=rng.randint(1, n + 1), replace=False).tolist())
    h = max(1, n // 2)
    lo, hi, every = list(range(h)), list(range(h, n)) or [0], list(range(n))
    S = sub()
    return [lo, S, [0, n - 1]], [(lo, hi), (hi, lo), (every, S), (S, every), (sub(), sub())]


def fetch(model, batch):
    ll, st = model.fetch_log_likelihoods(batch)
    return ll, st, model.fetch_totals(batch)


def check_loglik(model, batch, case, got=None):
    """Log-likelihoods, statuses and totals of the batch against the oracle."""
    ll, st, tot = got if got is not None else fetch(model, batch)
    want, wst = loglik_reference(model, case)
    np.testing.assert_array_equal(st, wst)
    ok = wst == 0
    np.testing.assert_allclose(ll[ok], want[ok], rtol=RTOL)
    assert np.all(np.isneginf(ll[~ok]))
    if case.zero_site is not None:
        assert st[case.zero_site] == 1
    ref = totals_reference(ll, st)
    assert tot[1] == ref[1] and tot[2] == ref[2]
    rel = 1e-11 if len(ll) > 100000 else 1e-12
    assert abs(tot[0] - ref[0]) <= rel * abs(ref[0]) + 1e-300, (tot, ref)
    assert abs(tot[0] - totals_reference(want, wst)[0]) <= RTOL * abs(ref[0])
    return ll, st, tot


def check_posteriors(model, batch, case, rng, recompute=False):
    node_sets, edge_sets = sets_of(case.n, rng)
    post = model.posteriors(batch, node_sets=node_sets, edge_sets=edge_sets, marginals=True,
                            recompute_transitions=recompute)
    S = batch.nsites
    picks = sorted(set([0, S - 1, S // 2, min(S - 1, 17)]))
    nv, ev, D, status = posterior_reference(model, case, node_sets, edge_sets, picks)
    np.testing.assert_array_equal(post.status, status)
    np.testing.assert_allclose(post.node_values, nv, rtol=RTOL, atol=1e-15)
    np.testing.assert_allclose(post.edge_values, ev, rtol=RTOL, atol=1e-15)
    np.testing.assert_allclose(post.marginals, D, rtol=RTOL, atol=1e-15)
    return post


def check_expectations(model, batch, case, Qs=None, recompute=True):
    dwell, rootp, trans, status = model.expected_history_statistics(
        batch, recompute_transitions=recompute, return_status=True)
    want = expectation_reference(model, case, Qs=Qs, check_sites=[0, batch.nsites // 2])
    bad = np.zeros(batch.nsites, dtype=np.int32)
    if case.zero_site is not None:
        bad[case.zero_site] = 2                    # a zero denominator (likelihood 0)
    np.testing.assert_array_equal(status, bad)
    scale = np.abs(want[0]).max()
    np.testing.assert_allclose(dwell, want[0], rtol=1e-9, atol=1e-13 * scale)
    np.testing.assert_allclose(rootp, want[1], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(trans, want[2], rtol=1e-9, atol=1e-13 * scale)
    return dwell, rootp, trans


def assert_same(a, b):
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)


def assert_relaid(got, pre):
    """The same results from a kernel with another site-block layout: log-likelihoods and
    statuses bit for bit, the totals' counts exactly; their sum is reduced in the new layout's
    block order, so it is the same number to rounding."""
    assert_same(got[:2], pre[:2])
    assert got[2][1:].tolist() == pre[2][1:].tolist()
    assert abs(got[2][0] - pre[2][0]) <= 1e-13 * abs(pre[2][0]), (got[2], pre[2])


def check_no_side_effects(ra, model, batch, case, rng, passes=True):
    """S4: prune -> posteriors -> expectation -> fetch: the batch's log-likelihoods, statuses,
    totals (bit for bit) and kernel are what the prune left."""
    model.prune(batch)
    before, name = fetch(model, batch), batch.kernel_name
    if passes:
        model.posteriors(batch, node_sets=[[0]], edge_sets=[([0], [1])], marginals=True)
        if case.n <= 64:
            model.expected_history_statistics(batch)
    else:
        for call in (lambda: model.posteriors(batch, node_sets=[[0]]),
                     lambda: model.expected_history_statistics(batch)):
            with pytest.raises(ra.lib.RaotehHipError) as e:
                call()
            assert e.value.code == ra.lib.RT_ERR_UNSUPPORTED
    assert_same(fetch(model, batch), before)
    assert batch.kernel_name == name


def never_pruned(ra, model, batch):
    """S6: nothing has written the batch's log-likelihoods: the C ABI says RT_ERR_INVALID (which
    the wrapper raises as ValueError, as every bad-argument error)."""
    import ctypes
    ll = np.zeros(batch.nsites)
    st = np.zeros(batch.nsites, dtype=np.int32)
    rc = ra.lib.lib().rt_sites_get_logliks(batch._h, ll.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                          st.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == ra.lib.RT_ERR_INVALID
    assert b'no pruning kernel' in ra.lib.lib().rt_last_error()
    with pytest.raises(ValueError):
        model.fetch_log_likelihoods(batch)
    assert model.fetch_totals(batch).tolist() == [0.0, 0.0, 0.0]


def check_clone(model, batch, pre):
    """S3: the clone carries the source's results without a prune; pruned, the same numbers."""
    twin = batch.clone()
    assert_same(fetch(model, batch), pre)
    assert_same(fetch(model, twin), pre)
    model.prune(twin)
    assert_same(fetch(model, twin), pre)
    assert twin.kernel_name == batch.kernel_name
    twin.close()


def check_new_rates(model, batch, case, rng, passes=True):
    """S5: set_rates(Q1) -> step -> every read under Q1; the expectation step without
    recomputing the transitions."""
    Q1 = np.stack([rate_matrix(case.n, rng) for _ in range(len(case.Qs))])
    set_rates(model, case, Q1)
    model.step(batch)
    check_loglik(model, batch, case)
    if passes:
        check_posteriors(model, batch, case, rng)
        if case.n <= 64:
            check_expectations(model, batch, case, Qs=Q1, recompute=False)


@pytest.mark.parametrize('r', ROWS, ids=[r.name for r in ROWS])
def test_every_read_in_every_layout(ra, r):
    seed = 1000 + sum(map(ord, r.name))
    rng = np.random.RandomState(seed)
    case = case_of(r, seed)
    ctx = open_context(ra, r.opts)
    try:
        model = ra.device.TreeModel(case.T, case.root, r.n, ctx=ctx)
        set_rates(model, case)
        model.set_root_distn(case.root_distn)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=r.kind)
        passes = not r.opts.get('force_generic')
        # S1
        model.prune(batch)
        check_name(r, batch.kernel_name)
        pre = check_loglik(model, batch, case)
        if passes:
            check_posteriors(model, batch, case, rng)
            if r.n <= 64:
                check_expectations(model, batch, case)
        assert_same(fetch(model, batch), pre)
        # S4, S3, S5
        check_no_side_effects(ra, model, batch, case, rng, passes)
        check_clone(model, batch, pre)
        check_name(r, batch.kernel_name)
        check_new_rates(model, batch, case, rng, passes)
        check_name(r, batch.kernel_name)
    finally:
        ctx.close()


NEVER = [r for r in ROWS if r.name in ('lane-interp-n4-mask-129', 'lane-jit-n3-state-63',
                                       'lane-jit37-n2-state-116', 'mfma-interp-n17-mask-17',
                                       'leaf-states-n20-mask-47', 'generic-n20-dense-40')]


@pytest.mark.parametrize('r', NEVER, ids=[r.name for r in NEVER])
def test_a_batch_never_pruned_has_no_log_likelihoods(ra, r):
    """S6: uploaded, cloned, but no pruning kernel has run: no log-likelihoods to read, totals
    zero; the first prune makes them readable."""
    seed = 3000 + sum(map(ord, r.name))
    case = case_of(r, seed)
    ctx = open_context(ra, r.opts)
    try:
        model = ra.device.TreeModel(case.T, case.root, r.n, ctx=ctx)
        set_rates(model, case)
        model.set_root_distn(case.root_distn)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=r.kind)
        never_pruned(ra, model, batch)
        twin = batch.clone()
        never_pruned(ra, model, twin)
        model.prune(twin)
        check_loglik(model, twin, case)
        never_pruned(ra, model, batch)
    finally:
        ctx.close()


def test_lane_expectation_reads_dense_data_as_allowed_sets(ra):
    """n <= 4 (the fused lane kernel): a dense batch counts a state as allowed where its
    likelihood is not zero -- the documented reading, pinned: other non-zero values give the
    same statistics."""
    case = make_case(4, 15, 70, 'dense', 7)
    ctx = open_context(ra, {'jit': 0})
    try:
        model = ra.device.TreeModel(case.T, case.root, 4, ctx=ctx)
        set_rates(model, case)
        model.set_root_distn(case.root_distn)
        ones = model.upload_sites(case.obs_nodes, case.obs_lik, kind='dense')
        scaled = np.random.RandomState(8).uniform(0.1, 0.9, size=case.obs_lik.shape) * case.obs_lik
        other = model.upload_sites(case.obs_nodes, scaled, kind='dense')
        for a, b in zip(model.expected_history_statistics(ones),
                        model.expected_history_statistics(other)):
            np.testing.assert_allclose(a, b, rtol=1e-12, atol=1e-15)
    finally:
        ctx.close()


# ---- S2: the background switch ------------------------------------------------------------

BACKGROUND = [
    row('lane-bg-n4-state', 4, 'state', 16400, 23, {}, 'prune_lane', need=(',states',)),
    row('lane-bg-n3-dense', 3, 'dense', 21900, 19, {}, 'prune_lane', avoid=(',states', ',masks')),
    row('lane-bg-n4-mask', 4, 'mask', 16400, 21, {}, 'prune_lane', need=(',masks',)),
    row('mfma-bg-n20-dense', 20, 'dense', 3300, 17, {}, 'prune_mfma'),
]


@pytest.mark.parametrize('via', ['wait', 'clone'])
@pytest.mark.parametrize('r', BACKGROUND, ids=[r.name for r in BACKGROUND])
def test_reads_across_the_background_switch(ra, r, via, tmp_path, monkeypatch):
    """jit automatic, jit_async on, a cold cache directory: the first prune runs the interpreter
    kernel; then the batch switches (wait_for_kernel, or a clone, which waits for a lane-family
    source) and every read without a new prune still gives the interpreter's results; the
    tree-specialised kernel then gives them again bit for bit."""
    monkeypatch.setenv('RAOTEH_JIT_CACHE_DIR', str(tmp_path / 'jit'))
    seed = 2000 + sum(map(ord, r.name))
    rng = np.random.RandomState(seed)
    case = case_of(r, seed)
    assert r.nsites * r.n >= 65536                 # the automatic policy compiles
    ctx = open_context(ra, {'jit': -1, 'jit_async': 1})
    try:
        model = ra.device.TreeModel(case.T, case.root, r.n, ctx=ctx)
        set_rates(model, case)
        model.set_root_distn(case.root_distn)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=r.kind)
        model.prune(batch)
        first = batch.kernel_name
        assert first.startswith('prune_lane' if r.n <= 4 else 'prune_mfma'), (
            'the background compile was done before the first prune (%s): the interpreter '
            'kernel never ran, nothing is tested' % first)
        pre = check_loglik(model, batch, case)
        if via == 'wait':
            batch.wait_for_kernel()
            assert_same(fetch(model, batch), pre)          # no prune since the switch
            model.prune(batch)
        else:
            twin = batch.clone()
            assert_same(fetch(model, batch), pre)
            assert_same(fetch(model, twin), pre)
            model.prune(twin)
            assert_relaid(fetch(model, twin), pre)
            twin.wait_for_kernel()
            model.prune(twin)
            assert_relaid(fetch(model, twin), pre)
            batch.wait_for_kernel()
            model.prune(batch)
        jit = 'prune_tree_jit<%d' % r.n if r.n <= 4 else 'prune_tree_jit_mfma'
        assert batch.kernel_name.startswith(jit), batch.kernel_name
        for part in r.need:
            assert part in batch.kernel_name, batch.kernel_name
        for part in r.avoid:
            assert part not in batch.kernel_name, batch.kernel_name
        post = fetch(model, batch)
        assert_relaid(post, pre)
        check_posteriors(model, batch, case, rng)
        check_expectations(model, batch, case)
        check_no_side_effects(ra, model, batch, case, rng)
        check_clone(model, batch, post)
    finally:
        ctx.close()


# ---- rescale (S7) ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_rescale_batches(ra, n):
    """'rescale' on a tree whose likelihood underflows f64: log-likelihoods and totals against the
    long-double recursion, across clone and the error paths; the posterior and expectation passes
    refuse such a batch (they do not rescale) and leave it as it was."""
    rng = np.random.RandomState(700 + n)
    nleaves = 2048 if n <= 4 else 1024
    T, root, leaves = ra.synth.balanced_tree(nleaves, seed=n)
    for a, b in T.edges():
        T[a][b]['weight'] *= 8.0
    Q = rng.uniform(0.1, 1.0, size=(n, n))
    np.fill_diagonal(Q, 0.0)
    Q -= np.diag(Q.sum(axis=1))
    pi = rng.dirichlet(np.ones(n))
    nsites = 17 if n > 4 else 65
    states = rng.randint(0, n, size=(nsites, nleaves)).astype(np.uint8)
    states[rng.uniform(size=states.shape) < 0.03] = 255
    ctx = open_context(ra, {'rescale': 1})
    try:
        model = ra.device.TreeModel(T, root, n, ctx=ctx)
        model.set_rates(Q_default=Q)
        model.set_root_distn(pi)
        batch = model.upload_sites(leaves, states, kind='state')
        model.prune(batch)
        name = batch.kernel_name
        assert 'rescale' in name or name.startswith('prune_generic'), name
        ll, st, tot = fetch(model, batch)
        want = _extended_log_likelihoods(model.tree, model.get_transitions(),
                                         [model.tree.node_to_index[v] for v in leaves], states, n, pi)
        assert want.max() < -745.0
        assert not st.any()
        np.testing.assert_allclose(ll, want, rtol=RTOL)
        ref = totals_reference(ll, st)
        assert tot[1] == 0 and tot[2] == nsites
        assert abs(tot[0] - ref[0]) <= 1e-12 * abs(ref[0])
        for call in (lambda: model.expected_history_statistics(batch),
                     lambda: model.expected_history_statistics(batch, return_status=True),
                     lambda: model.posteriors(batch, node_sets=[[0]])):
            with pytest.raises(ra.lib.RaotehHipError) as e:
                call()
            assert e.value.code == ra.lib.RT_ERR_UNSUPPORTED
        assert_same(fetch(model, batch), (ll, st, tot))
        assert batch.kernel_name == name
        check_clone(model, batch, (ll, st, tot))
        # a small tree (the expectation passes would take it, without the option)
        T16, root16, leaves16 = ra.synth.balanced_tree(16, seed=n)
        m16 = ra.device.TreeModel(T16, root16, n, ctx=ctx)
        m16.set_rates(Q_default=Q)
        b16 = m16.upload_sites(leaves16, states[:, :16], kind='state')
        m16.prune(b16)
        with pytest.raises(ra.lib.RaotehHipError) as e:
            m16.expected_history_statistics(b16)
        assert e.value.code == ra.lib.RT_ERR_UNSUPPORTED
    finally:
        ctx.close()
