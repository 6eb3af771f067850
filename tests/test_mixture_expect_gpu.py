"""rt_sites_branch_expectations_mixture (TreeModel.branch_expectations_mixture / class_posteriors /
branch_length_gradient_mixture) on the GPU: an ordinary batch under a site-class mixture over the
model's rate sets.  Every output against the host reference that no device path enters
(tests/_mixture_cases.py); bit for bit against the ordinary call at K = 1 and under one-hot class
weights; sets that are not live; the device's sums against host re-summation; the log-likelihoods
against step_multi + mixture_log_likelihoods; repeatability and side effects; the analytic
gradients; the documented errors."""
import ctypes

import numpy as np
import pytest

import _mixture_cases as mc
import _partition_cases as pc
import _step_multi_cases as smc
from _branch_cases import make_coefs

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


@pytest.fixture(scope='module')
def contexts():
    from raoteh_amd import device
    made = {}

    def get(**opts):
        key = tuple(sorted(opts.items()))
        if key not in made:
            ctx = device.Context(0)
            for k, v in dict(DEFAULTS, **opts).items():
                ctx.set_option(k, v)
            made[key] = ctx
        return made[key]
    yield get
    made.clear()


def build(contexts, case, weights=None, **opts):
    from raoteh_amd import device
    model, batch = smc.upload(device, contexts(**opts), case)
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


def ordinary(contexts, case, k, coefs, weights=None):
    """branch_expectations of the same data under set_rates with set k's Q and t."""
    from raoteh_amd import device
    model, batch = smc.upload(device, contexts(), case)
    model.set_rates(Q=case.Q[k], node_q=case.node_q, t=case.t[k])
    if weights is not None:
        batch.set_weights(weights)
    got = model.branch_expectations(batch, coefs)
    batch.close()
    model.close()
    return got


def check_values(got, want, label):
    """check_values of test_branch_expect_gpu.py and test_partition_reads_gpu.py: the project's
    tolerances for expected history statistics at every n up to 128."""
    scale = np.abs(want[np.isfinite(want)]).max()
    both = np.isfinite(want) & np.isfinite(got)
    print('%s: max |value - ref| / scale %.2e (scale %.3g)'
          % (label, np.abs(got[both] - want[both]).max() / scale, scale))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-13 * scale)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(smc.bits(a), smc.bits(b))


def class_weights(K, seed):
    c = np.random.RandomState(seed).uniform(0.2, 1.0, K)
    return c / c.sum()


def site_weights(nsites, seed):
    w = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(float)
    w[2] = 0.0
    return w


# ---- 1. every output against the host reference ---------------------------------------------

# lane kernels odd and even (n = 3, 4; 300 sites: a second, partial workgroup of 256), one wave
# (5), two tiles (20), split-M four tiles (61), the wide derivative route (122); every observation
# kind in both layouts; K = 1, 2, 3, 5 and 64; both trees; 1 and RT_MAX_BRANCH_COEFS matrices,
# shared and per set; with and without site weights (one of them 0).  K >= 2: the last set has
# Q = 0 (P = I), under which the sites whose leaves disagree have zero likelihood.
REFERENCE_CASES = [
    # n, tree, kind, K, coefficient matrices, per set, weights, sites
    (3, 'balanced', 'state', 2, 1, False, False, mc.NSITES),
    (4, 'random', 'dense', 3, 8, True, True, mc.NSITES),
    (4, 'balanced', 'mask', 5, 1, False, True, 300),
    (4, 'balanced', 'state', 64, 1, False, False, mc.NSITES),
    (5, 'random', 'dense', 3, 8, False, False, mc.NSITES),
    (20, 'balanced', 'mask', 5, 1, True, True, mc.NSITES),
    (61, 'random', 'state', 3, 1, False, True, mc.NSITES),
    (61, 'balanced', 'dense', 1, 1, True, False, mc.NSITES),
    (122, 'balanced', 'state', 2, 1, True, False, mc.NSITES),
]


@pytest.mark.parametrize('n,tree,kind,K,ncoefs,per_set,weighted,nsites', REFERENCE_CASES,
                         ids=['n%d-%s-%s-K%d-c%d%s%s-s%d' % (c[0], c[1], c[2], c[3], c[4],
                                                            '-perset' if c[5] else '',
                                                            '-w' if c[6] else '', c[7])
                              for c in REFERENCE_CASES])
def test_against_the_host_reference(contexts, n, tree, kind, K, ncoefs, per_set, weighted, nsites):
    from raoteh_amd import _lib
    assert _lib.RT_MAX_BRANCH_COEFS == 8
    seed = 9900 + n + K
    case = mc.make_case(n, tree, kind, K, seed, nsites=nsites)
    coefs = make_coefs(n, ncoefs, seed)
    if per_set:
        coefs = np.array([make_coefs(n, ncoefs, seed + 100 * (k % 5)) for k in range(K)])
    c = class_weights(K, seed)
    w = site_weights(nsites, seed) if weighted else None
    model, batch = build(contexts, case, w)
    try:
        got = model.branch_expectations_mixture(batch, coefs, c)
        want = mc.mixture_reference(model.tree, case, coefs, c, w)
        N = model.tree.nnodes
        assert got.values.shape == (nsites, N, ncoefs) and got.edge_sums.shape == (N, ncoefs)
        assert got.set_edge_sums.shape == (K, N, ncoefs)
        assert got.class_posteriors.shape == (nsites, K) and got.class_sums.shape == (K,)
        np.testing.assert_array_equal(got.status, want.status)
        assert not got.values[:, 0].any()
        label = 'n=%d %s K=%d' % (n, kind, K)
        if K >= 2:
            # the zero set: dead sites have posterior exactly 0 there, live ones not
            dead = ~(want.L[K - 1] > 0)
            assert dead.any() and not got.class_posteriors[dead, K - 1].any()
            assert got.class_posteriors[~dead, K - 1].all()
        check_values(got.values, want.values, label + ' values')
        check_values(got.set_edge_sums, want.set_edge_sums, label + ' per-set sums')
        check_values(got.edge_sums, want.edge_sums, label + ' edge sums')
        check_values(got.class_posteriors, want.post, label + ' posteriors')
        check_values(got.class_sums, want.class_sums, label + ' class sums')
        check_values(got.log_likelihoods, want.loglik, label + ' log-likelihoods')
        for x in got[:6]:
            assert np.isfinite(x).all()
        # the sums alone: the same bits, nothing per site
        sums_only = model.branch_expectations_mixture(batch, coefs, c, per_site=False)
        assert sums_only.values is None
        for x, y in zip(sums_only[1:], got[1:]):
            assert same_bits(x, y)
    finally:
        batch.close()
        model.close()


# ---- 2. bit for bit against the ordinary call -----------------------------------------------

@pytest.mark.parametrize('n,kind,nsites', [(4, 'state', 300), (20, 'dense', mc.NSITES),
                                           (122, 'mask', mc.NSITES)])
def test_one_set_is_the_ordinary_call_bit_for_bit(contexts, n, kind, nsites):
    """K = 1 and any positive class weight: the posterior is exactly 1, so values, edge_sums and
    status are those of set_rates + branch_expectations with the same Q and t."""
    seed = 10000 + n
    case = mc.make_case(n, 'random', kind, 1, seed, nsites=nsites)
    coefs = make_coefs(n, 3, seed)
    w = site_weights(nsites, seed)
    want = ordinary(contexts, case, 0, coefs, w)
    model, batch = build(contexts, case, w)
    for c in (1.0, 0.37, 5e-3):
        got = model.branch_expectations_mixture(batch, coefs, [c])
        assert same_bits(got.values, want.values), c
        assert same_bits(got.edge_sums, want.edge_sums), c
        assert same_bits(got.set_edge_sums[0], want.edge_sums), c
        assert np.array_equal(got.status, want.status), c
        assert (got.class_posteriors == 1.0).all()
    batch.close()
    model.close()


@pytest.mark.parametrize('n,kind', [(3, 'mask'), (5, 'state'), (61, 'dense')])
def test_one_hot_weights_select_a_set_bit_for_bit(contexts, n, kind):
    """class_weights = e_k at K = 3: values are branch_expectations under set k, for every k --
    the per-set table offsets.  Then with all three classes on: the device's sums against the
    host re-summation of w post x_k (x_k from the one-hot calls; coefficients not negative, so
    only the summation order separates them: 1e-12 relative), and the log-likelihoods against
    step_multi + mixture_log_likelihoods."""
    seed = 10100 + n
    K = 3
    case = mc.make_case(n, 'balanced', kind, K, seed, zero_set=False)
    coefs = make_coefs(n, 2, seed)
    assert (coefs >= 0).all()
    w = np.random.RandomState(seed).uniform(0.5, 3.0, mc.NSITES)
    model, batch = build(contexts, case, w)
    x = []
    for k in range(K):
        want = ordinary(contexts, case, k, coefs)
        got = model.branch_expectations_mixture(batch, coefs, np.eye(K)[k])
        assert same_bits(got.values, want.values), k
        assert np.array_equal(got.status, want.status), k
        assert same_bits(got.class_posteriors, np.tile(np.eye(K)[k], (mc.NSITES, 1))), k
        x.append(got.values)
    c = class_weights(K, seed)
    got = model.branch_expectations_mixture(batch, coefs, c)
    post = got.class_posteriors
    for k in range(K):
        np.testing.assert_allclose(got.set_edge_sums[k],
                                   np.einsum('i,ivc->vc', w * post[:, k], x[k]), rtol=1e-12)
    np.testing.assert_allclose(got.edge_sums, got.set_edge_sums.sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(got.class_sums, (w[:, None] * post).sum(axis=0), rtol=1e-12)
    np.testing.assert_allclose(post.sum(axis=1), 1.0, rtol=1e-14)
    model.step_multi(batch)
    ll, st, _ = model.mixture_log_likelihoods(batch, c)
    assert not st.any()
    np.testing.assert_allclose(got.log_likelihoods, ll, rtol=1e-12)
    batch.close()
    model.close()


# ---- 3. sets that are not live --------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_skipped_sets_and_dead_sites(contexts, n):
    """K = 4, dense data: set 1 has weight 0, set 3 is the zero set (P = I), site 9 observes
    nothing at one leaf (likelihood zero under every set).  Posteriors of sets that are not live
    are exactly 0; nothing is NaN; a dead set leaks no status bit; the dead site has
    RT_SITE_ZERO_PROB, zeros and -inf and adds nothing to any sum; and a set of weight 0 gives
    what the call without that set gives."""
    from raoteh_amd import _lib
    seed = 10200 + n
    K, dead_site = 4, 9
    case = mc.make_case(n, 'random', 'dense', K, seed, dead_site=dead_site)
    coefs = make_coefs(n, 2, seed)
    c = np.array([0.3, 0.0, 0.5, 0.2])
    w = np.random.RandomState(seed).uniform(0.5, 2.0, mc.NSITES)
    model, batch = build(contexts, case, w)
    got = model.branch_expectations_mixture(batch, coefs, c)
    want = mc.mixture_reference(model.tree, case, coefs, c, w)
    for a in got[:5]:
        assert np.isfinite(a).all()
    np.testing.assert_array_equal(got.status,
                                  np.where(np.arange(mc.NSITES) == dead_site, _lib.RT_SITE_ZERO_PROB, 0))
    np.testing.assert_array_equal(got.status, want.status)
    assert not got.class_posteriors[:, 1].any() and not got.set_edge_sums[1].any()
    assert got.class_sums[1] == 0.0
    dead3 = ~(want.L[3] > 0)
    assert dead3.sum() >= 2 and not got.class_posteriors[dead3, 3].any()
    assert got.log_likelihoods[dead_site] == -np.inf
    assert not got.values[dead_site].any() and not got.class_posteriors[dead_site].any()
    live = np.arange(mc.NSITES) != dead_site
    assert np.isfinite(got.log_likelihoods[live]).all()
    check_values(got.values, want.values, 'n=%d values' % n)
    check_values(got.set_edge_sums, want.set_edge_sums, 'n=%d per-set sums' % n)
    check_values(got.class_posteriors, want.post, 'n=%d posteriors' % n)
    # the dead site adds nothing: ten times its weight, the same bits in every sum
    w2 = w.copy()
    w2[dead_site] *= 10.0
    batch.set_weights(w2)
    more = model.branch_expectations_mixture(batch, coefs, c)
    for a, b in zip(more[1:5], got[1:5]):
        assert same_bits(a, b)
    # without set 1 at all
    keep = [0, 2, 3]
    three = case._replace(Q=case.Q[keep], t=case.t[keep])
    model3, batch3 = build(contexts, three, w)
    less = model3.branch_expectations_mixture(batch3, coefs, c[keep])
    assert same_bits(less.values, got.values)
    assert same_bits(less.log_likelihoods, got.log_likelihoods)
    assert same_bits(less.set_edge_sums, np.ascontiguousarray(got.set_edge_sums[keep]))
    for b in (batch, batch3):
        b.close()
    model.close()
    model3.close()


# ---- 4. repeatability and side effects ------------------------------------------------------

@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense'), (61, 'mask')])
def test_repeatability_and_side_effects(contexts, n, kind):
    from raoteh_amd import device, _lib as lib
    seed = 10300 + n
    K = 3
    case = mc.make_case(n, 'balanced', kind, K, seed)
    coefs = make_coefs(n, 3, seed)
    c = class_weights(K, seed)
    w = np.random.RandomState(n).uniform(0.5, 2.0, mc.NSITES)
    model, batch = build(contexts, case, w)
    model.set_rates(Q=case.Q[1], node_q=case.node_q, t=case.t[1])     # the model's own rates
    own = model.get_transitions()
    first = model.branch_expectations_mixture(batch, coefs, c)       # no earlier step is needed
    model.step(batch)
    model.step_multi(batch)
    ll, st = model.fetch_log_likelihoods(batch)
    mll, mst = model.fetch_multi_log_likelihoods(batch)
    name = batch.kernel_name
    a = model.branch_expectations_mixture(batch, coefs, c)
    b = model.branch_expectations_mixture(batch, coefs, c)
    for x, y, z in zip(a, b, first):
        assert same_bits(x, y) and same_bits(x, z)
    post, pll = model.class_posteriors(batch, c)
    assert same_bits(post, a.class_posteriors) and same_bits(pll, a.log_likelihoods)
    # the raw call with nothing at all
    p_f64 = ctypes.POINTER(ctypes.c_double)
    rc = lib.lib().rt_sites_branch_expectations_mixture(
        model._h, batch._h, 0, c.ctypes.data_as(p_f64), 3, 0, coefs.ctypes.data_as(p_f64), None, None,
        None, None, None, None, None)
    assert rc == lib.RT_OK
    # one matrix alone gives the bits it gives among others
    one = model.branch_expectations_mixture(batch, coefs[1], c)
    assert same_bits(one.values[:, :, 0], np.ascontiguousarray(a.values[:, :, 1]))
    # what was fetched before is unchanged
    ll2, st2 = model.fetch_log_likelihoods(batch)
    assert same_bits(ll2, ll) and np.array_equal(st2, st)
    mll2, mst2 = model.fetch_multi_log_likelihoods(batch)
    assert same_bits(mll2, mll) and np.array_equal(mst2, mst)
    assert batch.kernel_name == name
    assert same_bits(model.get_transitions(), own)
    # new rate sets: recompute_transitions on the old model, and a fresh model
    Q2, t2 = case.Q[::-1].copy(), case.t[::-1] * 1.25
    model.set_rate_sets(Q2, t=t2, node_q=case.node_q)
    again = model.branch_expectations_mixture(batch, coefs, c, recompute_transitions=True)
    fmodel, fbatch = smc.upload(device, contexts(), case)
    fbatch.set_weights(w)
    fmodel.set_rate_sets(Q2, t=t2, node_q=case.node_q)
    fresh = fmodel.branch_expectations_mixture(fbatch, coefs, c)
    for x, y in zip(again, fresh):
        assert same_bits(x, y)
    assert not same_bits(again.values, a.values)
    assert same_bits(model.get_transitions(), own)
    for x in (batch, fbatch):
        x.close()
    model.close()
    fmodel.close()


# ---- 5. the gradients -----------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 61])
def test_gradients_against_the_host_reference(contexts, n):
    """branch_length_gradient_mixture (g_t, g_c, total) and the gradient in a kappa-style rate
    parameter (rate_parameter_coefs per class, summed over the branches) against the host
    reference, at the tolerances of the per-site values; tests/test_mixture_expect_cpu.py holds
    that reference to central differences of the oracle's mixture total."""
    seed = 10400 + n
    case = mc.gradient_case(n, seed, nsites=53)
    c = np.array([0.5, 0.3, 0.2])
    w = np.random.RandomState(seed).randint(1, 4, size=53).astype(float)
    model, batch = build(contexts, case, w)
    want_t, want_c, want_kappa, want_total = mc.reference_gradients(model.tree, case, c, w)
    g_t, g_c, total = model.branch_length_gradient_mixture(batch, c)
    assert g_t.shape == case.t.shape and not g_t[:, 0].any() and g_c.shape == (3,)
    check_values(g_t, want_t, 'n=%d g_t' % n)
    check_values(g_c, want_c, 'n=%d g_c' % n)
    assert total == pytest.approx(want_total, rel=1e-12)
    kap = model.branch_expectations_mixture(batch, mc.kappa_coefs(case), c, per_site=False)
    got_kappa = kap.edge_sums[:, 0].sum()
    print('n=%d d/dkappa: device %.12g reference %.12g' % (n, got_kappa, want_kappa))
    scale = np.abs(mc.mixture_reference(model.tree, case, mc.kappa_coefs(case), c, w,
                                        check=0).edge_sums).max()
    np.testing.assert_allclose(got_kappa, want_kappa, rtol=1e-9, atol=1e-13 * scale * len(case.t[0]))
    # a class of weight 0 has derivative 0 by the convention of the call
    g_t0, g_c0, _ = model.branch_length_gradient_mixture(batch, [0.6, 0.0, 0.4])
    assert g_c0[1] == 0.0 and not g_t0[1].any()
    # a resident branch length of 0 says nothing about its derivative
    t0 = case.t.copy()
    t0[1, 3] = 0.0
    model.set_rate_sets(case.Q, t=t0, node_q=case.node_q)
    with pytest.raises(ValueError, match='branch length'):
        model.branch_length_gradient_mixture(batch, c)
    batch.close()
    model.close()


# ---- 6. the documented errors ---------------------------------------------------------------

def test_documented_errors(contexts):
    from raoteh_amd import device, _lib
    n, K = 20, 3
    case = mc.make_case(n, 'balanced', 'dense', K, 10500)
    model, batch = build(contexts, case)
    N = model.tree.nnodes
    E = np.ones((n, n))
    c = class_weights(K, 10500)
    good = model.branch_expectations_mixture(batch, E, c)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    sums = np.zeros((N, 9))

    def raw(m, b, cw, ncoefs, per_set, coefs):
        return _lib.lib().rt_sites_branch_expectations_mixture(
            m._h, b._h, 0, None if cw is None else np.ascontiguousarray(cw).ctypes.data_as(p_f64),
            ncoefs, per_set, None if coefs is None else coefs.ctypes.data_as(p_f64), None,
            sums.ctypes.data_as(p_f64), None, None, None, None, None)
    # no rate sets
    bare, bbatch = smc.upload(device, contexts(), case)
    with pytest.raises(ValueError, match='set_rate_sets'):
        bare.branch_expectations_mixture(bbatch, E, c)
    assert raw(bare, bbatch, c, 1, 0, E) == _lib.RT_ERR_INVALID
    assert 'rate sets' in _lib.last_error()
    # a batch of another model
    bare.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    with pytest.raises(ValueError, match='another model'):
        bare.branch_expectations_mixture(batch, E, c)
    # the class weights
    assert raw(model, batch, None, 1, 0, E) == _lib.RT_ERR_INVALID
    for bad in ([0.5, -0.1, 0.6], [0.5, np.nan, 0.5], [np.inf, 0.0, 0.0], [0.0, 0.0, 0.0]):
        assert raw(model, batch, np.array(bad), 1, 0, E) == _lib.RT_ERR_INVALID
        assert 'class_weights' in _lib.last_error()
        with pytest.raises(ValueError):
            model.branch_expectations_mixture(batch, E, bad)
    with pytest.raises(ValueError):
        model.branch_expectations_mixture(batch, E, [0.5, 0.5])
    # no matrix, no coefficients, a coefficient that is not finite (shared, and in the last set's)
    assert raw(model, batch, c, 0, 0, E) == _lib.RT_ERR_INVALID
    assert raw(model, batch, c, 1, 0, None) == _lib.RT_ERR_INVALID
    bad = E.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        model.branch_expectations_mixture(batch, bad, c)
    assert raw(model, batch, c, 1, 0, bad) == _lib.RT_ERR_INVALID
    per_set = np.ones((K, 1, n, n))
    per_set[K - 1, 0, 19, 19] = np.inf
    assert raw(model, batch, c, 1, 1, per_set) == _lib.RT_ERR_INVALID
    with pytest.raises(ValueError, match='nsets'):
        model.branch_expectations_mixture(batch, np.ones((K + 1, 1, n, n)), c)
    # nine matrices (the Python check comes first; the C ABI has its own)
    with pytest.raises(ValueError):
        model.branch_expectations_mixture(batch, np.zeros((9, n, n)), c)
    assert raw(model, batch, c, 9, 0, np.zeros((9, n, n))) == _lib.RT_ERR_UNSUPPORTED
    assert 'coefficient matrices' in _lib.last_error()
    # a partitioned batch: the Python surface and the C ABI
    pcase = pc.make_case(n, 'dense', 10500)
    pmodel, pbatch = pc.upload(device, contexts(), pcase)
    pmodel.set_rate_sets(pcase.Q, t=pcase.t, node_q=pcase.node_q)
    pc_w = class_weights(pcase.nsets, 1)
    with pytest.raises(ValueError, match='ordinary batch'):
        pmodel.branch_expectations_mixture(pbatch, E, pc_w)
    assert raw(pmodel, pbatch, pc_w, 1, 0, E) == _lib.RT_ERR_UNSUPPORTED
    assert 'partitioned' in _lib.last_error()
    pmodel.step_partitioned(pbatch)
    pll = pmodel.fetch_log_likelihoods(pbatch)[0]
    assert np.isfinite(pll).all()
    # a "rescale" batch
    rmodel, rbatch = smc.upload(device, contexts(rescale=1), case)
    rmodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    with pytest.raises(_lib.RaotehHipError) as err:
        rmodel.branch_expectations_mixture(rbatch, E, c)
    assert err.value.code == _lib.RT_ERR_UNSUPPORTED and 'rescale' in str(err.value)
    # the batch is untouched by all that, and the context still works
    again = model.branch_expectations_mixture(batch, E, c)
    for x, y in zip(again, good):
        assert same_bits(x, y)
    for x in (batch, bbatch, pbatch, rbatch):
        x.close()
    for m in (model, bare, pmodel, rmodel):
        m.close()
