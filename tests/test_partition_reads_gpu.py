"""rt_sites_branch_expectations_partitioned (TreeModel.branch_expectations_partitioned /
branch_length_gradient_partitioned) on the GPU: per-site, per-branch expected history statistics
of a partitioned batch, every site under its own rate set.  Against the host reference that no
device path enters (tests/_partition_read_cases.py); bit for bit against the ordinary call on
each set's sites; pads, order and weights; a zero-probability status that depends on the set; the
analytic gradient in every set's branch lengths against central differences of the partitioned
likelihood; side effects and repeatability; the documented errors."""
import ctypes

import numpy as np
import pytest

import _partition_cases as pc
import _partition_read_cases as prc
import _step_multi_cases as smc
from _branch_cases import make_coefs

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
GRADIENT_H = 1e-5


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


def build(contexts, case, weights=None):
    from raoteh_amd import device
    model, batch = pc.upload(device, contexts(), case)
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


def check_values(got, want, label):
    """check_values of test_branch_expect_gpu.py: the project's tolerances for expected history
    statistics at every n up to 128."""
    scale = np.abs(want).max()
    print('%s: max |value - ref| / scale %.2e (scale %.3g)'
          % (label, np.abs(got - want).max() / scale, scale))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-13 * scale)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(smc.bits(a), smc.bits(b))


# ---- 1. against the host reference ---------------------------------------------------------

# the lane kernel with both granules, one to eight row tiles, both derivative routes (block
# exponential up to 64 states, pair recurrence above), every observation kind; 1 / 4 / 8
# coefficient matrices, shared or per set; weights in half.  sets: 'empty' = site i in set i % 3
# of 4 (set 3 empty), 'single' = the same with one site moved to set 3 (its granule: one real
# site and pads), 'runs' = a random order of runs that are no multiple of the granule
REFERENCE_CASES = [
    # n, kind, coefficient matrices, per set, weights, RAOTEH_LANE_NO_PLDS, sets
    (3, 'state', 1, False, False, False, 'empty'),
    (4, 'dense', 8, True, True, False, 'single'),
    (4, 'dense', 4, False, True, True, 'runs'),
    (5, 'dense', 4, True, False, False, 'empty'),
    (20, 'mask', 1, True, True, False, 'single'),
    (61, 'state', 4, False, True, False, 'empty'),
    (64, 'dense', 8, False, False, False, 'empty'),
    (65, 'state', 4, False, True, False, 'runs'),
    (122, 'mask', 1, True, False, False, 'empty'),
    (128, 'dense', 1, True, True, False, 'single'),
]


def reference_case(n, kind, sets, seed):
    if sets == 'runs':
        G = 64 if n <= 4 else 16
        site_sets = np.random.RandomState(seed).permutation(
            np.repeat([0, 1, 2, 3], [G + 6, G - 4, G + 3, 2]))
        return pc.make_case(n, kind, seed, nsites=len(site_sets), site_sets=site_sets)
    case = pc.make_case(n, kind, seed)
    if sets == 'single':
        site_sets = case.site_sets.copy()
        site_sets[7] = 3
        case = case._replace(site_sets=site_sets)
    return case


@pytest.mark.parametrize('n,kind,ncoefs,per_set,weighted,no_plds,sets', REFERENCE_CASES,
                         ids=['n%d-%s-k%d-%s%s' % (c[0], c[1], c[2], c[6], '-noplds' if c[5] else '')
                              for c in REFERENCE_CASES])
def test_against_the_host_reference(contexts, monkeypatch, n, kind, ncoefs, per_set, weighted,
                                    no_plds, sets):
    seed = 9000 + n + (50 if no_plds else 0)
    if no_plds:
        monkeypatch.setenv('RAOTEH_LANE_NO_PLDS', '1')
    case = reference_case(n, kind, sets, seed)
    nsites = len(case.site_sets)
    coefs = make_coefs(n, ncoefs, seed)
    if per_set:
        coefs = np.array([make_coefs(n, ncoefs, seed + 100 * k) for k in range(case.nsets)])
    weights = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(float) if weighted else None
    model, batch = build(contexts, case, weights)
    try:
        got = model.branch_expectations_partitioned(batch, coefs)
        want, wstatus, want_sets, want_sums = prc.partition_reference(model.tree, case, coefs, weights)
        N = model.tree.nnodes
        assert got.nodes == list(model.tree.preorder_nodes)
        assert got.values.shape == (nsites, N, ncoefs)
        assert got.set_edge_sums.shape == (case.nsets, N, ncoefs) and got.edge_sums.shape == (N, ncoefs)
        np.testing.assert_array_equal(got.status, wstatus)
        assert not got.values[:, 0].any()
        if ncoefs >= 4 and not per_set:
            assert not got.values[:, :, 3].any()           # the all-zero matrix
        check_values(got.values, want, 'n=%d %s values' % (n, kind))
        check_values(got.set_edge_sums, want_sets, 'n=%d %s per-set sums' % (n, kind))
        check_values(got.edge_sums, want_sums, 'n=%d %s edge sums' % (n, kind))
        counts = np.bincount(case.site_sets, minlength=case.nsets)
        if sets == 'empty':
            assert counts[3] == 0 and not got.set_edge_sums[3].any()     # exactly zero
        if sets == 'single':
            assert counts[3] == 1
            w7 = 1.0 if weights is None else weights[7]
            np.testing.assert_allclose(got.set_edge_sums[3], w7 * got.values[7], rtol=1e-15)
        sums_only = model.branch_expectations_partitioned(batch, coefs, per_site=False)
        assert sums_only.values is None
        assert same_bits(sums_only.set_edge_sums, got.set_edge_sums)
        assert same_bits(sums_only.edge_sums, got.edge_sums)
        assert np.array_equal(sums_only.status, got.status)
    finally:
        batch.close()
        model.close()


# ---- 2. bit for bit against the ordinary call ----------------------------------------------

@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense'), (61, 'state')])
def test_bit_for_bit_against_the_ordinary_call(contexts, n, kind):
    """Set k's sites as an ordinary batch under set_rates(Q[k], node_q, t[k]) on a jit = 0
    context: the same arithmetic per site column and per edge, and set k's transition matrices
    are those of rt_model_set_rates bit for bit -- a difference is a wrong table or slot."""
    from raoteh_amd import device
    case = pc.make_case(n, kind, seed=9100 + n)
    coefs = make_coefs(n, 2, 9100 + n)
    model, batch = build(contexts, case)
    got = model.branch_expectations_partitioned(batch, coefs)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        om = device.TreeModel(case.T, case.root, n, ctx=contexts())
        om.set_root_distn(case.root_distn)
        om.set_rates(Q=case.Q[k], node_q=case.node_q, t=case.t[k])
        ob = om.upload_sites(case.leaves, case.data[mine], kind=kind)
        want = om.branch_expectations(ob, coefs)
        assert same_bits(np.ascontiguousarray(got.values[mine]), want.values), k
        assert np.array_equal(got.status[mine], want.status), k
        ob.close()
        om.close()
    batch.close()
    model.close()


# ---- 3. pads and order ---------------------------------------------------------------------

@pytest.mark.parametrize('n,kind', [(4, 'dense'), (20, 'state')])
def test_pads_order_and_weights(contexts, n, kind):
    """A random, unsorted site_sets whose runs all end in pads.  The coefficients are not
    negative, so every sum has terms of one sign and only the summation order separates the
    device's sums from numpy's: 1e-12 relative (the criterion of test_partition_gpu.py)."""
    G = pc.granule(n)
    rng = np.random.RandomState(9200 + n)
    site_sets = rng.permutation(np.repeat([0, 1, 2, 3], [G + 9, 7, 2 * G - 5, 1]))
    case = pc.make_case(n, kind, 9200 + n, nsites=len(site_sets), site_sets=site_sets)
    nsites = len(site_sets)
    coefs = make_coefs(n, 2, 9200 + n)
    assert (coefs >= 0).all()
    w = rng.uniform(0.5, 3.0, nsites)
    model, batch = build(contexts, case, w)
    got = model.branch_expectations_partitioned(batch, coefs)
    assert got.values.shape[0] == nsites and (got.values >= 0).all()
    for k in range(case.nsets):
        mine = case.site_sets == k
        np.testing.assert_allclose(got.set_edge_sums[k],
                                   np.einsum('i,ivc->vc', w[mine], got.values[mine]), rtol=1e-12)
    np.testing.assert_allclose(got.edge_sums, got.set_edge_sums.sum(axis=0), rtol=1e-12)
    # twice the weight of one site: its set's sums grow by that site's values, the others stay
    i = int(np.flatnonzero(case.site_sets == 2)[3])
    w2 = w.copy()
    w2[i] *= 2.0
    batch.set_weights(w2)
    more = model.branch_expectations_partitioned(batch, coefs)
    assert same_bits(more.values, got.values)
    np.testing.assert_allclose(more.set_edge_sums[2], got.set_edge_sums[2] + w[i] * got.values[i],
                               rtol=1e-12)
    for k in (0, 1, 3):
        assert same_bits(more.set_edge_sums[k], got.set_edge_sums[k])
    # no weights: every real site once, no pad at all
    batch.set_weights(None)
    plain = model.branch_expectations_partitioned(batch, coefs)
    np.testing.assert_allclose(plain.edge_sums, got.values.sum(axis=0), rtol=1e-12)
    batch.close()
    model.close()


# ---- 4. zero probability depends on the set ------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_zero_probability_depends_on_the_set(contexts, n):
    """Set 0 has Q = 0 (P = I): its sites whose leaves disagree have likelihood zero -- status
    RT_SITE_ZERO_PROB, values 0, nothing added to any sum.  The same data under another set is
    live, and the other sets' sites get the bits they get when set 0 has rates like the rest."""
    from raoteh_amd import _lib
    seed = 9300 + n
    case = pc.make_case(n, 'state', seed, zero_set=0)
    coefs = make_coefs(n, 2, seed)
    model, batch = build(contexts, case)
    got = model.branch_expectations_partitioned(batch, coefs)
    in0 = case.site_sets == 0
    zero = in0 & (case.data != case.data[:, :1]).any(axis=1)
    assert zero.sum() >= 10 and (in0 & ~zero).sum() >= 3
    np.testing.assert_array_equal(got.status, np.where(zero, _lib.RT_SITE_ZERO_PROB, 0))
    assert not got.values[zero].any()
    assert got.values[~zero][:, 1:, 1].all()
    live0 = in0 & ~zero
    np.testing.assert_allclose(got.set_edge_sums[0], got.values[live0].sum(axis=0), rtol=1e-12)
    want = prc.partition_reference(model.tree, case, coefs)
    np.testing.assert_array_equal(got.status, want[1])
    check_values(got.values, want[0], 'n=%d zero set values' % n)
    check_values(got.set_edge_sums, want[2], 'n=%d zero set sums' % n)
    batch.close()
    model.close()
    # the other sets are untouched by what set 0 holds
    other = pc.make_case(n, 'state', seed)
    assert np.array_equal(other.Q[1:], case.Q[1:]) and np.array_equal(other.data, case.data)
    model, batch = build(contexts, other)
    ref = model.branch_expectations_partitioned(batch, coefs)
    assert same_bits(np.ascontiguousarray(ref.values[~in0]), np.ascontiguousarray(got.values[~in0]))
    assert same_bits(ref.set_edge_sums[1:], got.set_edge_sums[1:])
    assert not ref.status.any()
    batch.close()
    model.close()


# ---- 5. the gradient -----------------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(4, 773), (61, 53)])
def test_branch_length_gradient_partitioned(contexts, n, nsites):
    """branch_length_gradient_partitioned (analytic, one call with per-set coefficients) against
    the central difference of fetch_partition_totals(...)[k, 0] in t[k][v], taken through
    set_rate_sets + step_partitioned, step h = 1e-5 (on the truncation side of the central
    difference, as in test_branch_expect_gpu.test_branch_length_gradient, so that the oracle's
    difference and the device's share their dominant error).

    The bound is measured, not chosen: the same central difference of the ORACLE's per-set
    log-likelihood sum (scipy expm, oracle passes) against the host reference's analytic value
    (tests/_partition_read_cases.py) for the same case and step; the device is allowed ten times
    that gap.  Measured on the CPU for these two cases (max over sets and branches, absolute):
    n = 4: gap 4.4e-07 (gradients up to 3.4e+02), bound 4.4e-06;
    n = 61: gap 5.1e-07 (gradients up to 1.1e+02), bound 5.1e-06.
    The device's analytic value is also held to the host's analytic value directly, at the
    tolerances of the per-site values."""
    case = prc.gradient_case(n, 9500 + n, nsites)
    assert case.Q.shape[1] == 1
    h = GRADIENT_H
    model, batch = build(contexts, case)
    ta = model.tree
    N = ta.nnodes
    analytic, gap = prc.gradient_gap(ta, case, h)
    bound = 10.0 * gap
    print('n=%d: oracle central difference vs host analytic: max gap %.2e (max |gradient| %.2e); '
          'device bound %.2e' % (n, gap, np.abs(analytic).max(), bound))
    grad = model.branch_length_gradient_partitioned(batch)
    assert grad.shape == (case.nsets, N) and not grad[:, 0].any() and not grad[3].any()
    fd = np.zeros((case.nsets, N))
    for k in range(3):
        for v in range(1, N):
            tot = []
            for sign in (1.0, -1.0):
                t = case.t.copy()
                t[k, v] += sign * h
                model.set_rate_sets(case.Q, t=t, node_q=case.node_q)
                model.step_partitioned(batch, recompute_transitions=False)
                ptot = model.fetch_partition_totals(batch)
                assert ptot[k, 1] == 0
                tot.append(ptot[k, 0])
            fd[k, v] = (tot[0] - tot[1]) / (2 * h)
    print('n=%d: device analytic vs device central difference: max gap %.2e; vs host analytic '
          '%.2e' % (n, np.abs(grad - fd).max(), np.abs(grad - analytic).max()))
    assert np.abs(grad - fd).max() <= bound
    np.testing.assert_allclose(grad, analytic, rtol=1e-9, atol=1e-13 * np.abs(analytic).max())
    # the chain rule of t[k][v] = r_k tau_v is a contraction of that array
    from raoteh_amd import device
    d_tau, d_r = device.partition_chain_rule(grad, np.ones(case.nsets), np.ones(N))
    np.testing.assert_allclose(d_tau, grad.sum(axis=0), rtol=1e-14)
    np.testing.assert_allclose(d_r, grad.sum(axis=1), rtol=1e-14)
    batch.close()
    model.close()


def test_gradient_refuses_several_rate_matrices_per_set(contexts):
    from raoteh_amd import device
    case = pc.make_case(5, 'state', 9600)
    model, batch = build(contexts, case)
    with pytest.raises(ValueError, match='one rate matrix per set'):
        model.branch_length_gradient_partitioned(batch)
    fresh = pc.upload(device, contexts(), case)
    with pytest.raises(ValueError, match='set_rate_sets'):
        fresh[0].branch_length_gradient_partitioned(fresh[1])
    for x in (batch, fresh[1]):
        x.close()
    model.close()
    fresh[0].close()


# ---- 6. side effects and repeatability -----------------------------------------------------

@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense'), (97, 'mask')])
def test_side_effects_and_repeatability(contexts, n, kind):
    from raoteh_amd import device, _lib as lib
    seed = 9700 + n
    case = pc.make_case(n, kind, seed, zero_set=2)
    coefs = make_coefs(n, 3, seed)
    w = np.random.RandomState(n).uniform(0.5, 2.0, len(case.site_sets))
    model, batch = build(contexts, case, w)
    model.set_rates(Q=case.Q[1], node_q=case.node_q, t=case.t[1])     # the model's own rates
    own = model.get_transitions()
    # no earlier step is needed
    first = model.branch_expectations_partitioned(batch, coefs)
    model.step_partitioned(batch)
    ll, st = model.fetch_log_likelihoods(batch)
    totals = model.fetch_totals(batch)
    ptot, ws = model.fetch_partition_totals(batch, weighted=True)
    name = batch.kernel_name
    a = model.branch_expectations_partitioned(batch, coefs)
    b = model.branch_expectations_partitioned(batch, coefs)
    for x, y, z in zip(a[:4], b[:4], first[:4]):
        assert same_bits(x, y) and same_bits(x, z)
    # the raw call with nothing but the status, and with nothing at all
    status = np.full(len(case.site_sets), -1, dtype=np.int32)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    rc = lib.lib().rt_sites_branch_expectations_partitioned(
        model._h, batch._h, 0, 3, 0, coefs.ctypes.data_as(p_f64), None, None, None,
        status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
    assert rc == lib.RT_OK and np.array_equal(status, a.status)
    rc = lib.lib().rt_sites_branch_expectations_partitioned(
        model._h, batch._h, 0, 3, 0, coefs.ctypes.data_as(p_f64), None, None, None, None)
    assert rc == lib.RT_OK
    # one matrix alone gives the bits it gives among others
    one = model.branch_expectations_partitioned(batch, coefs[1])
    assert same_bits(one.values[:, :, 0], np.ascontiguousarray(a.values[:, :, 1]))
    # what was fetched before is unchanged, and the getters still answer
    ll2, st2 = model.fetch_log_likelihoods(batch)
    assert same_bits(ll2, ll) and np.array_equal(st2, st)
    assert same_bits(model.fetch_totals(batch), totals)
    ptot2, ws2 = model.fetch_partition_totals(batch, weighted=True)
    assert same_bits(ptot2, ptot) and same_bits(ws2, ws)
    assert batch.kernel_name == name
    assert same_bits(model.get_transitions(), own)
    # new rates: recompute_transitions on the old model, and a fresh model
    Q2, t2 = case.Q[::-1].copy(), case.t[::-1] * 1.25
    model.set_rate_sets(Q2, t=t2, node_q=case.node_q)
    again = model.branch_expectations_partitioned(batch, coefs, recompute_transitions=True)
    fmodel, fbatch = pc.upload(device, contexts(), case)
    fbatch.set_weights(w)
    fmodel.set_rate_sets(Q2, t=t2, node_q=case.node_q)
    fresh = fmodel.branch_expectations_partitioned(fbatch, coefs)
    for x, y in zip(again[:4], fresh[:4]):
        assert same_bits(x, y)
    assert not same_bits(again.values, a.values)
    assert same_bits(model.get_transitions(), own)
    for x in (batch, fbatch):
        x.close()
    model.close()
    fmodel.close()


# ---- 7. the documented errors --------------------------------------------------------------

def test_documented_errors(contexts):
    from raoteh_amd import device, _lib
    n = 20
    case = pc.make_case(n, 'dense', 9800)
    model, batch = build(contexts, case)
    N = model.tree.nnodes
    E = np.ones((n, n))
    good = model.branch_expectations_partitioned(batch, E)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    sums = np.zeros((N, 9))

    def raw(m, b, ncoefs, per_set, coefs):
        return _lib.lib().rt_sites_branch_expectations_partitioned(
            m._h, b._h, 0, ncoefs, per_set, None if coefs is None else coefs.ctypes.data_as(p_f64),
            None, sums.ctypes.data_as(p_f64), None, None)
    # an ordinary batch: the Python surface and the C ABI
    omodel, obatch = pc.upload(device, contexts(), case, partitioned=False)
    omodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    with pytest.raises(ValueError, match='site_sets'):
        omodel.branch_expectations_partitioned(obatch, E)
    assert raw(omodel, obatch, 1, 0, E) == _lib.RT_ERR_INVALID
    assert 'ordinary batch' in _lib.last_error()
    # a batch of another model
    with pytest.raises(ValueError, match='another model'):
        omodel.branch_expectations_partitioned(batch, E)
    # fewer rate sets in the model than the batch uses (none at all included)
    few = device.TreeModel(case.T, case.root, n, ctx=contexts())
    fb = few.upload_sites(case.leaves, case.data, kind=case.kind, site_sets=case.site_sets,
                          nsets=case.nsets)
    with pytest.raises(ValueError, match='rate sets'):
        few.branch_expectations_partitioned(fb, E)
    few.set_rate_sets(case.Q[:3], t=case.t[:3], node_q=case.node_q)
    with pytest.raises(ValueError, match='rate sets'):
        few.branch_expectations_partitioned(fb, E)
    # nine matrices (the Python check comes first; the C ABI has its own)
    with pytest.raises(ValueError):
        model.branch_expectations_partitioned(batch, np.zeros((9, n, n)))
    assert raw(model, batch, 9, 0, np.zeros((9, n, n))) == _lib.RT_ERR_UNSUPPORTED
    assert 'coefficient matrices' in _lib.last_error()
    # no matrix, no coefficients
    assert raw(model, batch, 0, 0, E) == _lib.RT_ERR_INVALID
    assert raw(model, batch, 1, 0, None) == _lib.RT_ERR_INVALID
    # a NaN coefficient, shared and in the last set's matrix
    bad = E.copy()
    bad[3, 4] = np.nan
    with pytest.raises(ValueError):
        model.branch_expectations_partitioned(batch, bad)
    assert raw(model, batch, 1, 0, bad) == _lib.RT_ERR_INVALID
    per_set = np.ones((case.nsets, 1, n, n))
    per_set[3, 0, 19, 19] = np.nan
    assert raw(model, batch, 1, 1, per_set) == _lib.RT_ERR_INVALID
    # a per-set array with the wrong leading dimension
    with pytest.raises(ValueError, match='nsets'):
        model.branch_expectations_partitioned(batch, np.ones((3, 1, n, n)))
    # the ordinary call keeps refusing the partitioned batch, and the context still works
    model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])
    with pytest.raises(_lib.RaotehHipError) as err:
        model.branch_expectations(batch, E)
    assert err.value.code == _lib.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
    again = model.branch_expectations_partitioned(batch, E)
    assert same_bits(again.values, good.values)
    for x in (batch, obatch, fb):
        x.close()
    for m in (model, omodel, few):
        m.close()
