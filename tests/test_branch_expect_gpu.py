"""rt_sites_branch_expectations (TreeModel.branch_expectations / branch_length_gradient,
_mjp_dense.get_expected_ntransitions) on the GPU: per-site, per-branch expected history
statistics against a host reference that no device path enters (tests/_branch_cases.py: the
oracle's D and J, scipy expm and expm_frechet), the invariants that need no reference, the
reference's own record of examples/code2x3/run.py, the analytic branch-length gradient against
finite differences, side effects, determinism and the documented errors."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_numpy as orc
from _branch_cases import branch_reference, load_golden, make_coefs
from _resident_cases import make_case, set_rates

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


@pytest.fixture(scope='module')
def ra():
    from raoteh_amd import device, _lib

    class NS(object):
        pass
    ns = NS()
    ns.device, ns.lib = device, _lib
    return ns


def open_context(ra, opts):
    ctx = ra.device.Context(0)
    for k, v in dict(DEFAULTS, **opts).items():
        ctx.set_option(k, v)
    return ctx


def build(ra, ctx, case, weights=None):
    model = ra.device.TreeModel(case.T, case.root, case.n, ctx=ctx)
    set_rates(model, case)
    model.set_root_distn(case.root_distn)
    batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


# ---- 1. against the host reference ---------------------------------------------------------

# both layouts (n <= 4: a lane per site), one to eight row tiles, every observation kind, the
# interpreter and the tree-specialised pruning kernel, weights, site counts that are no multiple
# of 16 or 64, 1 / 4 / 8 coefficient matrices (make_coefs: the second has a non-zero diagonal,
# the third negative entries, the fourth is all zero); per-edge rate matrices, internal observed
# nodes and a zero-likelihood site (the last) in every case
REFERENCE_CASES = [
    # n, kind, sites, tree nodes, jit, weights, coefficient matrices
    (2, 'state', 70, 9, 0, False, 1),
    (3, 'mask', 130, 10, 1, True, 4),
    (4, 'dense', 67, 8, 0, True, 8),
    (5, 'dense', 21, 9, 0, False, 4),
    (8, 'state', 37, 10, 1, True, 8),
    (20, 'mask', 50, 11, 0, False, 1),
    (61, 'state', 33, 12, 1, True, 4),
    (64, 'dense', 19, 9, 0, False, 8),
    (65, 'state', 17, 9, 0, True, 1),
    (97, 'mask', 50, 10, 1, False, 4),
    (122, 'mask', 45, 9, 1, False, 8),
    (128, 'dense', 19, 8, 0, True, 4),
]


def check_values(got, want, label):
    """check_step of test_expect_wide_gpu.py (the project's tolerances for expected history
    statistics at every n up to 128), on the per-site, per-edge values."""
    scale = np.abs(want).max()
    print('%s: max |value - ref| / scale %.2e (scale %.3g)'
          % (label, np.abs(got - want).max() / scale, scale))
    np.testing.assert_allclose(got, want, rtol=1e-9, atol=1e-13 * scale)


@pytest.mark.parametrize('n,kind,nsites,nnodes,jit,weighted,ncoefs', REFERENCE_CASES,
                         ids=['n%d-%s-jit%d-k%d' % (c[0], c[1], c[4], c[6])
                              for c in REFERENCE_CASES])
def test_against_the_host_reference(ra, n, kind, nsites, nnodes, jit, weighted, ncoefs):
    seed = 7000 + n
    case = make_case(n, nnodes, nsites, kind, seed, internal=True, per_edge=True)
    assert case.zero_site == nsites - 1
    coefs = make_coefs(n, ncoefs, seed)
    weights = None
    if weighted:
        weights = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(np.float64)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        got = model.branch_expectations(batch, coefs, recompute_transitions=True)
        want, wstatus = branch_reference(model, case, coefs, check_sites=[0, nsites // 2,
                                                                          nsites - 1])
        assert got.nodes == list(model.tree.preorder_nodes)
        np.testing.assert_array_equal(got.status, wstatus)
        assert wstatus[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB and wstatus.sum() == 1
        assert got.values.shape == (nsites, model.tree.nnodes, ncoefs)
        assert not got.values[:, 0].any() and not got.values[case.zero_site].any()
        if ncoefs >= 4:
            assert not got.values[:, :, 3].any()           # the all-zero matrix
        check_values(got.values, want, 'n=%d %s values' % (n, kind))
        w = np.ones(nsites) if weights is None else weights
        want_sums = np.einsum('i,ivk->vk', w, want)
        check_values(got.edge_sums, want_sums, 'n=%d %s edge sums' % (n, kind))
    finally:
        ctx.close()


# ---- 2. invariants that need no reference --------------------------------------------------

@pytest.mark.parametrize('n,kind,nsites,jit', [(3, 'state', 75, 1), (20, 'dense', 23, 0),
                                               (61, 'mask', 30, 1), (122, 'state', 18, 0)])
def test_identity_coefficients_give_the_branch_lengths(ra, n, kind, nsites, jit):
    """E = I weighs every unit of time by one: the expectation is the branch length, at every
    live site (the bound of the dwell.sum() invariant of test_expect_wide_gpu.py)."""
    case = make_case(n, 10, nsites, kind, 7100 + n, internal=True, per_edge=True)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case)
        got = model.branch_expectations(batch, np.eye(n))
        t = model.tree.branch_lengths().copy()
        t[0] = 0.0
        live = got.status == 0
        assert live.sum() == nsites - 1
        for i in np.nonzero(live)[0]:
            assert got.values[i, :, 0] == pytest.approx(t, rel=1e-10)
        assert not got.values[~live].any()
        assert got.edge_sums[:, 0] == pytest.approx(t * live.sum(), rel=1e-10)
    finally:
        ctx.close()


@pytest.mark.parametrize('n,kind,nsites', [(4, 'state', 90), (20, 'mask', 35), (97, 'state', 21)])
def test_indicator_coefficients_sum_to_the_history_statistics(ra, n, kind, nsites):
    """E = the indicator of one transition (c, d) resp. of one state c on the diagonal: summed
    over the branches, the edge sums are trans[c][d] resp. dwell[c] of
    expected_history_statistics on the same batch -- two routes through different contraction
    code (per site and branch here, summed over sites before the derivative there)."""
    case = make_case(n, 11, nsites, kind, 7200 + n, internal=False, per_edge=True)
    assert case.zero_site is None
    c, d = 1, 2
    assert all(Q[c, d] != 0 for Q in case.Qs)
    E = np.zeros((2, n, n))
    E[0, c, d] = 1.0
    E[1, c, c] = 1.0
    weights = np.random.RandomState(n).randint(1, 4, size=nsites).astype(np.float64)
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case, weights)
        dwell, rootp, trans = model.expected_history_statistics(batch)
        got = model.branch_expectations(batch, E, per_site=False)
        assert got.values is None
        total = got.edge_sums.sum(axis=0)
        print('n=%d: trans[%d][%d] %.17g vs %.17g, dwell[%d] %.17g vs %.17g'
              % (n, c, d, total[0], trans[c, d], c, total[1], dwell[c]))
        np.testing.assert_allclose(total, [trans[c, d], dwell[c]], rtol=1e-9)
    finally:
        ctx.close()


# ---- 3. the reference's record -------------------------------------------------------------

def test_reference_record_through_the_python_surface(ra):
    """Every call examples/code2x3/run.py makes to the reference's
    extras.get_expected_ntransitions (tests/golden/branch_expectations.json)."""
    from raoteh_amd import _mjp_dense
    _, calls = load_golden()
    ra.lib.check(ra.lib.lib().rt_set_option(b'jit', 0))
    try:
        for k, c in enumerate(calls):
            got = _mjp_dense.get_expected_ntransitions(
                c['T'], c['allowed'], c['root'], c['nstates'], root_distn=c['root_distn'],
                Q_default=c['Q'], E=c['E'])
            assert set(got) == set(c['expectations'])
            gap = max(abs(got[e] - x) for e, x in c['expectations'].items())
            print('call %d (%d states): max |value - reference| %.2e' % (k, c['nstates'], gap))
            for edge, want in c['expectations'].items():
                assert got[edge] == pytest.approx(want, rel=1e-10, abs=1e-13), (k, edge)
    finally:
        ra.lib.check(ra.lib.lib().rt_set_option(b'jit', -1))


def test_batch_form_of_the_python_surface(ra):
    """The same site three times with weights: per-site values repeat, the sums are weighted."""
    from raoteh_amd import _mjp_dense
    _, calls = load_golden()
    c = calls[-1]
    w = [1.0, 2.0, 0.5]
    ra.lib.check(ra.lib.lib().rt_set_option(b'jit', 0))
    try:
        out = _mjp_dense.get_expected_ntransitions_batch(
            c['T'], c['root'], c['nstates'], sites=[c['allowed']] * 3,
            root_distn=c['root_distn'], Q_default=c['Q'], E=c['E'], weights=w)
    finally:
        ra.lib.check(ra.lib.lib().rt_set_option(b'jit', -1))
    assert not out['status'].any()
    for edge, want in c['expectations'].items():
        assert out['values'][edge] == pytest.approx([want] * 3, rel=1e-10, abs=1e-13)
        assert out['edge_sums'][edge] == pytest.approx(3.5 * want, rel=1e-10, abs=1e-13)


# ---- 4. the branch-length gradient ---------------------------------------------------------

GRADIENT_H = 1e-5


def oracle_total(ta, case, t):
    import scipy.linalg
    esd = np.zeros((ta.nnodes, case.n, case.n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * case.Qs[case.node_q[v]])
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    ll, st = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                       case.root_distn)
    assert not st.any()
    return float(np.sum(ll))


@pytest.mark.parametrize('n,nsites', [(4, 300), (61, 200)])
def test_branch_length_gradient(ra, n, nsites):
    """branch_length_gradient (analytic, one call) against the central difference of
    total_log_likelihood in each branch length, step h = 1e-5.  (A central difference has the
    truncation error h^2 |f'''| / 6 and the rounding error eps |f| / h; with |f| ~ 4e3 and
    f''' ~ 5e4 here the two meet near h = 4e-6.  h = 1e-5 stays on the truncation side, so
    that the oracle's difference and the device's share their dominant error.)

    The bound is measured, not chosen: the same central difference of the ORACLE's
    log-likelihood (scipy expm, oracle passes) against the host reference's analytic value
    (tests/_branch_cases.py) for the same case and step; the device is allowed ten times that
    gap (finite differencing, not the device, dominates; ten covers the different summation
    order).  Measured on the CPU for these two cases (max over the branches, absolute):
    n = 4: gap 9.4e-07 (gradients up to 6.0e+02), bound 9.4e-06;
    n = 61: gap 7.6e-07 (gradients up to 2.9e+01), bound 7.6e-06.
    The device's analytic value is also held to the host's analytic value directly, at the
    tolerances of the per-site values."""
    case = make_case(n, 10, nsites, 'state', 7300 + n, internal=False, per_edge=False)
    assert case.zero_site is None and len(case.Qs) == 1
    h = GRADIENT_H
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        ta = model.tree
        t0 = ta.branch_lengths().copy()
        N = ta.nnodes
        # the host side: analytic value of the reference, central difference of the oracle
        E = np.ones((n, n))
        np.fill_diagonal(E, np.diag(case.Qs[0]))
        values, _ = branch_reference(model, case, E[None])
        analytic = np.zeros(N)
        analytic[1:] = values[:, 1:, 0].sum(axis=0) / t0[1:]
        fd_oracle = np.zeros(N)
        for v in range(1, N):
            tp, tm = t0.copy(), t0.copy()
            tp[v] += h
            tm[v] -= h
            fd_oracle[v] = (oracle_total(ta, case, tp) - oracle_total(ta, case, tm)) / (2 * h)
        gap = np.abs(fd_oracle - analytic).max()
        bound = 10.0 * gap
        print('n=%d: oracle central difference vs host analytic: max gap %.2e (max |gradient| '
              '%.2e); device bound %.2e' % (n, gap, np.abs(analytic).max(), bound))
        # the device: analytic in one call, central difference through the likelihood path
        grad = model.branch_length_gradient(batch)
        assert grad.shape == (N,) and grad[0] == 0.0
        fd = np.zeros(N)
        for v in range(1, N):
            tot = []
            for sign in (1.0, -1.0):
                t = t0.copy()
                t[v] += sign * h
                model.set_rates(Q=case.Qs, node_q=case.node_q, t=t)
                total, nzero = model.total_log_likelihood(batch)
                assert nzero == 0
                tot.append(total)
            fd[v] = (tot[0] - tot[1]) / (2 * h)
        print('n=%d: device analytic vs device central difference: max gap %.2e; vs host '
              'analytic %.2e' % (n, np.abs(grad - fd).max(), np.abs(grad - analytic).max()))
        assert np.abs(grad - fd).max() <= bound
        np.testing.assert_allclose(grad, analytic, rtol=1e-9, atol=1e-13 * np.abs(analytic).max())
    finally:
        ctx.close()


def test_gradient_refuses_per_edge_rate_matrices(ra):
    case = make_case(5, 8, 20, 'state', 7400, internal=False, per_edge=True)
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        with pytest.raises(ValueError):
            model.branch_length_gradient(batch)
    finally:
        ctx.close()


# ---- 5. side effects and determinism -------------------------------------------------------

@pytest.mark.parametrize('n,kind,nsites,jit', [(4, 'state', 131, 1), (20, 'dense', 37, 1),
                                               (97, 'mask', 29, 0)])
def test_side_effects_and_determinism(ra, n, kind, nsites, jit):
    case = make_case(n, 10, nsites, kind, 7500 + n, internal=True, per_edge=True)
    coefs = make_coefs(n, 3, 7500 + n)
    weights = np.random.RandomState(n).uniform(0.5, 2.0, size=nsites)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        ll, st = model.log_likelihoods(batch)
        totals = model.fetch_totals(batch)
        name = batch.kernel_name
        a = model.branch_expectations(batch, coefs)
        b = model.branch_expectations(batch, coefs)
        for x, y in zip(a[:3], b[:3]):
            assert x.tobytes() == y.tobytes()
        sums_only = model.branch_expectations(batch, coefs, per_site=False)
        assert sums_only.values is None
        assert sums_only.edge_sums.tobytes() == a.edge_sums.tobytes()
        assert sums_only.status.tobytes() == a.status.tobytes()
        # the raw call without edge sums, and without anything but the status
        N = model.tree.nnodes
        vals = np.full((nsites, N, 3), np.nan)
        status = np.full(nsites, -1, dtype=np.int32)
        p_f64 = ctypes.POINTER(ctypes.c_double)
        rc = ra.lib.lib().rt_sites_branch_expectations(
            model._h, batch._h, 0, 3, coefs.ctypes.data_as(p_f64), vals.ctypes.data_as(p_f64),
            None, status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert rc == ra.lib.RT_OK
        assert vals.tobytes() == a.values.tobytes() and status.tobytes() == a.status.tobytes()
        rc = ra.lib.lib().rt_sites_branch_expectations(
            model._h, batch._h, 0, 3, coefs.ctypes.data_as(p_f64), None, None, None)
        assert rc == ra.lib.RT_OK
        # one matrix alone gives the bits it gives among others
        one = model.branch_expectations(batch, coefs[1])
        assert one.values[:, :, 0].tobytes() == np.ascontiguousarray(a.values[:, :, 1]).tobytes()
        # the batch is as it was
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert model.fetch_totals(batch).tobytes() == totals.tobytes()
        assert batch.kernel_name == name
        ll3, st3 = model.log_likelihoods(batch)
        assert ll3.tobytes() == ll.tobytes() and st3.tobytes() == st.tobytes()
    finally:
        ctx.close()


# ---- 6. errors ------------------------------------------------------------------------------

def test_documented_errors(ra):
    n = 20
    case = make_case(n, 9, 25, 'state', 7600, internal=False, per_edge=False)
    E = np.ones((n, n))
    p_f64 = ctypes.POINTER(ctypes.c_double)
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        good = model.branch_expectations(batch, E)
        N = model.tree.nnodes
        # too many matrices (the Python check comes first; the C ABI has its own)
        with pytest.raises(ValueError):
            model.branch_expectations(batch, np.zeros((9, n, n)))
        many = np.zeros((9, n, n))
        sums = np.zeros((N, 9))
        rc = ra.lib.lib().rt_sites_branch_expectations(
            model._h, batch._h, 0, 9, many.ctypes.data_as(p_f64), None,
            sums.ctypes.data_as(p_f64), None)
        assert rc == ra.lib.RT_ERR_UNSUPPORTED
        assert 'coefficient matrices' in ra.lib.last_error()
        # non-finite coefficients at the C ABI
        bad = E.copy()
        bad[3, 4] = np.inf
        rc = ra.lib.lib().rt_sites_branch_expectations(
            model._h, batch._h, 0, 1, bad.ctypes.data_as(p_f64), None,
            sums.ctypes.data_as(p_f64), None)
        assert rc == ra.lib.RT_ERR_INVALID
        # a batch of another model
        other = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(other, case)
        with pytest.raises(ValueError, match='another model'):
            other.branch_expectations(batch, E)
        # transitions set directly: no rate matrices to differentiate
        direct = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        direct.set_transitions(model.get_transitions())
        direct.set_root_distn(case.root_distn)
        db = direct.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        with pytest.raises(ValueError, match='rt_model_set_rates'):
            direct.branch_expectations(db, E)
        # spectral rates
        spectral = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        spectral.set_rates_spectral(np.eye(n), -np.ones(n), np.eye(n))
        sb = spectral.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        with pytest.raises(ValueError, match='rt_model_set_rates'):
            spectral.branch_expectations(sb, E)
        # a "rescale" batch
        ctx.set_option('rescale', 1)
        try:
            rb = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        finally:
            ctx.set_option('rescale', 0)
        with pytest.raises(ra.lib.RaotehHipError) as err:
            model.branch_expectations(rb, E)
        assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED
        # the context still works
        again = model.branch_expectations(batch, E)
        assert again.values.tobytes() == good.values.tobytes()
    finally:
        ctx.close()


def test_one_node_tree_is_answered_on_the_host(ra):
    import networkx as nx
    T = nx.Graph()
    T.add_node(0)
    ctx = open_context(ra, {})
    try:
        model = ra.device.TreeModel(T, 0, 3, ctx=ctx)
        batch = model.upload_sites([0], np.array([[1], [255]], dtype=np.uint8), kind='state')
        got = model.branch_expectations(batch, np.eye(3))
        assert got.values.shape == (2, 1, 1) and not got.values.any()
        assert got.edge_sums.shape == (1, 1) and not got.status.any()
        assert got.nodes == [0]
    finally:
        ctx.close()
