"""rt_sites_branch_profiles (TreeModel.branch_profiles) on the GPU: per-site, per-branch
log-likelihood changes at a grid of trial lengths against a host reference that no device path
enters (tests/_profile_cases.py: scipy expm per trial length, the oracle's pruning), the
resident length, the library's own set_rates + step path, spectral rates, the slope against
branch_length_gradient, zero-length resident edges, side effects, determinism and the
documented errors."""
import ctypes

import numpy as np
import pytest

from oracle import oracle_numpy as orc
from _branch_cases import branch_reference
from _profile_cases import make_grid, profile_reference, site_bounds
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


def build(ra, ctx, case, weights=None, t=None):
    model = ra.device.TreeModel(case.T, case.root, case.n, ctx=ctx)
    model.set_rates(Q=case.Qs, node_q=case.node_q, t=t)
    model.set_root_distn(case.root_distn)
    batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


def check_profile(got, want, wstatus, loglik, weights, label, rows=None, tol=1e-10):
    """|got - want| <= tol max(1, |log L_i|) per site, tol max(1, sum_i w_i |log L_i|) for the
    sums (site_bounds), on the given rows (all by default); the worst gaps are printed in units
    of the bound's scale."""
    per_site, sum_bound = site_bounds(loglik, weights, tol)
    N = want.shape[1]
    rows = list(range(N)) if rows is None else rows
    np.testing.assert_array_equal(got.status, wstatus)
    w = np.ones(len(loglik)) if weights is None else weights
    live = wstatus == 0
    want_sums = np.einsum('i,ivg->vg', w[live], want[live])
    assert np.isfinite(want[:, rows]).all()
    gap = np.abs(got.values[:, rows] - want[:, rows]) / (per_site / tol)[:, None, None]
    sgap = np.abs(got.sums[rows] - want_sums[rows]) / (sum_bound / tol)
    print('%s: worst per-site gap %.2e, worst sum gap %.2e (units of max(1, |log L|); bound %.0e)'
          % (label, gap.max(), sgap.max(), tol))
    assert gap.max() <= tol
    assert sgap.max() <= tol


# ---- 1. against the host reference ---------------------------------------------------------

# the shapes of test_branch_expect_gpu.py's REFERENCE_CASES: both layouts (n <= 4: a lane per
# site), one to eight row tiles, every observation kind, the interpreter and the tree-specialised
# pruning kernel, weights, site counts that are no multiple of 16 or 64; per-edge rate matrices,
# internal observed nodes and a zero-likelihood site (the last) in every case.  The grid points
# cycle over 1, 3, 8, 9 (8: one whole chunk of the downward kernel, 9: a chunk and one) and are
# 64 once
REFERENCE_CASES = [
    # n, kind, sites, tree nodes, jit, weights, grid points
    (2, 'state', 70, 9, 0, False, 1),
    (3, 'mask', 130, 10, 1, True, 3),
    (4, 'dense', 67, 8, 0, True, 8),
    (5, 'dense', 21, 9, 0, False, 64),
    (8, 'state', 37, 10, 1, True, 9),
    (20, 'mask', 50, 11, 0, False, 1),
    (61, 'state', 33, 12, 1, True, 3),
    (64, 'dense', 19, 9, 0, False, 8),
    (65, 'state', 17, 9, 0, True, 9),
    (97, 'mask', 50, 10, 1, False, 1),
    (122, 'mask', 45, 9, 1, False, 3),
    (128, 'dense', 19, 8, 0, True, 8),
]


@pytest.mark.parametrize('n,kind,nsites,nnodes,jit,weighted,npoints', REFERENCE_CASES,
                         ids=['n%d-%s-jit%d-g%d' % (c[0], c[1], c[4], c[6])
                              for c in REFERENCE_CASES])
def test_against_the_host_reference(ra, n, kind, nsites, nnodes, jit, weighted, npoints):
    """Worst gap measured on the MI355X over these cases: 2.1e-15 of max(1, |log L|) per site
    (n = 128) and 1.7e-15 for the sums, against the bound 1e-10."""
    seed = 8000 + n
    case = make_case(n, nnodes, nsites, kind, seed, internal=True, per_edge=True)
    assert case.zero_site == nsites - 1
    weights = None
    if weighted:
        weights = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(np.float64)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        t = model.branch_lengths()
        assert np.array_equal(t[1:], model.tree.branch_lengths()[1:]) and t[0] == 0.0
        grid, factors = make_grid(t, npoints, seed)
        got = model.branch_profiles(batch, lengths=grid, per_site=True,
                                    recompute_transitions=True)
        want, wstatus, loglik = profile_reference(model, case, grid)
        N = model.tree.nnodes
        assert got.nodes == list(model.tree.preorder_nodes)
        assert got.values.shape == (nsites, N, npoints) and got.sums.shape == (N, npoints)
        assert got.lengths.tobytes() == grid.tobytes()
        assert wstatus[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB and wstatus.sum() == 1
        assert not got.values[:, 0].any() and not got.values[case.zero_site].any()
        assert not got.sums[0].any()
        check_profile(got, want, wstatus, loglik, weights, 'n=%d %s G=%d' % (n, kind, npoints))
        # the same grid as factors of the resident lengths
        again = model.branch_profiles(batch, factors=factors, per_site=True)
        assert again.lengths.tobytes() == grid.tobytes()
        assert again.values.tobytes() == got.values.tobytes()
        assert again.sums.tobytes() == got.sums.tobytes()
    finally:
        ctx.close()


# ---- 2. the resident length gives zero -----------------------------------------------------

@pytest.mark.parametrize('n,kind,nsites,jit', [(3, 'state', 75, 1), (20, 'dense', 23, 0),
                                               (61, 'mask', 30, 1), (122, 'state', 18, 0)])
def test_the_resident_length_gives_zero(ra, n, kind, nsites, jit):
    """At tau = t_v the ratio is sum_a D_p[a] = 1 to rounding: |value| <= 1e-12 at every live
    site (a few ulps of 1 from the n-term sums and the rebuilt exponential)."""
    case = make_case(n, 10, nsites, kind, 8100 + n, internal=True, per_edge=True)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case)
        got = model.branch_profiles(batch, factors=[1.0], per_site=True)
        live = got.status == 0
        assert live.sum() == nsites - 1
        print('n=%d: max |value| at the resident length %.2e' % (n, np.abs(got.values).max()))
        assert np.abs(got.values[live]).max() <= 1e-12
        assert not got.values[~live].any()
        assert np.abs(got.sums).max() <= 1e-12 * live.sum()
    finally:
        ctx.close()


# ---- 3. against the library's own likelihood path ------------------------------------------

@pytest.mark.parametrize('n,kind,nsites', [(4, 'state', 77), (61, 'state', 21)])
def test_against_set_rates_and_step(ra, n, kind, nsites):
    """For every (branch, point): set_rates with that one length changed, step, fetch; the
    per-site difference of the log-likelihoods at the tolerance of the reference test.  Then the
    first rates again: the first log-likelihoods bit for bit."""
    case = make_case(n, 9, nsites, kind, 8200 + n, internal=True, per_edge=True)
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        t0 = model.branch_lengths()
        ll0, st0 = model.log_likelihoods(batch)
        grid, _ = make_grid(t0, 3, 8200 + n)
        got = model.branch_profiles(batch, lengths=grid, per_site=True)
        np.testing.assert_array_equal(got.status, st0)
        live = st0 == 0
        per_site, _ = site_bounds(np.where(live, ll0, 0.0))
        worst = 0.0
        for v in range(1, model.tree.nnodes):
            for g in range(3):
                t = t0.copy()
                t[v] = grid[v, g]
                model.set_rates(Q=case.Qs, node_q=case.node_q, t=t)
                model.step(batch)
                ll, st = model.fetch_log_likelihoods(batch)
                assert np.array_equal(st, st0)
                gap = np.abs(got.values[live, v, g] - (ll[live] - ll0[live])) / per_site[live]
                worst = max(worst, gap.max())
        print('n=%d: worst gap to set_rates + step %.2e of the bound' % (n, worst))
        assert worst <= 1.0
        model.set_rates(Q=case.Qs, node_q=case.node_q, t=t0)
        model.step(batch)
        ll1, st1 = model.fetch_log_likelihoods(batch)
        assert ll1.tobytes() == ll0.tobytes() and st1.tobytes() == st0.tobytes()
    finally:
        ctx.close()


# ---- 4. spectral rates ---------------------------------------------------------------------

def test_spectral_rates(ra):
    """n = 20, one reversible rate matrix through raoteh_amd._spectral: P(tau) is rebuilt by
    rt_launch_spectral.  Same host reference (scipy expm of Q = A diag(lam) B); the tolerance is
    the one test_gpu_parity.test_spectral_reconstruction_matches_the_reference_qtop holds
    log-likelihoods from the spectral path to against those from expm: rtol = 1e-5 of
    |log L_i| (the spectral form holds entries of P absolutely, not relatively)."""
    from raoteh_amd import _spectral
    n, nsites, seed = 20, 35, 8300
    case = make_case(n, 10, nsites, 'state', seed, internal=False, per_edge=False)
    assert case.zero_site is None
    rng = np.random.RandomState(seed)
    pi = rng.uniform(0.5, 1.5, n)
    pi /= pi.sum()
    S = rng.uniform(0.2, 1.0, (n, n))
    S = 0.5 * (S + S.T)
    Q = S * pi[None, :]
    np.fill_diagonal(Q, 0.0)
    Q -= np.diag(Q.sum(axis=1))
    A, lam, B, D = _spectral.decompose_rate_matrix(Q, pi)
    case = case._replace(Qs=Q[None], node_q=np.zeros_like(case.node_q), root_distn=pi)
    weights = rng.randint(1, 4, size=nsites).astype(np.float64)
    ctx = open_context(ra, {})
    try:
        model = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        model.set_rates_spectral(A, lam, B, D=D)
        model.set_root_distn(pi)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        batch.set_weights(weights)
        t = model.branch_lengths()
        assert np.array_equal(t[1:], model.tree.branch_lengths()[1:])
        grid, factors = make_grid(t, 8, seed)
        before = model.get_transitions()
        got = model.branch_profiles(batch, factors=factors, per_site=True)
        assert got.lengths.tobytes() == grid.tobytes()
        assert model.get_transitions().tobytes() == before.tobytes()
        want, wstatus, loglik = profile_reference(model, case, grid)
        assert not wstatus.any()
        check_profile(got, want, wstatus, loglik, weights, 'n=20 spectral', tol=1e-5)
    finally:
        ctx.close()


# ---- 5. the slope --------------------------------------------------------------------------

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


@pytest.mark.parametrize('n,nsites', [(4, 150), (61, 60)])
def test_slope_is_the_branch_length_gradient(ra, n, nsites):
    """The central difference of `sums` at the factors 1 -+ 1e-5 against branch_length_gradient
    (analytic), with the bound of test_branch_expect_gpu.test_branch_length_gradient, for the
    same reason: finite differencing, not the device, dominates, so the bound is measured -- the
    same central difference (step 1e-5 t_v) of the ORACLE's total log-likelihood against the
    host reference's analytic value (tests/_branch_cases.py), times ten."""
    case = make_case(n, 10, nsites, 'state', 8400 + n, internal=False, per_edge=False)
    assert case.zero_site is None and len(case.Qs) == 1
    eps = 1e-5
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        ta = model.tree
        t0 = model.branch_lengths()
        N = ta.nnodes
        E = np.ones((n, n))
        np.fill_diagonal(E, np.diag(case.Qs[0]))
        values, _ = branch_reference(model, case, E[None])
        analytic = np.zeros(N)
        analytic[1:] = values[:, 1:, 0].sum(axis=0) / t0[1:]
        fd_oracle = np.zeros(N)
        for v in range(1, N):
            tp, tm = t0.copy(), t0.copy()
            tp[v] *= 1 + eps
            tm[v] *= 1 - eps
            fd_oracle[v] = (oracle_total(ta, case, tp) - oracle_total(ta, case, tm)) / (tp[v] - tm[v])
        bound = 10.0 * np.abs(fd_oracle - analytic).max()
        grad = model.branch_length_gradient(batch)
        got = model.branch_profiles(batch, factors=[1 + eps, 1 - eps])
        assert got.values is None
        fd = np.zeros(N)
        fd[1:] = (got.sums[1:, 0] - got.sums[1:, 1]) / (got.lengths[1:, 0] - got.lengths[1:, 1])
        print('n=%d: central difference of the profile vs branch_length_gradient: max gap %.2e '
              '(max |gradient| %.2e); bound %.2e' % (n, np.abs(fd - grad).max(),
                                                     np.abs(grad).max(), bound))
        assert np.abs(fd - grad).max() <= bound
    finally:
        ctx.close()


# ---- 6. zero-length resident edges ---------------------------------------------------------

def test_zero_length_resident_edges_give_nan_rows(ra):
    """n = 5, a leaf edge and an internal edge at t = 0: P = I there and the identity loses the
    states another length would reach -- NaN rows (values at live sites, sums); every other row
    against the reference."""
    n, nsites, seed = 5, 27, 8500
    case = make_case(n, 10, nsites, 'dense', seed, internal=False, per_edge=True)
    ctx = open_context(ra, {})
    try:
        probe = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        ta = probe.tree
        N = ta.nnodes
        inner = sorted(set(int(p) for p in ta.parent[1:]) - {0})
        leaves = sorted(set(range(1, N)) - set(int(p) for p in ta.parent[1:]))
        assert inner and leaves
        dead = [leaves[0], inner[0]]
        t = ta.branch_lengths().copy()
        t[dead] = 0.0
        model, batch = build(ra, ctx, case, t=t)
        assert np.array_equal(model.branch_lengths()[1:], t[1:])
        grid, _ = make_grid(t, 3, seed)
        grid[dead] = [0.1, 0.0, 0.7]
        got = model.branch_profiles(batch, lengths=grid, per_site=True)
        want, wstatus, loglik = profile_reference(model, case, grid)
        live = wstatus == 0
        assert live.sum() >= nsites - 1
        assert np.isnan(got.values[live][:, dead]).all() and np.isnan(got.sums[dead]).all()
        assert not got.values[~live].any()
        rows = [v for v in range(N) if v not in dead]
        check_profile(got, want, wstatus, loglik, None, 'n=5 zero-length edges', rows=rows)
    finally:
        ctx.close()


@pytest.mark.parametrize('n,nsites', [(4, 45), (20, 27)])
def test_a_trial_length_of_zero_gives_minus_infinity_where_the_endpoints_differ(ra, n, nsites):
    """tau = 0 on every branch: P(0) = I, so a site whose observed endpoints of the branch differ
    has likelihood 0 there -- the log of a ratio that is not positive is -inf, in the values and
    in the sums it enters; the other entries against the reference."""
    case = make_case(n, 9, nsites, 'state', 8550 + n, internal=True, per_edge=True)
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        N = model.tree.nnodes
        grid = np.zeros((N, 2))
        grid[:, 1] = model.branch_lengths()
        got = model.branch_profiles(batch, lengths=grid, per_site=True)
        want, wstatus, loglik = profile_reference(model, case, grid)
        np.testing.assert_array_equal(got.status, wstatus)
        lost = np.isneginf(want)
        assert lost.any() and not lost[:, :, 1].any() and not lost[wstatus != 0].any()
        assert np.isneginf(got.values[lost]).all()
        per_site, _ = site_bounds(loglik)
        gap = np.where(lost, 0.0, np.abs(got.values - np.where(lost, 0.0, want)))
        assert np.isfinite(gap).all() and (gap <= per_site[:, None, None]).all()
        rows = lost.any(axis=0)
        assert np.isneginf(got.sums[rows]).all() and np.isfinite(got.sums[~rows]).all()
        # a site of weight 0 adds nothing, whatever its value: with the sites that lose their
        # likelihood weighted 0, every sum is finite and the sum of the others
        w = np.where(lost[:, :, 0].any(axis=1), 0.0, 2.0)
        batch.set_weights(w)
        zeroed = model.branch_profiles(batch, lengths=grid)
        assert np.isfinite(zeroed.sums).all()
        keep = w > 0
        want_sums = 2.0 * want[keep].sum(axis=0)
        assert np.abs(zeroed.sums - want_sums).max() <= 2.0 * per_site[keep].sum()
    finally:
        ctx.close()


# ---- 7. side effects and determinism -------------------------------------------------------

@pytest.mark.parametrize('n,kind,nsites,jit', [(4, 'state', 131, 1), (20, 'dense', 37, 1),
                                               (97, 'mask', 29, 0)])
def test_side_effects_and_determinism(ra, n, kind, nsites, jit):
    case = make_case(n, 10, nsites, kind, 8600 + n, internal=True, per_edge=True)
    weights = np.random.RandomState(n).uniform(0.5, 2.0, size=nsites)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        ll, st = model.log_likelihoods(batch)
        totals = model.fetch_totals(batch)
        name = batch.kernel_name
        esd = model.get_transitions()
        grid, _ = make_grid(model.branch_lengths(), 5, 8600 + n)
        a = model.branch_profiles(batch, lengths=grid, per_site=True)
        b = model.branch_profiles(batch, lengths=grid, per_site=True)
        for x, y in ((a.values, b.values), (a.sums, b.sums), (a.status, b.status)):
            assert x.tobytes() == y.tobytes()
        sums_only = model.branch_profiles(batch, lengths=grid)
        assert sums_only.values is None
        assert sums_only.sums.tobytes() == a.sums.tobytes()
        assert sums_only.status.tobytes() == a.status.tobytes()
        # the raw call without sums, and without anything but the return code
        N = model.tree.nnodes
        vals = np.full((nsites, N, 5), np.nan)
        status = np.full(nsites, -1, dtype=np.int32)
        p_f64 = ctypes.POINTER(ctypes.c_double)
        rc = ra.lib.lib().rt_sites_branch_profiles(
            model._h, batch._h, 0, 5, grid.ctypes.data_as(p_f64), vals.ctypes.data_as(p_f64),
            None, status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert rc == ra.lib.RT_OK
        assert vals.tobytes() == a.values.tobytes() and status.tobytes() == a.status.tobytes()
        rc = ra.lib.lib().rt_sites_branch_profiles(
            model._h, batch._h, 0, 5, grid.ctypes.data_as(p_f64), None, None, None)
        assert rc == ra.lib.RT_OK
        # one point alone gives the bits it gives among others
        one = model.branch_profiles(batch, lengths=grid[:, 3:4], per_site=True)
        assert one.values[:, :, 0].tobytes() == np.ascontiguousarray(a.values[:, :, 3]).tobytes()
        # the model and the batch are as they were
        assert model.get_transitions().tobytes() == esd.tobytes()
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert model.fetch_totals(batch).tobytes() == totals.tobytes()
        assert batch.kernel_name == name
        ll3, st3 = model.log_likelihoods(batch)
        assert ll3.tobytes() == ll.tobytes() and st3.tobytes() == st.tobytes()
    finally:
        ctx.close()


# ---- 8. errors ------------------------------------------------------------------------------

def test_documented_errors(ra):
    n = 20
    case = make_case(n, 9, 25, 'state', 8700, internal=False, per_edge=False)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    ctx = open_context(ra, {})
    try:
        model, batch = build(ra, ctx, case)
        N = model.tree.nnodes
        ll, st = model.log_likelihoods(batch)
        name = batch.kernel_name
        factors = [0.5, 1.0, 2.0]
        good = model.branch_profiles(batch, factors=factors, per_site=True)

        def raw(npoints, lengths, m=model, b=batch):
            sums = np.zeros((N, max(int(npoints), 1)))
            return ra.lib.lib().rt_sites_branch_profiles(
                m._h, b._h, 0, npoints, None if lengths is None else lengths.ctypes.data_as(p_f64),
                None, sums.ctypes.data_as(p_f64), None)

        # G = 65, G = 0 (the Python check comes first; the C ABI has its own)
        with pytest.raises(ValueError):
            model.branch_profiles(batch, lengths=np.ones((N, 65)))
        assert raw(65, np.ones((N, 65))) == ra.lib.RT_ERR_INVALID
        assert 'grid points' in ra.lib.last_error()
        assert raw(0, np.ones((N, 1))) == ra.lib.RT_ERR_INVALID
        assert raw(2, None) == ra.lib.RT_ERR_INVALID
        # a negative, a non-finite length
        with pytest.raises(ValueError):
            model.branch_profiles(batch, factors=[1.0, -0.5])
        for x in (-1e-9, np.nan, np.inf):
            bad = np.ones((N, 2))
            bad[N - 1, 1] = x
            assert raw(2, bad) == ra.lib.RT_ERR_INVALID
            assert 'negative or not finite' in ra.lib.last_error()
        # (the root's row is ignored)
        rootrow = np.ones((N, 2))
        rootrow[0] = [-1.0, np.nan]
        assert raw(2, rootrow) == ra.lib.RT_OK
        # a batch of another model
        other = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(other, case)
        with pytest.raises(ValueError, match='another model'):
            other.branch_profiles(batch, factors=factors)
        # transitions set directly: no rate matrix to exponentiate at another length
        direct = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        direct.set_transitions(model.get_transitions())
        direct.set_root_distn(case.root_distn)
        db = direct.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        with pytest.raises(ValueError, match='no rates have been set'):
            direct.branch_profiles(db, lengths=np.ones((N, 2)))
        with pytest.raises(ValueError, match='no rates have been set'):
            direct.branch_profiles(db, factors=factors)
        # ... and after the rates: the resident rates no longer describe the transitions, until
        # they are set again or the call recomputes the transitions from them
        stale = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(stale, case)
        stale.set_root_distn(case.root_distn)
        sb = stale.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        fresh = stale.branch_profiles(sb, factors=factors, per_site=True)
        assert fresh.values.tobytes() == good.values.tobytes()
        stale.set_transitions(0.5 * (model.get_transitions() + np.eye(n)[None]))
        with pytest.raises(ValueError, match='set directly after the rates'):
            stale.branch_profiles(sb, factors=factors)
        back = stale.branch_profiles(sb, factors=factors, per_site=True,
                                     recompute_transitions=True)
        assert back.values.tobytes() == good.values.tobytes()
        assert stale.branch_profiles(sb, factors=factors).sums.tobytes() == good.sums.tobytes()
        # a "rescale" batch, a batch of the generic kernel
        for option in ('rescale', 'force_generic'):
            ctx.set_option(option, 1)
            try:
                ob = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
            finally:
                ctx.set_option(option, 0)
            with pytest.raises(ra.lib.RaotehHipError) as err:
                model.branch_profiles(ob, factors=factors)
            assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED, option
        # the batch is as it was, the context still works
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert batch.kernel_name == name
        again = model.branch_profiles(batch, factors=factors, per_site=True)
        assert again.values.tobytes() == good.values.tobytes()
        assert again.sums.tobytes() == good.sums.tobytes()
    finally:
        ctx.close()
