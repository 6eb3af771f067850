"""rt_sites_branch_profiles_mixture and rt_sites_nni_scores_mixture (TreeModel.branch_profiles_mixture
/ nni_scores_mixture) on the GPU: the tree-search reads of an ordinary batch under a site-class
mixture over the model's rate sets, trial lengths as factors of every set's own lengths.  Every
output against the host reference that no device path enters (tests/_mixture_search_cases.py),
each also asked for alone; the revival case (a set dead on the resident tree, live on the moved
one); sets of weight zero; determinism; chunks of moves; the log-likelihood against step_multi +
mixture_log_likelihoods; equal sets against the single-set calls; side effects; NaN rows; the
documented refusals."""
import ctypes

import networkx as nx
import numpy as np
import pytest

import _mixture_cases as mc
import _mixture_search_cases as msc
import _step_multi_cases as smc
from _profile_cases import site_bounds

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
P_F64 = ctypes.POINTER(ctypes.c_double)
P_I32 = ctypes.POINTER(ctypes.c_int32)


@pytest.fixture(scope='module')
def ctx():
    from raoteh_amd import device
    c = device.Context(0)
    for k, v in DEFAULTS.items():
        c.set_option(k, v)
    yield c
    c.close()


def build(ctx, case, weights=None, sets=None):
    from raoteh_amd import device
    model, batch = smc.upload(device, ctx, case)
    sel = slice(None) if sets is None else list(sets)
    model.set_rate_sets(case.Q[sel], t=case.t[sel], node_q=case.node_q)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


def release(model, batch):
    batch.close()
    model.close()


def raw(model, batch, call, c, factors, npoints=None, want=('values', 'sums', 'loglik', 'status'),
        recompute=0):
    """The C entry point with exactly the outputs of `want`, the others NULL -> (code, dict)."""
    from raoteh_amd import _lib
    N, S = model.tree.nnodes, batch.nsites
    rows = N if call == 'profile' else len(model.nni_moves())
    G = (1 if factors is None else np.asarray(factors).shape[1]) if npoints is None else npoints
    out = {'values': np.full((S, rows, max(G, 1)), 7.0), 'sums': np.full((rows, max(G, 1)), 7.0),
           'loglik': np.full(S, 7.0), 'status': np.full(S, 7, dtype=np.int32)}
    fn = getattr(_lib.lib(), 'rt_sites_branch_profiles_mixture' if call == 'profile'
                 else 'rt_sites_nni_scores_mixture')
    cw = None if c is None else np.ascontiguousarray(c, dtype=np.float64)
    f = None if factors is None else np.ascontiguousarray(factors, dtype=np.float64)

    def ptr(name, typ):
        return out[name].ctypes.data_as(typ) if name in want else None
    code = fn(model._h, batch._h, recompute, None if cw is None else cw.ctypes.data_as(P_F64), G,
              None if f is None else f.ctypes.data_as(P_F64), ptr('values', P_F64),
              ptr('sums', P_F64), ptr('loglik', P_F64), ptr('status', P_I32))
    return code, dict((k, out[k]) for k in want)


def wrapped(model, batch, call, c, factors, **kw):
    if call == 'profile':
        return model.branch_profiles_mixture(batch, c, factors, **kw)
    return model.nni_scores_mixture(batch, c, factors, **kw)


def check_against(got_values, got_sums, got_loglik, got_status, ref, weights, label):
    """The status exactly; -inf / NaN exactly where the reference has them; elsewhere |got - want|
    <= 1e-10 max(1, |log Lambda_i|) per site and 1e-10 max(1, sum_i w_i |log Lambda_i|) for the
    sums (_profile_cases.site_bounds with the reference's log Lambda_i).  The worst gaps are
    printed in units of the bound's scale before anything is asserted."""
    dead = ref.status != 0
    ll = np.where(dead, 0.0, ref.loglik)
    per_site, sum_bound = site_bounds(ll, weights)
    vgap = sgap = lgap = 0.0
    if got_values is not None:
        fin = np.isfinite(ref.values)
        d = np.abs(np.where(fin, got_values, 0.0) - np.where(fin, ref.values, 0.0))
        vgap = (d / (per_site / 1e-10)[:, None, None]).max()
    if got_sums is not None:
        sfin = np.isfinite(ref.sums)
        sgap = (np.abs(np.where(sfin, got_sums, 0.0) - np.where(sfin, ref.sums, 0.0)).max()
                / (sum_bound / 1e-10))
    if got_loglik is not None:
        lgap = (np.abs(np.where(dead, 0.0, got_loglik) - ll) / (per_site / 1e-10)).max()
    print('%s: worst gap / scale: values %.2e, sums %.2e, loglik %.2e (bound 1e-10)'
          % (label, vgap, sgap, lgap))
    if got_status is not None:
        np.testing.assert_array_equal(got_status, ref.status)
    if got_values is not None:
        assert got_values.shape == ref.values.shape
        assert np.array_equal(np.isneginf(got_values), np.isneginf(ref.values))
        assert np.array_equal(np.isnan(got_values), np.isnan(ref.values))
        assert not np.isposinf(got_values).any()
        assert vgap <= 1e-10
    if got_sums is not None:
        assert got_sums.shape == ref.sums.shape
        assert np.array_equal(np.isneginf(got_sums), np.isneginf(ref.sums))
        assert np.array_equal(np.isnan(got_sums), np.isnan(ref.sums))
        assert sgap <= 1e-10
    if got_loglik is not None:
        assert np.array_equal(np.isneginf(got_loglik), dead)
        assert lgap <= 1e-10


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


# ---- 1. parity against the host reference, both calls ---------------------------------------

# n = 2, 4: the lane kernels; 83 sites: six 16-site tiles with the last partial for n > 4, two
# lane blocks of 64; 5 the smallest matrix-pipe size; 20, 61; 122 with K = 2 and G = 2.  The
# 8-leaf balanced tree and the 12-node non-binary tree; K = 3 with the zero set; dense, state and
# mask; 1, 3 and 9 points (9 crosses BP_CHUNK / NNI_CHUNK = 8), 0: the plain swap (NNI only);
# site weights with zeros.
CASES = [
    # n, tree, kind, K, npoints, weighted
    (2, 'random', 'state', 3, 3, True),
    (4, 'balanced', 'dense', 3, 9, False),
    (4, 'random', 'mask', 3, 1, True),
    (5, 'balanced', 'mask', 3, 9, True),
    (20, 'random', 'dense', 3, 3, False),
    (61, 'balanced', 'state', 3, 1, True),
    (61, 'random', 'dense', 3, 9, False),
    (122, 'balanced', 'state', 2, 2, False),
]
SWAPS = [(4, 'random', 'state', 3, 0, True), (20, 'balanced', 'mask', 3, 0, True)]


def case_id(c):
    return 'n%d-%s-%s-K%d-g%d%s' % (c[0], c[1], c[2], c[3], c[4], '-w' if c[5] else '')


def parity(ctx, call, n, tree, kind, K, npoints, weighted):
    seed = 8800 + 7 * n + npoints
    case, ta, c, f, w, ref = msc.cached_reference(call, n, tree, kind, K, seed, npoints, weighted)
    assert (ref.status != 0).any() == (kind == 'dense')      # (a site dead under every set)
    assert (ref.status == 0).sum() > 40
    model, batch = build(ctx, case, w)
    try:
        got = wrapped(model, batch, call, c, f, per_site=True)
        if call == 'nni':
            assert np.array_equal(got.moves, ref.moves) and len(ref.moves) > 0
        label = '%s %s' % (call, case_id((n, tree, kind, K, npoints, weighted)))
        check_against(got.values, got.sums, got.loglik, got.status, ref, w, label)
        assert (f is None and got.factors is None) or same_bits(got.factors, f)
        # each output asked for alone: the bits of the full call
        code, full = raw(model, batch, call, c, f)
        assert code == 0
        assert same_bits(full['values'], got.values) and same_bits(full['sums'], got.sums)
        for name in ('values', 'sums', 'loglik', 'status'):
            code, alone = raw(model, batch, call, c, f, want=(name,))
            assert code == 0, name
            assert same_bits(alone[name], full[name]), name
        # sums alone through the wrapper (per_site=False)
        lean = wrapped(model, batch, call, c, f)
        assert lean.values is None and same_bits(lean.sums, got.sums)
    finally:
        release(model, batch)


@pytest.mark.parametrize('case', CASES, ids=case_id)
def test_profiles_against_the_host_reference(ctx, case):
    parity(ctx, 'profile', *case)


@pytest.mark.parametrize('case', CASES + SWAPS, ids=case_id)
def test_nni_scores_against_the_host_reference(ctx, case):
    parity(ctx, 'nni', *case)


# ---- 2. the revival case --------------------------------------------------------------------

@pytest.mark.parametrize('n', [3, 5])
def test_a_set_dead_on_the_resident_tree_counts_after_the_move(ctx, n):
    """n = 3: the lane kernel; n = 5: the matrix-pipe kernel."""
    case, ta = msc.revival_case(n)
    c = np.array([0.6, 0.4])
    L, moved = msc.revival_likelihoods(case, ta)
    i = case.site
    assert L[0, i] == 0.0 and moved[0, i] > 0.0 and L[1, i] > 0.0
    for f in (None, msc.make_factors(ta.nnodes, 3, 11)):
        ref = msc.nni_reference(ta, case, c, f)
        j = [tuple(mv) for mv in ref.moves].index(case.move)
        model, batch = build(ctx, case)
        try:
            got = model.nni_scores_mixture(batch, c, f, per_site=True)
            print('revival n=%d G=%d: device %r reference %r' % (n, got.values.shape[2],
                                                                got.values[i, j], ref.values[i, j]))
            assert np.isfinite(got.values[i, j]).all()
            bound = 1e-10 * max(1.0, abs(ref.loglik[i]))
            assert np.abs(got.values[i, j] - ref.values[i, j]).max() <= bound
            check_against(got.values, got.sums, got.loglik, got.status, ref, None, 'revival')
        finally:
            release(model, batch)
    # without the one-way set's term the value would be another one
    alone = np.log(c[1] * moved[1, i]) - np.log(c[1] * L[1, i])
    ref = msc.nni_reference(ta, case, c)
    j = [tuple(mv) for mv in ref.moves].index(case.move)
    assert abs(ref.values[i, j, 0] - alone) > 1e-3


@pytest.mark.parametrize('n', [3, 5])
def test_a_move_no_set_allows_gives_minus_infinity(ctx, n):
    case, ta = msc.lost_case(n)
    c = np.array([0.5, 0.5])
    for f in (None, msc.make_factors(ta.nnodes, 3, 11)):
        ref = msc.nni_reference(ta, case, c, f)
        j = [tuple(mv) for mv in ref.moves].index(case.move)
        assert np.isneginf(ref.values[case.site, j]).all() and ref.status[case.site] == 0
        model, batch = build(ctx, case)
        try:
            got = model.nni_scores_mixture(batch, c, f, per_site=True)
            assert np.isneginf(got.values[case.site, j]).all() and np.isneginf(got.sums[j]).all()
            check_against(got.values, got.sums, got.loglik, got.status, ref, None, 'lost n=%d' % n)
        finally:
            release(model, batch)


# ---- 3. sets of weight zero; determinism ----------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_a_set_of_weight_zero_is_as_if_absent(ctx, n):
    case, ta = msc.cached_case(n, 'balanced', 'dense', 3, 8700 + n)
    f = msc.make_factors(ta.nnodes, 3, 5)
    w = msc.site_weights(msc.NSITES, 6)
    c3 = np.array([0.3, 0.0, 0.7])
    full_model, full_batch = build(ctx, case, w)
    part_model, part_batch = build(ctx, case, w, sets=(0, 2))
    try:
        for call in ('profile', 'nni'):
            a = wrapped(full_model, full_batch, call, c3, f, per_site=True)
            b = wrapped(part_model, part_batch, call, c3[[0, 2]], f, per_site=True)
            for name in ('values', 'sums', 'loglik', 'status'):
                assert same_bits(getattr(a, name), getattr(b, name)), (call, name)
            assert np.isfinite(a.loglik).any()
        a = full_model.nni_scores_mixture(full_batch, c3, per_site=True)
        b = part_model.nni_scores_mixture(part_batch, c3[[0, 2]], per_site=True)
        assert same_bits(a.values, b.values) and same_bits(a.sums, b.sums)
    finally:
        release(full_model, full_batch)
        release(part_model, part_batch)


@pytest.mark.parametrize('n', [4, 61])
def test_two_calls_give_the_same_bits(ctx, n):
    case, ta = msc.cached_case(n, 'random', 'state', 3, 8600 + n)
    f = msc.make_factors(ta.nnodes, 9, 5)
    c = msc.class_weights(3, 2)
    model, batch = build(ctx, case, msc.site_weights(msc.NSITES, 6))
    try:
        for call in ('profile', 'nni'):
            a = wrapped(model, batch, call, c, f, per_site=True)
            other = wrapped(model, batch, 'nni' if call == 'profile' else 'profile', c, f)
            b = wrapped(model, batch, call, c, f, per_site=True, recompute_transitions=True)
            for name in ('values', 'sums', 'loglik', 'status'):
                assert same_bits(getattr(a, name), getattr(b, name)), (call, name)
            assert other.sums.shape[1] == 9
    finally:
        release(model, batch)


# ---- 4. chunks of moves ---------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_chunks_of_moves_give_the_bits_of_one_chunk(ctx, n, monkeypatch):
    case, ta = msc.cached_case(n, 'random', 'dense', 3, 8500 + n)
    f = msc.make_factors(ta.nnodes, 3, 5)
    c = msc.class_weights(3, 2)
    model, batch = build(ctx, case, msc.site_weights(msc.NSITES, 6))
    try:
        M = len(model.nni_moves())
        assert M >= 6
        whole = model.nni_scores_mixture(batch, c, f, per_site=True)
        whole_sums = model.nni_scores_mixture(batch, c, f)
        per_move = 3 * msc.NSITES * 8
        for moves_per_chunk, per_site in ((1, True), (2, False), (M - 1, True)):
            monkeypatch.setenv('RAOTEH_NNI_CHUNK_BYTES',
                               str(moves_per_chunk * per_move * (2 if per_site else 1)))
            got = model.nni_scores_mixture(batch, c, f, per_site=per_site)
            monkeypatch.delenv('RAOTEH_NNI_CHUNK_BYTES')
            assert same_bits(got.sums, whole.sums) and same_bits(got.sums, whole_sums.sums)
            assert same_bits(got.loglik, whole.loglik) and same_bits(got.status, whole.status)
            if per_site:
                assert same_bits(got.values, whole.values)
    finally:
        release(model, batch)


# ---- 5. the mixture log-likelihood; equal sets ----------------------------------------------

@pytest.mark.parametrize('n', [4, 61])
def test_loglik_is_the_mixture_log_likelihood_of_step_multi(ctx, n):
    case, ta = msc.cached_case(n, 'balanced', 'dense', 3, 8400 + n)
    c = msc.class_weights(3, 2)
    model, batch = build(ctx, case)
    try:
        model.step_multi(batch)
        want, wst, _ = model.mixture_log_likelihoods(batch, c)
        dead = (wst & 1) != 0
        assert dead.any() and not dead.all()
        per_site, _ = site_bounds(np.where(dead, 0.0, want))
        for call in ('profile', 'nni'):
            got = wrapped(model, batch, call, c, [1.0])
            assert np.array_equal((got.status & 1) != 0, dead)
            assert np.array_equal(np.isneginf(got.loglik), dead)
            gap = np.abs(np.where(dead, 0.0, got.loglik) - np.where(dead, 0.0, want))
            print('%s n=%d: loglik gap / bound %.2e' % (call, n, (gap / per_site).max()))
            assert (gap <= per_site).all()
    finally:
        release(model, batch)


@pytest.mark.parametrize('n', [4, 20])
def test_equal_sets_give_the_single_set_calls(ctx, n):
    """All K sets equal to one rate set: branch_profiles / nni_scores of that rate set at the
    lengths factors * t, to the tolerance (bit equality is not required)."""
    from raoteh_amd import device
    case, ta = msc.cached_case(n, 'random', 'dense', 2, 8300 + n)
    f = msc.make_factors(ta.nnodes, 3, 5)
    c = msc.class_weights(3, 2)
    w = msc.site_weights(msc.NSITES, 6)
    model, batch = smc.upload(device, ctx, case)
    try:
        batch.set_weights(w)
        model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])
        model.set_rate_sets(np.stack([case.Q[0]] * 3), t=np.stack([case.t[0]] * 3), node_q=case.node_q)
        grid = f * case.t[0][:, None]
        ll, st = model.log_likelihoods(batch)
        dead = (st & 1) != 0
        per_site, sum_bound = site_bounds(np.where(dead, 0.0, ll), w)
        pairs = ((model.branch_profiles(batch, lengths=grid, per_site=True),
                  model.branch_profiles_mixture(batch, c, f, per_site=True)),
                 (model.nni_scores(batch, lengths=grid, per_site=True),
                  model.nni_scores_mixture(batch, c, f, per_site=True)),
                 (model.nni_scores(batch, per_site=True),
                  model.nni_scores_mixture(batch, c, per_site=True)))
        for one, mix in pairs:
            assert np.array_equal((mix.status & 1) != 0, dead)
            assert np.array_equal(np.isfinite(one.values), np.isfinite(mix.values))
            fin = np.isfinite(one.values)
            gap = np.abs(np.where(fin, mix.values, 0.0) - np.where(fin, one.values, 0.0))
            sgap = np.abs(mix.sums - one.sums)
            print('equal sets n=%d: values gap / bound %.2e, sums %.2e'
                  % (n, (gap / per_site[:, None, None]).max(), sgap.max() / sum_bound))
            assert (gap <= per_site[:, None, None]).all() and np.isfinite(one.sums).all()
            assert (sgap <= sum_bound).all()
            lgap = np.abs(np.where(dead, 0.0, mix.loglik) - np.where(dead, 0.0, ll))
            assert (lgap <= per_site).all()
    finally:
        release(model, batch)


# ---- 6. nothing resident changes ------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_nothing_resident_changes(ctx, n):
    from raoteh_amd import device
    case, ta = msc.cached_case(n, 'balanced', 'state', 3, 8200 + n)
    f = msc.make_factors(ta.nnodes, 3, 5)
    c = msc.class_weights(3, 2)
    model, batch = smc.upload(device, ctx, case)
    try:
        model.set_rates(Q=case.Q[1], node_q=case.node_q, t=case.t[1])
        model.step(batch)
        model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
        model.step_multi(batch)

        def snapshot():
            ll, st = model.fetch_log_likelihoods(batch)
            mll, mst = model.fetch_multi_log_likelihoods(batch)
            return [ll, st, model.fetch_totals(batch), mll, mst, model.get_transitions(),
                    np.array([ord(ch) for ch in batch.kernel_name])]
        before = snapshot()
        model.branch_profiles_mixture(batch, c, f, per_site=True)
        model.nni_scores_mixture(batch, c, f, per_site=True)
        model.nni_scores_mixture(batch, c)
        for a, b in zip(before, snapshot()):
            assert same_bits(np.asarray(a), np.asarray(b))
        # the rate sets too: step_multi without recomputing gives what it gave
        model.step_multi(batch, recompute_transitions=False)
        mll, mst = model.fetch_multi_log_likelihoods(batch)
        assert same_bits(mll, before[3]) and same_bits(mst, before[4])
    finally:
        release(model, batch)


# ---- 7. an edge of resident length zero -----------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_a_resident_length_of_zero(ctx, n):
    """t[k][v] == 0 under a set with c_k > 0: a NaN row in the profile call (values at live sites
    and sums), finite values against the reference in the NNI call; no NaN where c_k == 0."""
    base, ta = msc.cached_case(n, 'balanced', 'dense', 2, 8100 + n)
    t = base.t.copy()
    v = 1                                        # (an internal node with moves)
    t[1, v] = 0.0
    case = base._replace(t=t)
    f = msc.make_factors(ta.nnodes, 3, 5)
    c = np.array([0.4, 0.6])
    model, batch = build(ctx, case)
    try:
        got = model.branch_profiles_mixture(batch, c, f, per_site=True)
        live = got.status == 0
        assert live.any() and not live.all()
        assert np.isnan(got.values[live][:, v]).all() and np.isnan(got.sums[v]).all()
        assert (got.values[~live] == 0).all()
        others = np.delete(np.arange(ta.nnodes), v)
        assert not np.isnan(got.values[:, others]).any() and not np.isnan(got.sums[others]).any()
        check_against(got.values, got.sums, got.loglik, got.status,
                      msc.profile_reference(ta, case, c, f), None, 'zero length, profile')
        nni = model.nni_scores_mixture(batch, c, f, per_site=True)
        assert (nni.moves[:, 0] == v).any()
        assert not np.isnan(nni.values).any() and not np.isnan(nni.sums).any()
        check_against(nni.values, nni.sums, nni.loglik, nni.status,
                      msc.nni_reference(ta, case, c, f), None, 'zero length, nni')
        one = model.branch_profiles_mixture(batch, [1.0, 0.0], f, per_site=True)
        assert not np.isnan(one.values).any() and not np.isnan(one.sums).any()
    finally:
        release(model, batch)


# ---- 8. the documented refusals -------------------------------------------------------------

def test_documented_refusals(ctx):
    from raoteh_amd import device, synth, _lib
    import _partition_cases as pc
    INVALID, UNSUPPORTED, SINGULAR = _lib.RT_ERR_INVALID, _lib.RT_ERR_UNSUPPORTED, _lib.RT_ERR_SINGULAR
    case, ta = msc.cached_case(20, 'random', 'state', 2, 8000)
    N = ta.nnodes
    c = np.array([0.5, 0.5])
    ones = np.ones((N, 2))
    model, batch = build(ctx, case)
    other, other_batch = build(ctx, case)
    bare, bare_batch = smc.upload(device, ctx, case)
    try:
        moves = model.nni_moves()
        with_move = int(moves[0, 0])
        without = [v for v in range(1, N) if v not in set(moves[:, 0].tolist())]
        assert without
        for call in ('profile', 'nni'):
            def code(cw, f, npoints=None, m=model, b=batch):
                return raw(m, b, call, cw, f, npoints=npoints, want=('sums',))[0]
            assert code(c, ones) == 0
            # no rate sets
            assert code(c, ones, m=bare, b=bare_batch) == INVALID
            with pytest.raises(ValueError, match='set_rate_sets'):
                wrapped(bare, bare_batch, call, c, [1.0])
            # a batch of another model
            assert code(c, ones, m=model, b=other_batch) == INVALID
            with pytest.raises(ValueError, match='another model'):
                wrapped(model, other_batch, call, c, [1.0])
            # class weights: NULL, negative, not finite, all zero, another length
            assert code(None, ones) == INVALID
            for bad in ([0.5, -0.5], [0.5, np.nan], [np.inf, 0.5], [0.0, 0.0]):
                assert code(np.array(bad), ones) == INVALID, bad
                with pytest.raises(ValueError):
                    wrapped(model, batch, call, bad, [1.0])
            with pytest.raises(ValueError):
                wrapped(model, batch, call, [1.0], [1.0])
            # npoints out of range; factors NULL
            assert code(c, np.ones((N, 65))) == INVALID
            assert code(c, ones, npoints=0) == INVALID
            with pytest.raises(ValueError):
                wrapped(model, batch, call, c, np.ones((N, 65)))
            with pytest.raises(ValueError):
                wrapped(model, batch, call, c, [])
            if call == 'profile':
                assert code(c, None, npoints=1) == INVALID
            else:
                assert code(c, None, npoints=2) == INVALID
                assert code(c, None, npoints=0) == INVALID
                assert code(c, None, npoints=1) == 0
            # a negative, a non-finite factor in a row that counts
            for x in (-1e-9, np.nan, np.inf):
                bad = ones.copy()
                bad[with_move, 1] = x
                assert code(c, bad) == INVALID
                assert 'negative or not finite' in _lib.last_error()
                with pytest.raises(ValueError):
                    wrapped(model, batch, call, c, bad)
            ignored = ones.copy()
            ignored[0] = [-1.0, np.nan]
            assert code(c, ignored) == 0
            if call == 'nni':                    # (rows of nodes without a move do not count)
                ignored[without] = [-1.0, np.nan]
                assert code(c, ignored) == 0
            # a failed exponential
            huge = ones.copy()
            huge[with_move, 0] = 1e308
            assert code(c, huge) == SINGULAR
            # a "rescale" batch, a batch of the generic kernel
            for option in ('rescale', 'force_generic'):
                ctx.set_option(option, 1)
                try:
                    ob = model.upload_sites(case.leaves, case.data, kind=case.kind)
                finally:
                    ctx.set_option(option, 0)
                assert code(c, ones, b=ob) == UNSUPPORTED, option
                with pytest.raises(_lib.RaotehHipError) as err:
                    wrapped(model, ob, call, c, [1.0])
                assert err.value.code == UNSUPPORTED, option
                ob.close()
        # a partitioned batch
        pcase = pc.make_case(20, 'dense', seed=6)
        pmodel, pbatch = pc.upload(device, ctx, pcase)
        pmodel.set_rate_sets(pcase.Q, t=pcase.t, node_q=pcase.node_q)
        pc_w = np.full(pcase.Q.shape[0], 1.0 / pcase.Q.shape[0])
        for call in ('profile', 'nni'):
            pf = np.ones((pmodel.tree.nnodes, 1))
            assert raw(pmodel, pbatch, call, pc_w, pf, want=('status',))[0] == UNSUPPORTED
            assert 'partitioned' in _lib.last_error()
            with pytest.raises(ValueError, match='ordinary'):
                wrapped(pmodel, pbatch, call, pc_w, [1.0])
        release(pmodel, pbatch)
        # a tree of one node; a tree deeper than the fast kernels take
        lone = nx.Graph()
        lone.add_node('r')
        single = device.TreeModel(lone, 'r', 20, ctx=ctx)
        single.set_rate_sets(case.Q[:1, 0], t=np.zeros((1, 1)))
        sb = single.upload_sites(['r'], np.ones((3, 1), dtype=np.uint8), kind='state')
        T9, root9, leaves9 = synth.balanced_tree(512, seed=0)
        deep = device.TreeModel(T9, root9, 122, ctx=ctx)
        assert deep.schedule_depth >= 9
        deep.set_rate_sets(smc.random_rates(122, np.random.RandomState(1))[None])
        db = deep.upload_sites(leaves9, np.ones((2, len(leaves9), 122)), kind='dense')
        for call in ('profile', 'nni'):
            for m, b in ((single, sb), (deep, db)):
                with pytest.raises(_lib.RaotehHipError) as err:
                    wrapped(m, b, call, [1.0], [1.0])
                assert err.value.code == UNSUPPORTED
        release(single, sb)
        release(deep, db)
        # more than 96 GB of scratch: refused before anything is reserved
        wide_model = device.TreeModel(T9, root9, 20, ctx=ctx)
        wide_model.set_rate_sets(smc.random_rates(20, np.random.RandomState(1))[None])
        wb = wide_model.upload_sites(leaves9, np.zeros((100000, len(leaves9)), dtype=np.uint8),
                                     kind='state')
        with pytest.raises(_lib.RaotehHipError) as err:
            wide_model.branch_profiles_mixture(wb, [1.0], np.ones(64))
        assert err.value.code == UNSUPPORTED and 'GB' in str(err.value)
        release(wide_model, wb)
        # the batch is as it was, the context still works
        again = model.nni_scores_mixture(batch, c, ones)
        assert np.isfinite(again.sums).all()
    finally:
        release(model, batch)
        release(other, other_batch)
        release(bare, bare_batch)
