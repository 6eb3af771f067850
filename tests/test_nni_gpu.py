"""rt_sites_nni_scores (TreeModel.nni_scores) on the GPU: the change of the per-site
log-likelihood for every nearest-neighbour interchange of the tree, with the edge above v at its
resident matrix or at a grid of trial lengths, against a host reference that no device path enters
(tests/_nni_cases.py: the rearranged arrays built by hand, scipy expm per trial length, the
oracle's pruning); the states where a division by the messages would lose the answer, -inf and
zero sites, zero-length resident edges, the library's own model build + step on the moved tree,
side effects and determinism, spectral rates, chunks of moves and the documented refusals."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from oracle import oracle_numpy as orc
from _nni_cases import brute_moves, move_terms, nni_reference, up_pass
from _profile_cases import make_grid, site_bounds
from _resident_cases import _encode, make_case, set_rates

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
FACTORS = (1.0, 0.5, 1.75)


@pytest.fixture(scope='module')
def ra():
    from raoteh_amd import device, _lib, _tree

    class NS(object):
        pass
    ns = NS()
    ns.device, ns.lib, ns.tree = device, _lib, _tree
    return ns


def open_context(ra, opts=None):
    ctx = ra.device.Context(0)
    for k, v in dict(DEFAULTS, **(opts or {})).items():
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


def some_weights(nsites, seed):
    """1, 2 or 3 per site, and one site of weight 0 (not the last, the zero-likelihood one)."""
    w = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(np.float64)
    w[nsites // 2] = 0.0
    return w


def check_scores(got, want_moves, want, wstatus, loglik, weights, label, tol=1e-10):
    """The moves and the status exactly; -inf exactly where the reference has it; elsewhere
    |got - want| <= tol max(1, |log L_i|) per site and tol max(1, sum_i w_i |log L_i|) for the
    sums (site_bounds).  The worst gaps are printed in units of the bound's scale."""
    per_site, sum_bound = site_bounds(loglik, weights, tol)
    assert got.moves.dtype == np.int32 and np.array_equal(got.moves, want_moves)
    np.testing.assert_array_equal(got.status, wstatus)
    S, M, G = want.shape
    assert got.values.shape == (S, M, G) and got.sums.shape == (M, G)
    assert not np.isnan(got.values).any() and not np.isnan(got.sums).any()
    lost = np.isneginf(want)
    assert np.array_equal(np.isneginf(got.values), lost)
    gap = np.abs(np.where(lost, 0.0, got.values) - np.where(lost, 0.0, want))
    gap = gap / (per_site / tol)[:, None, None]
    w = np.ones(S) if weights is None else weights
    use = (wstatus == 0) & (w != 0)
    want_sums = np.einsum('i,img->mg', w[use], np.where(lost, 0.0, want)[use])
    slost = lost[use].any(axis=0)
    assert np.array_equal(np.isneginf(got.sums), slost)
    sgap = np.abs(np.where(slost, 0.0, got.sums - want_sums)) / (sum_bound / tol)
    print('%s: %d moves, worst per-site gap %.2e, worst sum gap %.2e (units of max(1, |log L|); '
          'bound %.0e)' % (label, M, gap.max() if gap.size else 0.0,
                           sgap.max() if sgap.size else 0.0, tol))
    assert not gap.size or gap.max() <= tol
    assert not sgap.size or sgap.max() <= tol
    return gap


# ---- 1. against the host reference: the plain swap and a 3-point grid ------------------------

PARITY_CASES = ([(n, kind, 70) for n in (2, 4) for kind in ('state', 'mask', 'dense')] +
                [(n, kind, 37) for n in (5, 20, 61, 64) for kind in ('state', 'mask', 'dense')] +
                [(n, kind, 37) for n in (65, 122) for kind in ('mask', 'dense')])


@pytest.mark.parametrize('n,kind,nsites', PARITY_CASES,
                         ids=['n%d-%s' % c[:2] for c in PARITY_CASES])
def test_against_the_host_reference(ra, n, kind, nsites):
    """12-node trees with multifurcations and single-child nodes, per-edge rate matrices that
    never enter state 0, observed internal nodes, a zero-likelihood site (the last) and weights
    with a zero.  Worst gaps measured on the MI355X over these cases: 4.9e-15 of max(1, |log L|)
    per site (n = 20) and 8.2e-16 for the sums (n = 65), against the bound 1e-10."""
    seed = 9000 + n
    case = make_case(n, 12, nsites, kind, seed, internal=True, per_edge=True)
    assert case.zero_site == nsites - 1
    weights = some_weights(nsites, seed)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, weights)
        moves = model.nni_moves()
        assert np.array_equal(moves, brute_moves(model.tree.indices, model.tree.indptr))
        assert len(moves) >= 4
        label = 'n=%d %s' % (n, kind)
        # the plain swap
        got = model.nni_scores(batch, per_site=True)
        wmoves, want, wstatus, loglik = nni_reference(model, case)
        assert wstatus[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB and wstatus.sum() == 1
        assert not got.values[case.zero_site].any()
        check_scores(got, wmoves, want, wstatus, loglik, weights, label + ' swap')
        assert np.array_equal(got.lengths[:, 0], model.branch_lengths())
        # the grid: the factors 1, 0.5, 1.75 of every resident length, in make_grid's order
        grid, factors = make_grid(model.branch_lengths(), 3, seed)
        assert sorted(factors) == sorted(FACTORS)
        gg = model.nni_scores(batch, lengths=grid, per_site=True)
        assert gg.lengths.tobytes() == grid.tobytes()
        _, gwant, gstatus, _ = nni_reference(model, case, grid)
        check_scores(gg, wmoves, gwant, gstatus, loglik, weights, label + ' grid')
        again = model.nni_scores(batch, factors=factors, per_site=True)
        assert again.values.tobytes() == gg.values.tobytes()
        assert again.sums.tobytes() == gg.sums.tobytes()
        # the column of factor 1 is the plain swap, to the same tolerance
        one = int(np.nonzero(factors == 1.0)[0][0])
        col = gg._replace(values=gg.values[:, :, one:one + 1], sums=gg.sums[:, one:one + 1])
        check_scores(col, wmoves, want, wstatus, loglik, weights, label + ' factor 1')
    finally:
        ctx.close()


# ---- 2. where a division by the messages would lose the answer ------------------------------

def leaves_beside_an_internal_node(ta):
    kids = np.diff(ta.indptr)
    out = []
    for v in range(1, ta.nnodes):
        p = ta.parent[v]
        beside = [int(w) for w in ta.indices[ta.indptr[p]:ta.indptr[p + 1]] if w != v]
        if kids[v] == 0 and any(kids[w] > 0 for w in beside):
            out.append(v)
    return out


@pytest.mark.parametrize('n,nsites,seed', [(4, 70, 9304), (20, 37, 9320)])
def test_states_the_division_shortcut_would_lose(ra, n, nsites, seed):
    """Mask data, and length 0 on the edges above the leaves that have an internal sibling:
    M_s = P_s L_s is then the leaf's mask itself, so the posterior D_p is 0 at every state a the
    mask of s excludes, and D_p M_c / (M_v M_s) is 0 / 0 there -- yet once s hangs below v the
    state a of p is live again (the term W[a] M_c[a] (P_v L'_v)[a] is positive).  The test finds
    those (site, move) pairs on the host and holds the device to the reference at them."""
    case = make_case(n, 12, nsites, 'mask', seed, internal=True, per_edge=True)
    ctx = open_context(ra)
    try:
        ta = ra.device.TreeModel(case.T, case.root, n, ctx=ctx).tree
        dead = leaves_beside_an_internal_node(ta)
        assert dead
        t = ta.branch_lengths().copy()
        t[dead] = 0.0
        model, batch = build(ra, ctx, case, t=t)
        esd = model.get_transitions()
        for v in dead:
            assert np.array_equal(esd[v], np.eye(n))
        got = model.nni_scores(batch, per_site=True)
        wmoves, want, wstatus, loglik = nni_reference(model, case)
        cols = [ta.node_to_index[v] for v in case.obs_nodes]
        obs, _, M, up = up_pass(ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn)
        hit = np.zeros(want.shape[:2], dtype=bool)
        for k, mv in enumerate(wmoves):
            x, lp, zero_den = move_terms(ta.indices, ta.indptr, obs, M, up, mv)
            term = x * (lp @ esd[mv[0]].T)                   # the moved tree's term per state of p
            hit[:, k] = (zero_den & (term > 0)).any(axis=1) & (wstatus == 0)
        print('n=%d: %d (site, move) pairs with a live state over M_v M_s = 0' % (n, hit.sum()))
        assert hit.sum() >= 1
        gap = check_scores(got, wmoves, want, wstatus, loglik, None, 'n=%d zero-length leaves' % n)
        assert np.isfinite(want[hit]).all() and np.isfinite(got.values[:, :, 0][hit]).all()
        assert gap[:, :, 0][hit].max() <= 1e-10
    finally:
        ctx.close()


# ---- 3. -inf and zero sites ------------------------------------------------------------------

def minus_infinity_case(n, nsites, seed):
    """make_case (mask), with site 0 rewritten: an observed internal node v in state 1 whose
    sibling leaf s is in state 0, every observed node from the parent of v up to the root left
    free -- the root, ..., p are in state 0 (nothing enters state 0), so the site is live; after
    a move that puts s below v, P_s[1][0] = 0 and the likelihood is 0.  -> (case, v, s) labels."""
    from raoteh_amd import _tree
    for sd in range(seed, seed + 50):
        case = make_case(n, 12, nsites, 'mask', sd, internal=True, per_edge=True)
        ta = _tree.TreeArrays(case.T, case.root)
        kids = np.diff(ta.indptr)
        idx = ta.node_to_index
        observed = set(idx[x] for x in case.obs_nodes)
        for v in range(1, ta.nnodes):
            p = int(ta.parent[v])
            beside = [int(w) for w in ta.indices[ta.indptr[p]:ta.indptr[p + 1]]
                      if w != v and kids[w] == 0 and w in observed]
            if kids[v] == 0 or v not in observed or not beside:
                continue
            s = beside[0]
            lik = case.obs_lik.copy()
            col = dict((idx[x], k) for k, x in enumerate(case.obs_nodes))
            lik[0, col[v]] = np.eye(n)[1]
            lik[0, col[s]] = np.eye(n)[0]
            a = p
            while a >= 0:
                if a in col:
                    lik[0, col[a]] = 1.0
                a = int(ta.parent[a])
            case = case._replace(obs_lik=lik, data=_encode('mask', n, lik))
            return case, ta.preorder_nodes[v], ta.preorder_nodes[s]
    raise AssertionError('no tree with an observed internal node beside an observed leaf')


@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37)])
def test_minus_infinity_and_zero_sites(ra, n, nsites):
    case, v_label, s_label = minus_infinity_case(n, nsites, 9400 + n)
    assert case.zero_site == nsites - 1
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        ta = model.tree
        v, s = ta.node_to_index[v_label], ta.node_to_index[s_label]
        got = model.nni_scores(batch, per_site=True)
        wmoves, want, wstatus, loglik = nni_reference(model, case)
        assert wstatus[0] == 0 and np.isfinite(loglik[0])            # site 0 is live
        below = np.nonzero((wmoves[:, 0] == v) & (wmoves[:, 2] == s))[0]
        assert len(below) == int(np.diff(ta.indptr)[v]) >= 1
        assert np.isneginf(want[0, below, 0]).all()
        assert np.isneginf(got.values[0, below, 0]).all()
        assert np.isneginf(got.sums[below, 0]).all()
        check_scores(got, wmoves, want, wstatus, loglik, None, 'n=%d -inf' % n)
        # the zero-likelihood site: its status, zeros
        assert got.status[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB
        assert got.status.sum() == ra.lib.RT_SITE_ZERO_PROB
        assert not got.values[case.zero_site].any()
        # every site with a -inf at weight 0: nothing of it in the sums
        w = np.where(np.isneginf(want).any(axis=(1, 2)), 0.0, 2.0)
        assert w[0] == 0.0
        batch.set_weights(w)
        zeroed = model.nni_scores(batch, per_site=True)
        assert np.isfinite(zeroed.sums).all()
        assert zeroed.values.tobytes() == got.values.tobytes()
        check_scores(zeroed, wmoves, want, wstatus, loglik, w, 'n=%d -inf at weight 0' % n)
    finally:
        ctx.close()


# ---- 4. a resident length of zero ------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(3, 70), (20, 37)])
def test_a_resident_length_of_zero_is_nothing_special(ra, n, nsites):
    """t_v = 0 on an internal edge with moves: P_v = I.  The plain swap and a grid (two positive
    lengths and 0 for that edge) against the reference: finite where the reference is, no NaN."""
    seed = 9500 + n
    case = make_case(n, 12, nsites, 'dense', seed, internal=True, per_edge=True)
    ctx = open_context(ra)
    try:
        ta = ra.device.TreeModel(case.T, case.root, n, ctx=ctx).tree
        moves = brute_moves(ta.indices, ta.indptr)
        v = int(moves[len(moves) // 2, 0])
        t = ta.branch_lengths().copy()
        t[v] = 0.0
        model, batch = build(ra, ctx, case, t=t)
        assert model.branch_lengths()[v] == 0.0
        assert np.array_equal(model.get_transitions()[v], np.eye(n))
        got = model.nni_scores(batch, per_site=True)
        wmoves, want, wstatus, loglik = nni_reference(model, case)
        about = wmoves[:, 0] == v
        assert about.any() and np.isfinite(want[wstatus == 0][:, about]).any()
        check_scores(got, wmoves, want, wstatus, loglik, None, 'n=%d t_v = 0, swap' % n)
        grid, _ = make_grid(t, 3, seed)
        grid[v] = [0.1, 0.0, 0.7]
        gg = model.nni_scores(batch, lengths=grid, per_site=True)
        _, gwant, _, _ = nni_reference(model, case, grid)
        check_scores(gg, wmoves, gwant, wstatus, loglik, None, 'n=%d t_v = 0, grid' % n)
    finally:
        ctx.close()


# ---- 5. against the library's own path on the moved tree ------------------------------------

def test_against_a_fresh_model_of_the_moved_tree(ra):
    """n = 20: for two moves, nni_apply, a fresh TreeModel of the rearranged tree (every node
    keeps the rate matrix and the length of the edge above it), upload, step: the difference of
    the weighted totals is sums[mv], to the sums' tolerance."""
    n, nsites, seed = 20, 37, 9600
    case = make_case(n, 12, nsites, 'state', seed, internal=True, per_edge=True)
    weights = some_weights(nsites, seed)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, weights)
        ta = model.tree
        ll0, st0 = model.log_likelihoods(batch)
        live = (st0 == 0) & (weights != 0)
        got = model.nni_scores(batch)
        assert got.values is None
        _, sum_bound = site_bounds(np.where(st0 == 0, ll0, 0.0), weights)
        q_of = dict((ta.preorder_nodes[i], int(case.node_q[i])) for i in range(ta.nnodes))
        for k in (0, len(got.moves) - 1):
            v, c, s = (ta.preorder_nodes[int(x)] for x in got.moves[k])
            T2 = ra.tree.nni_apply(case.T, case.root, v, c, s)
            other = ra.device.TreeModel(T2, case.root, n, ctx=ctx)
            node_q = np.array([q_of[x] for x in other.tree.preorder_nodes], dtype=np.int64)
            other.set_rates(Q=case.Qs, node_q=node_q)
            other.set_root_distn(case.root_distn)
            ob = other.upload_sites(case.obs_nodes, case.data, kind=case.kind)
            ll1, st1 = other.log_likelihoods(ob)
            assert np.array_equal(st1, st0)
            diff = float(np.sum(weights[live] * (ll1[live] - ll0[live])))
            print('move %s: sums %.12g, model build + step %.12g, gap %.2e (bound %.2e)'
                  % (got.moves[k].tolist(), got.sums[k, 0], diff, abs(got.sums[k, 0] - diff),
                     sum_bound))
            assert abs(diff) > 1e-3
            assert abs(got.sums[k, 0] - diff) <= sum_bound
    finally:
        ctx.close()


# ---- 6. nothing is written; the same bits ----------------------------------------------------

@pytest.mark.parametrize('n,kind,nsites,jit', [(4, 'state', 131, 1), (20, 'dense', 37, 1),
                                               (97, 'mask', 29, 0)])
def test_side_effects_and_determinism(ra, n, kind, nsites, jit):
    case = make_case(n, 12, nsites, kind, 9700 + n, internal=True, per_edge=True)
    weights = np.random.RandomState(n).uniform(0.5, 2.0, size=nsites)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        ll, st = model.log_likelihoods(batch)
        totals = model.fetch_totals(batch)
        name = batch.kernel_name
        esd = model.get_transitions()
        grid, _ = make_grid(model.branch_lengths(), 5, 9700 + n)
        for lengths in (None, grid):
            a = model.nni_scores(batch, lengths=lengths, per_site=True)
            b = model.nni_scores(batch, lengths=lengths, per_site=True)
            for x, y in ((a.values, b.values), (a.sums, b.sums), (a.status, b.status)):
                assert x.tobytes() == y.tobytes()
            sums_only = model.nni_scores(batch, lengths=lengths)
            assert sums_only.values is None
            assert sums_only.sums.tobytes() == a.sums.tobytes()
            assert sums_only.status.tobytes() == a.status.tobytes()
        # the raw call without sums, and without anything but the return code
        M = len(a.moves)
        vals = np.full((nsites, M, 5), np.nan)
        status = np.full(nsites, -1, dtype=np.int32)
        p_f64 = ctypes.POINTER(ctypes.c_double)
        rc = ra.lib.lib().rt_sites_nni_scores(
            model._h, batch._h, 0, 5, grid.ctypes.data_as(p_f64), vals.ctypes.data_as(p_f64),
            None, status.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)))
        assert rc == ra.lib.RT_OK
        assert vals.tobytes() == a.values.tobytes() and status.tobytes() == a.status.tobytes()
        rc = ra.lib.lib().rt_sites_nni_scores(
            model._h, batch._h, 0, 5, grid.ctypes.data_as(p_f64), None, None, None)
        assert rc == ra.lib.RT_OK
        # one point alone gives the bits it gives among others
        one = model.nni_scores(batch, lengths=grid[:, 3:4], per_site=True)
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


# ---- 7. spectral rates -----------------------------------------------------------------------

def test_spectral_rates(ra):
    """n = 20, one reversible rate matrix through raoteh_amd._spectral: P_v(tau) is rebuilt by
    the spectral route.  The reference replaces the matrix of the edge above v by the oracle's
    own reconstruction A diag(exp(lam tau)) B from the same decomposition (the spectral model's
    matrices), at the tolerance of every other case here."""
    from raoteh_amd import _spectral
    n, nsites, seed = 20, 37, 9800
    case = make_case(n, 12, nsites, 'state', seed, internal=False, per_edge=False)
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
    weights = some_weights(nsites, seed)
    ctx = open_context(ra)
    try:
        model = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        model.set_rates_spectral(A, lam, B, D=D)
        model.set_root_distn(pi)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        batch.set_weights(weights)
        grid, factors = make_grid(model.branch_lengths(), 3, seed)
        before = model.get_transitions()
        got = model.nni_scores(batch, factors=factors, per_site=True)
        assert got.lengths.tobytes() == grid.tobytes()
        assert model.get_transitions().tobytes() == before.tobytes()
        wmoves, want, wstatus, loglik = nni_reference(
            model, case, grid, trial_matrix=lambda v, tau: orc.spectral_getp_v2(D, A, lam, B, tau))
        assert not wstatus.any()
        check_scores(got, wmoves, want, wstatus, loglik, weights, 'n=20 spectral')
    finally:
        ctx.close()


# ---- 8. chunks of moves ----------------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37)])
def test_chunks_of_moves_give_the_same_bits(ra, n, nsites, monkeypatch):
    """The moves pass through the device in chunks of RAOTEH_NNI_CHUNK_BYTES of result: one move,
    then three moves per chunk, against the call that holds them all."""
    case = make_case(n, 12, nsites, 'mask', 9900 + n, internal=True, per_edge=True)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, some_weights(nsites, n))
        grid, _ = make_grid(model.branch_lengths(), 3, 9900 + n)
        whole = model.nni_scores(batch, lengths=grid, per_site=True)
        whole_sums = model.nni_scores(batch, lengths=grid)
        assert len(whole.moves) >= 7
        per_move = 3 * nsites * 8
        for moves_per_chunk, per_site in ((1, True), (3, True), (3, False)):
            # (with the per-site array a chunk holds the result and its transpose)
            chunk = moves_per_chunk * per_move * (2 if per_site else 1)
            monkeypatch.setenv('RAOTEH_NNI_CHUNK_BYTES', str(chunk))
            got = model.nni_scores(batch, lengths=grid, per_site=per_site)
            monkeypatch.delenv('RAOTEH_NNI_CHUNK_BYTES')
            assert got.sums.tobytes() == whole.sums.tobytes() == whole_sums.sums.tobytes()
            assert got.status.tobytes() == whole.status.tobytes()
            if per_site:
                assert got.values.tobytes() == whole.values.tobytes()
    finally:
        ctx.close()


# ---- 9. refusals; a tree without moves -------------------------------------------------------

def test_documented_refusals(ra):
    import _partition_cases as pc
    n = 20
    case = make_case(n, 12, 25, 'state', 9950, internal=False, per_edge=False)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        N = model.tree.nnodes
        ll, st = model.log_likelihoods(batch)
        name = batch.kernel_name
        moves = model.nni_moves()
        M = len(moves)
        factors = [0.5, 1.0, 2.0]
        good = model.nni_scores(batch, factors=factors, per_site=True)
        swap = model.nni_scores(batch, per_site=True)

        def raw(npoints, lengths, m=model, b=batch):
            sums = np.zeros((M, max(int(npoints), 1)))
            return ra.lib.lib().rt_sites_nni_scores(
                m._h, b._h, 0, npoints, None if lengths is None else lengths.ctypes.data_as(p_f64),
                None, sums.ctypes.data_as(p_f64), None)

        # npoints out of range (the Python check comes first; the C ABI has its own)
        with pytest.raises(ValueError):
            model.nni_scores(batch, lengths=np.ones((N, 65)))
        assert raw(65, np.ones((N, 65))) == ra.lib.RT_ERR_INVALID
        assert 'grid points' in ra.lib.last_error()
        assert raw(0, np.ones((N, 1))) == ra.lib.RT_ERR_INVALID
        assert raw(2, None) == ra.lib.RT_ERR_INVALID
        assert raw(0, None) == ra.lib.RT_ERR_INVALID
        assert raw(1, None) == ra.lib.RT_OK
        # a negative, a non-finite length in the row of a node with moves ...
        with pytest.raises(ValueError):
            model.nni_scores(batch, factors=[1.0, -0.5])
        with_move = int(moves[0, 0])
        without = [v for v in range(N) if v not in set(moves[:, 0].tolist())]
        assert 0 in without and len(without) > 1
        for x in (-1e-9, np.nan, np.inf):
            bad = np.ones((N, 2))
            bad[with_move, 1] = x
            assert raw(2, bad) == ra.lib.RT_ERR_INVALID
            assert 'negative or not finite' in ra.lib.last_error()
        # ... while the rows of the nodes without a move are ignored
        ignored = np.ones((N, 2))
        ignored[without] = [-1.0, np.nan]
        assert raw(2, ignored) == ra.lib.RT_OK
        # a failed exponential
        huge = np.ones((N, 2))
        huge[with_move, 0] = 1e308
        assert raw(2, huge) == ra.lib.RT_ERR_SINGULAR
        # a batch of another model
        other = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(other, case)
        with pytest.raises(ValueError, match='another model'):
            other.nni_scores(batch)
        # transitions set directly: the plain swap works (the same bits), lengths are refused
        direct = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        direct.set_transitions(model.get_transitions())
        direct.set_root_distn(case.root_distn)
        db = direct.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        plain = direct.nni_scores(db, per_site=True)
        assert plain.lengths is None
        assert plain.values.tobytes() == swap.values.tobytes()
        assert plain.sums.tobytes() == swap.sums.tobytes()
        with pytest.raises(ValueError, match='no rates have been set'):
            direct.nni_scores(db, lengths=np.ones((N, 2)))
        assert raw(2, np.ones((N, 2)), direct, db) == ra.lib.RT_ERR_INVALID
        # a "rescale" batch, a batch of the generic kernel
        for option in ('rescale', 'force_generic'):
            ctx.set_option(option, 1)
            try:
                ob = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
            finally:
                ctx.set_option(option, 0)
            with pytest.raises(ra.lib.RaotehHipError) as err:
                model.nni_scores(ob)
            assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED, option
        # a partitioned batch
        pcase = pc.make_case(20, 'dense', seed=6)
        pmodel, pbatch = pc.upload(ra.device, ctx, pcase)
        pmodel.set_rates(Q=pcase.Q[0], node_q=pcase.node_q, t=pcase.t[0])
        with pytest.raises(ra.lib.RaotehHipError) as err:
            pmodel.nni_scores(pbatch)
        assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
        # the batch is as it was, the context still works
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert batch.kernel_name == name
        again = model.nni_scores(batch, factors=factors, per_site=True)
        assert again.values.tobytes() == good.values.tobytes()
        assert again.sums.tobytes() == good.sums.tobytes()
    finally:
        ctx.close()


def test_a_tree_of_one_node_is_refused(ra):
    n = 20
    lone = nx.Graph()
    lone.add_node('r')
    ctx = open_context(ra)
    try:
        single = ra.device.TreeModel(lone, 'r', n, ctx=ctx)
        single.set_transitions(np.zeros((1, n, n)))
        sb = single.upload_sites(['r'], np.ones((3, 1), dtype=np.uint8), kind='state')
        assert single.nni_moves().shape == (0, 3)
        with pytest.raises(ra.lib.RaotehHipError) as err:
            single.nni_scores(sb)
        assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED
    finally:
        ctx.close()


@pytest.mark.parametrize('n', [4, 20])
def test_a_tree_without_moves(ra, n):
    """A star and a path: RT_OK, empty arrays, the status alone (a zero-likelihood site: leaf in
    state 0 below the root observed in state 1)."""
    rng = np.random.RandomState(n)
    Q = make_case(n, 4, 2, 'state', 1, internal=False).Qs
    for shape in ('star', 'path'):
        T = nx.Graph()
        for child in range(1, 6):
            T.add_edge(0 if shape == 'star' else child - 1, child, weight=0.1 + 0.05 * child)
        obs_nodes = [0, 5] if shape == 'path' else [0, 1, 2, 3, 4, 5]
        states = rng.randint(1, n, size=(21, len(obs_nodes))).astype(np.uint8)
        states[-1, 0], states[-1, -1] = 1, 0
        ctx = open_context(ra)
        try:
            model = ra.device.TreeModel(T, 0, n, ctx=ctx)
            model.set_rates(Q=Q, node_q=np.zeros(6, dtype=np.int64))
            batch = model.upload_sites(obs_nodes, states, kind='state')
            assert model.nni_moves().shape == (0, 3)
            for lengths in (None, np.ones((6, 2))):
                got = model.nni_scores(batch, lengths=lengths, per_site=True)
                G = 1 if lengths is None else 2
                assert got.moves.shape == (0, 3)
                assert got.sums.shape == (0, G) and got.values.shape == (21, 0, G)
                assert got.status.tolist() == [0] * 20 + [ra.lib.RT_SITE_ZERO_PROB]
            _, st = model.log_likelihoods(batch)
            assert np.array_equal(st, got.status)
        finally:
            ctx.close()
