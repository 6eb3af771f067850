"""rt_sites_placements (TreeModel.place_queries) on the GPU: the change of the per-site
log-likelihood when a query sequence is attached to an edge of the tree, for every query, edge,
attachment fraction and pendant length, against a host reference that no device path enters
(tests/_place_cases.py: the extended arrays built by hand, scipy expm for the three new edges,
the oracle's pruning); zeros of the messages, -inf and zero sites, zero-length resident edges,
queries that carry no information, the library's own model build + step on the extended tree,
spectral rates, chunks of queries, side effects and determinism, and the documented refusals."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from oracle import oracle_numpy as orc
from _place_cases import field_terms, place_reference, query_likelihoods
from _profile_cases import site_bounds
from _resident_cases import _encode, make_case, set_rates

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
NQ = 3                                           # queries, 2 fractions, 2 pendant lengths


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


def make_queries(n, nsites, seed):
    """(dense f64[NQ, S, n], states uint8[NQ, S]): dense values with exact zeros and nothing in
    state 0; states 1 .. n - 1 with about one entry in eight unobserved (255)."""
    rng = np.random.RandomState(seed)
    dense = rng.uniform(0.0, 1.0, size=(NQ, nsites, n))
    dense[rng.uniform(size=dense.shape) < 0.2] = 0.0
    dense[:, :, 0] = 0.0
    dense[:, :, 1] += 0.05
    states = rng.randint(1, n, size=(NQ, nsites)).astype(np.uint8)
    states[rng.uniform(size=states.shape) < 0.125] = 255
    assert (states == 255).any()
    return dense, states


def check_placements(got, want, wstatus, loglik, weights, label, tol=1e-10):
    """The status exactly; -inf exactly where the reference has it; elsewhere |got - want| <=
    tol max(1, |log L_i|) per site and tol max(1, sum_i w_i |log L_i|) for the sums
    (site_bounds); every (site, placement) pair is compared.  The worst gaps are printed in
    units of the bound's scale."""
    per_site, sum_bound = site_bounds(loglik, weights, tol)
    np.testing.assert_array_equal(got.status, wstatus)
    S = want.shape[0]
    assert got.values.shape == want.shape and got.sums.shape == want.shape[1:]
    assert not np.isnan(got.values).any() and not np.isnan(got.sums).any()
    assert not got.values[wstatus != 0].any() and not want[wstatus != 0].any()
    assert not got.values[:, :, 0].any() and not got.sums[:, 0].any()      # the root's row
    lost = np.isneginf(want)
    assert np.array_equal(np.isneginf(got.values), lost)
    gap = np.abs(np.where(lost, 0.0, got.values) - np.where(lost, 0.0, want))
    gap = gap / (per_site / tol).reshape((S,) + (1,) * (want.ndim - 1))
    w = np.ones(S) if weights is None else weights
    use = (wstatus == 0) & (w != 0)
    want_sums = np.tensordot(w[use], np.where(lost, 0.0, want)[use], axes=(0, 0))
    slost = lost[use].any(axis=0)
    assert np.array_equal(np.isneginf(got.sums), slost)
    sgap = np.abs(np.where(slost, 0.0, got.sums - want_sums)) / (sum_bound / tol)
    print('%s: %d placements per site, worst per-site gap %.2e, worst sum gap %.2e (units of '
          'max(1, |log L|); bound %.0e)' % (label, int(np.prod(want.shape[1:])), gap.max(),
                                            sgap.max(), tol))
    assert gap.max() <= tol
    assert sgap.max() <= tol
    # best: the arg-max of the sums over the non-root rows, ties to the lowest index
    for q in range(want.shape[1]):
        flat = got.sums[q, 1:].reshape(-1)
        v, r, k = np.unravel_index(int(np.argmax(flat)),
                                   (got.sums.shape[1] - 1,) + got.sums.shape[2:])
        assert got.best[q].tolist() == [v + 1, r, k]
    return gap


# ---- 1. against the host reference -----------------------------------------------------------

PARITY_CASES = ([(n, kind, 70) for n in (2, 4) for kind in ('state', 'mask', 'dense')] +
                [(n, kind, 37) for n in (5, 20, 61, 64) for kind in ('state', 'mask', 'dense')] +
                [(n, kind, 37) for n in (65, 122) for kind in ('mask', 'dense')])
GRIDS = {'state': ((0.0, 0.6), (0.08, 0.45)), 'mask': ((0.35, 1.0), (0.08, 0.45)),
         'dense': ((0.25, 0.7), (0.0, 0.3))}


@pytest.mark.parametrize('n,kind,nsites', PARITY_CASES,
                         ids=['n%d-%s' % c[:2] for c in PARITY_CASES])
def test_against_the_host_reference(ra, n, kind, nsites):
    """12-node trees with multifurcations, a single-child node and observed internal nodes; rate
    matrices that never enter state 0, per edge (two distinct ones) for the 'state' and 'dense'
    batches and one shared matrix for the 'mask' batches; a zero-likelihood site (the last) and
    weights with a zero; dense and state queries.  Worst gaps measured on the MI355X over these
    cases: 5.1e-15 of max(1, |log L|) per site (n = 4, dense batch, state queries) and 1.7e-15 for
    the sums (n = 2), against the bound 1e-10."""
    seed = 9000 + n
    case = make_case(n, 12, nsites, kind, seed, internal=True, per_edge=kind != 'mask')
    assert case.zero_site == nsites - 1
    weights = some_weights(nsites, seed)
    dense, states = make_queries(n, nsites, seed)
    fractions, pendant = GRIDS[kind]
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, weights)
        kids = np.diff(model.tree.indptr)
        assert kids.max() >= 3 and (kids == 1).any()
        both = np.concatenate([dense, query_likelihoods(states, 'state', n)])
        want, wstatus, loglik = place_reference(model, case, both, 'dense', fractions, pendant)
        assert wstatus[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB and wstatus.sum() == 1
        assert np.isfinite(want[wstatus == 0]).any()
        for qkind, queries, rows in (('dense', dense, slice(0, NQ)),
                                     ('state', states, slice(NQ, 2 * NQ))):
            got = model.place_queries(batch, queries, kind=qkind, fractions=fractions,
                                      pendant=pendant, per_site=True)
            assert got.fractions.tolist() == list(fractions)
            assert got.pendant.tolist() == list(pendant)
            check_placements(got, want[:, rows], wstatus, loglik, weights,
                             'n=%d %s, %s queries' % (n, kind, qkind))
    finally:
        ctx.close()


# ---- 2. zeros are exact ----------------------------------------------------------------------

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
def test_zeros_of_the_messages_are_exact(ra, n, nsites, seed):
    """Mask data, and length 0 on the edges above the leaves that have an internal sibling:
    M_v = P_v L_v is then the leaf's mask itself, so the posterior D_p is 0 at every state a the
    mask excludes and the shortcut A_v = D_p / M_v is 0 / 0 there, while A_v[a] itself is
    positive.  The test finds those (site, edge) pairs on the host, with rho = 0 among the
    fractions, and holds the device to the reference at them.  (With all three new edges under
    Q_v, Chapman-Kolmogorov gives P_v[a][c] >= P_v(rho t)[a][b] P_v((1 - rho) t)[b][c]: a state a
    of p with M_v[a] = 0 stays without weight wherever the query attaches on the edge above v, so
    what such a state can break is the division, not the sum -- the case checks that no NaN or
    lost value comes of it.)"""
    case = make_case(n, 12, nsites, 'mask', seed, internal=True, per_edge=True)
    dense, states = make_queries(n, nsites, seed)
    fractions, pendant = (0.0, 0.5), (0.0, 0.2)
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
        got = model.place_queries(batch, dense, fractions=fractions, pendant=pendant, per_site=True)
        want, wstatus, loglik = place_reference(model, case, dense, 'dense', fractions, pendant)
        cols = [ta.node_to_index[v] for v in case.obs_nodes]
        hit = np.zeros((nsites, ta.nnodes), dtype=bool)
        eye = np.eye(n)
        for v in dead:
            A, F, h, Mv = field_terms(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                      case.root_distn, v, eye, eye, eye, dense)
            hit[:, v] = ((Mv == 0) & (A > 0)).any(axis=1) & (wstatus == 0)
            # at rho = 0 and tau = 0 the ratio is sum_b A_v[b] M_v[b] o_q[b] / L_i
            ratio = np.einsum('ib,qib->iq', A * Mv, dense) / np.exp(loglik)[:, None]
            live = wstatus == 0
            with np.errstate(divide='ignore'):
                assert np.allclose(np.log(ratio[live]), want[live][:, :, v, 0, 0], rtol=0, atol=1e-9)
        print('n=%d: %d (site, edge) pairs with A_v > 0 over M_v = 0' % (n, hit.sum()))
        assert hit.sum() >= 1
        gap = check_placements(got, want, wstatus, loglik, None, 'n=%d zero-length leaves' % n)
        at = np.broadcast_to(hit[:, None, :, None, None], want.shape)
        assert np.isfinite(got.values[at]).any() and gap[at].max() <= 1e-10
    finally:
        ctx.close()


@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37)])
def test_minus_infinity_and_zero_sites(ra, n, nsites):
    """A state query in state 0 at site 0, pendant lengths 0 and 0.2: nothing enters state 0, so
    below an observed internal node (never in state 0 at a live site) no live state of the cut
    node reaches the query's state: -inf in the values, -inf in the sums where the weight is
    positive, and nothing of it where the weight is 0."""
    seed = 9400 + n
    case = make_case(n, 12, nsites, 'mask', seed, internal=True, per_edge=True)
    assert case.zero_site == nsites - 1
    _, states = make_queries(n, nsites, seed)
    states[0, 0] = 0
    fractions, pendant = (0.5, 0.75), (0.0, 0.2)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        got = model.place_queries(batch, states, kind='state', fractions=fractions,
                                  pendant=pendant, per_site=True)
        want, wstatus, loglik = place_reference(model, case, states, 'state', fractions, pendant)
        assert wstatus[0] == 0 and np.isfinite(loglik[0])            # site 0 is live
        lost = np.isneginf(want)
        assert lost[0, 0, :, :, 0].any() and np.isfinite(want[0, 1:, 1:]).any()
        assert np.isneginf(got.values[lost]).all()
        assert np.isneginf(got.sums[lost[0]]).all()
        check_placements(got, want, wstatus, loglik, None, 'n=%d -inf' % n)
        assert got.status[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB
        assert got.status.sum() == ra.lib.RT_SITE_ZERO_PROB
        assert not got.values[case.zero_site].any()
        # every site with a -inf at weight 0: nothing of it in the sums
        w = np.where(lost.reshape(nsites, -1).any(axis=1), 0.0, 2.0)
        assert w[0] == 0.0 and (w > 0).sum() >= nsites // 2
        batch.set_weights(w)
        zeroed = model.place_queries(batch, states, kind='state', fractions=fractions,
                                     pendant=pendant, per_site=True)
        assert np.isfinite(zeroed.sums).all()
        assert zeroed.values.tobytes() == got.values.tobytes()
        check_placements(zeroed, want, wstatus, loglik, w, 'n=%d -inf at weight 0' % n)
    finally:
        ctx.close()


# ---- 3. a resident length of zero ------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(3, 70), (20, 37)])
def test_a_resident_length_of_zero_is_nothing_special(ra, n, nsites):
    """t_v = 0 on an internal edge: P_v = I and all three of its grid lengths but tau are 0."""
    seed = 9500 + n
    case = make_case(n, 12, nsites, 'dense', seed, internal=True, per_edge=True)
    dense, states = make_queries(n, nsites, seed)
    fractions, pendant = (0.0, 0.4), (0.0, 0.3)
    ctx = open_context(ra)
    try:
        ta = ra.device.TreeModel(case.T, case.root, n, ctx=ctx).tree
        v = int(np.nonzero(np.diff(ta.indptr)[1:] > 0)[0][0]) + 1
        t = ta.branch_lengths().copy()
        t[v] = 0.0
        model, batch = build(ra, ctx, case, t=t)
        assert model.branch_lengths()[v] == 0.0
        assert np.array_equal(model.get_transitions()[v], np.eye(n))
        got = model.place_queries(batch, dense, fractions=fractions, pendant=pendant, per_site=True)
        want, wstatus, loglik = place_reference(model, case, dense, 'dense', fractions, pendant)
        assert np.isfinite(want[wstatus == 0][:, :, v]).any()
        check_placements(got, want, wstatus, loglik, None, 'n=%d t_v = 0' % n)
    finally:
        ctx.close()


# ---- 4. queries that say nothing -------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37), (122, 37)])
def test_queries_without_information_change_nothing(ra, n, nsites):
    """An all-ones dense query and an all-unobserved state query: h = P 1 = 1 and sum_b F[b] = 1
    (Chapman-Kolmogorov), so every value of a live site is 0 to 1e-12; a zero-likelihood site
    stays at exact zeros.  Through the C ABI a state >= n reads as unobserved."""
    seed = 9550 + n
    case = make_case(n, 12, nsites, 'dense' if n > 4 else 'mask', seed, internal=True, per_edge=True)
    fractions, pendant = (0.0, 0.3, 1.0), (0.0, 0.25)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        _, st = model.log_likelihoods(batch)
        assert st[case.zero_site] == 1 and st.sum() == 1
        ones = model.place_queries(batch, np.ones((2, nsites, n)), fractions=fractions,
                                   pendant=pendant, per_site=True)
        none = model.place_queries(batch, np.full((2, nsites), 255, dtype=np.uint8), kind='state',
                                   fractions=fractions, pendant=pendant, per_site=True)
        for name, got in (('all-ones dense', ones), ('all-unobserved state', none)):
            np.testing.assert_array_equal(got.status, st)
            worst = np.abs(got.values[st == 0]).max()
            print('n=%d %s: worst |value| %.2e (bound 1e-12)' % (n, name, worst))
            assert worst <= 1e-12
            assert not got.values[st != 0].any()
            assert np.abs(got.sums).max() <= 1e-12 * nsites
        if n < 255:
            f = np.array(fractions)
            tau = np.array(pendant)
            vals = np.full(none.values.shape, np.nan)
            p_f64 = ctypes.POINTER(ctypes.c_double)
            q = np.full((2, nsites), n, dtype=np.uint8)
            rc = ra.lib.lib().rt_sites_placements(
                model._h, batch._h, 0, 2, ra.lib.RT_OBS_STATE, q.ctypes.data_as(ctypes.c_void_p),
                3, f.ctypes.data_as(p_f64), 2, tau.ctypes.data_as(p_f64),
                vals.ctypes.data_as(p_f64), None, None)
            assert rc == ra.lib.RT_OK and vals.tobytes() == none.values.tobytes()
    finally:
        ctx.close()


# ---- 5. against the library's own path on the extended tree ----------------------------------

def test_against_a_fresh_model_of_the_extended_tree(ra):
    """n = 20: for two placements, place_apply, a fresh TreeModel of the extended tree (the new
    edges under the rate matrix of the cut edge), upload of reference plus query, step: the
    difference of the weighted totals is sums[q, v, r, k], to the sums' tolerance."""
    n, nsites, seed = 20, 37, 9600
    case = make_case(n, 12, nsites, 'state', seed, internal=True, per_edge=True)
    weights = some_weights(nsites, seed)
    _, states = make_queries(n, nsites, seed)
    fractions, pendant = (0.0, 0.6), (0.0, 0.3)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, weights)
        ta = model.tree
        ll0, st0 = model.log_likelihoods(batch)
        live = (st0 == 0) & (weights != 0)
        got = model.place_queries(batch, states, kind='state', fractions=fractions, pendant=pendant)
        assert got.values is None
        _, sum_bound = site_bounds(np.where(st0 == 0, ll0, 0.0), weights)
        q_of = dict((ta.preorder_nodes[i], int(case.node_q[i])) for i in range(ta.nnodes))
        for q, v, r, k in ((0, 1, 1, 1), (2, ta.nnodes - 1, 0, 1)):
            label = ta.preorder_nodes[v]
            T2 = ra.tree.place_apply(case.T, case.root, label, fractions[r], pendant[k], 'query')
            q_of['query'] = q_of[('cut', 'query')] = q_of[label]
            other = ra.device.TreeModel(T2, case.root, n, ctx=ctx)
            node_q = np.array([q_of[x] for x in other.tree.preorder_nodes], dtype=np.int64)
            other.set_rates(Q=case.Qs, node_q=node_q)
            other.set_root_distn(case.root_distn)
            data = np.concatenate([case.data, states[q][:, None]], axis=1)
            ob = other.upload_sites(list(case.obs_nodes) + ['query'], data, kind='state')
            ll1, st1 = other.log_likelihoods(ob)
            assert np.array_equal(st1, st0)
            diff = float(np.sum(weights[live] * (ll1[live] - ll0[live])))
            print('placement %s: sums %.12g, model build + step %.12g, gap %.2e (bound %.2e)'
                  % ((q, v, r, k), got.sums[q, v, r, k], diff, abs(got.sums[q, v, r, k] - diff),
                     sum_bound))
            assert abs(diff) > 1e-3
            assert abs(got.sums[q, v, r, k] - diff) <= sum_bound
    finally:
        ctx.close()


# ---- 6. spectral rates -----------------------------------------------------------------------

def test_spectral_rates(ra):
    """n = 20, one reversible rate matrix through raoteh_amd._spectral: the matrices of the three
    new edges come from the spectral route; the reference takes the oracle's own reconstruction
    A diag(exp(lam tau)) B from the same decomposition."""
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
    dense, states = make_queries(n, nsites, seed)
    fractions, pendant = (0.3, 1.0), (0.0, 0.2)
    ctx = open_context(ra)
    try:
        model = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        model.set_rates_spectral(A, lam, B, D=D)
        model.set_root_distn(pi)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        batch.set_weights(weights)
        before = model.get_transitions()
        trial = lambda v, tau: orc.spectral_getp_v2(D, A, lam, B, tau)
        for qkind, queries in (('dense', dense), ('state', states)):
            got = model.place_queries(batch, queries, kind=qkind, fractions=fractions,
                                      pendant=pendant, per_site=True)
            assert model.get_transitions().tobytes() == before.tobytes()
            want, wstatus, loglik = place_reference(model, case, queries, qkind, fractions, pendant,
                                                    trial_matrix=trial)
            assert not wstatus.any()
            check_placements(got, want, wstatus, loglik, weights, 'n=20 spectral, %s' % qkind)
    finally:
        ctx.close()


# ---- 7. chunks of queries --------------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37)])
def test_chunks_of_queries_give_the_same_bits(ra, n, nsites, monkeypatch):
    """The queries pass through the device in chunks of RAOTEH_PLACE_CHUNK_BYTES of result: one
    query, then two of the three per chunk, against the call that holds them all."""
    case = make_case(n, 12, nsites, 'mask', 9900 + n, internal=True, per_edge=True)
    dense, states = make_queries(n, nsites, 9900 + n)
    fractions, pendant = (0.2, 1.0), (0.0, 0.3)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, some_weights(nsites, n))
        N = model.tree.nnodes
        per_query = N * 2 * 2 * nsites * 8
        for qkind, queries in (('dense', dense), ('state', states)):
            kw = dict(kind=qkind, fractions=fractions, pendant=pendant)
            whole = model.place_queries(batch, queries, per_site=True, **kw)
            whole_sums = model.place_queries(batch, queries, **kw)
            assert np.abs(whole.sums[np.isfinite(whole.sums)]).max() > 1e-3
            for queries_per_chunk, per_site in ((1, True), (2, True), (2, False)):
                # (with the per-site array a chunk holds the result and its transpose)
                chunk = queries_per_chunk * per_query * (2 if per_site else 1)
                monkeypatch.setenv('RAOTEH_PLACE_CHUNK_BYTES', str(chunk))
                got = model.place_queries(batch, queries, per_site=per_site, **kw)
                monkeypatch.delenv('RAOTEH_PLACE_CHUNK_BYTES')
                assert got.sums.tobytes() == whole.sums.tobytes() == whole_sums.sums.tobytes()
                assert got.status.tobytes() == whole.status.tobytes()
                assert np.array_equal(got.best, whole.best)
                if per_site:
                    assert got.values.tobytes() == whole.values.tobytes()
    finally:
        ctx.close()


# ---- 8. nothing is written; the same bits ----------------------------------------------------

@pytest.mark.parametrize('n,kind,nsites,jit', [(4, 'state', 131, 1), (20, 'dense', 37, 1),
                                               (97, 'mask', 29, 0), (4, 'mask', 70, 0)])
def test_side_effects_and_determinism(ra, n, kind, nsites, jit):
    case = make_case(n, 12, nsites, kind, 9700 + n, internal=True, per_edge=True)
    weights = np.random.RandomState(n).uniform(0.5, 2.0, size=nsites)
    dense, states = make_queries(n, nsites, 9700 + n)
    f, tau = np.array([0.0, 0.5]), np.array([0.1, 0.4])
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        ll, st = model.log_likelihoods(batch)
        totals = model.fetch_totals(batch)
        name = batch.kernel_name
        esd = model.get_transitions()
        N = model.tree.nnodes
        p_f64, p_i32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        for qkind, queries, code in (('dense', dense, ra.lib.RT_OBS_DENSE),
                                     ('state', states, ra.lib.RT_OBS_STATE)):
            kw = dict(kind=qkind, fractions=f, pendant=tau)
            a = model.place_queries(batch, queries, per_site=True, **kw)
            b = model.place_queries(batch, queries, per_site=True, **kw)
            for x, y in ((a.values, b.values), (a.sums, b.sums), (a.status, b.status)):
                assert x.tobytes() == y.tobytes()
            sums_only = model.place_queries(batch, queries, **kw)
            assert sums_only.values is None
            assert sums_only.sums.tobytes() == a.sums.tobytes()
            assert sums_only.status.tobytes() == a.status.tobytes()
            # every NULL combination of values / sums / status through the raw call
            queries = np.ascontiguousarray(queries)
            for mask in range(8):
                vals = np.full((nsites, NQ, N, 2, 2), np.nan)
                sums = np.full((NQ, N, 2, 2), np.nan)
                status = np.full(nsites, -1, dtype=np.int32)
                rc = ra.lib.lib().rt_sites_placements(
                    model._h, batch._h, 0, NQ, code, queries.ctypes.data_as(ctypes.c_void_p), 2,
                    f.ctypes.data_as(p_f64), 2, tau.ctypes.data_as(p_f64),
                    vals.ctypes.data_as(p_f64) if mask & 1 else None,
                    sums.ctypes.data_as(p_f64) if mask & 2 else None,
                    status.ctypes.data_as(p_i32) if mask & 4 else None)
                assert rc == ra.lib.RT_OK
                assert vals.tobytes() == a.values.tobytes() if mask & 1 else np.isnan(vals).all()
                assert sums.tobytes() == a.sums.tobytes() if mask & 2 else np.isnan(sums).all()
                assert status.tobytes() == a.status.tobytes() if mask & 4 else (status == -1).all()
            # one query, one fraction, one pendant length alone give the bits they give among others
            one = model.place_queries(batch, queries[1:2], kind=qkind, fractions=f[1:], pendant=tau[:1],
                                      per_site=True)
            assert one.values[:, 0, :, 0, 0].tobytes() == \
                np.ascontiguousarray(a.values[:, 1, :, 1, 0]).tobytes()
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


# ---- 10. refusals ----------------------------------------------------------------------------

def test_documented_refusals(ra):
    import _partition_cases as pc
    n, nsites = 20, 25
    case = make_case(n, 12, nsites, 'state', 9950, internal=False, per_edge=False)
    dense, states = make_queries(n, nsites, 9950)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    L = ra.lib
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        N = model.tree.nnodes
        ll, st = model.log_likelihoods(batch)
        name = batch.kernel_name
        good = model.place_queries(batch, dense, fractions=(0.0, 0.5), pendant=(0.1,), per_site=True)
        assert np.array_equal(good.pendant, [0.1])
        default = model.place_queries(batch, dense)
        assert default.fractions.tolist() == [0.5]
        assert default.pendant.tolist() == [float(np.mean(model.branch_lengths()[1:]))]

        def raw(nq=NQ, kind=L.RT_OBS_DENSE, queries=dense, fractions=(0.5,), pendant=(0.1,),
                nf=None, npd=None, m=model, b=batch):
            f = None if fractions is None else np.array(fractions, dtype=np.float64)
            t = None if pendant is None else np.array(pendant, dtype=np.float64)
            nf = (0 if f is None else len(f)) if nf is None else nf
            npd = (0 if t is None else len(t)) if npd is None else npd
            sums = np.zeros((max(nq, 1), N, max(nf, 1), max(npd, 1)))
            return L.lib().rt_sites_placements(
                m._h, b._h, 0, nq, kind,
                None if queries is None else queries.ctypes.data_as(ctypes.c_void_p), nf,
                None if f is None else f.ctypes.data_as(p_f64), npd,
                None if t is None else t.ctypes.data_as(p_f64), None, sums.ctypes.data_as(p_f64),
                None)

        assert raw() == L.RT_OK
        # nqueries < 1, counts out of range
        assert raw(nq=0) == L.RT_ERR_INVALID
        assert raw(nq=-1) == L.RT_ERR_INVALID
        assert raw(fractions=(0.5,), nf=0) == L.RT_ERR_INVALID
        assert raw(fractions=(0.5,) * 9) == L.RT_ERR_INVALID
        assert 'fractions' in L.last_error()
        assert raw(pendant=(0.1,), npd=0) == L.RT_ERR_INVALID
        assert raw(pendant=(0.1,) * 17) == L.RT_ERR_INVALID
        assert 'pendant' in L.last_error()
        assert raw(fractions=(0.5,) * 8, pendant=(0.1,) * 16) == L.RT_OK          # 2 * 8 + 16 = 32
        with pytest.raises(ValueError):
            model.place_queries(batch, dense, fractions=(0.5,) * 9)
        # a fraction outside [0, 1] or not finite; a negative or non-finite pendant length
        for x in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert raw(fractions=(0.5, x)) == L.RT_ERR_INVALID
            assert 'outside [0, 1] or not finite' in L.last_error()
        for x in (-1e-9, np.nan, np.inf):
            assert raw(pendant=(0.1, x)) == L.RT_ERR_INVALID
            assert 'negative or not finite' in L.last_error()
        with pytest.raises(ValueError):
            model.place_queries(batch, dense, pendant=(-0.5,))
        # NULL queries, fractions or pendant
        assert raw(queries=None) == L.RT_ERR_INVALID
        assert raw(fractions=None, nf=1) == L.RT_ERR_INVALID
        assert raw(pendant=None, npd=1) == L.RT_ERR_INVALID
        # mask queries, another kind
        assert raw(kind=L.RT_OBS_MASK) == L.RT_ERR_UNSUPPORTED
        assert raw(kind=7) == L.RT_ERR_INVALID
        with pytest.raises(ValueError):
            model.place_queries(batch, dense, kind='mask')
        # a failed exponential
        assert raw(pendant=(1e308,)) == L.RT_ERR_SINGULAR
        # a batch of another model
        other = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(other, case)
        with pytest.raises(ValueError, match='another model'):
            other.place_queries(batch, dense)
        # no rates; transitions set directly after the rates
        direct = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        direct.set_transitions(model.get_transitions())
        direct.set_root_distn(case.root_distn)
        db = direct.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        with pytest.raises(ValueError, match='no rates have been set'):
            direct.place_queries(db, dense, pendant=(0.1,))
        assert raw(m=direct, b=db) == L.RT_ERR_INVALID
        after = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(after, case)
        after.set_root_distn(case.root_distn)
        after.set_transitions(model.get_transitions())
        ab = after.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        assert raw(m=after, b=ab) == L.RT_ERR_INVALID
        assert 'set directly after the rates' in L.last_error()
        again = after.place_queries(ab, dense, fractions=(0.0, 0.5), pendant=(0.1,), per_site=True,
                                    recompute_transitions=True)
        assert again.values.tobytes() == good.values.tobytes()
        # a "rescale" batch, a batch of the generic kernel
        for option in ('rescale', 'force_generic'):
            ctx.set_option(option, 1)
            try:
                ob = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
            finally:
                ctx.set_option(option, 0)
            with pytest.raises(L.RaotehHipError) as err:
                model.place_queries(ob, dense)
            assert err.value.code == L.RT_ERR_UNSUPPORTED, option
        # a partitioned batch
        pcase = pc.make_case(20, 'dense', seed=6)
        pmodel, pbatch = pc.upload(ra.device, ctx, pcase)
        pmodel.set_rates(Q=pcase.Q[0], node_q=pcase.node_q, t=pcase.t[0])
        with pytest.raises(L.RaotehHipError) as err:
            pmodel.place_queries(pbatch, np.ones((1, pbatch.nsites, 20)))
        assert err.value.code == L.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
        # the batch is as it was, the context still works
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert batch.kernel_name == name
        once_more = model.place_queries(batch, dense, fractions=(0.0, 0.5), pendant=(0.1,),
                                        per_site=True)
        assert once_more.values.tobytes() == good.values.tobytes()
        assert once_more.sums.tobytes() == good.sums.tobytes()
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
        with pytest.raises(ra.lib.RaotehHipError) as err:
            single.place_queries(sb, np.ones((1, 3, n)), pendant=(0.1,))
        assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED
    finally:
        ctx.close()
