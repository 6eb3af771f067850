"""rt_sites_spr_scores (TreeModel.spr_scores) on the GPU: the change of the per-site
log-likelihood for every subtree pruning and regrafting move of the tree and every fraction,
against a host reference that no device path enters (tests/_spr_cases.py: the moves by brute
force, the rearranged arrays built by hand, scipy expm for the halves of the cut edge, the
oracle's pruning); zeros of the messages, -inf and zero sites, zero-length resident edges, parents
left childless, the moves that leave the tree unchanged, the library's own model build + step on
the moved tree, spectral rates, chunks of pruned nodes, side effects and determinism, and the
documented refusals."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from oracle import oracle_numpy as orc
from _nni_cases import children_of, parents_of, up_pass
from _spr_cases import (brute_moves, moved_arrays, spr_formula, spr_reference,
                        unlimited_count)
from _profile_cases import site_bounds
from _resident_cases import _encode, make_case, set_rates

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


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


def check_scores(got, wmoves, want, wstatus, loglik, weights, label, tol=1e-10):
    """The moves and the status exactly; -inf exactly where the reference has it; elsewhere
    |got - want| <= tol max(1, |log L_i|) per site and tol max(1, sum_i w_i |log L_i|) for the
    sums (site_bounds); every (site, move, fraction) triple is compared.  The worst gaps are
    printed in units of the bound's scale."""
    per_site, sum_bound = site_bounds(loglik, weights, tol)
    np.testing.assert_array_equal(got.moves, wmoves)
    np.testing.assert_array_equal(got.status, wstatus)
    S = want.shape[0]
    assert got.values.shape == want.shape and got.sums.shape == want.shape[1:]
    assert not np.isnan(got.values).any() and not np.isnan(got.sums).any()
    assert not got.values[wstatus != 0].any() and not want[wstatus != 0].any()
    lost = np.isneginf(want)
    assert np.array_equal(np.isneginf(got.values), lost)
    gap = np.abs(np.where(lost, 0.0, got.values) - np.where(lost, 0.0, want))
    gap = gap / (per_site / tol).reshape((S, 1, 1))
    w = np.ones(S) if weights is None else weights
    use = (wstatus == 0) & (w != 0)
    want_sums = np.tensordot(w[use], np.where(lost, 0.0, want)[use], axes=(0, 0))
    slost = lost[use].any(axis=0)
    assert np.array_equal(np.isneginf(got.sums), slost)
    sgap = np.abs(np.where(slost, 0.0, got.sums - want_sums)) / (sum_bound / tol)
    print('%s: %d moves x %d fractions per site, worst per-site gap %.2e, worst sum gap %.2e '
          '(units of max(1, |log L|); bound %.0e)' % (label, want.shape[1], want.shape[2],
                                                      gap.max(), sgap.max(), tol))
    assert gap.max() <= tol
    assert sgap.max() <= tol
    # best: the arg-max of the sums, ties to the lowest index
    assert got.best == tuple(int(x) for x in
                             np.unravel_index(int(np.argmax(got.sums.reshape(-1))), got.sums.shape))
    return gap


# ---- 1. against the host reference -----------------------------------------------------------

PARITY_CASES = ([(n, kind, 70, None) for n in (2, 4) for kind in ('state', 'mask', 'dense')] +
                [(n, kind, 37, None) for n in (5, 20, 61, 64) for kind in ('state', 'mask', 'dense')] +
                [(n, kind, 37, None) for n in (65, 122) for kind in ('mask', 'dense')] +
                [(4, 'mask', 70, 1), (20, 'dense', 37, 1)])
FRACTIONS = {'state': (0.0, 0.6), 'mask': (0.35, 1.0), 'dense': (0.0, 0.6)}


@pytest.mark.parametrize('n,kind,nsites,radius', PARITY_CASES,
                         ids=['n%d-%s-r%s' % (c[0], c[1], c[3]) for c in PARITY_CASES])
def test_against_the_host_reference(ra, n, kind, nsites, radius):
    """12-node trees with multifurcations, a single-child node and observed internal nodes; rate
    matrices that never enter state 0, per edge (two distinct ones) for the 'state' and 'dense'
    batches and one shared matrix for the 'mask' batches; a zero-likelihood site (the last) and
    weights with a zero; every move without a limit of the radius, and radius 1 at n = 4 and
    20."""
    seed = 9000 + n
    case = make_case(n, 12, nsites, kind, seed, internal=True, per_edge=kind != 'mask')
    assert case.zero_site == nsites - 1
    weights = some_weights(nsites, seed)
    fractions = FRACTIONS[kind]
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, weights)
        ta = model.tree
        kids = np.diff(ta.indptr)
        assert kids.max() >= 3 and (kids == 1).any()
        wmoves, want, wstatus, loglik = spr_reference(model, case, fractions, radius)
        if radius is None:
            assert len(wmoves) == unlimited_count(ta.indices, ta.indptr)
            # a pruned node whose parent is left childless is among the moves
            assert any(kids[ta.parent[c]] == 1 for c in wmoves[:, 0])
        else:
            assert 0 < len(wmoves) < unlimited_count(ta.indices, ta.indptr)
        assert wstatus[case.zero_site] == ra.lib.RT_SITE_ZERO_PROB and wstatus.sum() == 1
        assert np.isfinite(want[wstatus == 0]).any()
        got = model.spr_scores(batch, radius=radius, fractions=fractions, per_site=True)
        assert got.fractions.tolist() == list(fractions)
        assert np.array_equal(model.spr_moves(radius), wmoves)
        check_scores(got, wmoves, want, wstatus, loglik, weights,
                     'n=%d %s radius %s' % (n, kind, radius))
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


def live_states_after(ta, esd, cols, obs_lik, root_distn, c, y, Pa, Pb, n):
    """bool[S, n]: state a of v = parent(c) has positive weight at the site on the tree after the
    move (c, y) -- the oracle's likelihood of the moved tree with v observed in state a too."""
    N = ta.nnodes
    v = int(ta.parent[c])
    ni, npt, old_of_new = moved_arrays(ta.indices, ta.indptr, int(c), int(y))
    new_of_old = np.empty_like(old_of_new)
    new_of_old[old_of_new] = np.arange(N + 1)
    ext = np.concatenate([esd, Pa[None]])
    ext[y] = Pb
    out = np.zeros((obs_lik.shape[0], n), dtype=bool)
    for a in range(n):
        e = np.zeros(n)
        e[a] = 1.0
        lik, columns = obs_lik, list(cols)
        if v in columns:
            lik = obs_lik.copy()
            lik[:, columns.index(v)] *= e
        else:
            lik = np.concatenate([obs_lik, np.tile(e, (obs_lik.shape[0], 1, 1))], axis=1)
            columns.append(v)
        ll, st = orc.batch_log_likelihoods(ni, npt, ext[old_of_new],
                                           [int(new_of_old[k]) for k in columns], lik, root_distn)
        out[:, a] = st == 0
    return out


@pytest.mark.parametrize('n,nsites,seed', [(4, 70, 9304), (20, 37, 9320)])
def test_zeros_of_the_messages_are_exact(ra, n, nsites, seed):
    """Mask data, and length 0 on the edges above the leaves that have an internal sibling: the
    message M_c = P_c L_c of such a leaf c is its mask itself, so L_v and the posterior of
    v = parent(c) are 0 at every state a the mask excludes, and every quotient form
    (L-_v = L_v / M_c, A = D / M) is 0 / 0 there -- yet once c is pruned such a state of v may be
    live.  The test counts the (site, move) pairs where a state a with M_c[a] = 0 has positive
    weight at v after the move (by the oracle, on the moved tree with v observed in a too),
    asserts there are some, and holds the device to the reference at them."""
    case = make_case(n, 12, nsites, 'mask', seed, internal=True, per_edge=True)
    fractions = (0.0, 0.6)
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
        got = model.spr_scores(batch, fractions=fractions, per_site=True)
        wmoves, want, wstatus, loglik = spr_reference(model, case, fractions)
        cols = [ta.node_to_index[v] for v in case.obs_nodes]
        obs, L, M, up = up_pass(ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn)
        hit = np.zeros((nsites, len(wmoves)), dtype=bool)
        import scipy.linalg
        for k, (c, y) in enumerate(wmoves):
            if c not in dead:
                continue
            v = int(ta.parent[c])
            if v == 0:
                continue
            Q = case.Qs[case.node_q[y]]
            Pa, Pb = scipy.linalg.expm(Q * 0.6 * t[y]), scipy.linalg.expm(Q * 0.4 * t[y])
            alive = live_states_after(ta, esd, cols, case.obs_lik, case.root_distn, c, y, Pa, Pb, n)
            hit[:, k] = ((M[:, c] == 0) & alive).any(axis=1) & (wstatus == 0)
        print('n=%d: %d (site, move) pairs with a state of v live after the move over M_c = 0'
              % (n, hit.sum()))
        assert hit.sum() >= 1
        # the other quotient form, A = D / M: a target y that is such a leaf, a state a its
        # message excludes (M_y[a] = 0, so the posterior of parent(y) is 0 there) and A-_y[a] > 0
        hit_a = np.zeros((nsites, len(wmoves)), dtype=bool)
        eye = np.eye(n)
        for k, (c, y) in enumerate(wmoves):
            if y not in dead:
                continue
            _, _, A, _ = spr_formula(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                     case.root_distn, int(c), int(y), eye, eye)
            hit_a[:, k] = ((M[:, y] == 0) & (A > 0)).any(axis=1) & (wstatus == 0)
        print('n=%d: %d (site, move) pairs with A-_y > 0 over M_y = 0' % (n, hit_a.sum()))
        assert hit_a.sum() >= 1
        gap = check_scores(got, wmoves, want, wstatus, loglik, None, 'n=%d zero-length leaves' % n)
        assert np.isfinite(got.values[hit][:, 1]).all() and gap[hit].max() <= 1e-10
        assert np.isfinite(got.values[hit_a]).any() and gap[hit_a].max() <= 1e-10
    finally:
        ctx.close()


@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37)])
def test_minus_infinity_and_zero_sites(ra, n, nsites):
    """Leaves only observed, but for one internal node z whose mask excludes state 0; at site 0
    a leaf c outside the subtree of z is in state 0.  Nothing enters state 0, so the site is live
    only with every ancestor of c in state 0: hung on an edge below z, c has an ancestor that
    cannot be -- -inf in the values, -inf in the sums where the weight is positive, and nothing
    of it where the weight is 0."""
    seed = 9400 + n
    case = make_case(n, 12, nsites, 'mask', seed, internal=False, per_edge=True)
    assert case.zero_site is None
    ctx = open_context(ra)
    try:
        ta = ra.device.TreeModel(case.T, case.root, n, ctx=ctx).tree
        parent, kids = parents_of(ta.indices, ta.indptr), children_of(ta.indices, ta.indptr)
        z = [v for v in range(1, ta.nnodes) if kids[v]][-1]

        def under(a, b):
            while a >= 0 and a != b:
                a = parent[a]
            return a == b
        leaves = [ta.node_to_index[x] for x in case.obs_nodes]
        c = [v for v in leaves if not under(v, z)][0]
        lik = np.concatenate([case.obs_lik, np.ones((nsites, 1, n))], axis=1)
        lik[:, -1, 0] = 0.0
        lik[0, leaves.index(c)] = 0.0
        lik[0, leaves.index(c), 0] = 1.0
        case = case._replace(obs_nodes=list(case.obs_nodes) + [ta.preorder_nodes[z]],
                             obs_lik=lik, data=_encode('mask', n, lik))
        fractions = (0.5, 1.0)
        model, batch = build(ra, ctx, case)
        got = model.spr_scores(batch, fractions=fractions, per_site=True)
        wmoves, want, wstatus, loglik = spr_reference(model, case, fractions)
        assert wstatus[0] == 0 and np.isfinite(loglik[0])            # site 0 is live
        lost = np.isneginf(want)
        below_z = np.array([m[0] == c and under(int(m[1]), z) and m[1] != z for m in wmoves])
        assert below_z.any() and lost[0, below_z].all()
        assert np.isfinite(want[0, wmoves[:, 0] == c]).any()
        assert np.isneginf(got.values[lost]).all()
        assert np.isneginf(got.sums[lost[0]]).all()
        check_scores(got, wmoves, want, wstatus, loglik, None, 'n=%d -inf' % n)
        # every site with a -inf at weight 0: nothing of it in the sums
        w = np.where(lost.reshape(nsites, -1).any(axis=1), 0.0, 2.0)
        assert w[0] == 0.0 and (w > 0).sum() >= nsites // 2
        batch.set_weights(w)
        zeroed = model.spr_scores(batch, fractions=fractions, per_site=True)
        assert np.isfinite(zeroed.sums).all()
        assert zeroed.values.tobytes() == got.values.tobytes()
        check_scores(zeroed, wmoves, want, wstatus, loglik, w, 'n=%d -inf at weight 0' % n)
    finally:
        ctx.close()


# ---- 3. special cases ------------------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(3, 70), (20, 37)])
def test_zero_lengths_childless_parents_and_a_single_child_of_the_root(ra, n, nsites):
    """t = 0 on an internal edge and on a leaf's edge (each is a target edge and a pruned edge
    among the moves: P = I and both of its grid lengths are 0); a pruned node whose parent is left
    childless, observed or not; a root with two children, one of which is pruned into the other's
    subtree, so the root's remaining child is single."""
    from raoteh_amd import _tree, synth

    def child_counts(s):
        T, root, _ = synth.random_tree(12, seed=s, max_children=3)
        return np.diff(_tree.TreeArrays(T, root).indptr)
    seed = [s for s in range(9500, 9600)
            if child_counts(s)[0] == 2 and (child_counts(s) == 1).any()][0]
    case = make_case(n, 12, nsites, 'dense', seed, internal=True, per_edge=True)
    fractions = (0.0, 0.4)
    ctx = open_context(ra)
    try:
        ta = ra.device.TreeModel(case.T, case.root, n, ctx=ctx).tree
        kids = np.diff(ta.indptr)
        assert kids[0] == 2 and (kids == 1).any()
        v = int(np.nonzero(kids[1:] > 0)[0][0]) + 1
        leaf = int(np.nonzero(kids == 0)[0][-1])
        t = ta.branch_lengths().copy()
        t[[v, leaf]] = 0.0
        model, batch = build(ra, ctx, case, t=t)
        assert model.branch_lengths()[v] == 0.0 and model.branch_lengths()[leaf] == 0.0
        assert np.array_equal(model.get_transitions()[v], np.eye(n))
        got = model.spr_scores(batch, fractions=fractions, per_site=True)
        wmoves, want, wstatus, loglik = spr_reference(model, case, fractions)
        for node in (v, leaf):
            assert (wmoves[:, 0] == node).any() and (wmoves[:, 1] == node).any()
        assert any(kids[ta.parent[c]] == 1 for c in wmoves[:, 0])
        assert any(ta.parent[c] == 0 and ta.parent[y] != 0 for c, y in wmoves)
        assert np.isfinite(want[wstatus == 0]).any()
        check_scores(got, wmoves, want, wstatus, loglik, None, 'n=%d special cases' % n)
    finally:
        ctx.close()


# ---- 4. the moves that leave the tree unchanged ----------------------------------------------

@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37), (122, 37)])
def test_identity_moves_score_zero(ra, n, nsites):
    """(c, v) at rho = 1 and (c, sibling of c) at rho = 0, for every c: the cut node coincides
    with v across an identity matrix, every value of a live site is 0 to 1e-12 -- no reference
    enters; a zero-likelihood site stays at exact zeros."""
    seed = 9550 + n
    case = make_case(n, 12, nsites, 'dense' if n > 4 else 'mask', seed, internal=True, per_edge=True)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        ta = model.tree
        _, st = model.log_likelihoods(batch)
        assert st[case.zero_site] == 1 and st.sum() == 1
        got = model.spr_scores(batch, radius=0, fractions=(0.0, 1.0), per_site=True)
        np.testing.assert_array_equal(got.status, st)
        seen = set()
        worst = 0.0
        for k, (c, y) in enumerate(got.moves):
            r = 1 if y == ta.parent[c] else 0
            assert r == 1 or ta.parent[y] == ta.parent[c]
            worst = max(worst, np.abs(got.values[st == 0, k, r]).max())
            assert abs(got.sums[k, r]) <= 1e-12 * nsites
            seen.add(int(c))
        print('n=%d: %d identity moves, worst |value| %.2e (bound 1e-12)' % (n, len(got.moves), worst))
        assert worst <= 1e-12
        # every c but an only child of the root has such a move
        assert seen >= set(c for c in range(1, ta.nnodes)
                           if ta.parent[c] != 0 or np.diff(ta.indptr)[0] > 1)
        assert not got.values[st != 0].any()
        assert np.abs(got.values[st == 0]).max() > 1e-3          # (the other fraction moves c)
    finally:
        ctx.close()


# ---- 5. against the library's own path on the moved tree -------------------------------------

def test_against_a_fresh_model_of_the_moved_tree(ra):
    """n = 20: for two moves, spr_apply, a fresh TreeModel of the moved tree (the halves of the
    cut edge under its rate matrix), upload, step: the difference of the weighted totals is
    sums[mv, r], to the sums' tolerance."""
    n, nsites, seed = 20, 37, 9600
    case = make_case(n, 12, nsites, 'state', seed, internal=True, per_edge=True)
    weights = some_weights(nsites, seed)
    fractions = (0.0, 0.6)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, weights)
        ta = model.tree
        ll0, st0 = model.log_likelihoods(batch)
        live = (st0 == 0) & (weights != 0)
        got = model.spr_scores(batch, fractions=fractions)
        assert got.values is None
        _, sum_bound = site_bounds(np.where(st0 == 0, ll0, 0.0), weights)
        q_of = dict((ta.preorder_nodes[i], int(case.node_q[i])) for i in range(ta.nnodes))
        finite = np.nonzero(np.isfinite(got.sums).all(axis=1))[0]
        for mv, r in ((int(finite[1]), 1), (int(finite[-2]), 0)):
            c, y = (ta.preorder_nodes[int(x)] for x in got.moves[mv])
            T2 = ra.tree.spr_apply(case.T, case.root, c, y, fractions[r], cut_label='cut')
            other = ra.device.TreeModel(T2, case.root, n, ctx=ctx)
            names = dict(q_of, cut=q_of[y])
            node_q = np.array([names[x] for x in other.tree.preorder_nodes], dtype=np.int64)
            other.set_rates(Q=case.Qs, node_q=node_q)
            other.set_root_distn(case.root_distn)
            ob = other.upload_sites(case.obs_nodes, case.data, kind='state')
            ll1, st1 = other.log_likelihoods(ob)
            assert np.array_equal(st1, st0)
            diff = float(np.sum(weights[live] * (ll1[live] - ll0[live])))
            print('move %s at %g: sums %.12g, model build + step %.12g, gap %.2e (bound %.2e)'
                  % (got.moves[mv].tolist(), fractions[r], got.sums[mv, r], diff,
                     abs(got.sums[mv, r] - diff), sum_bound))
            assert abs(diff) > 1e-3
            assert abs(got.sums[mv, r] - diff) <= sum_bound
    finally:
        ctx.close()


# ---- 6. spectral rates -----------------------------------------------------------------------

def test_spectral_rates(ra):
    """n = 20, one reversible rate matrix through raoteh_amd._spectral: the matrices of the two
    halves come from the spectral route; the reference takes the oracle's own reconstruction
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
    fractions = (0.3, 1.0)
    ctx = open_context(ra)
    try:
        model = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        model.set_rates_spectral(A, lam, B, D=D)
        model.set_root_distn(pi)
        batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        batch.set_weights(weights)
        before = model.get_transitions()
        trial = lambda v, tau: orc.spectral_getp_v2(D, A, lam, B, tau)
        got = model.spr_scores(batch, radius=2, fractions=fractions, per_site=True)
        assert model.get_transitions().tobytes() == before.tobytes()
        wmoves, want, wstatus, loglik = spr_reference(model, case, fractions, 2, trial_matrix=trial)
        assert not wstatus.any()
        check_scores(got, wmoves, want, wstatus, loglik, weights, 'n=20 spectral')
    finally:
        ctx.close()


# ---- 7. chunks of pruned nodes ---------------------------------------------------------------

@pytest.mark.parametrize('n,nsites', [(4, 70), (20, 37)])
def test_chunks_of_pruned_nodes_give_the_same_bits(ra, n, nsites, monkeypatch):
    """The pruned nodes pass through the device in chunks of RAOTEH_SPR_CHUNK_BYTES of result:
    one pruned node per chunk (a chunk never splits the moves of one), then about three (the
    bytes of three times the largest pruned node's moves), against the call that holds them
    all."""
    case = make_case(n, 12, nsites, 'mask', 9900 + n, internal=True, per_edge=True)
    fractions = (0.2, 1.0)
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case, some_weights(nsites, n))
        whole = model.spr_scores(batch, fractions=fractions, per_site=True)
        whole_sums = model.spr_scores(batch, fractions=fractions)
        assert np.abs(whole.sums[np.isfinite(whole.sums)]).max() > 1e-3
        per_move = 2 * nsites * 8
        most = int(np.bincount(whole.moves[:, 0]).max())
        assert len(whole.moves) > 3 * most
        for moves_per_chunk, per_site in ((1, True), (3 * most, True), (3 * most, False)):
            # (with the per-site array a chunk holds the result and its transpose)
            chunk = moves_per_chunk * per_move * (2 if per_site else 1)
            monkeypatch.setenv('RAOTEH_SPR_CHUNK_BYTES', str(chunk))
            got = model.spr_scores(batch, fractions=fractions, per_site=per_site)
            monkeypatch.delenv('RAOTEH_SPR_CHUNK_BYTES')
            assert got.sums.tobytes() == whole.sums.tobytes() == whole_sums.sums.tobytes()
            assert got.status.tobytes() == whole.status.tobytes()
            assert got.best == whole.best
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
    f = np.array([0.0, 0.5])
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        ll, st = model.log_likelihoods(batch)
        totals = model.fetch_totals(batch)
        name = batch.kernel_name
        esd = model.get_transitions()
        nni = model.nni_scores(batch, per_site=True)
        p_f64, p_i32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
        a = model.spr_scores(batch, radius=2, fractions=f, per_site=True)
        b = model.spr_scores(batch, radius=2, fractions=f, per_site=True)
        for x, y in ((a.values, b.values), (a.sums, b.sums), (a.status, b.status)):
            assert x.tobytes() == y.tobytes()
        sums_only = model.spr_scores(batch, radius=2, fractions=f)
        assert sums_only.values is None
        assert sums_only.sums.tobytes() == a.sums.tobytes()
        assert sums_only.status.tobytes() == a.status.tobytes()
        M = len(a.moves)
        # every NULL combination of values / sums / status through the raw call
        for mask in range(8):
            vals = np.full((nsites, M, 2), np.nan)
            sums = np.full((M, 2), np.nan)
            status = np.full(nsites, -1, dtype=np.int32)
            rc = ra.lib.lib().rt_sites_spr_scores(
                model._h, batch._h, 0, 2, 2, f.ctypes.data_as(p_f64),
                vals.ctypes.data_as(p_f64) if mask & 1 else None,
                sums.ctypes.data_as(p_f64) if mask & 2 else None,
                status.ctypes.data_as(p_i32) if mask & 4 else None)
            assert rc == ra.lib.RT_OK
            assert vals.tobytes() == a.values.tobytes() if mask & 1 else np.isnan(vals).all()
            assert sums.tobytes() == a.sums.tobytes() if mask & 2 else np.isnan(sums).all()
            assert status.tobytes() == a.status.tobytes() if mask & 4 else (status == -1).all()
        # one fraction alone gives the bits it gives among others; a move within a smaller radius
        # gives the bits it gives within a larger one
        one = model.spr_scores(batch, radius=2, fractions=f[1:], per_site=True)
        assert one.values[:, :, 0].tobytes() == np.ascontiguousarray(a.values[:, :, 1]).tobytes()
        near = model.spr_scores(batch, radius=0, fractions=f, per_site=True)
        where = [a.moves.tolist().index(mv) for mv in near.moves.tolist()]
        assert near.values.tobytes() == np.ascontiguousarray(a.values[:, where]).tobytes()
        # the model and the batch are as they were
        assert model.get_transitions().tobytes() == esd.tobytes()
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert model.fetch_totals(batch).tobytes() == totals.tobytes()
        assert batch.kernel_name == name
        nni2 = model.nni_scores(batch, per_site=True)
        assert nni2.values.tobytes() == nni.values.tobytes()
        assert nni2.sums.tobytes() == nni.sums.tobytes()
        ll3, st3 = model.log_likelihoods(batch)
        assert ll3.tobytes() == ll.tobytes() and st3.tobytes() == st.tobytes()
    finally:
        ctx.close()


# ---- 9. refusals -----------------------------------------------------------------------------

def test_documented_refusals(ra):
    import _partition_cases as pc
    n, nsites = 20, 25
    case = make_case(n, 12, nsites, 'state', 9950, internal=False, per_edge=False)
    p_f64 = ctypes.POINTER(ctypes.c_double)
    L = ra.lib
    ctx = open_context(ra)
    try:
        model, batch = build(ra, ctx, case)
        ll, st = model.log_likelihoods(batch)
        name = batch.kernel_name
        good = model.spr_scores(batch, radius=1, fractions=(0.0, 0.5), per_site=True)
        default = model.spr_scores(batch)
        assert default.fractions.tolist() == [0.5]
        assert len(default.moves) == unlimited_count(model.tree.indices, model.tree.indptr)
        M = len(default.moves)

        def raw(fractions=(0.5,), nf=None, radius=-1, m=model, b=batch):
            f = None if fractions is None else np.array(fractions, dtype=np.float64)
            nf = (0 if f is None else len(f)) if nf is None else nf
            sums = np.zeros((M, max(nf, 1)))
            return L.lib().rt_sites_spr_scores(
                m._h, b._h, 0, radius, nf, None if f is None else f.ctypes.data_as(p_f64), None,
                sums.ctypes.data_as(p_f64), None)

        assert raw() == L.RT_OK
        assert raw(radius=0) == L.RT_OK and raw(radius=-5) == L.RT_OK
        # counts out of range
        assert raw(fractions=(0.5,), nf=0) == L.RT_ERR_INVALID
        assert raw(fractions=(0.5,) * 9) == L.RT_ERR_INVALID
        assert 'fractions' in L.last_error()
        assert raw(fractions=(0.5,) * 8) == L.RT_OK
        with pytest.raises(ValueError):
            model.spr_scores(batch, fractions=(0.5,) * 9)
        with pytest.raises(ValueError):
            model.spr_scores(batch, radius=-1)
        # a fraction outside [0, 1] or not finite
        for x in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
            assert raw(fractions=(0.5, x)) == L.RT_ERR_INVALID
            assert 'outside [0, 1] or not finite' in L.last_error()
        with pytest.raises(ValueError):
            model.spr_scores(batch, fractions=(1.5,))
        # NULL fractions
        assert raw(fractions=None, nf=1) == L.RT_ERR_INVALID
        # a batch of another model
        other = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(other, case)
        with pytest.raises(ValueError, match='another model'):
            other.spr_scores(batch)
        # no rates; transitions set directly after the rates
        direct = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        direct.set_transitions(model.get_transitions())
        direct.set_root_distn(case.root_distn)
        db = direct.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        with pytest.raises(ValueError, match='no rates have been set'):
            direct.spr_scores(db)
        assert raw(m=direct, b=db) == L.RT_ERR_INVALID
        after = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(after, case)
        after.set_root_distn(case.root_distn)
        after.set_transitions(model.get_transitions())
        ab = after.upload_sites(case.obs_nodes, case.data, kind=case.kind)
        assert raw(m=after, b=ab) == L.RT_ERR_INVALID
        assert 'set directly after the rates' in L.last_error()
        again = after.spr_scores(ab, radius=1, fractions=(0.0, 0.5), per_site=True,
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
                model.spr_scores(ob)
            assert err.value.code == L.RT_ERR_UNSUPPORTED, option
        # a tree deeper than the fast kernels take: 122 states and nine accumulator slots
        from raoteh_amd import synth
        T9, root9, leaves9 = synth.balanced_tree(512, seed=0)
        deep = ra.device.TreeModel(T9, root9, 122, ctx=ctx)
        assert deep.schedule_depth >= 9
        deep.set_rates(Q=make_case(122, 12, 2, 'dense', 1).Qs[:1],
                       node_q=np.zeros(deep.tree.nnodes, dtype=np.int64))
        deep_batch = deep.upload_sites(leaves9, np.ones((2, len(leaves9), 122)), kind='dense')
        with pytest.raises(L.RaotehHipError) as err:
            deep.spr_scores(deep_batch, radius=0)
        assert err.value.code == L.RT_ERR_UNSUPPORTED
        deep.close()
        # more than 96 GB of scratch: 2 047 nodes x 64 000 sites x 256 bytes x (L, M, up), refused
        # before anything is reserved; the batch is as it was
        Tb, rootb, leavesb = synth.balanced_tree(1024, seed=0)
        big = ra.device.TreeModel(Tb, rootb, n, ctx=ctx)
        big.set_rates(Q=case.Qs[:1], node_q=np.zeros(big.tree.nnodes, dtype=np.int64))
        big.set_root_distn(case.root_distn)
        bb = big.upload_sites(leavesb, np.ones((64000, len(leavesb)), dtype=np.uint8), kind='state')
        llb, stb = big.log_likelihoods(bb)
        nameb = bb.kernel_name
        with pytest.raises(L.RaotehHipError) as err:
            big.spr_scores(bb, radius=0)
        assert err.value.code == L.RT_ERR_UNSUPPORTED and 'GB of scratch' in str(err.value)
        llb2, stb2 = big.fetch_log_likelihoods(bb)
        assert llb2.tobytes() == llb.tobytes() and stb2.tobytes() == stb.tobytes()
        assert bb.kernel_name == nameb
        llb3, stb3 = big.log_likelihoods(bb)
        assert llb3.tobytes() == llb.tobytes() and stb3.tobytes() == stb.tobytes()
        big.close()
        assert model.spr_scores(batch, radius=1, fractions=(0.0, 0.5),
                                per_site=True).values.tobytes() == good.values.tobytes()
        # 2^31 (move, fraction) pairs: a star of 16 385 leaves has 16 385 x 16 384 moves; at 8
        # fractions that is 2^31 + 2^17 pairs; refused on the host, before any device work
        star = nx.Graph()
        for leaf in range(1, 16386):
            star.add_edge(0, leaf, weight=0.1)
        wide = ra.device.TreeModel(star, 0, n, ctx=ctx)
        wide.set_rates(Q=case.Qs[:1], node_q=np.zeros(16386, dtype=np.int64))
        wb = wide.upload_sites(list(range(1, 16386)), np.ones((2, 16385), dtype=np.uint8),
                               kind='state')
        assert raw(fractions=(0.5,) * 8, m=wide, b=wb) == L.RT_ERR_INVALID
        assert 'too many moves' in L.last_error()
        wide.close()
        # a partitioned batch
        pcase = pc.make_case(20, 'dense', seed=6)
        pmodel, pbatch = pc.upload(ra.device, ctx, pcase)
        pmodel.set_rates(Q=pcase.Q[0], node_q=pcase.node_q, t=pcase.t[0])
        with pytest.raises(L.RaotehHipError) as err:
            pmodel.spr_scores(pbatch)
        assert err.value.code == L.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
        # the batch is as it was, the context still works
        ll2, st2 = model.fetch_log_likelihoods(batch)
        assert ll2.tobytes() == ll.tobytes() and st2.tobytes() == st.tobytes()
        assert batch.kernel_name == name
        once_more = model.spr_scores(batch, radius=1, fractions=(0.0, 0.5), per_site=True)
        assert once_more.values.tobytes() == good.values.tobytes()
        assert once_more.sums.tobytes() == good.sums.tobytes()
    finally:
        ctx.close()


def test_trees_of_one_and_two_nodes(ra):
    """One node: refused.  Two nodes: no move, RT_OK and the status alone."""
    n = 20
    lone = nx.Graph()
    lone.add_node('r')
    pair = nx.Graph()
    pair.add_edge('r', 'a', weight=0.2)
    ctx = open_context(ra)
    try:
        single = ra.device.TreeModel(lone, 'r', n, ctx=ctx)
        single.set_transitions(np.zeros((1, n, n)))
        sb = single.upload_sites(['r'], np.ones((3, 1), dtype=np.uint8), kind='state')
        assert single.spr_moves().shape == (0, 2)
        with pytest.raises(ra.lib.RaotehHipError) as err:
            single.spr_scores(sb)
        assert err.value.code == ra.lib.RT_ERR_UNSUPPORTED
        case = make_case(n, 12, 3, 'state', 1, internal=False)
        two = ra.device.TreeModel(pair, 'r', n, ctx=ctx)
        two.set_rates(Q=case.Qs[:1], node_q=np.zeros(2, dtype=np.int64))
        tb = two.upload_sites(['a'], np.array([[1], [2], [0]], dtype=np.uint8), kind='state')
        got = two.spr_scores(tb, per_site=True)
        assert got.moves.shape == (0, 2) and got.sums.shape == (0, 1)
        assert got.values.shape == (3, 0, 1) and got.best is None
        _, st = two.log_likelihoods(tb)
        np.testing.assert_array_equal(got.status, st)
    finally:
        ctx.close()
