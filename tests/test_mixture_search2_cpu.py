"""The host side of spr_scores_mixture and place_queries_mixture (no GPU):
device.check_pendant_scale, and the host reference of tests/_mixture_search2_cases.py against the
single-set references and against the properties the revival and the lost cases are built for."""
import numpy as np
import pytest

import _mixture_cases as mc
import _mixture_search_cases as msc
import _mixture_search2_cases as m2
import _place_cases as plc
import _spr_cases as sc


def test_check_pendant_scale_accepts_the_documented_forms():
    from raoteh_amd import device
    ones = device.check_pendant_scale(None, 3)
    assert ones.dtype == np.float64 and np.array_equal(ones, np.ones(3))
    s = device.check_pendant_scale([0.5, 1, 2.25], 3)
    assert s.dtype == np.float64 and s.flags['C_CONTIGUOUS'] and np.array_equal(s, [0.5, 1.0, 2.25])
    assert np.array_equal(device.check_pendant_scale(np.arange(8.0)[::2], 4), [0.0, 2.0, 4.0, 6.0])
    assert device.check_pendant_scale(np.arange(8.0)[::2], 4).flags['C_CONTIGUOUS']
    assert np.array_equal(device.check_pendant_scale((0.0,), 1), [0.0])      # (0 is allowed)
    given = np.array([1.0, 3.0])
    out = device.check_pendant_scale(given, 2)
    assert np.array_equal(out, given)


@pytest.mark.parametrize('bad', [
    [], [1.0], [1.0, 2.0], [1.0, 2.0, 3.0, 4.0], np.ones((3, 1)), np.ones((1, 3)), 1.0, 'abc',
    [1.0, -0.5, 1.0], [1.0, np.nan, 1.0], [np.inf, 1.0, 1.0], [-np.inf, 1.0, 1.0],
    [[1.0, 2.0], [1.0]], {0: 1.0},
], ids=lambda b: repr(b)[:24].replace('\n', ' '))
def test_check_pendant_scale_rejects_every_other(bad):
    from raoteh_amd import device
    with pytest.raises(ValueError):
        device.check_pendant_scale(bad, 3)


@pytest.mark.parametrize('n,tree,kind', [(4, 'balanced', 'state'), (5, 'random', 'dense')])
def test_one_set_is_the_single_set_reference(n, tree, kind):
    """K = 1, c = [1]: the mixture references equal _spr_cases.spr_from_transitions and
    _place_cases.place_from_transitions on the set's own matrices."""
    case = mc.make_case(n, tree, kind, 1, 7300 + n, nsites=21)
    ta = mc.tree_arrays(case)
    cols = [ta.node_to_index[v] for v in case.leaves]
    esd = mc.set_transitions(ta, case, 0)
    w = msc.site_weights(21, 3)
    args = (ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn, case.t[0])
    f = m2.FRACTIONS[3]
    for radius in (1, None):
        moves, want, wst, wll = sc.spr_from_transitions(*args, f, radius, case.Q[0], case.node_q)
        got = m2.spr_reference(ta, case, [1.0], f, radius, w)
        live = wst == 0
        assert np.array_equal(got.moves, moves) and len(moves) > 0 and live.any()
        assert np.array_equal(got.status, wst)
        np.testing.assert_allclose(got.loglik[live], wll[live], rtol=0, atol=1e-12)
        assert np.array_equal(np.isneginf(got.values), np.isneginf(want))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got.values[fin], want[fin], rtol=0, atol=1e-12)
    tau = m2.PENDANT[3]
    for qkind in ('dense', 'state'):
        q = m2.make_queries(case, 2, qkind, 9)
        qlik = plc.query_likelihoods(q, qkind, n)
        want, wst, wll = plc.place_from_transitions(*args, qlik, f, tau, case.Q[0], case.node_q)
        got = m2.place_reference(ta, case, [1.0], q, qkind, f, tau, None, w)
        live = wst == 0
        assert np.array_equal(got.status, wst) and got.values.shape == want.shape
        assert (got.values[:, :, 0] == 0).all() and (got.sums[:, 0] == 0).all()
        assert np.array_equal(np.isneginf(got.values), np.isneginf(want))
        fin = np.isfinite(want)
        np.testing.assert_allclose(got.values[fin], want[fin], rtol=0, atol=1e-12)
        if fin.all():
            np.testing.assert_allclose(got.sums, np.einsum('i,iqvrk->qvrk', w[live], want[live]),
                                       rtol=0, atol=1e-10)
        # a scale of 2 is the pendant lengths doubled
        twice = m2.place_reference(ta, case, [1.0], q, qkind, f, tau, [2.0], w)
        want2, _, _ = plc.place_from_transitions(*args, qlik, f, [2 * x for x in tau], case.Q[0],
                                                 case.node_q)
        fin = np.isfinite(want2)
        np.testing.assert_allclose(twice.values[fin], want2[fin], rtol=0, atol=1e-12)


@pytest.mark.parametrize('n', [3, 5])
def test_the_spr_revival_case_has_its_property_under_the_oracle(n):
    """Prune c, regraft above s: L_i0 == 0 before and > 0 after under the one-way set."""
    case, ta = msc.revival_case(n)
    move = m2.revival_move(ta)
    moves = sc.brute_moves(ta.indices, ta.indptr, 1)
    assert any(tuple(mv) == move for mv in moves)
    L, moved = m2.spr_move_likelihoods(case, ta, move, 0.5)
    i = case.site
    assert L[0, i] == 0.0 and moved[0, i] > 0.0
    assert L[1, i] > 0.0 and moved[1, i] > 0.0
    c = np.array([0.6, 0.4])
    ref = m2.spr_reference(ta, case, c, (0.5,), 1)
    j = [tuple(mv) for mv in ref.moves].index(move)
    assert ref.status[i] == 0 and np.isfinite(ref.loglik[i])
    want = np.log(c[0] * moved[0, i] + c[1] * moved[1, i]) - np.log(c[1] * L[1, i])
    assert np.isfinite(ref.values[i, j, 0]) and abs(ref.values[i, j, 0] - want) < 1e-12
    # what a per-set ratio could not give: the one-way set's term counts on the moved tree
    alone = np.log(c[1] * moved[1, i]) - np.log(c[1] * L[1, i])
    assert abs(ref.values[i, j, 0] - alone) > 1e-3
    assert (L[:, 1] > 0).all()


@pytest.mark.parametrize('n', [3, 5])
def test_the_lost_cases_give_minus_infinity_in_the_reference(n):
    """The move of lost_case as an SPR move, and a state query that no set can reach below the
    cut edge: a live site, likelihood 0 under every set after the change."""
    case, ta = msc.lost_case(n)
    move = m2.lost_move(ta)
    i = case.site
    for rho in (0.0, 0.5, 1.0):
        L, moved = m2.spr_move_likelihoods(case, ta, move, rho)
        assert (L[:, i] > 0).all() and (moved[:, i] == 0).all()
    ref = m2.spr_reference(ta, case, [0.5, 0.5], m2.FRACTIONS[3])
    j = [tuple(mv) for mv in ref.moves].index(move)
    assert ref.status[i] == 0 and np.isneginf(ref.values[i, j]).all() and np.isneginf(ref.sums[j]).all()
    assert np.isfinite(ref.values[1]).all()
    # the query: state 0 at the site, placed above c -- below v, which is observed in state 1
    q = np.array([[0, 2]], dtype=np.uint8)
    below_v = ta.node_to_index[3]
    ref = m2.place_reference(ta, case, [0.5, 0.5], q, 'state', m2.FRACTIONS[3], m2.PENDANT[3])
    assert ref.status[i] == 0
    assert np.isneginf(ref.values[i, 0, below_v]).all() and np.isneginf(ref.sums[0, below_v]).all()
    assert np.isfinite(ref.values[1]).all() and (ref.values[:, :, 0] == 0).all()
