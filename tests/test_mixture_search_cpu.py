"""The host side of the tree-search reads under a site-class mixture (no GPU):
device.check_profile_factors, and the host reference of tests/_mixture_search_cases.py against the
single-set references and against the property the revival case is built for."""
import numpy as np
import pytest

import _mixture_cases as mc
import _mixture_search_cases as msc
import _nni_cases as nc
import _profile_cases as pfc
from oracle import oracle_numpy as orc


def test_check_profile_factors_accepts_the_documented_forms():
    from raoteh_amd import device, _lib
    f = device.check_profile_factors([0.5, 1.0, 2.0], 7)
    assert f.shape == (7, 3) and f.dtype == np.float64 and f.flags['C_CONTIGUOUS']
    assert np.array_equal(f[0], np.zeros(3))
    assert np.array_equal(f[1:], np.repeat([[0.5, 1.0, 2.0]], 6, axis=0))
    grid = np.arange(14, dtype=float).reshape(7, 2)
    g = device.check_profile_factors(grid, 7)
    assert g.shape == (7, 2) and g.flags['C_CONTIGUOUS'] and np.array_equal(g[1:], grid[1:])
    assert np.array_equal(g[0], np.zeros(2)) and grid[0, 1] == 1.0        # (a copy)
    # row 0 is ignored: anything may stand there
    grid[0] = np.nan
    assert np.array_equal(device.check_profile_factors(grid, 7)[0], np.zeros(2))
    # a non-contiguous view, integers, 0 and the largest G
    assert device.check_profile_factors(np.ones((7, 6))[:, ::2], 7).flags['C_CONTIGUOUS']
    assert device.check_profile_factors([0, 1], 3).dtype == np.float64
    assert device.check_profile_factors(np.ones(_lib.RT_MAX_PROFILE_POINTS), 4).shape == \
        (4, _lib.RT_MAX_PROFILE_POINTS)


@pytest.mark.parametrize('bad', [
    [], np.ones((7, 0)), np.ones((6, 2)), np.ones((8, 2)), np.ones((7, 2, 1)), 1.0, None, 'ab',
    [[1.0, 2.0], [1.0]], [1.0, -0.5], [1.0, np.nan], [np.inf], np.ones(65), np.ones((7, 65)),
    {1: [1.0]},
], ids=lambda b: repr(b)[:24].replace('\n', ' '))
def test_check_profile_factors_rejects_every_other(bad):
    from raoteh_amd import device
    with pytest.raises(ValueError):
        device.check_profile_factors(bad, 7)
    bad_row = np.ones((7, 2))
    bad_row[3, 1] = -1.0
    with pytest.raises(ValueError):
        device.check_profile_factors(bad_row, 7)


@pytest.mark.parametrize('n,tree,kind', [(4, 'balanced', 'state'), (5, 'random', 'dense')])
def test_one_set_is_the_single_set_reference(n, tree, kind):
    """K = 1, c = [1]: the mixture reference equals _profile_cases.profile_from_transitions and
    _nni_cases.nni_from_transitions at the lengths factors * t."""
    case = mc.make_case(n, tree, kind, 1, 7100 + n, nsites=21)
    ta = mc.tree_arrays(case)
    cols = [ta.node_to_index[v] for v in case.leaves]
    f = msc.make_factors(ta.nnodes, 3, 5)
    grid = f * case.t[0][:, None]
    esd = mc.set_transitions(ta, case, 0)
    w = msc.site_weights(21, 3)
    args = (ta.indices, ta.indptr, esd, cols, case.obs_lik, case.root_distn)
    want, wst, wll = pfc.profile_from_transitions(*args, case.Q[0], case.node_q, grid)
    got = msc.profile_reference(ta, case, [1.0], f, w)
    live = wst == 0
    assert np.array_equal(got.status, wst) and live.any()
    np.testing.assert_allclose(got.loglik[live], wll[live], rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.values, want, rtol=0, atol=1e-12)
    np.testing.assert_allclose(got.sums, np.einsum('i,ivg->vg', w[live], want[live]), rtol=0,
                               atol=1e-10)
    for fac, gr in ((None, None), (f, grid)):
        moves, want, wst, wll = nc.nni_from_transitions(*args, case.Q[0], case.node_q, gr)
        got = msc.nni_reference(ta, case, [1.0], fac, w)
        assert np.array_equal(got.moves, moves) and len(moves) > 0
        assert np.array_equal(got.status, wst)
        np.testing.assert_allclose(got.values, want, rtol=0, atol=1e-12)


def test_a_zero_length_edge_is_a_nan_row_of_the_profile_reference():
    case = mc.make_case(4, 'balanced', 'state', 2, 7200, zero_set=False, nsites=9)
    ta = mc.tree_arrays(case)
    case.t[1, 3] = 0.0
    ref = msc.profile_reference(ta, case, [0.5, 0.5], msc.make_factors(ta.nnodes, 2, 1))
    live = ref.status == 0
    assert live.any() and np.isnan(ref.values[live][:, 3]).all() and np.isnan(ref.sums[3]).all()
    assert np.isfinite(np.delete(ref.values[live], 3, axis=1)).all()
    # ... and not where that set's weight is zero
    ref = msc.profile_reference(ta, case, [1.0, 0.0], msc.make_factors(ta.nnodes, 2, 1))
    assert np.isfinite(ref.values).all() and np.isfinite(ref.sums).all()


@pytest.mark.parametrize('n', [3, 5])
def test_the_revival_case_has_its_property_under_the_oracle(n):
    """At the chosen site and move: L_ik == 0 on the resident tree under the one-way set with
    c_k > 0, L_ik > 0 under it on the moved tree, and Lambda_i > 0."""
    case, ta = msc.revival_case(n)
    moves = nc.brute_moves(ta.indices, ta.indptr)
    assert any(tuple(mv) == case.move for mv in moves)
    L, moved = msc.revival_likelihoods(case, ta)
    i = case.site
    assert L[0, i] == 0.0 and moved[0, i] > 0.0
    assert L[1, i] > 0.0 and moved[1, i] > 0.0
    c = np.array([0.6, 0.4])
    ref = msc.nni_reference(ta, case, c)
    j = [tuple(mv) for mv in ref.moves].index(case.move)
    assert ref.status[i] == 0 and np.isfinite(ref.loglik[i])
    want = np.log(c[0] * moved[0, i] + c[1] * moved[1, i]) - np.log(c[1] * L[1, i])
    assert np.isfinite(ref.values[i, j, 0]) and abs(ref.values[i, j, 0] - want) < 1e-12
    # what a per-set ratio could not give: the one-way set's term is most of the moved tree's
    assert c[0] * moved[0, i] > 0.1 * c[1] * moved[1, i]
    # the other site is an ordinary one under both sets
    assert (L[:, 1] > 0).all()


@pytest.mark.parametrize('n', [3, 5])
def test_the_lost_case_has_its_property_under_the_oracle(n):
    """A live site with likelihood 0 under every set after the move: -inf in the reference."""
    case, ta = msc.lost_case(n)
    L, moved = msc.revival_likelihoods(case, ta)
    i = case.site
    assert (L[:, i] > 0).all() and (moved[:, i] == 0).all()
    ref = msc.nni_reference(ta, case, [0.5, 0.5], msc.make_factors(ta.nnodes, 3, 11))
    j = [tuple(mv) for mv in ref.moves].index(case.move)
    assert ref.status[i] == 0 and np.isneginf(ref.values[i, j]).all() and np.isneginf(ref.sums[j]).all()
    assert np.isfinite(ref.values[1]).all()
