"""Host side of rt_sites_branch_profiles_partitioned and rt_sites_nni_scores_partitioned: the entry
points, their bindings and the Python surface exist; the Python-side argument checks; and the host
reference the GPU tests compare against (tests/_partition_search_cases.py) -- equal to a brute-force
sum over every assignment of states on a few sites of every set, equal to the single-set references
for one rate set, consistent in its sums, its NaN rule and its planted -inf sites."""
import re
import types

import numpy as np
import pytest

from conftest import ROOT
import _nni_cases as nc
import _partition_cases as pc
import _partition_search_cases as psc
import _profile_cases as pfc


def test_entry_points_are_declared_bound_and_surfaced():
    from raoteh_amd import _lib, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    for name in ('rt_sites_branch_profiles_partitioned', 'rt_sites_nni_scores_partitioned'):
        assert re.search(r'\bint %s\(' % name, header)
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == 9
        assert getattr(_lib.lib(), name) is not None
    assert callable(device.TreeModel.branch_profiles_partitioned)
    assert callable(device.TreeModel.nni_scores_partitioned)
    assert device.PartitionedBranchProfiles._fields == (
        'factors', 'values', 'sums', 'set_sums', 'status', 'nodes')
    assert device.PartitionedNniScores._fields == (
        'moves', 'factors', 'values', 'sums', 'set_sums', 'status')
    # the single-set and mixture reads are still listed as refusing a partitioned batch
    refusals = header[header.index('Everything else refuses a partitioned batch'):]
    for name in ('rt_sites_branch_profiles,', 'rt_sites_branch_profiles_mixture,',
                 'rt_sites_nni_scores_mixture,', 'rt_sites_nni_scores,'):
        assert name in refusals[:900]


def test_python_side_argument_checks():
    """What the wrappers refuse before the library is called (no device is touched: the model and
    the batches are stand-ins with the attributes the checks read)."""
    from raoteh_amd import device
    N = 7
    model = types.SimpleNamespace(_nsets=3, tree=types.SimpleNamespace(nnodes=N, preorder_nodes=range(N)))
    args = device.TreeModel._partitioned_search_args
    part = types.SimpleNamespace(site_sets=np.zeros(5, int), nsets=3, nsites=5)
    assert args(model, part, 'branch_profiles_partitioned') == 3
    plain = types.SimpleNamespace(site_sets=None, nsets=0, nsites=5)
    with pytest.raises(ValueError, match='site_sets'):
        args(model, plain, 'nni_scores_partitioned')
    with pytest.raises(ValueError, match='rate sets'):
        args(model, types.SimpleNamespace(site_sets=np.zeros(5, int), nsets=4, nsites=5),
             'nni_scores_partitioned')
    with pytest.raises(ValueError, match='set_rate_sets'):
        args(types.SimpleNamespace(_nsets=0), part, 'branch_profiles_partitioned')
    # both wrappers make that check, and the factors' check, before anything else
    for call in (device.TreeModel.branch_profiles_partitioned, device.TreeModel.nni_scores_partitioned):
        stand_in = types.SimpleNamespace(
            _nsets=3, tree=model.tree, nni_moves=lambda: np.zeros((0, 3), np.int32),
            _partitioned_search_args=lambda b, who: args(model, b, who))
        with pytest.raises(ValueError, match='site_sets'):
            call(stand_in, plain, [1.0])
        for bad in ([], np.ones(65), [-1.0], [np.nan], [np.inf], np.ones((N - 1, 2)), np.ones((N, 0)),
                    np.ones((2, N, 2)), 'x'):
            with pytest.raises(ValueError):
                call(stand_in, part, bad)
    f = device.check_profile_factors([0.5, 1.0], N)
    assert f.shape == (N, 2) and not f[0].any() and (f[1:] == [0.5, 1.0]).all()
    np.testing.assert_array_equal(psc.device_factors([0.5, 1.0], N), f)


def test_reference_against_brute_force():
    """n = 3 (3^7 assignments of the seven internal nodes), two sites of every set, the planted
    -inf sites among them: profile values and NNI values, with factors and for the plain swap."""
    case, ta, (lost0, lost1, v, k) = psc.cached_case(3, 'state', 'empty', 6100)
    case = case._replace(obs_lik=case.obs_lik[:60], data=case.data[:60],
                         site_sets=case.site_sets[:60])
    assert lost0 < 60 and lost1 < 60
    f = psc.make_factors(ta.nnodes, 3, 6101)
    prof = psc.profile_reference(ta, case, f)
    nni = psc.nni_reference(ta, case, f)
    swap = psc.nni_reference(ta, case)
    assert np.isneginf(prof.values[lost1, v, 1]) and prof.status[lost1] == 0
    checked = 0
    for s in range(case.nsets):
        mine = np.flatnonzero((case.site_sets == s) & (prof.status == 0))
        if s == k:
            mine = np.array([lost0, lost1])
        sites = mine[:2]
        if not len(sites):
            continue
        for ref, brute in ((prof, psc.brute_profile(ta, case, s, sites, f)),
                           (nni, psc.brute_nni(ta, case, s, sites, f)),
                           (swap, psc.brute_nni(ta, case, s, sites))):
            got = ref.values[sites]
            assert np.array_equal(np.isneginf(got), np.isneginf(brute))
            fin = np.isfinite(brute)
            np.testing.assert_allclose(got[fin], brute[fin], rtol=0, atol=1e-12)
            checked += fin.sum()
    assert checked > 300


@pytest.mark.parametrize('n,kind', [(4, 'state'), (5, 'dense')])
def test_one_set_is_the_single_set_reference(n, kind):
    """nsets = 1: what profile_from_transitions / nni_from_transitions give for that one rate set
    on all sites at once."""
    case = pc.make_case(n, kind, seed=6200 + n, nsets=1, nsites=21, site_sets=np.zeros(21, int))
    ta = psc.tree_arrays(case)
    f = psc.make_factors(ta.nnodes, 2, 6200)
    cols = [ta.node_to_index[x] for x in case.leaves]
    esd = psc.set_transitions(ta, case, 0)
    w = np.random.RandomState(n).uniform(0.5, 2.0, 21)
    want, wst, wll = pfc.profile_from_transitions(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                                  case.root_distn, case.Q[0], case.node_q,
                                                  f * case.t[0][:, None])
    ref = psc.profile_reference(ta, case, f, w)
    np.testing.assert_array_equal(ref.values, want)
    np.testing.assert_array_equal(ref.status, wst)
    np.testing.assert_array_equal(ref.loglik, wll)
    assert ref.set_sums.shape == (1, ta.nnodes, 2)
    np.testing.assert_allclose(ref.sums, np.einsum('i,ivg->vg', w, want), rtol=1e-13)
    moves, want, wst, _ = nc.nni_from_transitions(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                                  case.root_distn, case.Q[0], case.node_q,
                                                  f * case.t[0][:, None])
    ref = psc.nni_reference(ta, case, f, w)
    np.testing.assert_array_equal(ref.moves, moves)
    np.testing.assert_array_equal(ref.values, want)
    np.testing.assert_allclose(ref.sums, np.einsum('i,img->mg', w, want), rtol=1e-13)


def test_reference_sums_empty_set_dead_sites_weights_and_nan_rule():
    n = 4
    case, ta, (lost0, lost1, v, k) = psc.cached_case(n, 'state', 'zero', 6300)
    sub = slice(0, 90)
    case = case._replace(obs_lik=case.obs_lik[sub], data=case.data[sub], site_sets=case.site_sets[sub])
    S = 90
    f = psc.make_factors(ta.nnodes, 3, 6301)
    w = psc.site_weights(S, 6302)
    w[lost0], w[lost1] = 0.0, 1.0
    ref = psc.profile_reference(ta, case, f, w)
    # set 3 is empty, set 1 has Q = 0: its sites with differing leaves are dead
    assert not ref.set_sums[3].any()
    differ = (case.data != case.data[:, :1]).any(axis=1)
    in1 = case.site_sets == 1
    np.testing.assert_array_equal(ref.status[in1], differ[in1].astype(np.int32))
    assert not ref.values[ref.status != 0].any()
    # the lost sites: -inf at the collapsed edge; weight 0 adds nothing, weight 1 makes the sum -inf
    assert np.isneginf(ref.values[[lost0, lost1], v, 1]).all()
    assert np.isneginf(ref.set_sums[k, v, 1]) and np.isneginf(ref.sums[v, 1])
    assert not np.isnan(ref.set_sums).any()
    w2 = w.copy()
    w2[lost1] = 0.0
    quiet = psc.profile_reference(ta, case, f, w2)
    others = (case.site_sets == k) & (w2 != 0) & (ref.status == 0)
    if np.isfinite(ref.values[others, v, 1]).all():
        assert np.isfinite(quiet.set_sums[k, v, 1])
    np.testing.assert_array_equal(ref.sums, ref.set_sums.sum(axis=0))
    # weights: a set's row is the weighted sum of its live sites
    use = (case.site_sets == 0) & (w != 0) & (ref.status == 0)
    np.testing.assert_allclose(ref.set_sums[0], np.einsum('i,ivg->vg', w[use], ref.values[use]),
                               rtol=1e-13)
    # the NaN rule: t[0][v0] = 0
    t = case.t.copy()
    t[0, 3] = 0.0
    nan = psc.profile_reference(ta, case._replace(t=t), f, w)
    in0 = (case.site_sets == 0) & (nan.status == 0)
    assert np.isnan(nan.values[in0, 3]).all() and not np.isnan(nan.values[~in0]).any()
    assert np.isnan(nan.set_sums[0, 3]).all() and np.isnan(nan.sums[3]).all()
    assert np.isnan(nan.set_sums).sum() == 3 and np.isnan(nan.sums).sum() == 3
    assert not np.isnan(psc.nni_reference(ta, case._replace(t=t), f, w).values).any()
