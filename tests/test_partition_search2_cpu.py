"""Host side of rt_sites_spr_scores_partitioned and rt_sites_placements_partitioned: the entry
points, their bindings and the Python surface exist; the Python-side argument checks; and the host
reference the GPU tests compare against (tests/_partition_search2_cases.py) -- equal to a
brute-force sum over every assignment of states on a few moved and placed trees, and fit for the
parity cases (no NaN, live sites in every set, -inf values of its own)."""
import re
import types

import numpy as np
import pytest

from conftest import ROOT
import _partition_search_cases as psc
import _partition_search2_cases as p2
import _place_cases as plc


def test_entry_points_are_declared_bound_and_surfaced():
    from raoteh_amd import _lib, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    for name, nargs in (('rt_sites_spr_scores_partitioned', 10), ('rt_sites_placements_partitioned', 15)):
        assert re.search(r'\bint %s\(' % name, header)
        restype, argtypes = _lib.SIGNATURES[name]
        assert len(argtypes) == nargs
        assert getattr(_lib.lib(), name) is not None
    assert callable(device.TreeModel.spr_scores_partitioned)
    assert callable(device.TreeModel.place_queries_partitioned)
    assert device.PartitionedSprScores._fields == (
        'moves', 'fractions', 'values', 'sums', 'set_sums', 'status', 'best')
    assert device.PartitionedPlacements._fields == (
        'fractions', 'pendant', 'pendant_scale', 'values', 'sums', 'set_sums', 'status', 'best')
    # nothing says the two reads are missing; the single-set and mixture reads still refuse
    assert 'not offered yet' not in header
    refusals = header[header.index('Everything else refuses a partitioned batch'):]
    for name in ('rt_sites_spr_scores,', 'rt_sites_placements and their _mixture forms'):
        assert name in refusals[:900]


def stand_in(N=7, nsets=3, t=None):
    from raoteh_amd import device
    args = device.TreeModel._partitioned_search_args
    model = types.SimpleNamespace(_nsets=nsets, nstates=4,
                                  tree=types.SimpleNamespace(nnodes=N, preorder_nodes=range(N)))
    model._partitioned_search_args = lambda b, who: args(model, b, who)
    model.spr_moves = lambda radius=None: np.zeros((0, 2), np.int32)
    if t is not None:
        model._rate_sets = (None, t)
    return model


def test_python_side_argument_checks():
    """What the wrappers refuse before the library is called (no device is touched: the model and
    the batches are stand-ins with the attributes the checks read; a call that got as far as the
    library would fail on the stand-in's missing handle with an AttributeError)."""
    from raoteh_amd import device
    S, n = 5, 4
    spr = device.TreeModel.spr_scores_partitioned
    place = device.TreeModel.place_queries_partitioned
    model = stand_in()
    part = types.SimpleNamespace(site_sets=np.zeros(S, int), nsets=3, nsites=S)
    plain = types.SimpleNamespace(site_sets=None, nsets=0, nsites=S)
    more = types.SimpleNamespace(site_sets=np.zeros(S, int), nsets=4, nsites=S)
    q = np.zeros((2, S), np.uint8)
    dense = np.ones((2, S, n))
    # an ordinary batch; too few rate sets, or none
    for batch, match in ((plain, 'site_sets'), (more, 'rate sets')):
        with pytest.raises(ValueError, match=match):
            spr(model, batch)
        with pytest.raises(ValueError, match=match):
            place(model, batch, q, kind='state')
    with pytest.raises(ValueError, match='set_rate_sets'):
        spr(stand_in(nsets=0), part)
    with pytest.raises(ValueError, match='set_rate_sets'):
        place(stand_in(nsets=0), part, q, kind='state')
    # fractions, the radius
    for bad in ([], [-0.1], [1.5], [np.nan], np.ones(33) * 0.5, 'x'):
        with pytest.raises(ValueError):
            spr(model, part, fractions=bad)
        with pytest.raises(ValueError):
            place(model, part, q, kind='state', fractions=bad, pendant=[0.1])
    for bad in (-1, 1.5, 'x'):
        with pytest.raises((ValueError, TypeError)):
            spr(model, part, radius=bad)
    # pendant lengths and scales
    for bad in ([], [-0.1], [np.inf], [np.nan], np.ones(33)):
        with pytest.raises(ValueError):
            place(model, part, q, kind='state', pendant=bad)
    for bad in ([1.0], [1.0, -1.0, 1.0], [1.0, np.nan, 1.0], np.ones((3, 1)), 'x'):
        with pytest.raises(ValueError):
            place(model, part, q, kind='state', pendant=[0.1], pendant_scale=bad)
    # mask queries, another kind, wrong shapes, no query
    with pytest.raises(ValueError, match="'dense' or 'state'"):
        place(model, part, q, kind='mask', pendant=[0.1])
    with pytest.raises(ValueError):
        place(model, part, q, kind='other', pendant=[0.1])
    for bad in (np.zeros((2, S + 1), np.uint8), np.zeros(S, np.uint8), np.zeros((0, S), np.uint8)):
        with pytest.raises(ValueError):
            place(model, part, bad, kind='state', pendant=[0.1])
    for bad in (np.ones((2, S, n + 1)), np.ones((2, S + 1, n)), np.ones((S, n)), np.ones((0, S, n))):
        with pytest.raises(ValueError):
            place(model, part, bad, kind='dense', pendant=[0.1])
    # good arguments reach the library (the stand-in has no handle)
    with pytest.raises(AttributeError):
        spr(model, part, fractions=[0.0, 1.0])
    t = np.arange(28, dtype=float).reshape(4, 7)
    with pytest.raises(AttributeError):
        place(stand_in(nsets=4, t=t), part, dense, pendant_scale=[1.0, 2.0, 0.0, 1.0])


def test_default_pendant_is_the_mean_length_of_the_batch_sets(monkeypatch):
    """pendant=None: mean(t[:nsets, 1:]) over the rate sets the batch uses."""
    from raoteh_amd import device
    S = 5
    t = np.arange(28, dtype=float).reshape(4, 7)
    part = types.SimpleNamespace(site_sets=np.zeros(S, int), nsets=3, nsites=S)
    seen = {}
    real = device.check_placement_grid

    def spy(fractions, pendant):
        seen['pendant'] = list(pendant)
        return real(fractions, pendant)
    monkeypatch.setattr(device, 'check_placement_grid', spy)
    with pytest.raises(AttributeError):
        device.TreeModel.place_queries_partitioned(stand_in(nsets=4, t=t), part,
                                                   np.zeros((1, S), np.uint8), kind='state')
    assert seen['pendant'] == [float(np.mean(t[:3, 1:]))]


def test_reference_against_brute_force():
    """n = 2 (2^8 and 2^9 assignments of the internal nodes of a moved and a placed tree), two live
    sites of one set and the planted sites of another: a few moves at three fractions, a few
    placements at three fractions and three scaled pendant lengths, state and dense queries."""
    case, ta, (lost0, lost1, v, k) = psc.cached_case(2, 'state', 'empty', p2.SEED)
    keep = 60
    case = case._replace(obs_lik=case.obs_lik[:keep], data=case.data[:keep],
                         site_sets=case.site_sets[:keep])
    assert lost0 < keep and lost1 < keep
    f, tau = p2.FRACTIONS[3], p2.PENDANT[3]
    scale = p2.case_scale(case.nsets, True)
    spr = p2.spr_reference(ta, case, f)
    assert len(spr.moves) == 156 and len(p2.spr_reference(ta, case, (0.5,), radius=1).moves) == 58
    checked = 0
    for s in (0, k):
        mine = np.flatnonzero((case.site_sets == s) & (spr.status == 0))
        sites = np.array([lost0, lost1]) if s == k else mine[:2]
        pick = [0, 7, 58, 101, 155]
        brute = p2.brute_spr(ta, case, s, sites, spr.moves[pick], f)
        got = spr.values[np.ix_(sites, pick)]
        assert np.array_equal(np.isneginf(got), np.isneginf(brute))
        fin = np.isfinite(brute)
        np.testing.assert_allclose(got[fin], brute[fin], rtol=0, atol=1e-12)
        checked += fin.sum()
        for qkind in ('state', 'dense'):
            q = p2.make_queries(case, 2, qkind, 6404)
            ref = p2.place_reference(ta, case, q, qkind, f, tau, scale)
            assert not ref.values[:, :, 0].any()
            nodes = [1, 6, ta.nnodes - 1]
            qlik = plc.query_likelihoods(q, qkind, case.n)[:, sites]
            brute = p2.brute_place(ta, case, s, sites, qlik, nodes, f, scale[s] * np.asarray(tau))
            got = ref.values[sites][:, :, nodes]
            assert np.array_equal(np.isneginf(got), np.isneginf(brute))
            fin = np.isfinite(brute)
            np.testing.assert_allclose(got[fin], brute[fin], rtol=0, atol=1e-12)
            checked += fin.sum()
    assert checked > 300


def test_reference_sums_and_weights():
    """set_sums are the weighted sums of the set's live sites of non-zero weight, zeros for the
    empty set, sums their sum in set order; a -inf of weight 0 adds nothing."""
    case, ta, (lost0, lost1, v, k) = psc.cached_case(2, 'state', 'empty', p2.SEED)
    w = p2.case_weights(case, (lost0, lost1), p2.SEED, True)
    ref = p2.spr_reference(ta, case, p2.FRACTIONS[3], radius=1, weights=w)
    assert not ref.set_sums[3].any()
    np.testing.assert_array_equal(ref.sums, ref.set_sums.sum(axis=0))
    use = (case.site_sets == 0) & (w != 0) & (ref.status == 0)
    with np.errstate(invalid='ignore'):
        want = np.einsum('i,imr->mr', w[use], ref.values[use])
    fin = np.isfinite(want)
    np.testing.assert_allclose(ref.set_sums[0][fin], want[fin], rtol=1e-13)
    rows = np.isneginf(ref.values[lost1])
    assert rows.any() and np.isneginf(ref.set_sums[k][rows]).all() and np.isneginf(ref.sums[rows]).all()
    # (other sites of the planted set share the lost sites' -inf: all of them at weight 0)
    row = tuple(np.argwhere(rows)[0])
    w2 = w.copy()
    w2[np.isneginf(ref.values[(slice(None),) + row])] = 0.0
    quiet = p2.spr_reference(ta, case, p2.FRACTIONS[3], radius=1, weights=w2)
    assert (w2[case.site_sets == k] != 0).any() and np.isfinite(quiet.set_sums[k][row])
    assert np.isfinite(quiet.sums[row])


@pytest.mark.parametrize('row', p2.PARITY, ids=p2.PARITY_IDS)
def test_the_parity_cases_fit(row):
    """What the GPU parity cases ask of their references: no NaN, at least 2 live sites in every
    set with a site, and -inf values among the live sites (every SPR case has them, from the
    identity edges of the planted set at fractions 0 and 1 or from the move itself; the placement
    cases with state queries have them)."""
    n, kind, sets, qkind, radius, nf, npend, scaled, weighted = row
    case, ta, special, f, w, ref = p2.cached_spr_reference(n, kind, sets, radius, nf, weighted)
    assert len(case.site_sets) == (len(psc.runs_site_sets(n, 0)) if sets == 'runs'
                                   else 3 * psc.pc.granule(n) + 5)
    assert len(ref.moves) == (58 if radius == 1 else 156)
    assert p2.check_reference(case, ref)
    ref = p2.cached_place_reference(n, kind, sets, qkind, nf, npend, scaled, weighted)[-1]
    assert p2.check_reference(case, ref) == (qkind == 'state')
