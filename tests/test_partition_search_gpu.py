"""rt_sites_branch_profiles_partitioned and rt_sites_nni_scores_partitioned
(TreeModel.branch_profiles_partitioned / nni_scores_partitioned) on the GPU: per-branch likelihood
profiles and the scores of every NNI neighbour of a partitioned batch, every site under its own
rate set.  Against the host reference that no device path enters
(tests/_partition_search_cases.py); bit for bit against the ordinary calls on each set's sites;
the NaN rule per set; repeatability, every output alone, chunks of moves, side effects, both
granules of the lane kernel; the documented refusals; the example.

On the -inf cases: the sites lost0 (weight 0) and lost1 (weight 1) of
_partition_search_cases.plant_lost_sites are alive on the resident tree and have likelihood exactly
0 where an edge is collapsed (factor 0) -- every profile case with three or more points holds
them.  An NNI move can strand them too (the identity edges move with their subtrees); where the
reference has such a -inf the device must have it."""
import ctypes
import os
import re
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
import _partition_cases as pc
import _partition_search_cases as psc
import _profile_cases as pfc
import _step_multi_cases as smc

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
TOL = 1e-10                                      # the project's tolerance for log-likelihoods


@pytest.fixture(scope='module')
def contexts():
    from raoteh_amd import device
    made = {}

    def get(**opts):
        key = tuple(sorted(opts.items()))
        if key not in made:
            ctx = device.Context(0)
            for k, v in dict(DEFAULTS, **opts).items():
                ctx.set_option(k, v)
            made[key] = ctx
        return made[key]
    yield get
    made.clear()


def build(contexts, case, weights=None):
    from raoteh_amd import device
    model, batch = pc.upload(device, contexts(), case)
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


def release(*things):
    for x in things:
        x.close()


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(smc.bits(a), smc.bits(b))


def close_to(got, want, bound, label):
    """NaN and -inf where the reference has them, and nowhere else; the rest within `bound`
    (broadcast against the arrays)."""
    assert got.shape == want.shape, label
    assert np.array_equal(np.isnan(got), np.isnan(want)), label + ': NaN pattern'
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), label + ': -inf pattern'
    assert not np.isposinf(got).any(), label
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    print('%s: max |got - ref| / bound %.3g' % (label, float((err / bound).max())))
    assert (err <= bound).all(), label


def check_against(got, ref, case, w, label):
    """site_bounds with the project's 1e-10: tol max(1, |log L_i|) per site, tol max(1, sum_i w_i
    |log L_i|) per sum -- the sum of a set over that set's sites."""
    S = len(case.site_sets)
    per_site, per_sum = pfc.site_bounds(ref.loglik, w, tol=TOL)
    ww = np.ones(S) if w is None else w
    np.testing.assert_array_equal(got.status, ref.status)
    close_to(got.values, ref.values, per_site[:, None, None], label + ' values')
    per_set = np.array([pfc.site_bounds(ref.loglik[case.site_sets == k], ww[case.site_sets == k],
                                        tol=TOL)[1] for k in range(case.nsets)])
    close_to(got.set_sums, ref.set_sums, per_set[:, None, None], label + ' set sums')
    close_to(got.sums, ref.sums, per_sum, label + ' sums')
    dead = ref.status != 0
    assert not got.values[dead].any()
    for k in range(case.nsets):
        if not (case.site_sets == k).any():
            assert not got.set_sums[k].any() and not np.signbit(got.set_sums[k]).any()   # exactly 0


# ---- 1. against the host reference ---------------------------------------------------------

# the lane kernel at 2 and 4 states, one wave, the split-M family at two and four tiles of states,
# 122 states with two sets; every upload kind; 1, 3 and 9 points (nine crosses BP_CHUNK = 8; from
# three on one factor is 0 and one is 1), NNI also the plain swap (0); 'empty' = site i in set
# i % 3 of 4, 'runs' = a random order of runs that do not end on a granule, 'zero' = Q = 0 in set
# 1, 'two' = two sets
PARITY = [
    # n, kind, sets, points, weights
    (2, 'state', 'empty', 1, False),
    (4, 'dense', 'runs', 3, True),
    (4, 'mask', 'zero', 9, True),
    (5, 'dense', 'empty', 3, True),
    (20, 'mask', 'runs', 9, True),
    (20, 'state', 'zero', 1, False),
    (61, 'state', 'zero', 3, True),
    (61, 'dense', 'runs', 9, False),
    (122, 'state', 'two', 2, True),
]
PARITY_IDS = ['n%d-%s-%s-g%d%s' % (c[0], c[1], c[2], c[3], '-w' if c[4] else '') for c in PARITY]


def parity(call, contexts, n, kind, sets, npoints, weighted):
    case, ta, special, f, w, ref = psc.cached_reference(call, n, kind, sets, 7000 + n, npoints, weighted)
    S = len(case.site_sets)
    assert S == (len(psc.runs_site_sets(n, 0)) if sets == 'runs' else 3 * pc.granule(n) + 5)
    model, batch = build(contexts, case, w)
    try:
        if call == 'profile':
            got = model.branch_profiles_partitioned(batch, f, per_site=True)
            assert got.nodes == list(ta.preorder_nodes) and same_bits(got.factors, f)
            assert got.values.shape == (S, ta.nnodes, npoints)
            assert not got.values[:, 0].any() and not got.sums[0].any()
            sums_only = model.branch_profiles_partitioned(batch, f)
        else:
            got = model.nni_scores_partitioned(batch, f, per_site=True)
            np.testing.assert_array_equal(got.moves, ref.moves)
            assert got.values.shape == (S, len(ref.moves), max(npoints, 1))
            assert not np.isnan(got.values).any()
            sums_only = model.nni_scores_partitioned(batch, f)
        label = '%s n=%d %s %s g=%d' % (call, n, kind, sets, npoints)
        check_against(got, ref, case, w, label)
        assert sums_only.values is None
        assert same_bits(sums_only.sums, got.sums) and same_bits(sums_only.set_sums, got.set_sums)
        assert np.array_equal(sums_only.status, got.status)
        # what the case is there for
        lost0, lost1, v, lk = special
        assert got.status[lost0] == 0 and got.status[lost1] == 0
        if call == 'profile' and npoints >= 3:
            assert np.isneginf(got.values[lost0, v, 1]) and np.isneginf(got.values[lost1, v, 1])
            assert np.isneginf(got.set_sums[lk, v, 1]) and np.isneginf(got.sums[v, 1])
        if kind != 'dense':
            assert (got.status[case.site_sets == lk] != 0).any()      # dead under its set
    finally:
        release(batch, model)


@pytest.mark.parametrize('n,kind,sets,npoints,weighted', PARITY, ids=PARITY_IDS)
def test_profiles_against_the_host_reference(contexts, n, kind, sets, npoints, weighted):
    parity('profile', contexts, n, kind, sets, npoints, weighted)


NNI_PARITY = PARITY + [(4, 'state', 'runs', 0, True), (20, 'dense', 'empty', 0, True),
                       (61, 'mask', 'empty', 0, False)]
NNI_IDS = ['n%d-%s-%s-g%d%s' % (c[0], c[1], c[2], c[3], '-w' if c[4] else '') for c in NNI_PARITY]


@pytest.mark.parametrize('n,kind,sets,npoints,weighted', NNI_PARITY, ids=NNI_IDS)
def test_nni_scores_against_the_host_reference(contexts, n, kind, sets, npoints, weighted):
    parity('nni', contexts, n, kind, sets, npoints, weighted)


# ---- 2. bit for bit against the ordinary calls ---------------------------------------------

@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense'), (61, 'state')])
def test_bit_for_bit_against_the_ordinary_calls(contexts, n, kind):
    """Set k's sites as an ordinary batch under set_rates(Q[k], node_q, t[k]) with lengths =
    factors * t[k], one f64 product per entry: the same arithmetic per site column and per edge,
    the exponential's variant chosen by one set's count -- a difference is a wrong table or
    slot."""
    from raoteh_amd import device
    case, ta, _ = psc.cached_case(n, kind, 'empty', 7100 + n)
    f = psc.make_factors(ta.nnodes, 3, 7100 + n)
    model, batch = build(contexts, case)
    prof = model.branch_profiles_partitioned(batch, f, per_site=True)
    nni = model.nni_scores_partitioned(batch, f, per_site=True)
    swap = model.nni_scores_partitioned(batch, per_site=True)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        om = device.TreeModel(case.T, case.root, n, ctx=contexts())
        om.set_root_distn(case.root_distn)
        om.set_rates(Q=case.Q[k], node_q=case.node_q, t=case.t[k])
        ob = om.upload_sites(case.leaves, case.data[mine], kind=kind)
        lengths = f * case.t[k][:, None]
        want = om.branch_profiles(ob, lengths=lengths, per_site=True)
        assert same_bits(np.ascontiguousarray(prof.values[mine]), want.values), k
        assert np.array_equal(prof.status[mine], want.status), k
        want = om.nni_scores(ob, lengths=lengths, per_site=True)
        assert same_bits(np.ascontiguousarray(nni.values[mine]), want.values), k
        assert np.array_equal(nni.status[mine], want.status), k
        want = om.nni_scores(ob, per_site=True)
        assert same_bits(np.ascontiguousarray(swap.values[mine]), want.values), k
        release(ob, om)
    release(batch, model)


# ---- 3. the NaN rule -----------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_nan_rule_per_set(contexts, n):
    """t[1][v0] = 0 on one internal, non-root edge (one with moves about it)."""
    case = pc.make_case(n, 'dense', 7200 + n)
    ta = psc.tree_arrays(case)
    kids = np.diff(ta.indptr)
    v0 = int(np.flatnonzero(kids[1:] > 0)[0]) + 1
    t = case.t.copy()
    t[1, v0] = 0.0
    case = case._replace(t=t)
    f = np.array([0.5, 1.0, 2.0])
    w = psc.site_weights(len(case.site_sets), 3)
    model, batch = build(contexts, case, w)
    prof = model.branch_profiles_partitioned(batch, f, per_site=True)
    in1 = case.site_sets == 1
    live = prof.status == 0
    assert live[in1].sum() > 10
    nan = np.isnan(prof.values)
    want = np.zeros_like(nan)
    want[np.ix_(in1 & live, [v0])] = True
    assert np.array_equal(nan, want)
    assert np.isfinite(prof.values[~nan]).all()
    nan = np.isnan(prof.set_sums)
    want = np.zeros_like(nan)
    want[1, v0] = True
    assert np.array_equal(nan, want) and np.isfinite(prof.set_sums[~nan]).all()
    assert np.isnan(prof.sums[v0]).all() and np.isfinite(np.delete(prof.sums, v0, axis=0)).all()
    ref = psc.profile_reference(ta, case, psc.device_factors(f, ta.nnodes), w)
    check_against(prof, ref, case, w, 'n=%d profile, t[1][%d] = 0' % (n, v0))
    nni = model.nni_scores_partitioned(batch, f, per_site=True)
    assert (nni.moves[:, 0] == v0).any()
    for a in (nni.values, nni.set_sums, nni.sums):
        assert not np.isnan(a).any()
    ref = psc.nni_reference(ta, case, psc.device_factors(f, ta.nnodes), w)
    check_against(nni, ref, case, w, 'n=%d nni, t[1][%d] = 0' % (n, v0))
    release(batch, model)


# ---- 4. determinism and isolation ----------------------------------------------------------

P_F64 = ctypes.POINTER(ctypes.c_double)
P_I32 = ctypes.POINTER(ctypes.c_int32)


def raw(name, model, batch, npoints, factors, values=None, sums=None, set_sums=None, status=None):
    from raoteh_amd import _lib

    def ptr(a, t):
        return None if a is None else a.ctypes.data_as(t)
    return getattr(_lib.lib(), name)(model._h, batch._h, 0, npoints, ptr(factors, P_F64),
                                     ptr(values, P_F64), ptr(sums, P_F64), ptr(set_sums, P_F64),
                                     ptr(status, P_I32))


@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'mask'), (61, 'dense')])
def test_two_calls_and_every_output_alone(contexts, n, kind):
    from raoteh_amd import _lib
    case, ta, _ = psc.cached_case(n, kind, 'runs', 7300 + n)
    f = psc.make_factors(ta.nnodes, 9, 7300 + n)
    w = psc.site_weights(len(case.site_sets), 4)
    model, batch = build(contexts, case, w)
    S = len(case.site_sets)
    for name, call, rows in (
            ('rt_sites_branch_profiles_partitioned', model.branch_profiles_partitioned, ta.nnodes),
            ('rt_sites_nni_scores_partitioned', model.nni_scores_partitioned, len(model.nni_moves()))):
        a = call(batch, f, per_site=True)
        b = call(batch, f, per_site=True)
        for x, y in ((a.values, b.values), (a.sums, b.sums), (a.set_sums, b.set_sums)):
            assert same_bits(x, y)
        assert np.array_equal(a.status, b.status)
        values = np.full((S, rows, 9), 7.0)
        assert raw(name, model, batch, 9, f, values=values) == _lib.RT_OK
        assert same_bits(values, a.values)
        sums = np.full((rows, 9), 7.0)
        assert raw(name, model, batch, 9, f, sums=sums) == _lib.RT_OK
        assert same_bits(sums, a.sums)
        set_sums = np.full((case.nsets, rows, 9), 7.0)
        assert raw(name, model, batch, 9, f, set_sums=set_sums) == _lib.RT_OK
        assert same_bits(set_sums, a.set_sums)
        status = np.full(S, -1, dtype=np.int32)
        assert raw(name, model, batch, 9, f, status=status) == _lib.RT_OK
        assert np.array_equal(status, a.status)
        assert raw(name, model, batch, 9, f) == _lib.RT_OK
    release(batch, model)


@pytest.mark.parametrize('n', [4, 20])
def test_chunks_of_moves_give_the_bits_of_one_chunk(contexts, n, monkeypatch):
    from raoteh_amd import _lib
    case, ta, _ = psc.cached_case(n, 'state', 'empty', 7400 + n)
    f = psc.make_factors(ta.nnodes, 3, 7400 + n)
    S = len(case.site_sets)
    model, batch = build(contexts, case, psc.site_weights(S, 5))
    try:
        M = len(model.nni_moves())
        assert M >= 6
        padded = ctypes.c_int64(0)
        _lib.check(_lib.lib().rt_sites_partition_info(batch._h, None, None, ctypes.byref(padded)))
        whole = model.nni_scores_partitioned(batch, f, per_site=True)
        # a move's bytes of the scratch: its rows in slot order and their stage-1 sums (one
        # workgroup per set at these sizes), with the values also in caller order and transposed
        for moves_per_chunk, per_site in ((1, True), (2, False), (M - 1, True)):
            per_move = 3 * (padded.value * 8 + case.nsets * 8 + (S * 16 if per_site else 0))
            monkeypatch.setenv('RAOTEH_NNI_CHUNK_BYTES', str(moves_per_chunk * per_move))
            got = model.nni_scores_partitioned(batch, f, per_site=per_site)
            monkeypatch.delenv('RAOTEH_NNI_CHUNK_BYTES')
            assert same_bits(got.sums, whole.sums) and same_bits(got.set_sums, whole.set_sums)
            assert np.array_equal(got.status, whole.status)
            if per_site:
                assert same_bits(got.values, whole.values)
    finally:
        release(batch, model)


@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense')])
def test_nothing_resident_changes(contexts, n, kind):
    from raoteh_amd import device
    from _branch_cases import make_coefs
    seed = 7500 + n
    case, ta, _ = psc.cached_case(n, kind, 'zero', seed)
    f = psc.make_factors(ta.nnodes, 3, seed)
    coefs = make_coefs(n, 2, seed)
    w = psc.site_weights(len(case.site_sets), 6)

    def fresh():
        model, batch = build(contexts, case, w)
        model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])     # the model's own rates
        return model, batch

    def reads(model, batch):
        model.step_partitioned(batch)
        ll, st = model.fetch_log_likelihoods(batch)
        ptot, ws = model.fetch_partition_totals(batch, weighted=True)
        be = model.branch_expectations_partitioned(batch, coefs)
        return [ll, st, ptot, ws, model.get_transitions(), be.values, be.edge_sums,
                be.set_edge_sums, be.status]
    model, batch = fresh()
    # no earlier step is needed, and a step changes nothing of the read
    first = model.branch_profiles_partitioned(batch, f, per_site=True)
    model.step_partitioned(batch)
    ll, st = model.fetch_log_likelihoods(batch)
    ptot, ws = model.fetch_partition_totals(batch, weighted=True)
    own = model.get_transitions()
    name = batch.kernel_name
    again = model.branch_profiles_partitioned(batch, f, per_site=True)
    assert same_bits(first.values, again.values) and same_bits(first.set_sums, again.set_sums)
    model.nni_scores_partitioned(batch, f, per_site=True)
    model.nni_scores_partitioned(batch)
    ll2, st2 = model.fetch_log_likelihoods(batch)
    ptot2, ws2 = model.fetch_partition_totals(batch, weighted=True)
    assert same_bits(ll2, ll) and np.array_equal(st2, st)
    assert same_bits(ptot2, ptot) and same_bits(ws2, ws)
    assert same_bits(model.get_transitions(), own) and batch.kernel_name == name
    fmodel, fbatch = fresh()
    for x, y in zip(reads(model, batch), reads(fmodel, fbatch)):
        assert same_bits(np.asarray(x), np.asarray(y))
    release(batch, fbatch, model, fmodel)


def test_both_granules_of_the_lane_kernel(contexts, monkeypatch):
    """RAOTEH_LANE_NO_PLDS=1: granules of 64 slots.  The values are per site: the same bits.  The
    sums add the same terms over runs of another shape: within 1e-12 of sum_i w_i |values| (773
    terms of one rounding each are below 1e-13 of it)."""
    n = 4
    case, ta, _ = psc.cached_case(n, 'dense', 'runs', 7600)
    f = np.array([0.5, 1.0, 2.0])                # (no -inf: the sums are compared)
    w = psc.site_weights(len(case.site_sets), 7)
    model, batch = build(contexts, case, w)
    prof = model.branch_profiles_partitioned(batch, f, per_site=True)
    nni = model.nni_scores_partitioned(batch, f, per_site=True)
    release(batch, model)
    monkeypatch.setenv('RAOTEH_LANE_NO_PLDS', '1')
    model, batch = build(contexts, case, w)
    from raoteh_amd import _lib
    G = ctypes.c_int64(0)
    _lib.check(_lib.lib().rt_sites_partition_info(batch._h, None, ctypes.byref(G), None))
    assert G.value == 64
    prof64 = model.branch_profiles_partitioned(batch, f, per_site=True)
    nni64 = model.nni_scores_partitioned(batch, f, per_site=True)
    release(batch, model)
    for a, b in ((prof, prof64), (nni, nni64)):
        assert same_bits(a.values, b.values) and np.array_equal(a.status, b.status)
        scale = np.einsum('i,irg->rg', w, np.abs(a.values))
        assert (np.abs(a.sums - b.sums) <= 1e-12 * np.maximum(scale, 1.0)).all()


@pytest.mark.parametrize('n', [4, 5])
def test_a_tree_without_moves(contexts, n):
    """A root with two leaves has no NNI: RT_OK, empty arrays, the status still written (site 1 of
    set 1 observes nothing at a leaf); the profiles of its two branches are there as usual."""
    import networkx as nx
    from raoteh_amd import device, _lib
    T = nx.Graph()
    T.add_edge(0, 1, weight=0.2)
    T.add_edge(0, 2, weight=0.3)
    rng = np.random.RandomState(7650 + n)
    S = 9
    lik = rng.uniform(0.1, 1.0, (S, 2, n))
    lik[1, 0] = 0.0
    site_sets = np.arange(S) % 2
    Q = np.array([smc.random_rates(n, rng), smc.random_rates(n, rng)])
    model = device.TreeModel(T, 0, n, ctx=contexts())
    batch = model.upload_sites([1, 2], lik, kind='dense', site_sets=site_sets, nsets=2)
    model.set_rate_sets(Q, t=np.array([[0.0, 0.2, 0.3], [0.0, 0.1, 0.4]]))
    got = model.nni_scores_partitioned(batch, [0.5, 2.0], per_site=True)
    assert got.moves.shape == (0, 3) and got.values.shape == (S, 0, 2)
    assert got.sums.shape == (0, 2) and got.set_sums.shape == (2, 0, 2)
    want = np.zeros(S, dtype=np.int32)
    want[1] = _lib.RT_SITE_ZERO_PROB
    np.testing.assert_array_equal(got.status, want)
    np.testing.assert_array_equal(model.nni_scores_partitioned(batch).status, want)
    prof = model.branch_profiles_partitioned(batch, [1.0, 2.0], per_site=True)
    np.testing.assert_array_equal(prof.status, want)
    assert np.abs(prof.values[:, :, 0]).max() < 1e-12 and not prof.values[1].any()   # factor 1; the dead site
    assert prof.values[want == 0][:, 1:, 1].all() and np.isfinite(prof.values).all()
    release(batch, model)


# ---- 5. the documented refusals ------------------------------------------------------------

def test_documented_refusals(contexts):
    from raoteh_amd import device, _lib
    n = 20
    case = pc.make_case(n, 'dense', 7700)
    model, batch = build(contexts, case)
    N = model.tree.nnodes
    f = np.ascontiguousarray(np.repeat([[0.5, 2.0]], N, axis=0))
    f[0] = 0.0
    good = model.branch_profiles_partitioned(batch, f, per_site=True)
    names = ('rt_sites_branch_profiles_partitioned', 'rt_sites_nni_scores_partitioned')
    calls = lambda m: (m.branch_profiles_partitioned, m.nni_scores_partitioned)      # noqa: E731
    sums = np.zeros((64, 66))
    # an ordinary batch
    omodel, obatch = pc.upload(device, contexts(), case, partitioned=False)
    omodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    for name, call in zip(names, calls(omodel)):
        with pytest.raises(ValueError, match='site_sets'):
            call(obatch, f)
        assert raw(name, omodel, obatch, 2, f, sums=sums) == _lib.RT_ERR_UNSUPPORTED
        assert 'ordinary batch' in _lib.last_error()
    # another model's batch
    for name, call in zip(names, calls(omodel)):
        with pytest.raises(ValueError, match='another model'):
            call(batch, f)
        assert raw(name, omodel, batch, 2, f, sums=sums) == _lib.RT_ERR_INVALID
    # fewer rate sets in the model than the batch uses, or none
    few = device.TreeModel(case.T, case.root, n, ctx=contexts())
    fb = few.upload_sites(case.leaves, case.data, kind=case.kind, site_sets=case.site_sets,
                          nsets=case.nsets)
    for name, call in zip(names, calls(few)):
        with pytest.raises(ValueError, match='set_rate_sets'):
            call(fb, f)
        assert raw(name, few, fb, 2, f, sums=sums) == _lib.RT_ERR_INVALID
        assert 'rate sets' in _lib.last_error()
    few.set_rate_sets(case.Q[:3], t=case.t[:3], node_q=case.node_q)
    for name, call in zip(names, calls(few)):
        with pytest.raises(ValueError, match='rate sets'):
            call(fb, f)
        assert raw(name, few, fb, 2, f, sums=sums) == _lib.RT_ERR_INVALID
    # npoints 0 and 65; factors NULL with two points; a negative and a NaN factor
    wide = np.ones((N, 65))
    neg, nan = f.copy(), f.copy()
    neg[N - 1, 1] = -0.5
    moved = int(model.nni_moves()[0, 0])                         # (a row NNI reads)
    nan[moved, 0] = np.nan
    neg[moved, 1] = -0.5
    for name, call in zip(names, calls(model)):
        assert raw(name, model, batch, 0, f, sums=sums) == _lib.RT_ERR_INVALID
        assert raw(name, model, batch, 65, wide, sums=sums) == _lib.RT_ERR_INVALID
        assert raw(name, model, batch, 2, None, sums=sums) == _lib.RT_ERR_INVALID
        assert raw(name, model, batch, 2, neg, sums=sums) == _lib.RT_ERR_INVALID
        assert raw(name, model, batch, 2, nan, sums=sums) == _lib.RT_ERR_INVALID
        for bad in (wide, neg, nan, np.ones((N, 0)), np.ones((N - 1, 2))):
            with pytest.raises(ValueError):
                call(batch, bad)
    # the ordinary and the mixture reads keep refusing the partitioned batch
    model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])
    cw = np.full(case.nsets, 1.0 / case.nsets)
    lib = _lib.lib()
    lengths = f * case.t[0][:, None]
    ll = np.zeros(len(case.site_sets))
    for rc in (
            lib.rt_sites_branch_profiles(model._h, batch._h, 0, 2, lengths.ctypes.data_as(P_F64), None,
                                         sums.ctypes.data_as(P_F64), None),
            lib.rt_sites_nni_scores(model._h, batch._h, 0, 2, lengths.ctypes.data_as(P_F64), None,
                                    sums.ctypes.data_as(P_F64), None),
            lib.rt_sites_branch_profiles_mixture(model._h, batch._h, 0, cw.ctypes.data_as(P_F64), 2,
                                                 f.ctypes.data_as(P_F64), None,
                                                 sums.ctypes.data_as(P_F64), ll.ctypes.data_as(P_F64),
                                                 None),
            lib.rt_sites_nni_scores_mixture(model._h, batch._h, 0, cw.ctypes.data_as(P_F64), 2,
                                            f.ctypes.data_as(P_F64), None, sums.ctypes.data_as(P_F64),
                                            ll.ctypes.data_as(P_F64), None)):
        assert rc == _lib.RT_ERR_UNSUPPORTED and 'partitioned' in _lib.last_error()
    with pytest.raises(_lib.RaotehHipError) as err:
        model.branch_profiles(batch, lengths=lengths)
    assert err.value.code == _lib.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
    with pytest.raises(_lib.RaotehHipError) as err:
        model.nni_scores(batch)
    assert err.value.code == _lib.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
    # the context still works
    again = model.branch_profiles_partitioned(batch, f, per_site=True)
    assert same_bits(again.values, good.values) and same_bits(again.set_sums, good.set_sums)
    release(batch, obatch, fb, model, omodel, few)


# ---- 6. the example ------------------------------------------------------------------------

def test_the_example_runs_and_never_loses_likelihood():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'nni_search_partitioned.py')],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith(('start:', 'round '))]
    ll = [float(re.search(r'log-likelihood (-?[0-9.]+)', x).group(1)) for x in lines]
    assert len(ll) >= 2 and 'done' in lines[-1]
    assert all(b >= a for a, b in zip(ll, ll[1:])), ll
    assert out.stdout.splitlines()[-1].startswith('final log-likelihood')
