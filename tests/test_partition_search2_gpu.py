"""rt_sites_spr_scores_partitioned and rt_sites_placements_partitioned
(TreeModel.spr_scores_partitioned / place_queries_partitioned) on the GPU: the scores of every SPR
move and the placements of queries on every branch of a partitioned batch, every site under its
own rate set.  Against the host reference that no device path enters
(tests/_partition_search2_cases.py); bit for bit against the ordinary calls on each set's sites;
repeatability, every output alone, chunks of pruned nodes and of queries, both granules of the lane
kernels; -inf and zero lengths; the queries in caller order; side effects; a tree without moves;
the documented refusals; the example.

On the -inf cases: the reference has -inf values of its own at live sites -- from the identity
edges of the planted set (_partition_search_cases.plant_lost_sites: Q[k][0] = 0) at the fractions
0 and 1, from moves that strand the planted sites and from state queries that contradict a leaf
across an edge of length 0.  Where the reference has one the device must have it, in the values,
in the set's sums and in the sums."""
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
import _partition_search2_cases as p2
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


def build(contexts, case, weights=None, **opts):
    from raoteh_amd import device
    model, batch = pc.upload(device, contexts(**opts), case)
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
    """-inf where the reference has it and nowhere else, no NaN; the rest within `bound` (broadcast
    against the arrays).  -> the worst gap over its bound."""
    assert got.shape == want.shape, label
    assert not np.isnan(got).any() and not np.isnan(want).any(), label + ': NaN'
    assert np.array_equal(np.isneginf(got), np.isneginf(want)), label + ': -inf pattern'
    assert not np.isposinf(got).any(), label
    fin = np.isfinite(want)
    err = np.where(fin, np.abs(np.where(fin, got, 0.0) - np.where(fin, want, 0.0)), 0.0)
    worst = float((err / bound).max()) if err.size else 0.0
    print('%s: max |got - ref| / bound %.3g' % (label, worst))
    assert (err <= bound).all(), label
    return worst


def set_sum_bound(set_sums):
    """The project's 1e-10 of max(1, |set sum|), entry by entry (a -inf entry is compared exactly)."""
    return TOL * np.maximum(1.0, np.where(np.isfinite(set_sums), np.abs(set_sums), 1.0))


def check_against(got, ref, case, w, label):
    """The project's 1e-10: of max(1, |log L_i|) per value, of max(1, |set sum|) per set sum, of
    max(1, sum_i w_i |log L_i|) per sum (site_bounds); -inf, zeros and the status exactly."""
    per_site, per_sum = pfc.site_bounds(ref.loglik, w, tol=TOL)
    np.testing.assert_array_equal(got.status, ref.status)
    tail = (None,) * (ref.values.ndim - 1)
    close_to(got.values, ref.values, per_site[(slice(None),) + tail], label + ' values')
    close_to(got.set_sums, ref.set_sums, set_sum_bound(ref.set_sums), label + ' set sums')
    close_to(got.sums, ref.sums, per_sum, label + ' sums')
    dead = ref.status != 0
    assert not got.values[dead].any()
    for k in range(case.nsets):
        if not (case.site_sets == k).any():
            assert not got.set_sums[k].any() and not np.signbit(got.set_sums[k]).any()   # exactly 0


# ---- 1. against the host reference ---------------------------------------------------------

@pytest.mark.parametrize('row', p2.PARITY, ids=p2.PARITY_IDS)
def test_spr_scores_against_the_host_reference(contexts, row):
    n, kind, sets, qkind, radius, nf, npend, scaled, weighted = row
    case, ta, special, f, w, ref = p2.cached_spr_reference(n, kind, sets, radius, nf, weighted)
    S = len(case.site_sets)
    assert S == (len(psc.runs_site_sets(n, 0)) if sets == 'runs' else 3 * pc.granule(n) + 5)
    assert len(ref.moves) == (58 if radius == 1 else 156)
    assert p2.check_reference(case, ref)         # (live sites in every set; -inf among them)
    model, batch = build(contexts, case, w)
    try:
        got = model.spr_scores_partitioned(batch, radius=radius, fractions=f, per_site=True)
        np.testing.assert_array_equal(got.moves, ref.moves)
        assert got.values.shape == (S, len(ref.moves), nf) and same_bits(got.fractions, np.array(f))
        check_against(got, ref, case, w, 'spr n=%d %s %s' % (n, kind, sets))
        flat = np.where(np.isnan(got.sums), -np.inf, got.sums).reshape(-1)
        assert got.best == tuple(int(x) for x in np.unravel_index(int(np.argmax(flat)), got.sums.shape))
        sums_only = model.spr_scores_partitioned(batch, radius=radius, fractions=f)
        assert sums_only.values is None
        assert same_bits(sums_only.sums, got.sums) and same_bits(sums_only.set_sums, got.set_sums)
        assert np.array_equal(sums_only.status, got.status)
        lost0, lost1, v, lk = special
        assert got.status[lost0] == 0 and got.status[lost1] == 0
        if kind != 'dense':
            assert (got.status[case.site_sets == lk] != 0).any()      # dead under its set
    finally:
        release(batch, model)


@pytest.mark.parametrize('row', p2.PARITY, ids=p2.PARITY_IDS)
def test_placements_against_the_host_reference(contexts, row):
    n, kind, sets, qkind, radius, nf, npend, scaled, weighted = row
    case, ta, special, q, f, tau, scale, w, ref = p2.cached_place_reference(
        n, kind, sets, qkind, nf, npend, scaled, weighted)
    S, N = len(case.site_sets), ta.nnodes
    assert p2.check_reference(case, ref) == (qkind == 'state')        # (-inf among the live sites)
    model, batch = build(contexts, case, w)
    try:
        got = model.place_queries_partitioned(batch, q, kind=qkind, fractions=f, pendant=tau,
                                              pendant_scale=scale, per_site=True)
        assert got.values.shape == (S, p2.NQ, N, nf, npend)
        assert not got.values[:, :, 0].any() and not got.sums[:, 0].any()
        assert not got.set_sums[:, :, 0].any()
        # (the reference's arrays are [S, ...]; the set sums [set, ...])
        check_against(got, ref, case, w, 'place n=%d %s %s %s' % (n, kind, sets, qkind))
        flat = got.sums[:, 1:].reshape(p2.NQ, -1)
        vv, rr, kk = np.unravel_index(np.argmax(flat, axis=1), (N - 1, nf, npend))
        np.testing.assert_array_equal(got.best, np.stack([vv + 1, rr, kk], axis=1))
        sums_only = model.place_queries_partitioned(batch, q, kind=qkind, fractions=f, pendant=tau,
                                                    pendant_scale=scale)
        assert sums_only.values is None
        assert same_bits(sums_only.sums, got.sums) and same_bits(sums_only.set_sums, got.set_sums)
        assert np.array_equal(sums_only.status, got.status)
    finally:
        release(batch, model)


# ---- 2. bit for bit against the ordinary calls ---------------------------------------------

@pytest.mark.parametrize('n,kind,qkind', [(4, 'state', 'dense'), (20, 'dense', 'state'),
                                          (61, 'state', 'dense')])
def test_bit_for_bit_against_the_ordinary_calls(contexts, n, kind, qkind):
    """Set k's sites as an ordinary batch under set_rates(Q[k], node_q, t[k]): spr_scores at the
    same fractions, place_queries with the pendant lengths pendant_scale[k] * tau (one f64 product
    per entry, as the device makes it) and the set's queries.  The same arithmetic per site column
    and per edge, the exponential's variant chosen by one set's count -- a difference is a wrong
    table or slot."""
    from raoteh_amd import device
    case, ta, _ = psc.cached_case(n, kind, 'empty', 8100 + n)
    f, tau = p2.FRACTIONS[3], np.array(p2.PENDANT[3])
    scale = p2.case_scale(case.nsets, True)
    q = p2.make_queries(case, p2.NQ, qkind, 8104)
    model, batch = build(contexts, case)
    spr = model.spr_scores_partitioned(batch, radius=2, fractions=f, per_site=True)
    plc = model.place_queries_partitioned(batch, q, kind=qkind, fractions=f, pendant=tau,
                                          pendant_scale=scale, per_site=True)
    for k in range(case.nsets):
        mine = np.flatnonzero(case.site_sets == k)
        if not len(mine):
            continue
        om = device.TreeModel(case.T, case.root, n, ctx=contexts())
        om.set_root_distn(case.root_distn)
        om.set_rates(Q=case.Q[k], node_q=case.node_q, t=case.t[k])
        ob = om.upload_sites(case.leaves, case.data[mine], kind=kind)
        want = om.spr_scores(ob, radius=2, fractions=f, per_site=True)
        np.testing.assert_array_equal(want.moves, spr.moves)
        assert same_bits(np.ascontiguousarray(spr.values[mine]), want.values), k
        assert np.array_equal(spr.status[mine], want.status), k
        want = om.place_queries(ob, np.ascontiguousarray(q[:, mine]), kind=qkind, fractions=f,
                                pendant=scale[k] * tau, per_site=True)
        assert same_bits(np.ascontiguousarray(plc.values[mine]), want.values), k
        assert np.array_equal(plc.status[mine], want.status), k
        release(ob, om)
    release(batch, model)


# ---- 3. determinism, every output alone, chunks --------------------------------------------

P_F64 = ctypes.POINTER(ctypes.c_double)
P_I32 = ctypes.POINTER(ctypes.c_int32)


def ptr(a, t):
    return None if a is None else a.ctypes.data_as(t)


def raw_spr(model, batch, radius, f, values=None, sums=None, set_sums=None, status=None, nf=None):
    from raoteh_amd import _lib
    return _lib.lib().rt_sites_spr_scores_partitioned(
        model._h, batch._h, 0, radius, len(f) if nf is None else nf, ptr(f, P_F64),
        ptr(values, P_F64), ptr(sums, P_F64), ptr(set_sums, P_F64), ptr(status, P_I32))


def raw_place(model, batch, q, code, f, tau, scale=None, values=None, sums=None, set_sums=None,
              status=None, nq=None, nf=None, npend=None):
    from raoteh_amd import _lib
    return _lib.lib().rt_sites_placements_partitioned(
        model._h, batch._h, 0, q.shape[0] if nq is None else nq, code,
        None if q is None else q.ctypes.data_as(ctypes.c_void_p),
        len(f) if nf is None else nf, ptr(f, P_F64), len(tau) if npend is None else npend,
        ptr(tau, P_F64), ptr(scale, P_F64), ptr(values, P_F64), ptr(sums, P_F64),
        ptr(set_sums, P_F64), ptr(status, P_I32))


@pytest.mark.parametrize('n,kind,qkind', [(4, 'state', 'state'), (20, 'mask', 'dense'),
                                          (61, 'dense', 'state')])
def test_two_calls_and_every_output_alone(contexts, n, kind, qkind):
    from raoteh_amd import _lib
    case, ta, _ = psc.cached_case(n, kind, 'runs', 8300 + n)
    f, tau = np.array(p2.FRACTIONS[3]), np.array(p2.PENDANT[3])
    w = psc.site_weights(len(case.site_sets), 4)
    q = p2.make_queries(case, p2.NQ, qkind, 8304)
    code = _lib.RT_OBS_DENSE if qkind == 'dense' else _lib.RT_OBS_STATE
    model, batch = build(contexts, case, w)
    S, N, K = len(case.site_sets), ta.nnodes, case.nsets
    M = len(model.spr_moves(1))
    spr = lambda **kw: model.spr_scores_partitioned(batch, radius=1, fractions=f, **kw)   # noqa: E731
    plc = lambda **kw: model.place_queries_partitioned(batch, q, kind=qkind, fractions=f,  # noqa: E731
                                                       pendant=tau, **kw)
    for call, raw, shape in ((spr, lambda **kw: raw_spr(model, batch, 1, f, **kw), (M, 3)),
                             (plc, lambda **kw: raw_place(model, batch, q, code, f, tau, **kw),
                              (p2.NQ, N, 3, 3))):
        a = call(per_site=True)
        b = call(per_site=True)
        for x, y in ((a.values, b.values), (a.sums, b.sums), (a.set_sums, b.set_sums)):
            assert same_bits(x, y)
        assert np.array_equal(a.status, b.status)
        values = np.full((S,) + shape, 7.0)
        assert raw(values=values) == _lib.RT_OK
        assert same_bits(values, a.values)
        sums = np.full(shape, 7.0)
        assert raw(sums=sums) == _lib.RT_OK
        assert same_bits(sums, a.sums)
        set_sums = np.full((K,) + shape, 7.0)
        assert raw(set_sums=set_sums) == _lib.RT_OK
        assert same_bits(set_sums, a.set_sums)
        status = np.full(S, -1, dtype=np.int32)
        assert raw(status=status) == _lib.RT_OK
        assert np.array_equal(status, a.status)
        assert raw() == _lib.RT_OK
    release(batch, model)


def padded_slots(batch):
    from raoteh_amd import _lib
    padded = ctypes.c_int64(0)
    _lib.check(_lib.lib().rt_sites_partition_info(batch._h, None, None, ctypes.byref(padded)))
    return padded.value


@pytest.mark.parametrize('n', [4, 20])
def test_chunks_give_the_bits_of_one_chunk(contexts, n, monkeypatch):
    """A limit of one byte holds no unit: the library then makes chunks of one unit each, whatever
    a unit's bytes are -- one pruned node (a chunk never splits a pruned node's moves), one query.
    The other limits come from a row's bytes of the scratch as the library counts them (its values
    in slot order and their stage-1 sums, one workgroup per set at these sizes, with the values
    also in caller order and transposed): two moves, all moves but one (everything but the last
    pruned node), two queries of three."""
    case, ta, _ = psc.cached_case(n, 'state', 'empty', 8400 + n)
    S, N = len(case.site_sets), ta.nnodes
    f, tau = p2.FRACTIONS[3], p2.PENDANT[1]
    q = p2.make_queries(case, 3, 'state', 8404)
    model, batch = build(contexts, case, psc.site_weights(S, 5))
    try:
        padded = padded_slots(batch)

        def row_bytes(per_site):
            return padded * 8 + case.nsets * 8 + (S * 16 if per_site else 0)
        whole = model.spr_scores_partitioned(batch, fractions=f, per_site=True)
        M = len(whole.moves)
        for moves_per_chunk, per_site in ((0, True), (0, False), (2, False), (M - 1, True)):
            monkeypatch.setenv('RAOTEH_SPR_CHUNK_BYTES',
                               str(max(1, moves_per_chunk * 3 * row_bytes(per_site))))
            got = model.spr_scores_partitioned(batch, fractions=f, per_site=per_site)
            monkeypatch.delenv('RAOTEH_SPR_CHUNK_BYTES')
            assert same_bits(got.sums, whole.sums) and same_bits(got.set_sums, whole.set_sums)
            assert np.array_equal(got.status, whole.status)
            if per_site:
                assert same_bits(got.values, whole.values)
        whole = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau,
                                                per_site=True)
        for queries_per_chunk, per_site in ((0, True), (0, False), (2, False), (2, True)):
            monkeypatch.setenv('RAOTEH_PLACE_CHUNK_BYTES',
                               str(max(1, queries_per_chunk * N * 3 * row_bytes(per_site))))
            got = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau,
                                                  per_site=per_site)
            monkeypatch.delenv('RAOTEH_PLACE_CHUNK_BYTES')
            assert same_bits(got.sums, whole.sums) and same_bits(got.set_sums, whole.set_sums)
            assert np.array_equal(got.status, whole.status)
            if per_site:
                assert same_bits(got.values, whole.values)
    finally:
        release(batch, model)


# ---- 4. both granules of the lane kernels --------------------------------------------------

def test_both_granules_of_the_lane_kernels(contexts, monkeypatch):
    """RAOTEH_LANE_NO_PLDS=1: granules of 64 slots.  The values are per site: the same bits.  The
    finite sums add the same terms over runs of another shape: within 1e-12 of sum_i w_i |values|
    (773 terms of one rounding each are below 1e-13 of it)."""
    n = 4
    case, ta, _ = psc.cached_case(n, 'dense', 'runs', 8600)
    f, tau = (0.25, 0.5), (0.07, 0.4)
    w = psc.site_weights(len(case.site_sets), 7)
    q = p2.make_queries(case, p2.NQ, 'dense', 8604)

    def both():
        model, batch = build(contexts, case, w)
        from raoteh_amd import _lib
        G = ctypes.c_int64(0)
        _lib.check(_lib.lib().rt_sites_partition_info(batch._h, None, ctypes.byref(G), None))
        out = (G.value, model.spr_scores_partitioned(batch, fractions=f, per_site=True),
               model.place_queries_partitioned(batch, q, fractions=f, pendant=tau, per_site=True))
        release(batch, model)
        return out
    G256, spr, plc = both()
    monkeypatch.setenv('RAOTEH_LANE_NO_PLDS', '1')
    G64, spr64, plc64 = both()
    assert (G256, G64) == (256, 64)
    for a, b in ((spr, spr64), (plc, plc64)):
        assert same_bits(a.values, b.values) and np.array_equal(a.status, b.status)
        # (a move can strand the planted sites whatever the fraction: such a row's sum is -inf)
        lost = np.isneginf(a.sums)
        assert np.array_equal(np.isneginf(b.sums), lost) and not lost.all()
        assert np.isfinite(a.sums[~lost]).all() and np.isfinite(b.sums[~lost]).all()
        scale = np.tensordot(w, np.where(np.isfinite(a.values), np.abs(a.values), 0.0), axes=1)
        assert (np.abs(a.sums[~lost] - b.sums[~lost]) <= 1e-12 * np.maximum(scale, 1.0)[~lost]).all()


# ---- 5. exactness --------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_lost_sites_and_zero_lengths(contexts, n):
    """The planted sites lost0 (weight 0) and lost1 (weight 1) of the set with identity edges: where
    the reference has lost1 at -inf, so are the values, the set's sum and the sum; with every site
    that is -inf in such a row at weight 0 the row's sums are finite.  Then t[1][v0] = 0 on an
    internal edge: no NaN anywhere, and the reference's values."""
    case, ta, (lost0, lost1, v, k) = psc.cached_case(n, 'state', 'empty', p2.SEED)
    S = len(case.site_sets)
    f, tau = p2.FRACTIONS[3], p2.PENDANT[3]
    w = p2.case_weights(case, (lost0, lost1), p2.SEED, True)
    q = p2.make_queries(case, p2.NQ, 'state', p2.SEED + 4)
    refs = (p2.spr_reference(ta, case, f, 1, w), p2.place_reference(ta, case, q, 'state', f, tau, None, w))
    model, batch = build(contexts, case, w)
    calls = (lambda: model.spr_scores_partitioned(batch, radius=1, fractions=f, per_site=True),
             lambda: model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau,
                                                     per_site=True))
    for ref, call in zip(refs, calls):
        batch.set_weights(w)
        got = call()
        rows = np.isneginf(ref.values[lost1])
        assert rows.any() and ref.status[lost1] == 0 and ref.status[lost0] == 0
        assert np.array_equal(np.isneginf(got.values[lost1]), rows)
        assert np.array_equal(np.isneginf(got.values[lost0]), np.isneginf(ref.values[lost0]))
        assert np.isneginf(got.set_sums[k][rows]).all() and np.isneginf(got.sums[rows]).all()
        row = tuple(np.argwhere(rows)[0])
        w2 = w.copy()
        w2[np.isneginf(ref.values[(slice(None),) + row])] = 0.0
        assert w2[lost0] == 0 and w2[lost1] == 0 and (w2[case.site_sets == k] != 0).any()
        batch.set_weights(w2)
        quiet = call()
        assert np.isfinite(quiet.set_sums[k][row]) and np.isfinite(quiet.sums[row])
        assert same_bits(quiet.values, got.values)
    release(batch, model)
    kids = np.diff(ta.indptr)
    v0 = int(np.flatnonzero(kids[1:] > 0)[0]) + 1
    t = case.t.copy()
    t[1, v0] = 0.0
    zcase = case._replace(t=t)
    model, batch = build(contexts, zcase, w)
    got = model.spr_scores_partitioned(batch, fractions=f, per_site=True)
    assert (got.moves[:, 1] == v0).any()
    check_against(got, p2.spr_reference(ta, zcase, f, None, w), zcase, w, 'n=%d spr, t[1][%d] = 0' % (n, v0))
    got = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau, per_site=True)
    check_against(got, p2.place_reference(ta, zcase, q, 'state', f, tau, None, w), zcase, w,
                  'n=%d place, t[1][%d] = 0' % (n, v0))
    release(batch, model)


# ---- 6. the queries in caller order --------------------------------------------------------

@pytest.mark.parametrize('n,qkind', [(4, 'dense'), (20, 'state'), (20, 'dense')])
def test_queries_follow_the_callers_sites(contexts, n, qkind):
    """'runs' site sets: slot order differs from caller order.  The caller's sites permuted together
    with their queries and site sets: the values permuted, the set sums as they were (to the bound
    of the parity tests: another order of the terms)."""
    case, ta, _ = psc.cached_case(n, 'dense', 'runs', 8700 + n)
    S = len(case.site_sets)
    assert (np.diff(case.site_sets) < 0).any()
    f, tau = p2.FRACTIONS[1], p2.PENDANT[3]
    q = p2.make_queries(case, p2.NQ, qkind, 8704)
    perm = np.random.RandomState(8705).permutation(S)
    pcase = case._replace(obs_lik=case.obs_lik[perm], data=case.data[perm],
                          site_sets=case.site_sets[perm])
    model, batch = build(contexts, case)
    a = model.place_queries_partitioned(batch, q, kind=qkind, fractions=f, pendant=tau, per_site=True)
    sa = model.spr_scores_partitioned(batch, radius=1, fractions=f, per_site=True)
    release(batch, model)
    model, batch = build(contexts, pcase)
    b = model.place_queries_partitioned(batch, np.ascontiguousarray(q[:, perm]), kind=qkind,
                                        fractions=f, pendant=tau, per_site=True)
    sb = model.spr_scores_partitioned(batch, radius=1, fractions=f, per_site=True)
    # a point mass as a dense query is the state query of that state
    if qkind == 'state':
        states = np.where(q[:, perm] < n, q[:, perm], 0).astype(np.uint8)
        dense = np.zeros(states.shape + (n,))
        np.put_along_axis(dense, states[..., None].astype(np.int64), 1.0, axis=2)
        as_state = model.place_queries_partitioned(batch, states, kind='state', fractions=f,
                                                   pendant=tau, per_site=True)
        as_dense = model.place_queries_partitioned(batch, dense, kind='dense', fractions=f,
                                                   pendant=tau, per_site=True)
        assert same_bits(as_state.values, as_dense.values)
        assert same_bits(as_state.set_sums, as_dense.set_sums)
    release(batch, model)
    ll = psc.profile_reference(ta, case, psc.device_factors([1.0], ta.nnodes)).loglik
    per_site, _ = pfc.site_bounds(ll, None, tol=TOL)
    for x, y in ((a, b), (sa, sb)):
        assert np.array_equal(x.status[perm], y.status)
        tail = (None,) * (x.values.ndim - 1)
        close_to(y.values, x.values[perm], per_site[perm][(slice(None),) + tail], 'permuted values')
        close_to(y.set_sums, x.set_sums, set_sum_bound(x.set_sums), 'permuted set sums')


# ---- 7. nothing resident changes -----------------------------------------------------------

@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense')])
def test_nothing_resident_changes(contexts, n, kind):
    from _branch_cases import make_coefs
    seed = 8500 + n
    case, ta, _ = psc.cached_case(n, kind, 'zero', seed)
    f, tau = p2.FRACTIONS[3], p2.PENDANT[3]
    q = p2.make_queries(case, p2.NQ, 'state', seed + 4)
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
    first = model.spr_scores_partitioned(batch, fractions=f, per_site=True)
    firstp = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau,
                                             per_site=True)
    model.step_partitioned(batch)
    ll, st = model.fetch_log_likelihoods(batch)
    ptot, ws = model.fetch_partition_totals(batch, weighted=True)
    own = model.get_transitions()
    name = batch.kernel_name
    sets = [np.array(x) for x in model._rate_sets]
    again = model.spr_scores_partitioned(batch, fractions=f, per_site=True)
    againp = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau,
                                             per_site=True)
    assert same_bits(first.values, again.values) and same_bits(first.set_sums, again.set_sums)
    assert same_bits(firstp.values, againp.values) and same_bits(firstp.set_sums, againp.set_sums)
    ll2, st2 = model.fetch_log_likelihoods(batch)
    ptot2, ws2 = model.fetch_partition_totals(batch, weighted=True)
    assert same_bits(ll2, ll) and np.array_equal(st2, st)
    assert same_bits(ptot2, ptot) and same_bits(ws2, ws)
    assert same_bits(model.get_transitions(), own) and batch.kernel_name == name
    for x, y in zip(sets, model._rate_sets):
        assert same_bits(x, np.asarray(y))
    # the rate sets on the device: a fresh model and batch read the same after the same calls
    fmodel, fbatch = fresh()
    for x, y in zip(reads(model, batch), reads(fmodel, fbatch)):
        assert same_bits(np.asarray(x), np.asarray(y))
    release(batch, fbatch, model, fmodel)


# ---- 8. a tree without moves ---------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 5])
def test_a_two_node_tree_has_no_move(contexts, n):
    """A root with one leaf has no SPR move: RT_OK, empty arrays, the status still written (site 1
    of set 1 observes nothing at the leaf); its one branch takes placements as usual."""
    import networkx as nx
    from raoteh_amd import device, _lib
    T = nx.Graph()
    T.add_edge(0, 1, weight=0.2)
    rng = np.random.RandomState(8650 + n)
    S = 9
    lik = rng.uniform(0.1, 1.0, (S, 1, n))
    lik[1, 0] = 0.0
    site_sets = np.arange(S) % 2
    Q = np.array([smc.random_rates(n, rng), smc.random_rates(n, rng)])
    model = device.TreeModel(T, 0, n, ctx=contexts())
    batch = model.upload_sites([1], lik, kind='dense', site_sets=site_sets, nsets=2)
    model.set_rate_sets(Q, t=np.array([[0.0, 0.2], [0.0, 0.1]]))
    got = model.spr_scores_partitioned(batch, fractions=(0.25, 0.5), per_site=True)
    assert got.moves.shape == (0, 2) and got.values.shape == (S, 0, 2) and got.best is None
    assert got.sums.shape == (0, 2) and got.set_sums.shape == (2, 0, 2)
    want = np.zeros(S, dtype=np.int32)
    want[1] = _lib.RT_SITE_ZERO_PROB
    np.testing.assert_array_equal(got.status, want)
    status = np.full(S, -1, dtype=np.int32)
    assert raw_spr(model, batch, -1, np.array([0.5]), status=status) == _lib.RT_OK
    np.testing.assert_array_equal(status, want)
    q = rng.uniform(0.1, 1.0, (1, S, n))
    plc = model.place_queries_partitioned(batch, q, fractions=(0.5,), pendant=(0.1,), per_site=True)
    np.testing.assert_array_equal(plc.status, want)
    assert np.isfinite(plc.values).all() and plc.values[want == 0][:, 0, 1].all()
    assert not plc.values[1].any() and not plc.values[:, :, 0].any()
    release(batch, model)


# ---- 9. the documented refusals ------------------------------------------------------------

def test_documented_refusals(contexts):
    from raoteh_amd import device, _lib
    n = 20
    case = pc.make_case(n, 'dense', 8800)
    model, batch = build(contexts, case)
    S, N = len(case.site_sets), model.tree.nnodes
    f, tau = np.array([0.25, 0.5]), np.array([0.1])
    q = p2.make_queries(case, p2.NQ, 'state', 8804)
    qd = p2.make_queries(case, p2.NQ, 'dense', 8804)
    STATE, DENSE, MASK = _lib.RT_OBS_STATE, _lib.RT_OBS_DENSE, _lib.RT_OBS_MASK
    good = model.spr_scores_partitioned(batch, radius=1, fractions=f, per_site=True)
    goodp = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau, per_site=True)
    sums = np.zeros(4 * N * N * 8)

    def both(m, b):
        return (raw_spr(m, b, 1, f, sums=sums), raw_place(m, b, q, STATE, f, tau, sums=sums))
    # an ordinary batch
    omodel, obatch = pc.upload(device, contexts(), case, partitioned=False)
    omodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    with pytest.raises(ValueError, match='site_sets'):
        omodel.spr_scores_partitioned(obatch)
    with pytest.raises(ValueError, match='site_sets'):
        omodel.place_queries_partitioned(obatch, q, kind='state')
    for rc in both(omodel, obatch):
        assert rc == _lib.RT_ERR_UNSUPPORTED and 'ordinary batch' in _lib.last_error()
    # another model's batch
    with pytest.raises(ValueError, match='another model'):
        omodel.spr_scores_partitioned(batch)
    with pytest.raises(ValueError, match='another model'):
        omodel.place_queries_partitioned(batch, q, kind='state')
    assert both(omodel, batch) == (_lib.RT_ERR_INVALID, _lib.RT_ERR_INVALID)
    # fewer rate sets in the model than the batch uses, or none
    few = device.TreeModel(case.T, case.root, n, ctx=contexts())
    fb = few.upload_sites(case.leaves, case.data, kind=case.kind, site_sets=case.site_sets,
                          nsets=case.nsets)
    with pytest.raises(ValueError, match='set_rate_sets'):
        few.spr_scores_partitioned(fb)
    for rc in both(few, fb):
        assert rc == _lib.RT_ERR_INVALID and 'rate sets' in _lib.last_error()
    few.set_rate_sets(case.Q[:3], t=case.t[:3], node_q=case.node_q)
    with pytest.raises(ValueError, match='rate sets'):
        few.place_queries_partitioned(fb, q, kind='state')
    assert both(few, fb) == (_lib.RT_ERR_INVALID, _lib.RT_ERR_INVALID)
    # (a "rescale" or generic-kernel partitioned batch cannot be made: the upload refuses it,
    # tests/test_partition_gpu.py)
    # counts and values out of range, NULL inputs
    INVALID = _lib.RT_ERR_INVALID
    wide = np.full(_lib.RT_MAX_PLACE_FRACTIONS + 1, 0.5)
    for bad in (np.array([-0.1]), np.array([1.5]), np.array([np.nan]), wide):
        assert raw_spr(model, batch, 1, bad, sums=sums) == INVALID
        assert raw_place(model, batch, q, STATE, bad, tau, sums=sums) == INVALID
        with pytest.raises(ValueError):
            model.spr_scores_partitioned(batch, fractions=bad)
        with pytest.raises(ValueError):
            model.place_queries_partitioned(batch, q, kind='state', fractions=bad, pendant=tau)
    assert raw_spr(model, batch, 1, f, sums=sums, nf=0) == INVALID
    assert raw_spr(model, batch, 1, None, sums=sums, nf=1) == INVALID
    long_tau = np.full(_lib.RT_MAX_PLACE_PENDANT + 1, 0.1)
    for bad in (np.array([-0.1]), np.array([np.inf]), np.array([np.nan]), long_tau):
        assert raw_place(model, batch, q, STATE, f, bad, sums=sums) == INVALID
        with pytest.raises(ValueError):
            model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=bad)
    for bad in (np.array([1.0, -1.0, 1.0, 1.0]), np.array([1.0, 1.0, np.nan, 1.0])):
        assert raw_place(model, batch, q, STATE, f, tau, scale=bad, sums=sums) == INVALID
        with pytest.raises(ValueError):
            model.place_queries_partitioned(batch, q, kind='state', pendant=tau, pendant_scale=bad)
    with pytest.raises(ValueError):                   # (one scale per set of the MODEL)
        model.place_queries_partitioned(batch, q, kind='state', pendant=tau, pendant_scale=np.ones(3))
    assert raw_place(model, batch, q, STATE, f, tau, sums=sums, nq=0) == INVALID
    assert raw_place(model, batch, q, STATE, f, tau, sums=sums, nf=0) == INVALID
    assert raw_place(model, batch, q, STATE, f, tau, sums=sums, npend=0) == INVALID
    assert raw_place(model, batch, None, STATE, f, tau, sums=sums, nq=2) == INVALID
    assert raw_place(model, batch, q, STATE, None, tau, sums=sums, nf=1) == INVALID
    assert raw_place(model, batch, q, STATE, f, None, sums=sums, npend=1) == INVALID
    assert raw_place(model, batch, q, 77, f, tau, sums=sums) == INVALID
    # mask queries
    assert raw_place(model, batch, q, MASK, f, tau, sums=sums) == _lib.RT_ERR_UNSUPPORTED
    assert 'RT_OBS_MASK' in _lib.last_error()
    with pytest.raises(ValueError):
        model.place_queries_partitioned(batch, q, kind='mask', pendant=tau)
    with pytest.raises(ValueError):
        model.place_queries_partitioned(batch, qd[:, :-1], kind='dense', pendant=tau)
    # the ordinary and the mixture reads keep refusing the partitioned batch
    model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])
    cw = np.full(case.nsets, 1.0 / case.nsets)
    lib = _lib.lib()
    ll = np.zeros(S)
    qp = q.ctypes.data_as(ctypes.c_void_p)
    for rc in (
            lib.rt_sites_spr_scores(model._h, batch._h, 0, 1, 2, ptr(f, P_F64), None, ptr(sums, P_F64),
                                    None),
            lib.rt_sites_spr_scores_mixture(model._h, batch._h, 0, ptr(cw, P_F64), 1, 2, ptr(f, P_F64),
                                            None, ptr(sums, P_F64), ptr(ll, P_F64), None),
            lib.rt_sites_placements(model._h, batch._h, 0, 2, STATE, qp, 2, ptr(f, P_F64), 1,
                                    ptr(tau, P_F64), None, ptr(sums, P_F64), None),
            lib.rt_sites_placements_mixture(model._h, batch._h, 0, ptr(cw, P_F64), 2, STATE, qp, 2,
                                            ptr(f, P_F64), 1, ptr(tau, P_F64), None, None,
                                            ptr(sums, P_F64), ptr(ll, P_F64), None)):
        assert rc == _lib.RT_ERR_UNSUPPORTED and 'partitioned' in _lib.last_error()
    with pytest.raises(_lib.RaotehHipError) as err:
        model.spr_scores(batch)
    assert err.value.code == _lib.RT_ERR_UNSUPPORTED and 'partitioned' in str(err.value)
    # the context still works
    again = model.spr_scores_partitioned(batch, radius=1, fractions=f, per_site=True)
    assert same_bits(again.values, good.values) and same_bits(again.set_sums, good.set_sums)
    againp = model.place_queries_partitioned(batch, q, kind='state', fractions=f, pendant=tau, per_site=True)
    assert same_bits(againp.values, goodp.values) and same_bits(againp.set_sums, goodp.set_sums)
    release(batch, obatch, fb, model, omodel, few)


# ---- 10. the example -----------------------------------------------------------------------

def test_the_example_runs_and_never_loses_likelihood():
    out = subprocess.run([sys.executable, os.path.join(ROOT, 'examples', 'spr_search_partitioned.py')],
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-3000:])
    assert out.returncode == 0, out.stderr[-2000:]
    lines = [x for x in out.stdout.splitlines() if x.startswith(('start:', 'round '))]
    ll = [float(re.search(r'log-likelihood (-?[0-9.]+)', x).group(1)) for x in lines]
    assert len(ll) >= 2
    assert all(b >= a for a, b in zip(ll, ll[1:])), ll
    assert out.stdout.splitlines()[-1].startswith('final log-likelihood')
