"""rt_sites_spr_scores_mixture and rt_sites_placements_mixture (TreeModel.spr_scores_mixture /
place_queries_mixture) on the GPU: SPR scores and query placements of an ordinary batch under a
site-class mixture over the model's rate sets.  Every output against the host reference that no
device path enters (tests/_mixture_search2_cases.py), each also asked for alone; the revival case
(a set dead on the resident tree, live on the moved one) and the lost cases; a resident length of
zero; sets of weight zero; determinism; chunks; the log-likelihood against step_multi +
mixture_log_likelihoods; equal sets against the single-set calls; side effects; the documented
refusals."""
import ctypes

import networkx as nx
import numpy as np
import pytest

import _mixture_search_cases as msc
import _mixture_search2_cases as m2
import _step_multi_cases as smc
from _profile_cases import site_bounds

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
P_F64 = ctypes.POINTER(ctypes.c_double)
P_I32 = ctypes.POINTER(ctypes.c_int32)
OUTPUTS = ('values', 'sums', 'loglik', 'status')


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


def _f64(x):
    return None if x is None else np.ascontiguousarray(x, dtype=np.float64)


def _p(x, typ=P_F64):
    return None if x is None else x.ctypes.data_as(typ)


def raw_spr(model, batch, c, radius, fractions, want=OUTPUTS, nfractions=None, recompute=0):
    """rt_sites_spr_scores_mixture with exactly the outputs of `want`, the others NULL ->
    (code, dict); every output is prefilled with 7."""
    from raoteh_amd import _lib
    S, M = batch.nsites, len(model.spr_moves(radius))
    f = _f64(fractions)
    R = (1 if f is None else len(f)) if nfractions is None else nfractions
    shape = max(min(R, 64), 1)
    out = {'values': np.full((S, M, shape), 7.0), 'sums': np.full((M, shape), 7.0),
           'loglik': np.full(S, 7.0), 'status': np.full(S, 7, dtype=np.int32)}
    cw = _f64(c)
    code = _lib.lib().rt_sites_spr_scores_mixture(
        model._h, batch._h, recompute, _p(cw), -1 if radius is None else radius, R, _p(f),
        _p(out['values']) if 'values' in want else None, _p(out['sums']) if 'sums' in want else None,
        _p(out['loglik']) if 'loglik' in want else None,
        _p(out['status'], P_I32) if 'status' in want else None)
    return code, out


def raw_place(model, batch, c, queries, kind, fractions, pendant, scale=None, want=OUTPUTS,
              nqueries=None, nfractions=None, npendant=None, code_of_kind=None):
    """rt_sites_placements_mixture, as raw_spr."""
    from raoteh_amd import _lib
    S, N = batch.nsites, model.tree.nnodes
    f, t, sc = _f64(fractions), _f64(pendant), _f64(scale)
    q = None
    if queries is not None:
        q = np.ascontiguousarray(queries, dtype=np.float64 if kind == 'dense' else np.uint8)
    Q = (1 if q is None else q.shape[0]) if nqueries is None else nqueries
    R = (1 if f is None else len(f)) if nfractions is None else nfractions
    K = (1 if t is None else len(t)) if npendant is None else npendant
    dims = (max(min(Q, 8), 1), N, max(min(R, 16), 1), max(min(K, 32), 1))
    out = {'values': np.full((S,) + dims, 7.0), 'sums': np.full(dims, 7.0),
           'loglik': np.full(S, 7.0), 'status': np.full(S, 7, dtype=np.int32)}
    cw = _f64(c)
    if code_of_kind is None:
        code_of_kind = _lib.RT_OBS_DENSE if kind == 'dense' else _lib.RT_OBS_STATE
    code = _lib.lib().rt_sites_placements_mixture(
        model._h, batch._h, 0, _p(cw), Q, code_of_kind,
        None if q is None else q.ctypes.data_as(ctypes.c_void_p), R, _p(f), K, _p(t), _p(sc),
        _p(out['values']) if 'values' in want else None, _p(out['sums']) if 'sums' in want else None,
        _p(out['loglik']) if 'loglik' in want else None,
        _p(out['status'], P_I32) if 'status' in want else None)
    return code, out


def untouched(out):
    return all((a == 7).all() for a in out.values())


def check_against(got_values, got_sums, got_loglik, got_status, ref, weights, label):
    """The status exactly; -inf exactly where the reference has it, no NaN; elsewhere |got - want|
    <= 1e-10 max(1, |log Lambda_i|) per site and 1e-10 max(1, sum_i w_i |log Lambda_i|) for the
    sums (_profile_cases.site_bounds with the reference's log Lambda_i).  The worst gaps are printed
    in units of the bound's scale before anything is asserted."""
    dead = ref.status != 0
    ll = np.where(dead, 0.0, ref.loglik)
    per_site, sum_bound = site_bounds(ll, weights)
    vgap = sgap = lgap = 0.0
    if got_values is not None:
        assert got_values.shape == ref.values.shape
        fin = np.isfinite(ref.values)
        d = np.abs(np.where(fin, got_values, 0.0) - np.where(fin, ref.values, 0.0))
        scale = (per_site / 1e-10).reshape((-1,) + (1,) * (d.ndim - 1))
        vgap = (d / scale).max() if d.size else 0.0
    if got_sums is not None:
        assert got_sums.shape == ref.sums.shape
        sfin = np.isfinite(ref.sums)
        d = np.abs(np.where(sfin, got_sums, 0.0) - np.where(sfin, ref.sums, 0.0))
        sgap = (d.max() if d.size else 0.0) / (sum_bound / 1e-10)
    if got_loglik is not None:
        lgap = (np.abs(np.where(dead, 0.0, got_loglik) - ll) / (per_site / 1e-10)).max()
    print('%s: worst gap / scale: values %.2e, sums %.2e, loglik %.2e (bound 1e-10)'
          % (label, vgap, sgap, lgap))
    if got_status is not None:
        np.testing.assert_array_equal(got_status, ref.status)
    if got_values is not None:
        assert np.array_equal(np.isneginf(got_values), np.isneginf(ref.values))
        assert not np.isnan(got_values).any() and not np.isposinf(got_values).any()
        assert vgap <= 1e-10
    if got_sums is not None:
        assert np.array_equal(np.isneginf(got_sums), np.isneginf(ref.sums))
        assert not np.isnan(got_sums).any()
        assert sgap <= 1e-10
    if got_loglik is not None:
        assert np.array_equal(np.isneginf(got_loglik), dead)
        assert lgap <= 1e-10


def same_bits(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


def all_same(a, b):
    return all(same_bits(getattr(a, name), getattr(b, name)) for name in OUTPUTS)


# ---- 1. parity against the host reference ---------------------------------------------------

# n = 2, 4: the lane kernels; 83 sites: six 16-site tiles with the last partial for n > 4, two
# lane blocks of 64; 5 the smallest matrix-pipe size; 20, 61; 122 with K = 2.  The 8-leaf balanced
# tree and the 12-node non-binary tree; K = 3 with the zero set; dense, state and mask uploads;
# radius 1, 2 and no limit; 1, 3 (0 and 1 among them) and RT_MAX_PLACE_FRACTIONS = 8 fractions;
# site weights with zeros; dense data: a site dead under every set.
SPR_CASES = [
    # n, tree, kind, K, radius, nfractions, weighted
    (2, 'random', 'state', 3, None, 3, True),
    (4, 'balanced', 'dense', 3, 1, 8, False),
    (4, 'random', 'mask', 3, 2, 1, True),
    (5, 'balanced', 'mask', 3, None, 3, True),
    (20, 'random', 'dense', 3, 2, 3, False),
    (20, 'balanced', 'state', 3, 1, 1, True),
    (61, 'balanced', 'state', 3, 2, 1, True),
    (61, 'random', 'dense', 3, 2, 3, False),
    (122, 'balanced', 'state', 2, 2, 1, False),
]
# dense and state queries (an unobserved 255 among the states), 1 and 5 queries, 1 and 3 pendant
# lengths (one of them 0), with and without pendant_scale
PLACE_CASES = [
    # n, tree, kind, K, query kind, queries, nfractions, npendant, scaled, weighted
    (2, 'random', 'state', 3, 'state', 5, 3, 3, True, True),
    (4, 'balanced', 'dense', 3, 'dense', 1, 8, 1, False, False),
    (4, 'random', 'mask', 3, 'state', 1, 1, 3, False, True),
    (5, 'balanced', 'mask', 3, 'dense', 5, 3, 1, True, True),
    (20, 'random', 'dense', 3, 'state', 5, 1, 3, True, False),
    (61, 'balanced', 'state', 3, 'dense', 1, 3, 3, False, True),
    (61, 'random', 'dense', 3, 'state', 5, 1, 1, True, False),
    (122, 'balanced', 'state', 2, 'dense', 1, 1, 1, False, False),
]


def spr_id(c):
    return 'n%d-%s-%s-K%d-r%s-f%d%s' % (c[0], c[1], c[2], c[3], c[4], c[5], '-w' if c[6] else '')


def place_id(c):
    return 'n%d-%s-%s-K%d-%s%d-f%d-p%d%s%s' % (c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7],
                                              '-s' if c[8] else '', '-w' if c[9] else '')


@pytest.mark.parametrize('case', SPR_CASES, ids=spr_id)
def test_spr_scores_against_the_host_reference(ctx, case):
    n, tree, kind, K, radius, nf, weighted = case
    seed = 9800 + 7 * n + nf
    case_, ta, c, f, w, ref = m2.cached_spr_reference(n, tree, kind, K, seed, radius, nf, weighted)
    assert (ref.status != 0).any() == (kind == 'dense')      # (a site dead under every set)
    assert (ref.status == 0).sum() > 40 and len(ref.moves) > 0
    model, batch = build(ctx, case_, w)
    try:
        got = model.spr_scores_mixture(batch, c, radius=radius, fractions=f, per_site=True)
        assert np.array_equal(got.moves, ref.moves) and same_bits(got.fractions, np.array(f))
        check_against(got.values, got.sums, got.loglik, got.status, ref, w, 'spr ' + spr_id(case))
        flat = np.where(np.isnan(got.sums), -np.inf, got.sums)
        assert got.best == tuple(int(x) for x in np.unravel_index(np.argmax(flat), flat.shape))
        # each output asked for alone: the bits of the full call
        code, full = raw_spr(model, batch, c, radius, f)
        assert code == 0
        assert same_bits(full['values'], got.values) and same_bits(full['sums'], got.sums)
        for name in OUTPUTS:
            code, alone = raw_spr(model, batch, c, radius, f, want=(name,))
            assert code == 0, name
            assert same_bits(alone[name], full[name]), name
            assert untouched(dict((k, v) for k, v in alone.items() if k != name))
        lean = model.spr_scores_mixture(batch, c, radius=radius, fractions=f)
        assert lean.values is None and same_bits(lean.sums, got.sums)
    finally:
        release(model, batch)


@pytest.mark.parametrize('case', PLACE_CASES, ids=place_id)
def test_placements_against_the_host_reference(ctx, case):
    n, tree, kind, K, qkind, nq, nf, npd, scaled, weighted = case
    seed = 9900 + 7 * n + nf + npd
    case_, ta, c, q, f, tau, scale, w, ref = m2.cached_place_reference(
        n, tree, kind, K, seed, qkind, nq, nf, npd, scaled, weighted)
    assert (ref.status != 0).any() == (kind == 'dense')
    assert (ref.status == 0).sum() > 40
    assert qkind == 'dense' or (q == 255).any()
    model, batch = build(ctx, case_, w)
    try:
        got = model.place_queries_mixture(batch, c, q, kind=qkind, fractions=f, pendant=tau,
                                          pendant_scale=scale, per_site=True)
        check_against(got.values, got.sums, got.loglik, got.status, ref, w, 'place ' + place_id(case))
        assert (got.values[:, :, 0] == 0).all() and (got.sums[:, 0] == 0).all()   # (the root's rows)
        assert same_bits(got.pendant_scale, np.ones(K) if scale is None else np.asarray(scale))
        assert got.best.shape == (nq, 3) and (got.best[:, 0] >= 1).all()
        code, full = raw_place(model, batch, c, q, qkind, f, tau, scale)
        assert code == 0
        assert same_bits(full['values'], got.values) and same_bits(full['sums'], got.sums)
        for name in OUTPUTS:
            code, alone = raw_place(model, batch, c, q, qkind, f, tau, scale, want=(name,))
            assert code == 0, name
            assert same_bits(alone[name], full[name]), name
            assert untouched(dict((k, v) for k, v in alone.items() if k != name))
        lean = model.place_queries_mixture(batch, c, q, kind=qkind, fractions=f, pendant=tau,
                                           pendant_scale=scale)
        assert lean.values is None and same_bits(lean.sums, got.sums)
    finally:
        release(model, batch)


# ---- 2. the revival case and the lost cases -------------------------------------------------

@pytest.mark.parametrize('n', [3, 5])
def test_a_set_dead_on_the_resident_tree_counts_after_the_spr_move(ctx, n):
    """n = 3: the lane kernels; n = 5: the matrix-pipe kernels."""
    case, ta = msc.revival_case(n)
    c = np.array([0.6, 0.4])
    move = m2.revival_move(ta)
    i = case.site
    f = m2.FRACTIONS[3]
    L, moved = m2.spr_move_likelihoods(case, ta, move, f[1])
    assert L[0, i] == 0.0 and moved[0, i] > 0.0 and L[1, i] > 0.0
    ref = m2.spr_reference(ta, case, c, f)
    j = [tuple(mv) for mv in ref.moves].index(move)
    model, batch = build(ctx, case)
    try:
        got = model.spr_scores_mixture(batch, c, fractions=f, per_site=True)
        print('revival n=%d: device %r reference %r' % (n, got.values[i, j], ref.values[i, j]))
        assert np.isfinite(got.values[i, j]).all()
        bound = 1e-10 * max(1.0, abs(ref.loglik[i]))
        assert np.abs(got.values[i, j] - ref.values[i, j]).max() <= bound
        check_against(got.values, got.sums, got.loglik, got.status, ref, None, 'revival n=%d' % n)
    finally:
        release(model, batch)
    # without the one-way set's term the value would be another one
    alone = np.log(c[1] * moved[1, i]) - np.log(c[1] * L[1, i])
    assert abs(ref.values[i, j, 1] - alone) > 1e-3


@pytest.mark.parametrize('n', [3, 5])
def test_what_no_set_allows_gives_minus_infinity(ctx, n):
    case, ta = msc.lost_case(n)
    c = np.array([0.5, 0.5])
    i = case.site
    f, tau = m2.FRACTIONS[3], m2.PENDANT[3]
    move = m2.lost_move(ta)
    ref = m2.spr_reference(ta, case, c, f)
    j = [tuple(mv) for mv in ref.moves].index(move)
    assert np.isneginf(ref.values[i, j]).all() and ref.status[i] == 0
    q = np.array([[0, 2]], dtype=np.uint8)
    v = ta.node_to_index[3]
    pref = m2.place_reference(ta, case, c, q, 'state', f, tau)
    assert np.isneginf(pref.values[i, 0, v]).all()
    model, batch = build(ctx, case)
    try:
        got = model.spr_scores_mixture(batch, c, fractions=f, per_site=True)
        assert np.isneginf(got.values[i, j]).all() and np.isneginf(got.sums[j]).all()
        check_against(got.values, got.sums, got.loglik, got.status, ref, None, 'lost spr n=%d' % n)
        got = model.place_queries_mixture(batch, c, q, kind='state', fractions=f, pendant=tau,
                                          per_site=True)
        assert np.isneginf(got.values[i, 0, v]).all() and np.isneginf(got.sums[0, v]).all()
        check_against(got.values, got.sums, got.loglik, got.status, pref, None, 'lost place n=%d' % n)
    finally:
        release(model, batch)


# ---- 3. a resident length of zero; sets of weight zero; determinism -------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_a_resident_length_of_zero(ctx, n):
    """t[k][y] == 0 under a running set, on a target edge with moves: no NaN, parity holds."""
    base, ta = msc.cached_case(n, 'balanced', 'dense', 2, 9700 + n)
    t = base.t.copy()
    t[1, 1] = 0.0                                # (an internal node: a target, and a pruned edge)
    t[0, 4] = 0.0
    case = base._replace(t=t)
    c = np.array([0.4, 0.6])
    f, tau = m2.FRACTIONS[3], m2.PENDANT[3]
    q = m2.make_queries(case, 2, 'dense', 3)
    model, batch = build(ctx, case)
    try:
        got = model.spr_scores_mixture(batch, c, radius=2, fractions=f, per_site=True)
        assert (got.moves[:, 1] == 1).any() and (got.moves[:, 0] == 1).any()
        assert not np.isnan(got.values).any() and not np.isnan(got.sums).any()
        check_against(got.values, got.sums, got.loglik, got.status,
                      m2.spr_reference(ta, case, c, f, 2), None, 'zero length, spr')
        got = model.place_queries_mixture(batch, c, q, fractions=f, pendant=tau, per_site=True)
        assert not np.isnan(got.values).any() and not np.isnan(got.sums).any()
        check_against(got.values, got.sums, got.loglik, got.status,
                      m2.place_reference(ta, case, c, q, 'dense', f, tau), None, 'zero length, place')
    finally:
        release(model, batch)


@pytest.mark.parametrize('n', [4, 20])
def test_a_set_of_weight_zero_is_as_if_absent(ctx, n):
    case, ta = msc.cached_case(n, 'balanced', 'dense', 3, 9600 + n)
    w = msc.site_weights(msc.NSITES, 6)
    c3 = np.array([0.3, 0.0, 0.7])
    f, tau = m2.FRACTIONS[3], m2.PENDANT[3]
    q = m2.make_queries(case, 2, 'state', 3)
    scale = np.array([0.5, 3.0, 1.5])
    full_model, full_batch = build(ctx, case, w)
    part_model, part_batch = build(ctx, case, w, sets=(0, 2))
    try:
        a = full_model.spr_scores_mixture(full_batch, c3, radius=2, fractions=f, per_site=True)
        b = part_model.spr_scores_mixture(part_batch, c3[[0, 2]], radius=2, fractions=f, per_site=True)
        assert all_same(a, b) and np.isfinite(a.loglik).any()
        a = full_model.place_queries_mixture(full_batch, c3, q, kind='state', fractions=f, pendant=tau,
                                             pendant_scale=scale, per_site=True)
        b = part_model.place_queries_mixture(part_batch, c3[[0, 2]], q, kind='state', fractions=f,
                                             pendant=tau, pendant_scale=scale[[0, 2]], per_site=True)
        assert all_same(a, b) and np.isfinite(a.loglik).any()
    finally:
        release(full_model, full_batch)
        release(part_model, part_batch)


@pytest.mark.parametrize('n', [4, 61])
def test_two_calls_give_the_same_bits(ctx, n):
    case, ta = msc.cached_case(n, 'random', 'state', 3, 9500 + n)
    c = msc.class_weights(3, 2)
    f, tau = m2.FRACTIONS[3], m2.PENDANT[3]
    q = m2.make_queries(case, 2, 'dense', 3)
    model, batch = build(ctx, case, msc.site_weights(msc.NSITES, 6))
    try:
        a = model.spr_scores_mixture(batch, c, radius=1, fractions=f, per_site=True)
        pa = model.place_queries_mixture(batch, c, q, fractions=f, pendant=tau, per_site=True)
        b = model.spr_scores_mixture(batch, c, radius=1, fractions=f, per_site=True,
                                     recompute_transitions=True)
        pb = model.place_queries_mixture(batch, c, q, fractions=f, pendant=tau, per_site=True,
                                         recompute_transitions=True)
        assert all_same(a, b) and all_same(pa, pb)
    finally:
        release(model, batch)


# ---- 4. chunks ------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_chunks_give_the_bits_of_one_chunk(ctx, n, monkeypatch):
    """Chunks of one unit, of two and of all but one: pruned nodes for SPR (a chunk holds whole
    pruned nodes: the bytes of the largest, of two and of all moves but one), queries for
    placements."""
    case, ta = msc.cached_case(n, 'random', 'dense', 3, 9400 + n)
    c = msc.class_weights(3, 2)
    f, tau = m2.FRACTIONS[3], m2.PENDANT[1]
    S = msc.NSITES
    model, batch = build(ctx, case, msc.site_weights(S, 6))
    try:
        moves = model.spr_moves(2)
        per_node = np.bincount(moves[:, 0])
        M = len(moves)
        assert M >= 6
        whole = model.spr_scores_mixture(batch, c, radius=2, fractions=f, per_site=True)
        whole_sums = model.spr_scores_mixture(batch, c, radius=2, fractions=f)
        per_move = len(f) * S * 8
        for nmoves, per_site in ((1, True), (int(per_node.max()), False),
                                 (2 * int(per_node.max()), True), (M - 1, True)):
            monkeypatch.setenv('RAOTEH_SPR_CHUNK_BYTES', str(nmoves * per_move * (2 if per_site else 1)))
            got = model.spr_scores_mixture(batch, c, radius=2, fractions=f, per_site=per_site)
            monkeypatch.delenv('RAOTEH_SPR_CHUNK_BYTES')
            assert same_bits(got.sums, whole.sums) and same_bits(got.sums, whole_sums.sums)
            assert same_bits(got.loglik, whole.loglik) and same_bits(got.status, whole.status)
            if per_site:
                assert same_bits(got.values, whole.values)
        Q = 5
        q = m2.make_queries(case, Q, 'state', 3)
        kw = dict(kind='state', fractions=f, pendant=tau, pendant_scale=[0.5, 1.0, 2.0])
        whole = model.place_queries_mixture(batch, c, q, per_site=True, **kw)
        whole_sums = model.place_queries_mixture(batch, c, q, **kw)
        per_query = ta.nnodes * len(f) * len(tau) * S * 8
        for nq, per_site in ((1, True), (2, False), (Q - 1, True)):
            monkeypatch.setenv('RAOTEH_PLACE_CHUNK_BYTES', str(nq * per_query * (2 if per_site else 1)))
            got = model.place_queries_mixture(batch, c, q, per_site=per_site, **kw)
            monkeypatch.delenv('RAOTEH_PLACE_CHUNK_BYTES')
            assert same_bits(got.sums, whole.sums) and same_bits(got.sums, whole_sums.sums)
            assert same_bits(got.loglik, whole.loglik) and same_bits(got.status, whole.status)
            if per_site:
                assert same_bits(got.values, whole.values)
    finally:
        release(model, batch)


# ---- 5. the mixture log-likelihood; equal sets ----------------------------------------------

@pytest.mark.parametrize('n', [4, 61])
def test_loglik_is_the_mixture_log_likelihood_of_step_multi(ctx, n):
    case, ta = msc.cached_case(n, 'balanced', 'dense', 3, 9300 + n)
    c = msc.class_weights(3, 2)
    q = m2.make_queries(case, 1, 'state', 3)
    model, batch = build(ctx, case)
    try:
        model.step_multi(batch)
        want, wst, _ = model.mixture_log_likelihoods(batch, c)
        dead = (wst & 1) != 0
        assert dead.any() and not dead.all()
        per_site, _ = site_bounds(np.where(dead, 0.0, want))
        for got in (model.spr_scores_mixture(batch, c, radius=1),
                    model.place_queries_mixture(batch, c, q, kind='state')):
            assert np.array_equal((got.status & 1) != 0, dead)
            assert np.array_equal(np.isneginf(got.loglik), dead)
            gap = np.abs(np.where(dead, 0.0, got.loglik) - np.where(dead, 0.0, want))
            print('n=%d: loglik gap / bound %.2e' % (n, (gap / per_site).max()))
            assert (gap <= per_site).all()
    finally:
        release(model, batch)


@pytest.mark.parametrize('n', [4, 20])
def test_equal_sets_give_the_single_set_calls(ctx, n):
    """All K sets equal to one rate set, any weights: spr_scores / place_queries of that rate set,
    to the tolerance (bit equality is not required); with K = 1 and c = [1] the log-likelihood is
    the batch's own."""
    from raoteh_amd import device
    case, ta = msc.cached_case(n, 'random', 'dense', 2, 9200 + n)
    c = msc.class_weights(3, 2)
    w = msc.site_weights(msc.NSITES, 6)
    f, tau = m2.FRACTIONS[3], m2.PENDANT[3]
    q = m2.make_queries(case, 2, 'dense', 3)
    model, batch = smc.upload(device, ctx, case)
    try:
        batch.set_weights(w)
        model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])
        model.set_rate_sets(np.stack([case.Q[0]] * 3), t=np.stack([case.t[0]] * 3), node_q=case.node_q)
        ll, st = model.log_likelihoods(batch)
        dead = (st & 1) != 0
        per_site, sum_bound = site_bounds(np.where(dead, 0.0, ll), w)
        pairs = ((model.spr_scores(batch, radius=2, fractions=f, per_site=True),
                  model.spr_scores_mixture(batch, c, radius=2, fractions=f, per_site=True)),
                 (model.place_queries(batch, q, fractions=f, pendant=tau, per_site=True),
                  model.place_queries_mixture(batch, c, q, fractions=f, pendant=tau, per_site=True)))
        for one, mix in pairs:
            assert np.array_equal((mix.status & 1) != 0, dead)
            assert np.array_equal(np.isfinite(one.values), np.isfinite(mix.values))
            fin = np.isfinite(one.values)
            gap = np.abs(np.where(fin, mix.values, 0.0) - np.where(fin, one.values, 0.0))
            scale = per_site.reshape((-1,) + (1,) * (gap.ndim - 1))
            # (a sum is -inf where a live site of positive weight has a -inf value: in both alike)
            assert np.array_equal(np.isneginf(one.sums), np.isneginf(mix.sums))
            assert not np.isnan(one.sums).any() and not np.isnan(mix.sums).any()
            sfin = np.isfinite(one.sums)
            sgap = np.abs(np.where(sfin, mix.sums, 0.0) - np.where(sfin, one.sums, 0.0))
            print('equal sets n=%d: values gap / bound %.2e, sums %.2e'
                  % (n, (gap / scale).max(), sgap.max() / sum_bound))
            assert (gap <= scale).all() and sfin.any()
            assert (sgap <= sum_bound).all()
            lgap = np.abs(np.where(dead, 0.0, mix.loglik) - np.where(dead, 0.0, ll))
            assert (lgap <= per_site).all()
        model.set_rate_sets(case.Q[:1], t=case.t[:1], node_q=case.node_q)
        for mix in (model.spr_scores_mixture(batch, [1.0], radius=1),
                    model.place_queries_mixture(batch, [1.0], q)):
            lgap = np.abs(np.where(dead, 0.0, mix.loglik) - np.where(dead, 0.0, ll))
            assert (lgap <= per_site).all() and np.array_equal(np.isneginf(mix.loglik), dead)
    finally:
        release(model, batch)


# ---- 6. nothing resident changes ------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_nothing_resident_changes(ctx, n):
    from raoteh_amd import device
    case, ta = msc.cached_case(n, 'balanced', 'state', 3, 9100 + n)
    c = msc.class_weights(3, 2)
    f, tau = m2.FRACTIONS[3], m2.PENDANT[3]
    q = m2.make_queries(case, 2, 'state', 3)
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
        spr_before = model.spr_scores(batch, radius=2, fractions=f, per_site=True)
        place_before = model.place_queries(batch, q, kind='state', fractions=f, pendant=tau,
                                           per_site=True)
        model.spr_scores_mixture(batch, c, radius=2, fractions=f, per_site=True)
        model.place_queries_mixture(batch, c, q, kind='state', fractions=f, pendant=tau,
                                    pendant_scale=[0.5, 1.0, 2.0], per_site=True)
        model.spr_scores_mixture(batch, c)
        for a, b in zip(before, snapshot()):
            assert same_bits(np.asarray(a), np.asarray(b))
        # the single-set calls on the same batch return what they returned
        spr_after = model.spr_scores(batch, radius=2, fractions=f, per_site=True)
        place_after = model.place_queries(batch, q, kind='state', fractions=f, pendant=tau,
                                          per_site=True)
        for name in ('values', 'sums', 'status'):
            assert same_bits(getattr(spr_before, name), getattr(spr_after, name)), name
            assert same_bits(getattr(place_before, name), getattr(place_after, name)), name
        # the rate sets too: step_multi without recomputing gives what it gave
        model.step_multi(batch, recompute_transitions=False)
        mll, mst = model.fetch_multi_log_likelihoods(batch)
        assert same_bits(mll, before[3]) and same_bits(mst, before[4])
    finally:
        release(model, batch)


# ---- 7. the documented refusals -------------------------------------------------------------

def test_documented_refusals(ctx):
    from raoteh_amd import device, synth, _lib
    import _partition_cases as pc
    INVALID, UNSUPPORTED = _lib.RT_ERR_INVALID, _lib.RT_ERR_UNSUPPORTED
    case, ta = msc.cached_case(20, 'random', 'state', 2, 9000)
    c = np.array([0.5, 0.5])
    f, tau = [0.25, 0.5], [0.1]
    q = m2.make_queries(case, 2, 'state', 3)
    model, batch = build(ctx, case)
    other, other_batch = build(ctx, case)
    bare, bare_batch = smc.upload(device, ctx, case)
    try:
        def spr(cw=c, fr=f, m=model, b=batch, **kw):
            code, out = raw_spr(m, b, cw, 1, fr, **kw)
            assert code == 0 or untouched(out)   # (a refusal writes nothing)
            return code

        def place(cw=c, qq=q, kind='state', fr=f, pd=tau, scale=None, m=model, b=batch, **kw):
            code, out = raw_place(m, b, cw, qq, kind, fr, pd, scale, **kw)
            assert code == 0 or untouched(out)
            return code
        calls = (('spr', spr, lambda m, b, cw: m.spr_scores_mixture(b, cw, radius=1, fractions=f)),
                 ('place', place, lambda m, b, cw: m.place_queries_mixture(
                     b, cw, q, kind='state', fractions=f, pendant=tau)))
        for name, code, wrapped in calls:
            assert code() == 0
            # no rate sets
            assert code(m=bare, b=bare_batch) == INVALID
            with pytest.raises(ValueError, match='set_rate_sets'):
                wrapped(bare, bare_batch, c)
            # a batch of another model
            assert code(m=model, b=other_batch) == INVALID
            with pytest.raises(ValueError, match='another model'):
                wrapped(model, other_batch, c)
            # class weights: NULL, negative, not finite, all zero, another length
            assert code(cw=None) == INVALID
            for bad in ([0.5, -0.5], [0.5, np.nan], [np.inf, 0.5], [0.0, 0.0]):
                assert code(cw=np.array(bad)) == INVALID, bad
                with pytest.raises(ValueError):
                    wrapped(model, batch, bad)
            with pytest.raises(ValueError):
                wrapped(model, batch, [1.0])
            # fractions: NULL, none, too many, outside [0, 1], not finite
            assert code(fr=None) == INVALID
            assert code(nfractions=0) == INVALID
            assert code(fr=np.full(_lib.RT_MAX_PLACE_FRACTIONS + 1, 0.5)) == INVALID
            for x in (-1e-9, 1.0 + 1e-9, np.nan, np.inf):
                assert code(fr=[0.5, x]) == INVALID, x
                assert 'fraction' in _lib.last_error()
            # a "rescale" batch, a batch of the generic kernel
            for option in ('rescale', 'force_generic'):
                ctx.set_option(option, 1)
                try:
                    ob = model.upload_sites(case.leaves, case.data, kind=case.kind)
                finally:
                    ctx.set_option(option, 0)
                assert code(b=ob) == UNSUPPORTED, option
                with pytest.raises(_lib.RaotehHipError) as err:
                    wrapped(model, ob, c)
                assert err.value.code == UNSUPPORTED, option
                ob.close()
        for bad in ([], np.full(9, 0.5), [0.5, 1.5], [np.nan]):
            with pytest.raises(ValueError):
                model.spr_scores_mixture(batch, c, radius=1, fractions=bad)
            with pytest.raises(ValueError):
                model.place_queries_mixture(batch, c, q, kind='state', fractions=bad)
        with pytest.raises(ValueError):
            model.spr_scores_mixture(batch, c, radius=-2)
        # placements: the queries, the pendant lengths, the counts, the scale
        assert place(code_of_kind=_lib.RT_OBS_MASK) == UNSUPPORTED
        assert 'RT_OBS_MASK' in _lib.last_error()
        assert place(code_of_kind=77) == INVALID
        assert place(qq=None) == INVALID
        assert place(nqueries=0) == INVALID
        assert place(pd=None) == INVALID
        assert place(npendant=0) == INVALID
        assert place(pd=np.full(_lib.RT_MAX_PLACE_PENDANT + 1, 0.1)) == INVALID
        assert place(fr=np.full(8, 0.5), pd=np.full(16, 0.1)) == 0           # (2 R + K = 32)
        assert place(fr=np.full(8, 0.5), pd=np.full(16, 0.1), nfractions=8, npendant=17) == INVALID
        for x in (-1e-9, np.nan, np.inf):
            assert place(pd=[x]) == INVALID
            assert 'pendant length' in _lib.last_error()
            assert place(scale=[1.0, x]) == INVALID
            assert 'pendant_scale' in _lib.last_error()
            with pytest.raises(ValueError):
                model.place_queries_mixture(batch, c, q, kind='state', pendant=[x])
            with pytest.raises(ValueError):
                model.place_queries_mixture(batch, c, q, kind='state', pendant_scale=[1.0, x])
        assert place(scale=[0.0, 2.0]) == 0
        for kw in (dict(kind='mask'), dict(kind='state', pendant_scale=[1.0]),
                   dict(kind='state', pendant=np.full(17, 0.1)),
                   dict(kind='state', fractions=np.full(8, 0.5), pendant=np.full(16, 0.1)[:, None])):
            with pytest.raises(ValueError):
                model.place_queries_mixture(batch, c, q, **kw)
        with pytest.raises(ValueError):
            model.place_queries_mixture(batch, c, q[:0], kind='state')
        with pytest.raises(ValueError):
            model.place_queries_mixture(batch, c, q[:, :5], kind='state')
        # a partitioned batch
        pcase = pc.make_case(20, 'dense', seed=6)
        pmodel, pbatch = pc.upload(device, ctx, pcase)
        pmodel.set_rate_sets(pcase.Q, t=pcase.t, node_q=pcase.node_q)
        pc_w = np.full(pcase.Q.shape[0], 1.0 / pcase.Q.shape[0])
        pq = np.zeros((1, pbatch.nsites), dtype=np.uint8)
        code, out = raw_spr(pmodel, pbatch, pc_w, 1, f, want=('status',))
        assert code == UNSUPPORTED and untouched(out) and 'partitioned' in _lib.last_error()
        code, out = raw_place(pmodel, pbatch, pc_w, pq, 'state', f, tau, want=('status',))
        assert code == UNSUPPORTED and untouched(out) and 'partitioned' in _lib.last_error()
        with pytest.raises(ValueError, match='ordinary'):
            pmodel.spr_scores_mixture(pbatch, pc_w)
        with pytest.raises(ValueError, match='ordinary'):
            pmodel.place_queries_mixture(pbatch, pc_w, pq, kind='state')
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
        for m, b in ((single, sb), (deep, db)):
            with pytest.raises(_lib.RaotehHipError) as err:
                m.spr_scores_mixture(b, [1.0], radius=0)
            assert err.value.code == UNSUPPORTED
            with pytest.raises(_lib.RaotehHipError) as err:
                m.place_queries_mixture(b, [1.0], np.zeros((1, b.nsites), dtype=np.uint8),
                                        kind='state', pendant=[0.1])
            assert err.value.code == UNSUPPORTED
        release(single, sb)
        release(deep, db)
        # more than 96 GB of scratch (2 047 nodes x 64 000 sites x 256 bytes x (L, M, up) are 100 GB):
        # refused before anything is reserved
        Tb, rootb, leavesb = synth.balanced_tree(1024, seed=0)
        wide_model = device.TreeModel(Tb, rootb, 20, ctx=ctx)
        wide_model.set_rate_sets(smc.random_rates(20, np.random.RandomState(1))[None])
        wb = wide_model.upload_sites(leavesb, np.zeros((64000, len(leavesb)), dtype=np.uint8),
                                     kind='state')
        with pytest.raises(_lib.RaotehHipError) as err:
            wide_model.spr_scores_mixture(wb, [1.0], radius=0)
        assert err.value.code == UNSUPPORTED and 'GB' in str(err.value)
        with pytest.raises(_lib.RaotehHipError) as err:
            wide_model.place_queries_mixture(wb, [1.0], np.zeros((1, 64000), dtype=np.uint8),
                                             kind='state', pendant=[0.1])
        assert err.value.code == UNSUPPORTED and 'GB' in str(err.value)
        release(wide_model, wb)
        # the batch is as it was, the context still works
        again = model.spr_scores_mixture(batch, c, radius=1, fractions=f)
        assert np.isfinite(again.sums).all()
    finally:
        release(model, batch)
        release(other, other_batch)
        release(bare, bare_batch)
