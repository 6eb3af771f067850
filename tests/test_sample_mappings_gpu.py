"""rt_sites_sample_mappings (TreeModel.sample_mappings) on the device.  The node states are
those of sample_states bit for bit; given them, the numpy mirror of the pinned branch rule
(tests/_mapping_cases.py) must reproduce every event count exactly (every case keeps its pick
targets a relative 1e-9 away from the cell boundaries, which the mirror checks) and every value
to rounding; the means over many draws must converge to the device's own exact expectations
(branch_expectations, which is pinned to the reference)."""
import ctypes
import itertools

import numpy as np
import pytest

import _mapping_cases as mc
import _sample_cases as sc

pytestmark = pytest.mark.gpu


@pytest.fixture(scope='module')
def ra():
    import raoteh_amd
    from raoteh_amd import device, _lib, synth

    class NS(object):
        pass
    ns = NS()
    ns.pkg = raoteh_amd
    ns.device, ns.lib, ns.synth = device, _lib, synth
    ns.ctx = device.get_context()
    # kernels are compiled inside rt_sites_create, not in the background
    _lib.check(_lib.lib().rt_set_option(b'jit_async', 0))
    return ns


def build(ra, T, root, n, Q=None, rd=None):
    model = ra.device.TreeModel(T, root, n)
    if Q is not None:
        model.set_rates(Q_default=Q)
    if rd is not None:
        model.set_root_distn(rd)
    return model


def host_rates(model, Q_default):
    """(Q f64[nq, n, n], node_q, t) as set_rates(Q_default=...) hands them to the library."""
    Q, node_q = model.tree.rate_matrices(model.nstates, Q_default)
    return Q, node_q, model.tree.branch_lengths()


def check_parity(model, got, rates, coefs, seed, first_draw=0, want_status=None):
    """The device's values and counts against the mirror, given the device's states."""
    Q, node_q, t = rates
    parent = model.tree.parent
    N = model.tree.nnodes
    mir = mc.numpy_mappings(Q, t, node_q, parent, got.states, coefs, seed, first_draw)
    assert mir['margin'] > mc.MARGIN, mir['margin']
    assert np.array_equal(got.counts, mir['counts'])
    np.testing.assert_allclose(got.values, mir['values'], rtol=1e-9, atol=1e-12)
    assert np.array_equal(got.status & 4, mir['status'])
    if want_status is not None:
        assert np.array_equal(got.status, want_status)
    st = got.states
    a, b = st[:, :, parent[1:]], st[:, :, 1:]
    live = (a != 255) & (b != 255)
    ident = [k for k in range(len(coefs)) if np.array_equal(coefs[k], np.eye(coefs.shape[1]))]
    for k in ident:
        tt = np.broadcast_to(t[1:], a.shape)
        np.testing.assert_allclose(got.values[:, :, 1:, k][live], tt[live], rtol=1e-12)
    real = got.counts[:, :, 1:, 1]
    assert (real[live & (a != b)] >= 1).all() and (real[live & (a == b)] != 1).all()
    assert (real <= got.counts[:, :, 1:, 0]).all()
    assert not got.values[:, :, 0].any() and not got.counts[:, :, 0].any()
    assert not got.values[:, :, 1:][~live].any() and not got.counts[:, :, 1:][~live].any()
    np.testing.assert_allclose(got.means, got.values.mean(axis=0), rtol=1e-13)
    assert got.means.shape == (st.shape[1], N, len(coefs))
    return mir


# ---- 1. states and mirror parity across the state counts --------------------------------------

_parity = {}


def parity_run(ra, n):
    if n not in _parity:
        T, root, leaves, Q, rd, data, lik, seed = mc.parity_case(n)
        model = build(ra, T, root, n, Q, rd)
        batch = model.upload_sites(leaves, data, kind='state')
        coefs = mc.parity_coefs(n, seed)
        got = model.sample_mappings(batch, coefs, ndraws=mc.PARITY_DRAWS, seed=seed,
                                    first_draw=mc.PARITY_FIRST)
        _parity[n] = (model, batch, coefs, seed, Q, got)
    return _parity[n]


@pytest.mark.parametrize('n', mc.PARITY_NS)
def test_states_are_those_of_sample_states(ra, n):
    model, batch, coefs, seed, Q, got = parity_run(ra, n)
    want = model.sample_states(batch, ndraws=mc.PARITY_DRAWS, seed=seed,
                               first_draw=mc.PARITY_FIRST)
    assert got.states.dtype == np.uint8 and got.states.shape == (3, 33, 14)
    assert np.array_equal(got.states, want.states) and np.array_equal(got.status, want.status)
    assert (got.states < n).all() and got.nodes == want.nodes


@pytest.mark.parametrize('n', mc.PARITY_NS)
def test_mirror_parity(ra, n):
    model, batch, coefs, seed, Q, got = parity_run(ra, n)
    mir = check_parity(model, got, host_rates(model, Q), coefs, seed, mc.PARITY_FIRST,
                       want_status=np.zeros(33, dtype=np.int32))
    assert mir['picks'] >= 3 * 33 * 13
    assert got.counts[..., 1].max() >= 1           # (some path has a real change)


# ---- 2. per-edge rate matrices, a second set_rates ----------------------------------------------

@pytest.mark.parametrize('n', [4, 20, 61])
def test_per_edge_rates_and_new_rates(ra, n):
    T, root, leaves, Q, rd, data, lik, seed = mc.per_edge_case(n)
    model = build(ra, T, root, n, Q, rd)
    Qs, node_q, t = host_rates(model, Q)
    assert Qs.shape[0] > 1
    batch = model.upload_sites(leaves, data, kind='state')
    coefs = mc.parity_coefs(n, seed)
    got = model.sample_mappings(batch, coefs, ndraws=3, seed=seed)
    check_parity(model, got, (Qs, node_q, t), coefs, seed)
    # other matrices: nothing of the first call's tables may survive
    Q2 = mc.second_rates(Qs, seed)
    model.set_rates(Q=Q2, node_q=node_q, t=t)
    coefs2 = mc.parity_coefs(n, seed + 1)
    got2 = model.sample_mappings(batch, coefs2, ndraws=3, seed=seed + 1)
    check_parity(model, got2, (Q2, node_q, t), coefs2, seed + 1)
    assert not np.array_equal(got2.counts, got.counts)


# ---- 3. branch lengths --------------------------------------------------------------------------

@pytest.mark.parametrize('n', [7, 20])
def test_a_long_and_an_empty_branch(ra, n):
    """lam near 40 on one branch (dozens of path picks, another k at every site of a wave) and a
    branch of length 0 in the same tree."""
    T, root, leaves, Q, rd, data, lik, t, seed = mc.length_case(n)
    model = build(ra, T, root, n, rd=rd)
    node_q = np.zeros(model.tree.nnodes, dtype=np.int64)
    model.set_rates(Q=Q[None], node_q=node_q, t=t)
    batch = model.upload_sites(leaves, data, kind='state')
    coefs = mc.parity_coefs(n, seed)
    got = model.sample_mappings(batch, coefs, ndraws=3, seed=seed)
    check_parity(model, got, (Q[None], node_q, t), coefs, seed,
                 want_status=np.zeros(21, dtype=np.int32))
    long_v = int(np.argmax(t))
    zero_v = [v for v in range(1, len(t)) if t[v] == 0][0]
    k = got.counts[:, :, long_v, 0]
    assert k.min() >= 10 and k.max() <= 124 and len(np.unique(k)) > 5
    assert not got.counts[:, :, zero_v].any() and not got.values[:, :, zero_v].any()


def test_too_many_events(ra):
    n = 7
    T, root, leaves, Q, rd, data, lik, t, seed = mc.length_case(n)
    model = build(ra, T, root, n, rd=rd)
    node_q = np.zeros(model.tree.nnodes, dtype=np.int64)
    mu = (-np.diag(Q)).max()
    t = t.copy()
    t[int(np.argmax(t))] = 330.0 / mu          # K_v = ceil(330 + 10 sqrt(330) + 20) = 532
    model.set_rates(Q=Q[None], node_q=node_q, t=t)
    batch = model.upload_sites(leaves, data, kind='state')
    ll0, st0 = model.log_likelihoods(batch)
    with pytest.raises(ra.lib.RaotehHipError) as e:
        model.sample_mappings(batch, np.eye(n))
    assert e.value.code == ra.lib.RT_ERR_UNSUPPORTED
    ll1, st1 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(ll0, ll1) and np.array_equal(st0, st1)
    # ... and just inside the cap: lam = 300 gives K_v = 494
    t[int(np.argmax(t))] = 300.0 / mu
    model.set_rates(Q=Q[None], node_q=node_q, t=t)
    got = model.sample_mappings(batch, np.eye(n), ndraws=1, seed=2)
    assert got.counts[..., 0].max() > 200 and not got.status.any()


# ---- 4. splitting the draws, the outputs ----------------------------------------------------------

@pytest.mark.parametrize('nnodes', [14, 300])
def test_split_calls_and_draw_blocks(ra, nnodes):
    """One draw more than the block sample_states picks for the tree; draws [f, f + k) of one
    call are a call with first_draw = f, bit for bit."""
    n = 7
    DB = ra.lib.lib().rt_sample_states_draw_block(nnodes)
    nd = DB + 1
    T, root, leaves, Q, rd, data, lik = mc.split_case(nnodes)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    coefs = mc.parity_coefs(n, 3)
    whole = model.sample_mappings(batch, coefs, ndraws=nd, seed=3, first_draw=7)
    assert np.array_equal(whole.states,
                          model.sample_states(batch, ndraws=nd, seed=3, first_draw=7).states)
    f = nd // 2
    tail = model.sample_mappings(batch, coefs, ndraws=nd - f, seed=3, first_draw=7 + f)
    assert np.array_equal(tail.states, whole.states[f:])
    assert np.array_equal(tail.values, whole.values[f:])
    assert np.array_equal(tail.counts, whole.counts[f:])
    one = model.sample_mappings(batch, coefs, ndraws=1, seed=3, first_draw=7 + nd - 1)
    assert np.array_equal(one.values[0], whole.values[-1])
    if nnodes == 14:
        check_parity(model, whole, host_rates(model, Q), coefs, 3, 7)


def test_chunks_of_draws(ra, monkeypatch):
    """The draws pass through the device in chunks of RAOTEH_MAPPING_CHUNK_BYTES of per-draw
    output (256 MB unless set): one draw per chunk and three give the bits of a single chunk, with
    and without the per-draw arrays."""
    n, nd = 20, 7
    T, root, leaves, Q, rd, data, lik, seed = mc.parity_case(n)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    coefs = mc.parity_coefs(n, seed)
    whole = model.sample_mappings(batch, coefs, ndraws=nd, seed=seed)
    per_draw = 33 * model.tree.nnodes * (3 * 8 + 8)
    for chunk in (1, 3 * per_draw):
        monkeypatch.setenv('RAOTEH_MAPPING_CHUNK_BYTES', str(chunk))
        got = model.sample_mappings(batch, coefs, ndraws=nd, seed=seed)
        lean = model.sample_mappings(batch, coefs, ndraws=nd, seed=seed, per_draw=False)
        for k in ('states', 'values', 'counts', 'means', 'status'):
            assert np.array_equal(getattr(got, k), getattr(whole, k)), (chunk, k)
        assert np.array_equal(lean.means, whole.means) and lean.values is None
    monkeypatch.delenv('RAOTEH_MAPPING_CHUNK_BYTES')
    check_parity(model, whole, host_rates(model, Q), coefs, seed)


def test_every_combination_of_outputs(ra):
    lib = ra.lib
    n, nd = 20, 3
    T, root, leaves, Q, rd, data, lik, seed = mc.parity_case(n)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    coefs = mc.parity_coefs(n, seed)
    full = model.sample_mappings(batch, coefs, ndraws=nd, seed=seed)
    lean = model.sample_mappings(batch, coefs, ndraws=nd, seed=seed, per_draw=False)
    assert lean.values is None and lean.counts is None
    assert np.array_equal(lean.means, full.means) and np.array_equal(lean.states, full.states)
    S, N, K = 33, model.tree.nnodes, len(coefs)
    names = ['states', 'values', 'counts', 'means', 'status']
    for mask in itertools.product([False, True], repeat=5):
        out = dict(states=np.full((nd, S, N), 77, dtype=np.uint8),
                   values=np.full((nd, S, N, K), 7.0),
                   counts=np.full((nd, S, N, 2), 7, dtype=np.int32),
                   means=np.full((S, N, K), 7.0), status=np.full(S, 7, dtype=np.int32))
        ctype = dict(states=ctypes.c_ubyte, values=ctypes.c_double, counts=ctypes.c_int32,
                     means=ctypes.c_double, status=ctypes.c_int32)
        args = [out[k].ctypes.data_as(ctypes.POINTER(ctype[k])) if on else None
                for k, on in zip(names, mask)]
        lib.check(lib.lib().rt_sites_sample_mappings(
            model._h, batch._h, 0, seed, 0, nd, K,
            coefs.ctypes.data_as(ctypes.POINTER(ctypes.c_double)), *args))
        for k, on in zip(names, mask):
            if on:
                assert np.array_equal(out[k], getattr(full, k)), (mask, k)
            else:
                assert (out[k] == (77 if k == 'states' else 7)).all(), (mask, k)


# ---- 5. the law -----------------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_law(ra, n):
    """8192 draws of 2 sites: the means against the device's own exact expectations, within
    5 s / sqrt(ndraws) + 1e-9 per cell, s the sample standard deviation over the draws."""
    T, root, leaves, Q, rd, data, lik = sc.law_case(n)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    coefs = mc.parity_coefs(n, 11)
    nd = sc.LAW_DRAWS
    got = model.sample_mappings(batch, coefs, ndraws=nd, seed=sc.LAW_SEED)
    assert not got.status.any()
    want = model.branch_expectations(batch, coefs).values
    s = got.values.std(axis=0, ddof=1)
    dev = np.abs(got.means - want)
    print('n = %d: largest deviation %.3e, in units of its bound %.3f'
          % (n, dev.max(), (dev / (5 * s / np.sqrt(nd) + 1e-9)).max()))
    assert (dev <= 5 * s / np.sqrt(nd) + 1e-9).all()
    assert dev[:, 1:, :2].max() > 0


# ---- 6. observation kinds ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20, 70])
@pytest.mark.parametrize('kind', ['state', 'mask', 'dense'])
def test_observation_kinds(ra, kind, n):
    """Unobserved leaves, an observed internal node and (dense) a site of likelihood zero."""
    T, root, obs_nodes, Q, rd, data, lik = mc.kinds_case(kind, n)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(obs_nodes, data, kind=kind)
    coefs = mc.parity_coefs(n, n)
    got = model.sample_mappings(batch, coefs, ndraws=3, seed=9)
    want = model.sample_states(batch, ndraws=3, seed=9)
    assert np.array_equal(got.states, want.states) and np.array_equal(got.status, want.status)
    check_parity(model, got, host_rates(model, Q), coefs, 9)
    if kind == 'dense':
        assert got.status[-1] == 1 and (got.states[:, -1] == 255).all()
        assert not got.values[:, -1].any() and not got.counts[:, -1].any()
        assert not got.means[-1].any() and not got.status.all()
    else:
        assert not got.status.any()


# ---- 7. refusals ------------------------------------------------------------------------------------

def test_refusals(ra):
    lib = ra.lib
    n = 20
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=3)
    data, _ = sc.state_observations(n, 20, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    ll0, st0 = model.log_likelihoods(batch)
    name = batch.kernel_name
    E = np.eye(n)

    def untouched(b=batch, ll=ll0, st=st0, nm=name):
        got = model.fetch_log_likelihoods(b)
        assert np.array_equal(got[0], ll) and np.array_equal(got[1], st)
        assert b.kernel_name == nm

    for key in ('rescale', 'force_generic'):
        ra.ctx.set_option(key, 1)
        try:
            rb = model.upload_sites(leaves, data, kind='state')
        finally:
            ra.ctx.set_option(key, None)
        llr, str_ = model.log_likelihoods(rb)
        with pytest.raises(lib.RaotehHipError) as e:
            model.sample_mappings(rb, E)
        assert e.value.code == lib.RT_ERR_UNSUPPORTED, key
        untouched(rb, llr, str_, rb.kernel_name)
    # more than 8 coefficient matrices; no draw
    pE = np.zeros((9, n, n)).ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.lib().rt_sites_sample_mappings(model._h, batch._h, 0, 1, 0, 1, 9, pE, None, None,
                                            None, None, None)
    assert rc == lib.RT_ERR_UNSUPPORTED
    rc = lib.lib().rt_sites_sample_mappings(model._h, batch._h, 0, 1, 0, 0, 1, pE, None, None,
                                            None, None, None)
    assert rc == lib.RT_ERR_INVALID
    rc = lib.lib().rt_sites_sample_mappings(model._h, batch._h, 0, 1, 0, 1, 0, pE, None, None,
                                            None, None, None)
    assert rc == lib.RT_ERR_INVALID
    with pytest.raises(ValueError):
        model.sample_mappings(batch, np.zeros((9, n, n)))
    with pytest.raises(ValueError):
        model.sample_mappings(batch, E, ndraws=0)
    untouched()
    # a batch of another model
    other = build(ra, T, root, n, Q, rd)
    with pytest.raises(ValueError):
        other.sample_mappings(batch, E)
    untouched()
    # spectral rates, transitions set directly: no rate matrices for the paths
    P = model.get_transitions()
    direct = ra.device.TreeModel(T, root, n)
    direct.set_transitions(P)
    db = direct.upload_sites(leaves, data, kind='state')
    assert direct.sample_states(db).states.shape == (1, 20, model.tree.nnodes)
    pI = E.ctypes.data_as(ctypes.POINTER(ctypes.c_double))
    rc = lib.lib().rt_sites_sample_mappings(direct._h, db._h, 0, 1, 0, 1, 1, pI, None, None,
                                            None, None, None)
    assert rc == lib.RT_ERR_INVALID
    Qr = sc.rate_matrix(n, rng)
    spec = build(ra, T, root, n, Qr, rd)       # (rate matrices on the device, then spectral rates)
    spec.set_rates_spectral(np.eye(n), -np.ones(n), np.eye(n))
    sb = spec.upload_sites(leaves, data, kind='state')
    rc = lib.lib().rt_sites_sample_mappings(spec._h, sb._h, 0, 1, 0, 1, 1, pI, None, None, None,
                                            None, None)
    assert rc == lib.RT_ERR_INVALID
    # ... and with set_rates again the call goes through
    spec.set_rates(Q_default=Qr)
    assert spec.sample_mappings(sb, E).means.shape == (20, model.tree.nnodes, 1)


def test_one_node_tree(ra):
    import networkx as nx
    T = nx.Graph()
    T.add_node(7)
    model = ra.device.TreeModel(T, 7, 4)
    model.set_rates(Q_default=ra.synth.jukes_cantor(4)[0])
    model.set_root_distn(np.array([0.25, 0.5, 0.0, 0.25]))
    batch = model.upload_sites([7], np.array([[255], [1], [2]], dtype=np.uint8), kind='state')
    got = model.sample_mappings(batch, np.eye(4), ndraws=8, seed=6, first_draw=10)
    want = model.sample_states(batch, ndraws=8, seed=6, first_draw=10)
    assert np.array_equal(got.states, want.states) and got.status.tolist() == [0, 0, 1]
    assert got.values.shape == (8, 3, 1, 1) and not got.values.any() and not got.means.any()
    assert got.counts.shape == (8, 3, 1, 2) and not got.counts.any()
