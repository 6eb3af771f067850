"""rt_sites_sample_states (TreeModel.sample_states, _sample_mcy_dense.resample_states) on the
device.  The central check is the replay of tests/_sample_cases.py: with the device's own P, the
oracle's subtree likelihoods and the uniforms of _philox, every node of every draw of every
site must be the state the pinned rule picks given the device's pick at the parent."""
import ctypes

import networkx as nx
import numpy as np
import pytest

from conftest import switching_cases
from _posterior_cases import oracle_pmaps, oracle_site
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


def observe(kind, n, nsites, nobs, rng):
    if kind == 'state':
        return sc.state_observations(n, nsites, nobs, rng)
    if kind == 'mask':
        return sc.mask_observations(n, nsites, nobs, rng)
    return sc.dense_observations(n, nsites, nobs, rng)


def build(ra, T, root, n, Q=None, rd=None, esd=None):
    model = ra.device.TreeModel(T, root, n)
    if esd is not None:
        model.set_transitions(esd)
    elif Q is not None:
        model.set_rates(Q_default=Q)
    if rd is not None:
        model.set_root_distn(rd)
    return model


def oracle_L(model, obs_nodes, lik):
    ta = model.tree
    esd = model.get_transitions()              # the device's own P
    cols = [ta.node_to_index[v] for v in obs_nodes]
    return esd, oracle_pmaps(ta.indices, ta.indptr, esd, cols, lik)


def sample_and_replay(ra, model, obs_nodes, data, lik, kind, rd, ndraws, seed, first_draw=0):
    batch = model.upload_sites(obs_nodes, data, kind=kind)
    got = model.sample_states(batch, ndraws=ndraws, seed=seed, first_draw=first_draw)
    assert got.nodes == list(model.tree.preorder_nodes)
    assert got.states.shape == (ndraws, len(lik), model.tree.nnodes)
    esd, L = oracle_L(model, obs_nodes, lik)
    checked = sc.replay_check(got.states, got.status, esd, L, rd, model.tree.parent, seed,
                              first_draw)
    return batch, got, esd, L, checked


# ---- 1. the replay check -------------------------------------------------------------------

@pytest.mark.parametrize('n', [2, 3, 4, 5, 16, 17, 20, 61, 64, 65, 122, 128])
def test_replay_across_state_counts(ra, n):
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=40 + n, nnodes=14)
    data, lik = sc.state_observations(n, 33, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    _, got, _, _, checked = sample_and_replay(ra, model, leaves, data, lik, 'state', rd, 3,
                                              seed=1000 + n, first_draw=2 ** 40 + 5)
    assert not got.status.any() and checked == 3 * 33 * 14


@pytest.mark.parametrize('nnodes', [14, 300, 1500])
def test_replay_draw_blocking(ra, nnodes):
    """One draw more than the block the host picks for the tree: 16, 6 and 1 draws."""
    n = 7
    DB = ra.lib.lib().rt_sample_states_draw_block(nnodes)
    assert DB == {14: 16, 300: 6, 1500: 1}[nnodes]
    T, root, leaves = sc.broom_tree(nnodes, nleaves=4, seed=nnodes)
    rng = np.random.RandomState(nnodes)
    Q = sc.rate_matrix(n, rng)
    rd = rng.uniform(0.1, 1.0, n)
    data, lik = sc.state_observations(n, 17, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    _, got, _, _, checked = sample_and_replay(ra, model, leaves, data, lik, 'state', rd, DB + 1,
                                              seed=3)
    assert not got.status.any() and checked == (DB + 1) * 17 * nnodes


@pytest.mark.parametrize('n', [4, 20, 70])
@pytest.mark.parametrize('kind', ['state', 'mask', 'dense'])
def test_replay_observation_kinds(ra, kind, n):
    """Unobserved leaves, an observed internal node and (dense) a site of likelihood zero."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=7 * n + len(kind), nnodes=14)
    internal = [v for v in T if v != root and v not in leaves][0]
    obs_nodes = list(leaves) + [internal]
    data, lik = observe(kind, n, 21, len(obs_nodes), rng)
    model = build(ra, T, root, n, Q, rd)
    _, got, _, L, _ = sample_and_replay(ra, model, obs_nodes, data, lik, kind, rd, 3, seed=9)
    if kind == 'state':
        assert (data == 255).any() and not got.status.any()
        # an observed node is sampled at its observed state
        for k, v in enumerate(obs_nodes):
            col = got.states[:, :, model.tree.node_to_index[v]]
            seen = data[:, k] != 255
            assert (col[:, seen] == data[seen, k]).all()
    if kind == 'dense':
        # (the replay check holds the status to the oracle's: other sites may be dead as well, a
        # dense vector of four states is all zero once in 600)
        assert got.status[-1] == 1 and (got.states[:, -1] == 255).all()
        assert not got.status.all()


@pytest.mark.parametrize('n', [4, 20, 61])
def test_replay_per_edge_rates(ra, n):
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=7 + n, nnodes=16, per_edge=True)
    assert any('Q' in d for _, _, d in T.edges(data=True))
    data, lik = sc.state_observations(n, 21, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    sample_and_replay(ra, model, leaves, data, lik, 'state', rd, 3, seed=n)


@pytest.mark.parametrize('n', [4, 24])
def test_replay_sparse_transitions(ra, n):
    """Transitions set directly, with structural zeros: no sampled edge uses one."""
    T, root, leaves, _, rd, rng = sc.random_case(n, seed=70 + n, nnodes=14)
    N = len(T)
    esd = rng.uniform(0.1, 1.0, (N, n, n)) * (rng.uniform(size=(N, n, n)) < 0.4)
    esd[:, np.arange(n), np.arange(n)] += 0.5
    esd /= esd.sum(axis=2, keepdims=True)
    esd[0] = 0.0
    data, lik = sc.state_observations(n, 33, len(leaves), rng, unobserved=0.3)
    model = build(ra, T, root, n, rd=rd, esd=esd)
    _, got, P, L, _ = sample_and_replay(ra, model, leaves, data, lik, 'state', rd, 4, seed=2)
    assert np.array_equal(P[1:], esd[1:]) and (esd[1:] == 0).any()
    live = got.status == 0
    assert live.any()
    st = got.states[:, live].astype(np.int64)
    parent = model.tree.parent
    for v in range(N):
        assert (L[live][np.arange(live.sum())[None, :], v, st[:, :, v]] > 0).all()
        if v:
            assert (esd[v][st[:, :, parent[v]], st[:, :, v]] > 0).all()


@pytest.mark.parametrize('n', [5, 61])
def test_round_trip(ra, n):
    """The draws uploaded as observed states at every node: each log-likelihood is the log of
    root_w[s_root] * prod_v P_v[s_parent][s_v]."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=11 + n, nnodes=14)
    data, lik = sc.state_observations(n, 19, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    ndraws = 3
    got = model.sample_states(batch, ndraws=ndraws, seed=8)
    assert not got.status.any() and (got.states < n).all()
    flat = got.states.reshape(ndraws * 19, -1)
    again = model.upload_sites(got.nodes, flat, kind='state')
    ll, st = model.log_likelihoods(again)
    assert not st.any() and np.isfinite(ll).all()
    P = model.get_transitions()
    parent = model.tree.parent
    s = flat.astype(np.int64)
    want = np.log(rd[s[:, 0]])
    for v in range(1, s.shape[1]):
        want = want + np.log(P[v][s[:, parent[v]], s[:, v]])
    np.testing.assert_allclose(ll, want, rtol=1e-10, atol=1e-10)
    # the sampled leaves are the observed ones
    for k, v in enumerate(leaves):
        seen = data[:, k] != 255
        assert (got.states[:, seen, model.tree.node_to_index[v]] == data[seen, k]).all()


# ---- 2. the law ----------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_law(ra, n):
    """8192 draws of 2 sites against the device's own posteriors, 5 sigma + 1e-9 per cell: every
    node marginal, eight joint endpoint sets per edge; at n = 4 also the oracle's full joint."""
    T, root, leaves, Q, rd, data, lik = sc.law_case(n)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    nd = sc.LAW_DRAWS
    got = model.sample_states(batch, ndraws=nd, seed=sc.LAW_SEED)
    assert not got.status.any()
    esets = sc.law_edge_sets(n)
    post = model.posteriors(batch, edge_sets=esets, marginals=True)
    parent = model.tree.parent
    st = got.states.astype(np.int64)
    for i in range(sc.LAW_SITES):
        assert sc.law_set_deviation(st[:, i], post.marginals[i], post.edge_values[i], esets,
                                    parent) <= 0.0, i
    if n == 4:
        esd, L = oracle_L(model, leaves, lik)
        ta = model.tree
        for i in range(sc.LAW_SITES):
            D, J = oracle_site(ta.indices, ta.indptr, esd, rd, L[i])
            assert sc.law_deviation(st[:, i], D, J, parent) <= 0.0


# ---- 3. the counter layout -----------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_reproducibility(ra, n):
    lib = ra.lib
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=21 + n, nnodes=21)
    data, _ = sc.state_observations(n, 70, len(leaves), rng, unobserved=0.0)
    model = build(ra, T, root, n, Q, rd)
    batches = {}
    try:
        for jit in (0, 1):
            lib.check(lib.lib().rt_set_option(b'jit', jit))
            batches[jit] = model.upload_sites(leaves, data, kind='state')
            model.prune(batches[jit])
    finally:
        lib.check(lib.lib().rt_set_option(b'jit', -1))
    assert 'jit' in batches[1].kernel_name and 'jit' not in batches[0].kernel_name
    a = model.sample_states(batches[0], ndraws=5, seed=123)
    b = model.sample_states(batches[0], ndraws=5, seed=123)
    assert np.array_equal(a.states, b.states) and np.array_equal(a.status, b.status)
    head = model.sample_states(batches[0], ndraws=2, seed=123)
    tail = model.sample_states(batches[0], ndraws=3, seed=123, first_draw=2)
    assert np.array_equal(np.concatenate([head.states, tail.states]), a.states)
    c = model.sample_states(batches[1], ndraws=5, seed=123)
    assert np.array_equal(c.states, a.states)
    assert 'jit' in batches[1].kernel_name
    d = model.sample_states(batches[0], ndraws=5, seed=124)
    assert not np.array_equal(d.states, a.states)
    # a draw does not depend on ndraws (more than one draw block)
    e = model.sample_states(batches[0], ndraws=40, seed=123)
    assert np.array_equal(e.states[:5], a.states)


@pytest.mark.parametrize('n', [4, 20, 90])
def test_the_batch_is_left_as_it_was(ra, n):
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=61 + n, nnodes=18)
    data, _ = sc.dense_observations(n, 70, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='dense')
    ll0, st0 = model.log_likelihoods(batch)
    tot0 = model.fetch_totals(batch)
    name = batch.kernel_name
    model.sample_states(batch, ndraws=2, seed=1)
    ll1, st1 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(ll0, ll1) and np.array_equal(st0, st1)
    assert np.array_equal(tot0, model.fetch_totals(batch))
    assert batch.kernel_name == name
    clone = batch.clone()
    ll2, st2 = model.fetch_log_likelihoods(clone)
    assert np.array_equal(ll0, ll2) and np.array_equal(st0, st2)
    ll3, st3 = model.log_likelihoods(batch)
    assert np.array_equal(ll0, ll3) and np.array_equal(st0, st3)
    assert np.array_equal(tot0, model.fetch_totals(batch))


# ---- 4. big trees --------------------------------------------------------------------------

@pytest.mark.parametrize('nnodes', [4096, 8192])
def test_big_tree(ra, nnodes):
    """4096 nodes (one draw per block, a 64 KB table) and the stated limit (128 KB), the shapes
    test_sample_states_cpu.py checks against underflow."""
    n = 5
    assert nnodes <= ra.lib.RT_MAX_SAMPLE_NODES
    T, root, leaves = sc.broom_tree(nnodes)
    rng = np.random.RandomState(8)
    Q = sc.rate_matrix(n, rng)
    _, lik = sc.state_observations(n, 17, len(leaves), rng, unobserved=0.0)
    data = lik.argmax(axis=2).astype(np.uint8)
    model = build(ra, T, root, n, Q)
    _, got, _, L, checked = sample_and_replay(ra, model, leaves, data, lik, 'state', None, 2,
                                              seed=nnodes)
    assert (L[:, 0].sum(axis=1) > 1e-280).all()
    assert not got.status.any() and checked == 2 * 17 * nnodes


def test_beyond_the_node_limit(ra):
    n = 5
    lim = ra.lib.RT_MAX_SAMPLE_NODES
    T, root, leaves = sc.broom_tree(lim + 1)
    rng = np.random.RandomState(9)
    data, _ = sc.state_observations(n, 3, len(leaves), rng, unobserved=0.0)
    model = build(ra, T, root, n, sc.rate_matrix(n, rng))
    batch = model.upload_sites(leaves, data, kind='state')
    ll0, st0 = model.log_likelihoods(batch)
    with pytest.raises(ra.lib.RaotehHipError) as e:
        model.sample_states(batch)
    assert e.value.code == ra.lib.RT_ERR_UNSUPPORTED
    ll1, st1 = model.log_likelihoods(batch)
    assert np.array_equal(ll0, ll1) and np.array_equal(st0, st1)


# ---- 5. errors -----------------------------------------------------------------------------

def test_errors(ra):
    lib = ra.lib
    n = 20
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=3)
    data, _ = sc.state_observations(n, 20, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    ll0, st0 = model.log_likelihoods(batch)
    name = batch.kernel_name

    def untouched(b=batch, ll=ll0, st=st0, nm=name):
        got = model.fetch_log_likelihoods(b)
        assert np.array_equal(got[0], ll) and np.array_equal(got[1], st)
        assert b.kernel_name == nm

    out = np.zeros((1, 20, model.tree.nnodes), dtype=np.uint8)
    rc = lib.lib().rt_sites_sample_states(model._h, batch._h, 0, 1, 0, 0,
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)), None)
    assert rc == lib.RT_ERR_INVALID
    rc = lib.lib().rt_sites_sample_states(model._h, batch._h, 0, 1, 0, 1, None, None)
    assert rc == lib.RT_ERR_INVALID
    with pytest.raises(ValueError):
        model.sample_states(batch, ndraws=0)
    untouched()
    # a batch of another model
    other = build(ra, T, root, n, Q, rd)
    with pytest.raises(ValueError):
        other.sample_states(batch)
    untouched()
    # a rescale batch, a generic-kernel batch
    for key in ('rescale', 'force_generic'):
        ra.ctx.set_option(key, 1)
        try:
            rb = model.upload_sites(leaves, data, kind='state')
        finally:
            ra.ctx.set_option(key, None)
        llr, str_ = model.log_likelihoods(rb)
        with pytest.raises(lib.RaotehHipError) as e:
            model.sample_states(rb)
        assert e.value.code == lib.RT_ERR_UNSUPPORTED, key
        untouched(rb, llr, str_, rb.kernel_name)
    # a model without transitions
    bare = ra.device.TreeModel(T, root, n)
    bb = bare.upload_sites(leaves, data, kind='state')
    with pytest.raises(ValueError):
        bare.sample_states(bb)
    bare.set_rates(Q_default=Q)
    assert bare.sample_states(bb).states.shape == (1, 20, model.tree.nnodes)


# ---- 6. the mirrors, the one-node tree -----------------------------------------------------

def test_mirror_on_the_switching_model(ra):
    """_sample_mcy_dense.resample_states, 122 states with allowed sets: every state inside its
    node's set, the replay check with the seed passed in; the structural-zero site raises."""
    from raoteh_amd import _sample_mcy_dense as smcy, StructuralZeroProb
    fx, cases = switching_cases()
    n2 = fx['ncompound']
    done = set()
    for c in cases:
        zero = c['want']['likelihood'] == 0.0     # (the reference's record of the site)
        if zero in done:
            continue
        done.add(zero)
        T = c['T'].copy()                      # (one graph for both: the same preorder)
        model = build(ra, T, c['root'], n2, c['Q_compound'], c['compound_distn'])
        esd = model.get_transitions()
        ta = model.tree
        for v in range(1, ta.nnodes):
            T[ta.preorder_nodes[ta.parent[v]]][ta.preorder_nodes[v]]['P'] = esd[v]
        if zero:
            with pytest.raises(StructuralZeroProb):
                smcy.resample_states(T, c['root'], n2, c['allowed'], c['compound_distn'], seed=5)
            continue
        got = smcy.resample_states(T, c['root'], n2, node_to_allowed_states=c['allowed'],
                                   root_distn=c['compound_distn'], seed=5)
        assert sorted(got) == sorted(T)
        assert all(got[v] in c['allowed'][v] for v in T)
        lik = np.zeros((1, ta.nnodes, n2))
        for i, v in enumerate(ta.preorder_nodes):
            lik[0, i, sorted(c['allowed'][v])] = 1.0
        L = oracle_pmaps(ta.indices, ta.indptr, esd, list(range(ta.nnodes)), lik)
        states = np.array([[[got[v] for v in ta.preorder_nodes]]], dtype=np.uint8)
        sc.replay_check(states, [0], esd, L, c['compound_distn'], ta.parent, seed=5)
    assert done == {False, True}


def test_one_node_tree_on_the_host(ra):
    T = nx.Graph()
    T.add_node(7)
    w = np.array([0.25, 0.5, 0.0, 0.25])
    model = ra.device.TreeModel(T, 7, 4)
    model.set_rates(Q_default=ra.synth.jukes_cantor(4)[0])
    model.set_root_distn(w)
    batch = model.upload_sites([7], np.array([[255], [1], [2]], dtype=np.uint8), kind='state')
    got = model.sample_states(batch, ndraws=64, seed=6, first_draw=10)
    assert got.status.tolist() == [0, 0, 1] and got.nodes == [7]
    assert (got.states[:, 1, 0] == 1).all() and (got.states[:, 2, 0] == 255).all()
    assert set(got.states[:, 0, 0].tolist()) == {0, 1, 3}
    L = np.array([[[1.0] * 4], [[0, 1.0, 0, 0]], [[0, 0, 1.0, 0]]])
    sc.replay_check(got.states, got.status, np.zeros((1, 4, 4)), L, w, np.array([-1]), 6, 10)
