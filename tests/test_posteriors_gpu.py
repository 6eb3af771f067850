"""rt_sites_posteriors (TreeModel.posteriors, _mjp_dense.get_posterior_summaries_batch) on the
device: the 122-state switching model against the reference's record
(tests/golden/switching_posteriors.json), the oracle's node marginals and joint endpoint
posteriors over random trees, sets and all three observation kinds, internal identities, the
batch left as it was, and the error cases."""
import networkx as nx
import numpy as np
import pytest

from conftest import load_golden, switching_cases
from oracle import oracle_numpy as orc
from _posterior_cases import oracle_pmaps, oracle_site, sums_over_sets

pytestmark = pytest.mark.gpu

RTOL = 1e-10


@pytest.fixture(scope='module')
def ra():
    import raoteh_amd
    from raoteh_amd import _mjp_dense, device, _lib, synth

    class NS(object):
        pass
    ns = NS()
    ns.pkg = raoteh_amd
    ns.mjp, ns.device, ns.lib, ns.synth = _mjp_dense, device, _lib, synth
    ns.ctx = device.get_context()
    # kernels are compiled inside rt_sites_create, not in the background
    _lib.check(_lib.lib().rt_set_option(b'jit_async', 0))
    return ns


def random_model(n, seed, nnodes=14, per_edge=False):
    from raoteh_amd import synth
    rng = np.random.RandomState(seed)
    T, root, leaves = synth.random_tree(nnodes, seed=seed)
    def rate():
        R = rng.uniform(0.1, 1.0, (n, n)) * (rng.uniform(size=(n, n)) < 0.7)
        np.fill_diagonal(R, 0.0)
        R[np.arange(n), (np.arange(n) + 1) % n] += 0.3            # irreducible
        return R - np.diag(R.sum(axis=1))
    Q = rate()
    if per_edge:
        for na, nb in nx.bfs_edges(T, root):
            if rng.uniform() < 0.5:
                T[na][nb]['Q'] = rate()
    root_distn = rng.uniform(0.1, 1.0, n)
    root_distn /= root_distn.sum()
    return T, root, leaves, Q, root_distn, rng


def random_sets(n, rng):
    def sub():
        k = rng.randint(1, n + 1)
        return sorted(rng.choice(n, size=k, replace=False).tolist())
    h = max(1, n // 2)
    lo, hi, every = list(range(h)), list(range(h, n)) or [0], list(range(n))
    node_sets = [lo, sub(), sub()]
    S = sub()
    edge_sets = [(lo, hi), (hi, lo), (every, S), (S, every), (sub(), sub())]
    return node_sets, edge_sets


def observations(kind, n, nsites, nobs, rng):
    """(data for upload_sites, obs_lik f64[nsites, nobs, n] as the oracle reads it)."""
    if kind == 'state':
        st = rng.randint(0, n, size=(nsites, nobs))
        st[rng.uniform(size=st.shape) < 0.1] = 255
        lik = np.zeros((nsites, nobs, n))
        for i in range(nsites):
            for k in range(nobs):
                if st[i, k] == 255:
                    lik[i, k] = 1.0
                else:
                    lik[i, k, st[i, k]] = 1.0
        return st.astype(np.uint8), lik
    if kind == 'mask':
        bits = rng.uniform(size=(nsites, nobs, n)) < 0.4
        bits[:, :, 0] |= ~bits.any(axis=2)
        words = np.zeros((nsites, nobs, 2), dtype=np.uint64)
        for s in range(n):
            words[:, :, s >> 6] |= bits[:, :, s].astype(np.uint64) << np.uint64(s & 63)
        data = words[:, :, 0].copy() if n <= 64 else words
        return data, bits.astype(np.float64)
    lik = rng.uniform(0.0, 1.0, size=(nsites, nobs, n))
    lik[rng.uniform(size=lik.shape) < 0.2] = 0.0
    lik[-1, 0] = 0.0                           # a site of likelihood zero
    return lik, lik


def check_against_oracle(ra, T, root, leaves, n, Q, root_distn, kind, nsites, rng,
                         check_sites=None, marginal_subset=True):
    obs_nodes = list(leaves)
    data, obs_lik = observations(kind, n, nsites, len(obs_nodes), rng)
    model = ra.device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    model.set_root_distn(root_distn)
    batch = model.upload_sites(obs_nodes, data, kind=kind)
    node_sets, edge_sets = random_sets(n, rng)
    nodes = model.tree.preorder_nodes
    mnodes = [nodes[0], nodes[-1], obs_nodes[0]] if marginal_subset else None
    post = model.posteriors(batch, node_sets=node_sets, edge_sets=edge_sets,
                            marginal_nodes=mnodes, marginals=True)
    assert post.nodes == list(nodes)
    pre, idx, ptr, esd = orc.get_expm_augmented_transitions(T, root, n, Q_default=Q)
    assert pre == list(nodes)
    esd = model.get_transitions()              # the device's P (the oracle's expm is checked
    cols = [pre.index(v) for v in obs_nodes]   # against it elsewhere)
    sites = check_sites if check_sites is not None else range(nsites)
    L = oracle_pmaps(idx, ptr, esd, cols, obs_lik[list(sites)])
    mrows = [pre.index(v) for v in post.marginal_nodes]
    for j, i in enumerate(sites):
        got = oracle_site(idx, ptr, esd, root_distn, L[j])
        if got is None:
            assert post.status[i] == 1
            assert not post.node_values[i].any() and not post.edge_values[i].any()
            assert not post.marginals[i].any()
            continue
        assert post.status[i] == 0, (i, post.status[i])
        D, J = got
        nv, ev = sums_over_sets(D, J, node_sets, edge_sets)
        np.testing.assert_allclose(post.node_values[i], nv, rtol=RTOL, atol=1e-15)
        np.testing.assert_allclose(post.edge_values[i], ev, rtol=RTOL, atol=1e-15)
        np.testing.assert_allclose(post.marginals[i], D[mrows], rtol=RTOL, atol=1e-15)
    return model, batch, post, node_sets, edge_sets


# ---- 1. reference pin ------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['mask', 'dense'])
def test_switching_model_matches_the_reference(ra, kind):
    fx, cases = switching_cases()
    ref = load_golden('switching_posteriors')
    n1, n2 = fx['nstates'], fx['ncompound']
    lo, hi = list(range(n1)), list(range(n1, n2))
    seen_zero = False
    for c, want in zip(cases, ref['sites']):
        assert sorted(want['benign_states']) == sorted(c['want']['benign_states'])
        model = ra.device.TreeModel(c['T'], c['root'], n2)
        model.set_rates(Q_default=c['Q_compound'])
        model.set_root_distn(c['compound_distn'])
        leaves = [v for v in model.tree.preorder_nodes if len(c['allowed'][v]) < n2]
        bits = np.zeros((1, len(leaves), n2), dtype=bool)
        for k, v in enumerate(leaves):
            bits[0, k, sorted(c['allowed'][v])] = True
        if kind == 'mask':
            data = np.zeros((1, len(leaves), 2), dtype=np.uint64)
            for s in range(n2):
                data[:, :, s >> 6] |= bits[:, :, s].astype(np.uint64) << np.uint64(s & 63)
        else:
            data = bits.astype(np.float64)
        batch = model.upload_sites(leaves, data, kind=kind)
        mnodes = [ref['original_root'], ref['leaf_node']]
        post = model.posteriors(batch, node_sets=[lo], edge_sets=[(lo, hi), (hi, lo)],
                                marginal_nodes=mnodes)
        if want['structural_zero']:
            seen_zero = True
            assert post.status[0] == 1
            assert not post.node_values.any() and not post.edge_values.any()
            assert not post.marginals.any()
            continue
        assert post.status[0] == 0
        pos = dict((v, i) for i, v in enumerate(post.nodes))
        for v, p in want['p_primary'].items():
            assert post.node_values[0, pos[int(v)], 0] == pytest.approx(p, rel=1e-10, abs=1e-13)
        for v, p in want['switch'].items():
            assert post.edge_values[0, pos[int(v)], 0] == pytest.approx(p, rel=1e-10, abs=1e-13)
        for v, p in want['switch_back'].items():
            assert post.edge_values[0, pos[int(v)], 1] == pytest.approx(p, rel=1e-10, abs=1e-13)
        assert post.edge_values[0, pos[c['root']]].tolist() == [0.0, 0.0]
        np.testing.assert_allclose(post.marginals[0, 0], want['original_root_distn'], rtol=1e-10,
                                   atol=1e-13)
        np.testing.assert_allclose(post.marginals[0, 1], want['leaf_distn'], rtol=1e-10,
                                   atol=1e-13)
    assert seen_zero


def test_batch_helper_matches_the_reference(ra):
    """get_posterior_summaries_batch with node_to_allowed_states dicts of 122 states."""
    fx, cases = switching_cases()
    ref = load_golden('switching_posteriors')
    n1, n2 = fx['nstates'], fx['ncompound']
    lo, hi = list(range(n1)), list(range(n1, n2))
    c, want = cases[0], ref['sites'][0]
    out = ra.mjp.get_posterior_summaries_batch(
        c['T'], c['root'], n2, sites=[c['allowed']] * 3, root_distn=c['compound_distn'],
        Q_default=c['Q_compound'], node_sets=[lo], edge_sets=[(lo, hi)],
        marginal_nodes=[ref['original_root']])
    assert out['status'].tolist() == [0, 0, 0]
    for (na, nb), arr in out['edge_values'].items():
        np.testing.assert_allclose(arr[:, 0], want['switch'][str(nb)], rtol=1e-10, atol=1e-13)
    for v, arr in out['node_values'].items():
        np.testing.assert_allclose(arr[:, 0], want['p_primary'][str(v)], rtol=1e-10, atol=1e-13)
    np.testing.assert_allclose(out['marginals'][ref['original_root']][2],
                               want['original_root_distn'], rtol=1e-10, atol=1e-13)


# ---- 2. oracle parity across sizes -----------------------------------------------------------

SIZES = [2, 3, 4, 5, 8, 13, 20, 33, 61, 64, 65, 90, 122, 128]


@pytest.mark.parametrize('n', SIZES)
def test_oracle_parity(ra, n):
    kinds = ['state', 'mask', 'dense']
    for k, kind in enumerate(kinds):
        T, root, leaves, Q, rd, rng = random_model(n, seed=100 * n + k, nnodes=9 + k)
        nsites = 37 if n > 64 else 53                       # not a multiple of 16
        check = [0, 1, 17, nsites - 1]
        check_against_oracle(ra, T, root, leaves, n, Q, rd, kind, nsites, rng, check_sites=check,
                             marginal_subset=(k != 1))


@pytest.mark.parametrize('n', [4, 20, 61])
def test_oracle_parity_per_edge_rates(ra, n):
    T, root, leaves, Q, rd, rng = random_model(n, seed=7 + n, nnodes=16, per_edge=True)
    assert any('Q' in d for _, _, d in T.edges(data=True))
    check_against_oracle(ra, T, root, leaves, n, Q, rd, 'dense', 21, rng)


def test_tree_specialised_batch(ra):
    """A batch that runs the tree-specialised kernel: same sums, and it keeps that kernel."""
    lib = ra.lib
    lib.check(lib.lib().rt_set_option(b'jit', 1))
    try:
        n = 20
        T, root, leaves, Q, rd, rng = random_model(n, seed=5, nnodes=21)
        model, batch, post, _, _ = check_against_oracle(
            ra, T, root, leaves, n, Q, rd, 'state', 300, np.random.RandomState(3),
            check_sites=[0, 150, 299])
        model.prune(batch)
        name = batch.kernel_name
        assert 'jit' in name, name
        model.posteriors(batch, node_sets=[[0, 1]])
        assert batch.kernel_name == name
    finally:
        lib.check(lib.lib().rt_set_option(b'jit', -1))


# ---- 3. identities ---------------------------------------------------------------------------

@pytest.mark.parametrize('n', [3, 13, 90])
def test_internal_identities(ra, n):
    T, root, leaves, Q, rd, rng = random_model(n, seed=31 + n, nnodes=15)
    data, _ = observations('state', n, 40, len(leaves), rng)
    model = ra.device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    model.set_root_distn(rd)
    batch = model.upload_sites(leaves, data, kind='state')
    every = list(range(n))
    S = sorted(rng.choice(n, size=max(1, n // 3), replace=False).tolist())
    post = model.posteriors(batch, node_sets=[every, S],
                            edge_sets=[(every, every), (every, S), (S, every)], marginals=True)
    assert not post.status.any()
    np.testing.assert_allclose(post.marginals.sum(axis=2), 1.0, rtol=1e-12)
    np.testing.assert_allclose(post.node_values[:, :, 0], 1.0, rtol=1e-12)
    np.testing.assert_allclose(post.edge_values[:, 1:, 0], 1.0, rtol=1e-12)
    # (all, S) at v = the node value of S at v; (S, all) at v = the node value of S at the parent
    parent = model.tree.parent
    np.testing.assert_allclose(post.edge_values[:, 1:, 1], post.node_values[:, 1:, 1],
                               rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(post.edge_values[:, 1:, 2], post.node_values[:, parent[1:], 1],
                               rtol=1e-12, atol=1e-15)
    again = model.posteriors(batch, node_sets=[every, S],
                             edge_sets=[(every, every), (every, S), (S, every)], marginals=True)
    for a, b in zip(post[:4], again[:4]):
        assert np.array_equal(a, b)


# ---- 4. no side effects ----------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20, 90])
def test_the_batch_is_left_as_it_was(ra, n):
    T, root, leaves, Q, rd, rng = random_model(n, seed=61 + n, nnodes=18)
    data, _ = observations('dense', n, 70, len(leaves), rng)
    model = ra.device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    model.set_root_distn(rd)
    batch = model.upload_sites(leaves, data, kind='dense')
    ll0, st0 = model.log_likelihoods(batch)
    tot0 = model.fetch_totals(batch)
    name = batch.kernel_name
    expect0 = model.expected_history_statistics(batch) if n <= 64 else None
    model.posteriors(batch, node_sets=[[0]], edge_sets=[([0], [1])], marginals=True)
    ll1, st1 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(ll0, ll1) and np.array_equal(st0, st1)
    assert np.array_equal(tot0, model.fetch_totals(batch))
    assert batch.kernel_name == name
    ll2, st2 = model.log_likelihoods(batch)
    assert np.array_equal(ll0, ll2) and np.array_equal(st0, st2)
    assert np.array_equal(tot0, model.fetch_totals(batch))
    if expect0 is not None:
        expect1 = model.expected_history_statistics(batch)
        for a, b in zip(expect0, expect1):
            assert np.array_equal(a, b)


# ---- 5. errors -------------------------------------------------------------------------------

def test_errors(ra):
    lib = ra.lib
    n = 20
    T, root, leaves, Q, rd, rng = random_model(n, seed=3)
    data, _ = observations('state', n, 20, len(leaves), rng)
    model = ra.device.TreeModel(T, root, n)
    model.set_rates(Q_default=Q)
    batch = model.upload_sites(leaves, data, kind='state')
    with pytest.raises(ValueError):
        model.posteriors(batch, node_sets=[[n]])
    with pytest.raises(ValueError):
        model.posteriors(batch, edge_sets=[([0], [-1])])
    with pytest.raises(ValueError):
        model.posteriors(batch, node_sets=[[0]] * 9)
    with pytest.raises(ValueError):
        model.posteriors(batch, marginal_nodes=['not a node'])
    # the C ABI itself: 9 sets
    import ctypes
    masks = np.zeros((9, 2), dtype=np.uint64)
    masks[:, 0] = 1
    out = np.zeros((20, model.tree.nnodes, 9))
    rc = lib.lib().rt_sites_posteriors(model._h, batch._h, 0, 9,
                                       masks.ctypes.data_as(ctypes.c_void_p), 0, None, 0, None,
                                       out.ctypes.data_as(ctypes.POINTER(ctypes.c_double)),
                                       None, None, None)
    assert rc == lib.RT_ERR_UNSUPPORTED
    # a rescale batch
    ra.ctx.set_option('rescale', 1)
    try:
        rb = model.upload_sites(leaves, data, kind='state')
    finally:
        ra.ctx.set_option('rescale', None)
    with pytest.raises(lib.RaotehHipError) as e:
        model.posteriors(rb, node_sets=[[0]])
    assert e.value.code == lib.RT_ERR_UNSUPPORTED


def test_one_node_tree_on_the_host(ra):
    T = nx.Graph()
    T.add_node(7)
    w = np.array([0.25, 0.5, 0.125, 0.125])
    model = ra.device.TreeModel(T, 7, 4)
    model.set_rates(Q_default=ra.synth.jukes_cantor(4)[0])
    model.set_root_distn(w)
    batch = model.upload_sites([7], np.array([[255], [1], [3]], dtype=np.uint8), kind='state')
    post = model.posteriors(batch, node_sets=[[0, 1]], edge_sets=[([0], [1])], marginals=True)
    np.testing.assert_allclose(post.marginals[0, 0], w / w.sum(), rtol=1e-15)
    np.testing.assert_allclose(post.marginals[1, 0], [0, 1, 0, 0])
    np.testing.assert_allclose(post.node_values[:, 0, 0], [0.75, 1.0, 0.0])
    assert not post.edge_values.any() and not post.status.any()
