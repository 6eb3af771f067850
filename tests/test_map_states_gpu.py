"""rt_sites_map_states (TreeModel.map_states) on the device: the joint maximum-likelihood
reconstruction.  Exact cases of powers of two, whose states (ties included) and probability have
one correct answer; real models held to optimality with the device's own P; a 1500-node tree that
f64 cannot carry without the scale; the enumeration of a small tree; no draw of the sampler beats
the reconstruction; independence of the tile and the batch; refusals, the batch left as it was."""
import numpy as np
import pytest

import _map_cases as mc
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


def build(ra, T, root, n, Q=None, rd=None, esd=None):
    model = ra.device.TreeModel(T, root, n)
    if esd is not None:
        model.set_transitions(esd)
    elif Q is not None:
        model.set_rates(Q_default=Q)
    if rd is not None:
        model.set_root_distn(rd)
    return model


def observe(kind, n, nsites, nobs, rng):
    if kind == 'state':
        return sc.state_observations(n, nsites, nobs, rng)
    if kind == 'mask':
        return sc.mask_observations(n, nsites, nobs, rng)
    return sc.dense_observations(n, nsites, nobs, rng)


def check_optimal(model, got, obs_nodes, lik, rd, label=''):
    """The optimality check with the device's own P: the device's assignment is worth the
    reference's maximum V*, and log_joint is V*, both to the rounding of 2 nnodes factors a side;
    dead sites are exactly the reference's.  Returns (V*, live)."""
    ta = model.tree
    n = model.nstates
    P = model.get_transitions()
    obs = mc.full_observations(ta, obs_nodes, lik, n)
    _, want, _ = mc.map_reference(P, obs, rd, ta.parent)
    live = np.isfinite(want)
    assert np.array_equal(got.status, np.where(live, 0, 1)), label
    assert (got.states[~live] == 255).all() and (got.log_joint[~live] == -np.inf).all()
    assert (got.states[live] < n).all()
    J = mc.joint_log(P, obs, rd, ta.parent, got.states)
    tol = mc.tolerance(ta.nnodes, want[live])
    print('%s: worst J - V* %.3e, worst |log_joint - V*| %.3e, smallest tol %.3e' % (
        label, (J[live] - want[live]).min(), np.abs(got.log_joint[live] - want[live]).max(),
        tol.min()))
    assert (J[live] >= want[live] - tol).all(), label
    assert (np.abs(got.log_joint[live] - want[live]) <= tol).all(), label
    return want, live


# ---- 1. exact cases --------------------------------------------------------------------------

@pytest.mark.parametrize('n', mc.EXACT_N)
def test_exact_cases(ra, n):
    c = mc.dyadic_case(n)
    want, wlj, tied = mc.map_reference(c.P, c.obs, c.w, c.parent)
    assert (tied > 0).sum() >= 5 and np.isfinite(wlj).all()
    model = build(ra, c.T, c.root, n, rd=c.w, esd=c.P)
    assert model.tree.preorder_nodes == c.ta.preorder_nodes
    batch = model.upload_sites(c.leaves, c.dense, kind='dense')
    got = model.map_states(batch)
    assert got.nodes == list(c.ta.preorder_nodes)
    assert got.states.dtype == np.uint8 and got.states.shape == (mc.EXACT_SITES, 14)
    wrong = np.nonzero((got.states != want).any(axis=1))[0]
    assert not len(wrong), (wrong.tolist(), got.states[wrong[0]].tolist(), want[wrong[0]].tolist())
    assert not got.status.any()
    err = np.abs(got.log_joint - wlj)
    print('n = %d: worst |log_joint - reference| / |log_joint| = %.3e' % (n, (err / np.maximum(np.abs(wlj), 1e-300)).max()))
    assert (err <= 4 * 2.0 ** -52 * np.abs(wlj)).all()
    # one more site whose first leaf's vector is all zero
    dense = np.concatenate([c.dense, c.dense[:1]])
    dense[-1, 0] = 0.0
    more = model.map_states(model.upload_sites(c.leaves, dense, kind='dense'))
    assert more.status[-1] == ra.lib.RT_SITE_ZERO_PROB and not more.status[:-1].any()
    assert (more.states[-1] == 255).all() and more.log_joint[-1] == -np.inf
    assert np.array_equal(more.states[:-1], got.states)
    assert np.array_equal(more.log_joint[:-1], got.log_joint)


# ---- 2. real models: optimality -------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20, 70])
@pytest.mark.parametrize('kind', ['state', 'mask', 'dense'])
def test_optimal_on_real_models(ra, kind, n):
    """Per-edge rate matrices, unobserved leaves, an observed internal node and (dense) a site
    that no assignment explains."""
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=7 * n + len(kind), nnodes=14, per_edge=True)
    assert any('Q' in d for _, _, d in T.edges(data=True))
    internal = [v for v in T if v != root and v not in leaves][0]
    obs_nodes = list(leaves) + [internal]
    data, lik = observe(kind, n, 21, len(obs_nodes), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(obs_nodes, data, kind=kind)
    got = model.map_states(batch)
    want, live = check_optimal(model, got, obs_nodes, lik, rd, '%s, n = %d' % (kind, n))
    if kind == 'state':
        assert (data == 255).any() and live.all()
        for k, v in enumerate(obs_nodes):
            col = got.states[:, model.tree.node_to_index[v]]
            seen = data[:, k] != 255
            assert (col[seen] == data[seen, k]).all()
    if kind == 'dense':
        assert not live[-1] and live.any()


# ---- 3. the scale ----------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 7])
def test_long_tree_needs_the_scale(ra, n):
    """1500 nodes, branch lengths 0.5 .. 1: the maximum is below the smallest f64 (the unscaled
    recursion returns -inf, test_map_states_cpu.py); n = 4 the lane kernels, n = 7 the wide."""
    T, root, tips, Q, rd, data, lik = mc.long_case(n)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(tips, data, kind='state')
    got = model.map_states(batch)
    assert not got.status.any() and np.isfinite(got.log_joint).all()
    assert (got.log_joint < -745.0).all()
    check_optimal(model, got, tips, lik, rd, 'long tree, n = %d' % n)


# ---- 4. the enumeration ----------------------------------------------------------------------

@pytest.mark.parametrize('n', [3, 5])
def test_against_the_enumeration(ra, n):
    T, root, leaves, Q, rd, lik = mc.small_case(n, seed=30 + n)
    model = build(ra, T, root, n, Q, rd)
    got = model.map_states(model.upload_sites(leaves, lik, kind='dense'))
    P = model.get_transitions()
    obs = mc.full_observations(model.tree, leaves, lik, n)
    want, wstates, unique = mc.brute_force(P, obs, rd, model.tree.parent)
    assert not got.status.any() and unique.sum() >= 15
    assert (np.abs(got.log_joint - want) <= mc.tolerance(7, want)).all()
    assert np.array_equal(got.states[unique], wstates[unique])


# ---- 5. against the sampler ------------------------------------------------------------------

def test_no_draw_beats_the_reconstruction(ra):
    n = 20
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=77, nnodes=14)
    data, lik = sc.state_observations(n, 33, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='state')
    got = model.map_states(batch)
    assert not got.status.any()
    draws = model.sample_states(batch, ndraws=64, seed=5)
    P = model.get_transitions()
    obs = mc.full_observations(model.tree, leaves, lik, n)
    tol = mc.tolerance(14, got.log_joint)
    for d in range(64):
        J = mc.joint_log(P, obs, rd, model.tree.parent, draws.states[d])
        assert np.isfinite(J).all()
        assert (J <= got.log_joint + tol).all()
    # the posterior probability of the reconstruction is a probability
    ll, _ = model.log_likelihoods(batch)
    assert (got.log_joint <= ll + 1e-12 * np.abs(ll)).all()


# ---- 6. independence -------------------------------------------------------------------------

@pytest.mark.parametrize('n', [4, 20])
def test_independence(ra, n):
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=21 + n, nnodes=21)
    lik, _ = sc.dense_observations(n, 33, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, lik, kind='dense')
    a = model.map_states(batch)
    b = model.map_states(batch)
    for x, y in zip(a[:3], b[:3]):
        assert x.tobytes() == y.tobytes()
    head = model.map_states(model.upload_sites(leaves, lik[:16], kind='dense'))
    for x, y in zip(a[:3], head[:3]):
        assert x[:16].tobytes() == y.tobytes()
    one = model.map_states(model.upload_sites(leaves, lik[20:21], kind='dense'))
    assert one.states.tobytes() == a.states[20:21].tobytes()
    assert one.log_joint.tobytes() == a.log_joint[20:21].tobytes()
    # other rates, the transitions recomputed in the call: a fresh model
    Q2 = sc.rate_matrix(n, rng)
    fresh = build(ra, T, root, n, Q2, rd)
    want = fresh.map_states(fresh.upload_sites(leaves, lik, kind='dense'))
    model.set_rates(Q_default=Q2)
    again = model.map_states(batch, recompute_transitions=True)
    for x, y in zip(again[:3], want[:3]):
        assert x.tobytes() == y.tobytes()
    assert again.log_joint.tobytes() != a.log_joint.tobytes()


# ---- 7. refusals, the batch is left as it was -------------------------------------------------

def test_refusals(ra):
    lib = ra.lib
    n = 20
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=3)
    data, _ = sc.state_observations(n, 20, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    for key, cause in (('rescale', 'rescale'), ('force_generic', 'fast kernels')):
        ra.ctx.set_option(key, 1)
        try:
            rb = model.upload_sites(leaves, data, kind='state')
        finally:
            ra.ctx.set_option(key, None)
        llr, str_ = model.log_likelihoods(rb)
        with pytest.raises(lib.RaotehHipError) as e:
            model.map_states(rb)
        assert e.value.code == lib.RT_ERR_UNSUPPORTED, key
        assert 'rt_sites_map_states' in str(e.value) and cause in str(e.value), str(e.value)
        got = model.fetch_log_likelihoods(rb)
        assert np.array_equal(got[0], llr) and np.array_equal(got[1], str_)
    # a partitioned batch
    model.set_rate_sets(np.stack([Q, 2.0 * Q]))
    pb = model.upload_sites(leaves, data, kind='state', site_sets=np.arange(20) % 2, nsets=2)
    with pytest.raises(lib.RaotehHipError) as e:
        model.map_states(pb)
    assert e.value.code == lib.RT_ERR_UNSUPPORTED
    assert 'rt_sites_map_states' in str(e.value) and 'partitioned' in str(e.value)
    # null states, a batch of another model, a model without transitions
    batch = model.upload_sites(leaves, data, kind='state')
    assert lib.lib().rt_sites_map_states(model._h, batch._h, 0, None, None, None) == lib.RT_ERR_INVALID
    other = build(ra, T, root, n, Q, rd)
    with pytest.raises(ValueError):
        other.map_states(batch)
    bare = ra.device.TreeModel(T, root, n)
    bb = bare.upload_sites(leaves, data, kind='state')
    with pytest.raises(ValueError):
        bare.map_states(bb)
    bare.set_rates(Q_default=Q)
    assert bare.map_states(bb).states.shape == (20, model.tree.nnodes)


@pytest.mark.parametrize('n', [4, 20, 90])
def test_the_batch_is_left_as_it_was(ra, n):
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=61 + n, nnodes=18)
    data, _ = sc.dense_observations(n, 70, len(leaves), rng)
    model = build(ra, T, root, n, Q, rd)
    batch = model.upload_sites(leaves, data, kind='dense')
    model.step(batch)
    ll0, st0 = model.fetch_log_likelihoods(batch)
    tot0 = model.fetch_totals(batch)
    name = batch.kernel_name
    got = model.map_states(batch)
    assert got.status[-1] == 1
    ll1, st1 = model.fetch_log_likelihoods(batch)
    assert ll0.tobytes() == ll1.tobytes() and np.array_equal(st0, st1)
    assert tot0.tobytes() == model.fetch_totals(batch).tobytes()
    assert batch.kernel_name == name
    model.step(batch)
    ll2, st2 = model.fetch_log_likelihoods(batch)
    assert ll0.tobytes() == ll2.tobytes() and np.array_equal(st0, st2)


def test_one_node_tree_on_the_host(ra):
    import networkx as nx
    T = nx.Graph()
    T.add_node(7)
    w = np.array([0.25, 0.5, 0.0, 0.5])
    model = ra.device.TreeModel(T, 7, 4)
    model.set_rates(Q_default=ra.synth.jukes_cantor(4)[0])
    model.set_root_distn(w)
    batch = model.upload_sites([7], np.array([[255], [0], [2]], dtype=np.uint8), kind='state')
    got = model.map_states(batch)
    assert got.nodes == [7] and got.status.tolist() == [0, 0, 1]
    assert got.states[:, 0].tolist() == [1, 0, 255]                # (the tie 1, 3 goes to 1)
    assert got.log_joint[0] == np.log(0.5) and got.log_joint[1] == np.log(0.25)
    assert got.log_joint[2] == -np.inf
