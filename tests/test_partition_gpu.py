"""Partitioned likelihood (TreeModel.upload_sites(..., site_sets=...) / step_partitioned): every
site under its own rate set in one pruning launch.  The per-site log-likelihoods against the
numpy oracle run with the site's own Q and, where the same kernel form runs, bit for bit against
step_multi on an ordinary batch; the reference's five switching columns under their five
compound matrices in one batch; a zero-probability status that depends on the set; totals,
weights and repeatability; the rate-set state; the refusals."""
import ctypes

import numpy as np
import pytest

import _partition_cases as pc
import _step_multi_cases as smc
from conftest import switching_cases

pytestmark = pytest.mark.gpu

RTOL_LL = 1e-10          # what test_config_fixtures_batched asks of a log-likelihood

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


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


def partition_info(batch):
    from raoteh_amd import _lib
    vals = [ctypes.c_int64(-1) for _ in range(3)]
    _lib.check(_lib.lib().rt_sites_partition_info(batch._h, *[ctypes.byref(v) for v in vals]))
    return tuple(v.value for v in vals)           # nsets, granule, padded


def step_and_fetch(model, batch, case, **kw):
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    model.step_partitioned(batch, **kw)
    return model.fetch_log_likelihoods(batch)


# ---- a. log-likelihoods ------------------------------------------------------------------------

@pytest.mark.parametrize('kind', ['dense', 'state', 'mask'])
@pytest.mark.parametrize('n', [3, 4, 8, 20, 40, 61, 122])
def test_log_likelihoods(contexts, n, kind):
    """K = 4 with set 3 empty, site i in set i % 3, 3 G + 5 sites (n = 8 and n = 20: the one-wave
    kernel, four tiles of different sets in one workgroup)."""
    from raoteh_amd import device
    case = pc.make_case(n, kind, seed=100 * n + len(kind))
    ctx = contexts()
    model, batch = pc.upload(device, ctx, case)
    G = pc.granule(n)
    nsites = 3 * G + 5
    assert len(case.site_sets) == nsites == batch.nsites
    per_set = [(case.site_sets == k).sum() for k in range(4)]
    want_padded = sum((c + G - 1) // G * G for c in per_set)
    assert partition_info(batch) == (4, G, want_padded)
    ll, st = step_and_fetch(model, batch, case)
    name = batch.kernel_name
    assert name.endswith(',partitioned'), name
    assert ll.shape == (nsites,) and st.shape == (nsites,)
    # 1. the oracle, each site with its own set's Q
    want, wst = pc.oracle(model, case)
    assert np.array_equal(st & 1, wst)
    live = wst == 0
    assert live.sum() > nsites // 2
    err = np.max(np.abs(ll[live] - want[live]) / np.abs(want[live]))
    print('n=%d %s %s: max rel err %.3e' % (n, kind, name, err))
    assert err < RTOL_LL, err
    assert np.isneginf(ll[~live]).all()
    # 2. step_multi on an ordinary batch of the same data, where it runs the same kernel form
    omodel, obatch = pc.upload(device, ctx, case, partitioned=False)
    omodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    omodel.step_multi(obatch)
    mll, mst = omodel.fetch_multi_log_likelihoods(obatch)
    oname = obatch.kernel_name
    idx = np.arange(nsites)
    same_form = name == oname + ',partitioned'
    if n in (20, 61, 122):
        assert same_form, (name, oname)
    if same_form:
        assert np.array_equal(smc.bits(ll), smc.bits(mll[case.site_sets, idx])), (name, oname)
        assert np.array_equal(st, mst[case.site_sets, idx])
    else:
        # another kernel form (at n <= 4 an ordinary batch runs the LDS-DMA lane kernel, which a
        # partitioned batch excludes): another order of the same arithmetic, so the comparison is
        # at the oracle's tolerance only
        got = mll[case.site_sets, idx]
        assert np.array_equal(st & 1, mst[case.site_sets, idx] & 1)
        assert np.max(np.abs(ll[live] - got[live]) / np.abs(got[live])) < RTOL_LL, (name, oname)
    for x in (batch, obatch):
        x.close()
    model.close()
    omodel.close()


def test_lane_kernel_without_the_staged_table(contexts, monkeypatch):
    """The lane kernel's other form (P through the scalar cache, one wave per workgroup: what a
    tree whose table does not fit LDS runs, forced here by RAOTEH_LANE_NO_PLDS): the granule is
    64 sites; runs of 70, 60 and 67 sites make five blocks, which the lane layout rounds up to
    six -- the sixth lies past the plan."""
    from raoteh_amd import device
    monkeypatch.setenv('RAOTEH_LANE_NO_PLDS', '1')
    site_sets = np.random.RandomState(1).permutation(np.repeat([0, 1, 2], [70, 60, 67]))
    case = pc.make_case(4, 'dense', seed=41, nsites=len(site_sets), site_sets=site_sets)
    model, batch = pc.upload(device, contexts(), case)
    assert partition_info(batch) == (4, 64, 320)
    ll, st = step_and_fetch(model, batch, case)
    assert batch.kernel_name == 'prune_lane<4,reg,R8>,partitioned'
    want, wst = pc.oracle(model, case)
    assert np.array_equal(st & 1, wst) and not wst.any()
    assert np.max(np.abs(ll - want) / np.abs(want)) < RTOL_LL
    ptot = model.fetch_partition_totals(batch)
    assert np.array_equal(ptot[:, 2], [70, 60, 67, 0])
    batch.close()
    model.close()


@pytest.mark.parametrize('n,kind,form', [(8, 'dense', 'prune_mfma<1,2'), (20, 'mask', 'prune_mfma<2,5'),
                                         (20, 'dense', 'prune_mfma<2,5')])
def test_split_kernel_with_several_tiles_per_workgroup(contexts, monkeypatch, n, kind, form):
    """Up to 32 states a batch runs the one-wave kernel; RAOTEH_MFMA_NO_SOLO gives it the split-M
    kernel, whose workgroup then holds four tiles (n = 8) or two (n = 20) that share the exchange
    and reduction buffers' allocation and the barriers -- each tile under its own set here, and
    the sets interleaved tile by tile (runs of 16: consecutive tiles differ)."""
    from raoteh_amd import device
    monkeypatch.setenv('RAOTEH_MFMA_NO_SOLO', '1')
    site_sets = np.repeat(np.arange(7) % 3, 16)[:-3]         # 109 sites: 48, 32 and 29 of a set
    site_sets = site_sets[np.random.RandomState(n).permutation(len(site_sets))]
    case = pc.make_case(n, kind, seed=9 * n, nsites=len(site_sets), site_sets=site_sets)
    ctx = contexts()
    model, batch = pc.upload(device, ctx, case)
    assert partition_info(batch) == (4, 16, 112)
    ll, st = step_and_fetch(model, batch, case)
    name = batch.kernel_name
    assert name.startswith(form) and name.endswith(',partitioned'), name
    want, wst = pc.oracle(model, case)
    assert np.array_equal(st & 1, wst)
    live = wst == 0
    assert np.max(np.abs(ll[live] - want[live]) / np.abs(want[live])) < RTOL_LL
    # the same form on an ordinary batch, one launch per set: the same bits
    omodel, obatch = pc.upload(device, ctx, case, partitioned=False)
    omodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    omodel.step_multi(obatch)
    mll, mst = omodel.fetch_multi_log_likelihoods(obatch)
    assert name == obatch.kernel_name + ',partitioned', (name, obatch.kernel_name)
    idx = np.arange(len(site_sets))
    assert np.array_equal(smc.bits(ll), smc.bits(mll[site_sets, idx]))
    assert np.array_equal(st, mst[site_sets, idx])
    for x in (batch, obatch):
        x.close()
    model.close()
    omodel.close()


# ---- b. the switching golden -------------------------------------------------------------------

def test_switching_columns_in_one_batch(contexts):
    """The five columns of tests/golden/switching.json under their five compound matrices (122
    states) in ONE partitioned batch.  The prior of the reference differs per column as well (it
    lives on the column's benign states), and a model has one root distribution: the root is an
    observed leaf here, so each column's prior is folded into the root's dense observation and
    the model keeps root weights of one -- the same product in another order."""
    from raoteh_amd import device
    fx, cases = switching_cases()
    n2 = fx['ncompound']
    T, root = cases[0]['T'], cases[0]['root']
    model = device.TreeModel(T, root, n2, ctx=contexts())
    obs_nodes = [v for v in T if len(cases[0]['allowed'][v]) < n2]
    assert root in obs_nodes
    data = np.zeros((len(cases), len(obs_nodes), n2))
    for i, c in enumerate(cases):
        assert c['T'] is T or sorted(c['T'].edges()) == sorted(T.edges())
        for j, v in enumerate(obs_nodes):
            data[i, j, sorted(c['allowed'][v])] = 1.0
            if v == root:
                data[i, j] *= c['compound_distn']
    batch = model.upload_sites(obs_nodes, data, kind='dense', site_sets=np.arange(len(cases)))
    assert batch.nsets == len(cases) == 5
    model.set_rate_sets(np.array([c['Q_compound'] for c in cases]))
    model.step_partitioned(batch)
    ll, st = model.fetch_log_likelihoods(batch)
    seen_zero = False
    for i, c in enumerate(cases):
        want = c['want']['log_likelihood']
        if want is None:                     # the reference raised StructuralZeroProb
            assert st[i] & 1 and np.isneginf(ll[i])
            seen_zero = True
        else:
            assert not st[i] & 1
            print('column %d: %.15g want %.15g' % (i, ll[i], want))
            assert abs(ll[i] - want) <= RTOL_LL * abs(want), (i, ll[i], want)
    assert seen_zero
    tot = model.fetch_partition_totals(batch)
    assert np.array_equal(tot[:, 1], (st & 1).astype(float)) and (tot[:, 2] == 1).all()
    batch.close()
    model.close()


# ---- c. a zero probability that depends on the set ---------------------------------------------

@pytest.mark.parametrize('n', [4, 8, 20, 61])
def test_zero_probability_depends_on_the_set(contexts, n):
    """Set 0 has a block-diagonal Q (two classes that never communicate) and every site observes
    leaves of both classes: zero probability under set 0, positive under set 1.  A tile that read
    another set's table would get the other status."""
    from raoteh_amd import device
    G = pc.granule(n)
    nsites = 3 * G + 5
    rng = np.random.RandomState(n)
    site_sets = rng.randint(0, 2, nsites)
    case = pc.make_case(n, 'state', seed=n, nsets=2, nsites=nsites, site_sets=site_sets)
    h = n // 2
    for q in range(2):
        Qa = case.Q[0, q]
        Qa[:h, h:] = 0.0
        Qa[h:, :h] = 0.0
        np.fill_diagonal(Qa, 0.0)
        np.fill_diagonal(Qa, -Qa.sum(axis=1))
    data = rng.randint(0, n, size=case.data.shape).astype(np.uint8)
    data[:, 0] = rng.randint(0, h, nsites)          # one leaf in each class
    data[:, 1] = rng.randint(h, n, nsites)
    case = case._replace(data=data)
    model, batch = pc.upload(device, contexts(), case)
    ll, st = step_and_fetch(model, batch, case)
    assert np.array_equal((st & 1) != 0, site_sets == 0), batch.kernel_name
    assert np.isneginf(ll[site_sets == 0]).all() and np.isfinite(ll[site_sets == 1]).all()
    tot = model.fetch_partition_totals(batch)
    assert tot[0, 1] == tot[0, 2] == (site_sets == 0).sum() and tot[0, 0] == 0.0
    assert tot[1, 1] == 0 and tot[1, 2] == (site_sets == 1).sum()
    batch.close()
    model.close()


# ---- d. totals, weights, repeatability ---------------------------------------------------------

def _close(got, want):
    return abs(got - want) <= 1e-12 * max(1.0, abs(want))


@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense'), (61, 'mask')])
def test_totals_weights_and_repeatability(contexts, n, kind):
    """Set 2 has Q = 0 (P = I): the sites of that set whose leaves differ have likelihood zero.
    Set 3 is empty.  The sums are compared with numpy sums of the per-site values (float
    summation order only: 1e-12 relative), the counts exactly."""
    from raoteh_amd import device
    case = pc.make_case(n, kind, seed=7 + n, zero_set=2)
    model, batch = pc.upload(device, contexts(), case)
    nsites = batch.nsites
    rng = np.random.RandomState(n)
    w = rng.uniform(0.5, 3.0, nsites)               # caller order
    batch.set_weights(w)
    ll, st = step_and_fetch(model, batch, case)
    tot = model.fetch_totals(batch)
    ptot, ws = model.fetch_partition_totals(batch, weighted=True)
    ok = (st & 1) == 0
    assert (~ok).any() and (case.site_sets[~ok] == 2).all()
    assert tot[1] == (~ok).sum() and tot[2] == nsites
    assert _close(tot[0], ll[ok].sum())
    assert ptot.shape == (4, 3) and ws.shape == (4,)
    for k in range(4):
        mine = case.site_sets == k
        assert ptot[k, 1] == (mine & ~ok).sum() and ptot[k, 2] == mine.sum()
        print('set %d: sum %.17g want %.17g, weighted %.17g want %.17g'
              % (k, ptot[k, 0], ll[mine & ok].sum(), ws[k], np.dot(w[mine & ok], ll[mine & ok])))
        assert _close(ptot[k, 0], ll[mine & ok].sum())
        assert _close(ws[k], np.dot(w[mine & ok], ll[mine & ok]))
    assert (ptot[3] == 0).all() and ws[3] == 0
    # a second call: the same bits everywhere
    model.step_partitioned(batch)
    ll2, st2 = model.fetch_log_likelihoods(batch)
    ptot2, ws2 = model.fetch_partition_totals(batch, weighted=True)
    assert np.array_equal(smc.bits(ll2), smc.bits(ll)) and np.array_equal(st2, st)
    assert np.array_equal(smc.bits(model.fetch_totals(batch)), smc.bits(tot))
    assert np.array_equal(smc.bits(ptot2), smc.bits(ptot)) and np.array_equal(smc.bits(ws2), smc.bits(ws))
    # the weights are the caller's: reversed weights give the reversed dot product; none: the sums
    batch.set_weights(w[::-1].copy())
    model.step_partitioned(batch, recompute_transitions=False)
    _, ws3 = model.fetch_partition_totals(batch, weighted=True)
    for k in range(3):
        mine = (case.site_sets == k) & ok
        assert _close(ws3[k], np.dot(w[::-1][mine], ll[mine]))
    batch.set_weights(None)
    model.step_partitioned(batch, recompute_transitions=False)
    ptot4, ws4 = model.fetch_partition_totals(batch, weighted=True)
    assert np.array_equal(smc.bits(ws4), smc.bits(ptot4[:, 0]))
    with pytest.raises(ValueError):
        batch.set_weights(np.ones(nsites + 1))
    batch.close()
    model.close()


# ---- e. the rate-set state ---------------------------------------------------------------------

def test_rate_set_state(contexts):
    from raoteh_amd import device
    case = pc.make_case(20, 'dense', seed=3)
    model, batch = pc.upload(device, contexts(), case)
    # before any set_rate_sets, and before any step
    with pytest.raises(ValueError):
        model.step_partitioned(batch)
    with pytest.raises(ValueError):
        model.fetch_log_likelihoods(batch)
    with pytest.raises(ValueError):
        model.fetch_partition_totals(batch)
    assert (model.fetch_totals(batch) == 0).all()
    # fewer sets in the model than the batch uses
    model.set_rate_sets(case.Q[:3], t=case.t[:3], node_q=case.node_q)
    with pytest.raises(ValueError):
        model.step_partitioned(batch)
    with pytest.raises(ValueError):
        model.fetch_log_likelihoods(batch)
    # the exponentials of a fresh set_rate_sets are resident: no recompute needed
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    model.step_partitioned(batch, recompute_transitions=False)
    ll0, st0 = model.fetch_log_likelihoods(batch)
    model.step_partitioned(batch, recompute_transitions=True)
    ll1, st1 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll0), smc.bits(ll1)) and np.array_equal(st0, st1)
    want, _ = pc.oracle(model, case)
    live = np.isfinite(want)
    assert np.max(np.abs(ll0[live] - want[live]) / np.abs(want[live])) < RTOL_LL
    # more sets than the batch uses: the same results; the count changed, so the getters refuse
    # until the next step
    Q6 = np.concatenate([case.Q, case.Q[:2]])
    t6 = np.concatenate([case.t, case.t[:2]])
    model.set_rate_sets(Q6, t=t6, node_q=case.node_q)
    for getter in (model.fetch_log_likelihoods, model.fetch_totals, model.fetch_partition_totals):
        with pytest.raises(ValueError):
            getter(batch)
    model.step_partitioned(batch, recompute_transitions=False)
    ll2, st2 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll2), smc.bits(ll0)) and np.array_equal(st2, st0)
    batch.close()
    model.close()


# ---- f. refusals -------------------------------------------------------------------------------

def _unsupported(call, *args, **kw):
    from raoteh_amd import _lib
    with pytest.raises(_lib.RaotehHipError) as e:
        call(*args, **kw)
    assert e.value.code == _lib.RT_ERR_UNSUPPORTED, e.value
    return str(e.value)


def test_creation_refusals(contexts):
    from raoteh_amd import device, synth, _lib
    case = pc.make_case(20, 'dense', seed=4)
    assert 'rescale' in _unsupported(pc.upload, device, contexts(rescale=1), case)
    assert 'force_generic' in _unsupported(pc.upload, device, contexts(force_generic=1), case)
    # a tree the fast kernels do not take: 122 states and nine accumulator slots
    T, root, leaves = synth.balanced_tree(512, seed=0)
    deep = device.TreeModel(T, root, 122, ctx=contexts())
    assert deep.schedule_depth >= 9
    data = np.ones((2, len(leaves), 122))
    assert 'tree' in _unsupported(deep.upload_sites, leaves, data, site_sets=[0, 1])
    deep.close()
    # the number of sets and the indices, at the C entry point (past the Python helper)
    model = device.TreeModel(case.T, case.root, case.n, ctx=contexts())
    lib = _lib.lib()
    idx = np.array([model.tree.node_to_index[v] for v in case.leaves], dtype=np.int64)
    data = np.ascontiguousarray(case.data[:4])

    def create(sets, nsets):
        sets = np.array(sets, dtype=np.int32)
        h = ctypes.c_void_p()
        rc = lib.rt_sites_create_partitioned(
            model._h, 4, _lib.RT_OBS_DENSE, len(idx), idx.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
            data.ctypes.data_as(ctypes.c_void_p), sets.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)),
            nsets, ctypes.byref(h))
        assert rc != 0 and not h.value
        return rc
    assert create([0, 0, 0, 0], 0) == _lib.RT_ERR_UNSUPPORTED
    assert create([0, 0, 0, 0], 65) == _lib.RT_ERR_UNSUPPORTED
    assert create([0, 1, 2, 1], 2) == _lib.RT_ERR_INVALID
    assert create([0, -1, 0, 1], 2) == _lib.RT_ERR_INVALID
    with pytest.raises(ValueError):
        model.upload_sites(case.leaves, case.data, site_sets=case.site_sets, nsets=2)
    model.close()


def test_everything_else_refuses_and_leaves_the_batch_alone(contexts):
    from raoteh_amd import device
    case = pc.make_case(20, 'dense', seed=6)
    model, batch = pc.upload(device, contexts(), case)
    # (the model's own rates as well, so that nothing but the batch stands in a call's way)
    model.set_rates(Q=case.Q[0], node_q=case.node_q, t=case.t[0])
    ll, st = step_and_fetch(model, batch, case)
    ptot = model.fetch_partition_totals(batch)
    name = batch.kernel_name
    E = np.ones((20, 20))
    for call, args in ((model.prune, ()), (model.step, ()), (model.step_multi, ()),
                       (model.expected_history_statistics, ()),
                       (model.posteriors, ([[0, 1]],)),
                       (model.branch_expectations, (E,)),
                       (model.branch_profiles, (None, [0.5, 2.0])),
                       (model.sample_states, ()),
                       (model.sample_mappings, (E,))):
        assert 'partitioned' in _unsupported(call, batch, *args), call
    assert 'partitioned' in _unsupported(batch.clone)
    assert 'partitioned' in _unsupported(model.allreduce, batch)
    assert 'partitioned' in _unsupported(model.allreduce_group, [batch])
    ll2, st2 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll2), smc.bits(ll)) and np.array_equal(st2, st)
    assert np.array_equal(smc.bits(model.fetch_partition_totals(batch)), smc.bits(ptot))
    assert batch.kernel_name == name
    # ... and step_partitioned / the per-set totals do not take an ordinary batch
    omodel, obatch = pc.upload(device, contexts(), case, partitioned=False)
    omodel.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    with pytest.raises(ValueError):
        omodel.step_partitioned(obatch)
    with pytest.raises(ValueError):
        omodel.fetch_partition_totals(obatch)
    assert obatch.site_sets is None and partition_info(obatch) == (0, 0, 0)
    # a batch of another model
    with pytest.raises(ValueError):
        omodel.step_partitioned(batch)
    for x in (batch, obatch):
        x.close()
    model.close()
    omodel.close()
