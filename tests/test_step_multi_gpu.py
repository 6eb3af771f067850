"""K rate sets against one resident batch in a single step (TreeModel.set_rate_sets /
step_multi): the per-set log-likelihoods, statuses and totals are, bit for bit, those of K
separate set_rates + step on the same batch, in every family of pruning kernel; the batch's own
results and the model's own transitions stay; the mixture over the sets and the weighted sums
agree with numpy; the error paths refuse."""
import os
import subprocess
import sys

import numpy as np
import pytest

import _step_multi_cases as smc

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


@pytest.fixture(scope='module')
def contexts():
    """One context per set of options, shared by the module (a context keeps its compiled
    tree-specialised kernels)."""
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


def kinds_of(n):
    if n == 61:
        return ('dense', 'state', 'mask')
    return ('dense', 'state') if n in (4, 33, 64) else ('dense', 'mask')


CASES = [(n, tree, kind) for n in (4, 20, 33, 48, 61, 64, 122)
         for tree in ('balanced', 'random') for kind in kinds_of(n)]


@pytest.mark.parametrize('jit', [0, 1])
@pytest.mark.parametrize('n,tree,kind', CASES)
def test_step_multi_is_k_separate_steps(contexts, n, tree, kind, jit):
    """K = 5, 2, 1 on one batch (set_rate_sets grows and shrinks); per-edge rate matrices with a
    node_q on the balanced tree, one matrix per set on the random tree; the last set of K >= 2
    has Q = 0, so that the sites whose leaves differ have likelihood zero in that set only."""
    from raoteh_amd import device
    case = smc.make_case(n, tree, kind, 5, seed=1000 * n + (tree == 'random'),
                         per_edge=tree == 'balanced')
    model, batch = smc.upload(device, contexts(jit=jit), case)
    if jit:
        batch.wait_for_kernel()
    for sets in ([0, 1, 2, 3, 4], [1, 4], [2]):
        ll, st, tot, name = smc.check_bit_identity(model, batch, case, sets)
        assert name.endswith(',loop') or name.endswith(',multi'), name
        assert name.startswith(batch.kernel_name), (name, batch.kernel_name)
        if jit:
            assert 'jit' in name, name
        if jit and n in (33, 48, 61, 64):
            # the split-M family: one launch for all sets, not the fallback
            assert name.endswith(',multi'), name
        else:
            assert name.endswith(',loop'), name
        if len(sets) > 1:
            # the zero set: status and zero count per set
            assert (st[-1] & 1).any() and not (st[0] & 1).any(), name
            assert tot[-1, 1] == (st[-1] & 1).sum() > 0 and tot[0, 1] == 0
            assert np.isneginf(ll[-1][(st[-1] & 1) != 0]).all()
        assert (tot[:, 2] == smc.NSITES).all()
    batch.close()
    model.close()


def _child(env):
    out = subprocess.run([sys.executable, smc.__file__], env=dict(os.environ, **env),
                         stdout=subprocess.PIPE, stderr=subprocess.STDOUT, universal_newlines=True,
                         timeout=300)
    assert out.returncode == 0, out.stdout[-3000:]
    names = [l for l in out.stdout.splitlines() if l.startswith('MULTI_KERNEL ')]
    assert len(names) == 1, out.stdout[-3000:]
    return names[0]


def test_forced_loop_form_in_a_fresh_process():
    """RAOTEH_MULTI=loop: the loop form, whatever the batch could run (61 states, specialised
    kernel), with the bits of the separate steps."""
    name = _child({'RAOTEH_MULTI': 'loop'})
    assert name.endswith(',loop') and 'jit' in name, name


@pytest.mark.parametrize('env,part,avoid', [
    ({'RAOTEH_JIT_HALVES': '0', 'RAOTEH_JIT_TILES': '2'}, 'T2', 'halves'),
    ({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '3'}, 'T3,halves', 'loop'),
    ({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_FOLD': '1', 'RAOTEH_JIT_NO_SPARSE': '1'}, 'halves', 'leaf'),
    ({'RAOTEH_JIT_HALVES': '0', 'RAOTEH_JIT_NO_SPARSE': '1'}, 'T1', 'halves'),
])
def test_every_form_of_the_one_launch_kernel(env, part, avoid):
    """The forms of the split-M kernel the small cases above do not reach by themselves (the
    whole tree in one program at two tiles, root halves at three, the folded combine, dense
    leaves), each in a fresh process: one launch, the bits of the separate steps."""
    name = _child(env)
    assert name.endswith(',multi') and part in name and avoid not in name, name


@pytest.mark.parametrize('kind', ['dense', 'state'])
def test_one_launch_form_arrives_in_the_background(contexts, kind):
    """Kernels on automatic, compiled in the background: the first multi step meets the batch
    with its own specialised kernel and no multi form, runs the loop form and asks for the
    multi form; wait_for_kernel joins that compile; the next multi step is one launch, with
    the same bits."""
    from raoteh_amd import device
    nsites = 1100                      # 61 states: enough work for a specialised kernel
    case = smc.make_case(61, 'balanced', kind, 3, seed=21, nsites=nsites)
    model, batch = smc.upload(device, contexts(jit=-1, jit_async=1), case)
    batch.wait_for_kernel()
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    model.step_multi(batch)
    first = batch.multi_kernel_name
    ll, st = model.fetch_multi_log_likelihoods(batch)
    tot = model.fetch_multi_totals(batch)
    assert 'jit' in first and first.endswith(',loop'), first
    batch.wait_for_kernel()
    model.step_multi(batch)
    second = batch.multi_kernel_name
    assert second.endswith(',multi') and second[:-6] == first[:-5], (first, second)
    ll2, st2 = model.fetch_multi_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll2), smc.bits(ll)) and np.array_equal(st2, st)
    assert np.array_equal(smc.bits(model.fetch_multi_totals(batch)), smc.bits(tot))
    wll, wst, wtot = smc.separate_steps(model, batch, case)
    assert np.array_equal(smc.bits(ll2), smc.bits(wll)) and np.array_equal(st2, wst)
    assert np.array_equal(smc.bits(tot), smc.bits(wtot))
    batch.close()
    model.close()


@pytest.mark.parametrize('n,kind,jit', [(4, 'state', 1), (20, 'dense', 0), (61, 'state', 1)])
def test_own_results_survive(contexts, n, kind, jit):
    from raoteh_amd import device
    case = smc.make_case(n, 'random', kind, 3, seed=11 + n, per_edge=False)
    model, batch = smc.upload(device, contexts(jit=jit), case)
    if jit:
        batch.wait_for_kernel()
    model.set_rates(Q=case.Q[1], t=case.t[1])
    model.step(batch)
    ll0, st0 = model.fetch_log_likelihoods(batch)
    tot0 = model.fetch_totals(batch)
    P0 = model.get_transitions()
    name0 = batch.kernel_name
    model.set_rate_sets(case.Q, t=case.t)
    assert np.array_equal(smc.bits(model.get_transitions()), smc.bits(P0))
    model.step_multi(batch)
    mll, mst = model.fetch_multi_log_likelihoods(batch)
    ll1, st1 = model.fetch_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll1), smc.bits(ll0)) and np.array_equal(st1, st0)
    assert np.array_equal(smc.bits(model.fetch_totals(batch)), smc.bits(tot0))
    assert np.array_equal(smc.bits(model.get_transitions()), smc.bits(P0))
    assert batch.kernel_name == name0
    assert np.array_equal(smc.bits(mll[1]), smc.bits(ll0))
    # ... and a step of the batch's own after the multi step
    model.step(batch, recompute_transitions=False)
    ll2, _ = model.fetch_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll2), smc.bits(ll0))
    # the resident rate sets again, without new exponentials: the same bits
    model.step_multi(batch, recompute_transitions=False)
    mll2, mst2 = model.fetch_multi_log_likelihoods(batch)
    assert np.array_equal(smc.bits(mll2), smc.bits(mll)) and np.array_equal(mst2, mst)
    batch.close()
    model.close()


@pytest.mark.parametrize('opts,n,part', [({'rescale': 1}, 20, 'rescale'),
                                         ({'rescale': 1}, 4, 'rescale'),
                                         ({'force_generic': 1}, 20, 'prune_generic'),
                                         ({'force_generic': 1}, 61, 'prune_generic')])
def test_rescale_and_generic_batches(contexts, opts, n, part):
    from raoteh_amd import device
    case = smc.make_case(n, 'random', 'dense', 3, seed=5 + n)
    model, batch = smc.upload(device, contexts(**opts), case)
    ll, st, tot, name = smc.check_bit_identity(model, batch, case)
    assert part in name and name.endswith(',loop'), name
    batch.close()
    model.close()


def test_against_the_oracle(contexts):
    """61 states, K = 2: scipy exponentials and the oracle's pruning, at the 1e-10 of the
    configuration tests."""
    import scipy.linalg
    from oracle import oracle_numpy as orc
    from raoteh_amd import device
    case = smc.make_case(61, 'balanced', 'state', 2, seed=3, zero_set=False)
    model, batch = smc.upload(device, contexts(jit=0), case)
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    model.step_multi(batch)
    ll, st = model.fetch_multi_log_likelihoods(batch)
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.leaves]
    for k in range(2):
        esd = np.zeros((ta.nnodes, 61, 61))
        for v in range(1, ta.nnodes):
            esd[v] = scipy.linalg.expm(case.t[k, v] * case.Q[k, case.node_q[v]])
        want, wst = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols, case.obs_lik,
                                              case.root_distn)
        assert (st[k] == wst).all()
        err = np.max(np.abs(ll[k] - want) / np.abs(want))
        print('set %d: max rel err %.3e' % (k, err))
        assert err < 1e-10, (k, err)
    batch.close()
    model.close()


def _close(got, want):
    return np.abs(got - want) <= 1e-12 * np.maximum(1.0, np.abs(want))


@pytest.mark.parametrize('n,kind', [(4, 'state'), (20, 'dense'), (61, 'mask')])
def test_mixture_and_weighted_sums(contexts, n, kind):
    from raoteh_amd import device
    K = 5
    case = smc.make_case(n, 'balanced', kind, K, seed=77 + n)
    if kind == 'dense':
        # a site that is zero in every set (a leaf that allows no state)
        case.data[9, 0, :] = 0.0
    model, batch = smc.upload(device, contexts(jit=0), case)
    rng = np.random.RandomState(n)
    w = rng.uniform(0.5, 3.0, smc.NSITES)
    batch.set_weights(w)
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    model.step_multi(batch)
    ll, st = model.fetch_multi_log_likelihoods(batch)
    tot, ws = model.fetch_multi_totals(batch, weighted=True)
    for k in range(K):
        ok = (st[k] & 1) == 0
        want = float(np.dot(w[ok], ll[k][ok]))
        print('set %d weighted sum %.17g want %.17g' % (k, ws[k], want))
        assert _close(ws[k], want)
    # the mixture: every class, then one class out, then only the zero set and one other
    for c in (rng.uniform(0.1, 1.0, K), np.array([0.3, 0.0, 0.2, 0.5, 0.0]),
              np.array([0.0, 0.0, 0.0, 0.25, 0.75])):
        mix, mst, mtot = model.mixture_log_likelihoods(batch, c)
        with np.errstate(divide='ignore'):
            terms = np.where(((st & 1) == 0) & (c[:, None] > 0), np.log(c)[:, None] + ll, -np.inf)
        want = np.logaddexp.reduce(terms, axis=0)
        live = np.isfinite(want)
        assert np.array_equal(live, (mst & 1) == 0)
        assert np.isneginf(mix[~live]).all() and (mst[~live] == 1).all()
        print('mixture max abs err %.3e' % np.max(np.abs(mix[live] - want[live])))
        assert _close(mix[live], want[live]).all()
        assert _close(mtot[0], np.dot(w[live], want[live]))
        assert mtot[1] == (~live).sum() and mtot[2] == smc.NSITES
        if kind == 'dense':
            assert not live[9] and (st[:, 9] & 1).all()
        mix2, mst2, mtot2 = model.mixture_log_likelihoods(batch, c)
        assert np.array_equal(smc.bits(mix2), smc.bits(mix)) and np.array_equal(mst2, mst)
        assert np.array_equal(smc.bits(mtot2), smc.bits(mtot))
    # only the set with P = I: the sites whose leaves differ are zero in every remaining set
    only = np.zeros(K)
    only[K - 1] = 2.0
    mix, mst, mtot = model.mixture_log_likelihoods(batch, only)
    dead = (st[K - 1] & 1) != 0
    assert dead.any() and not dead.all()
    assert np.array_equal(dead, mst == 1) and np.isneginf(mix[dead]).all()
    assert _close(mix[~dead], np.log(2.0) + ll[K - 1][~dead]).all()
    assert mtot[1] == dead.sum()
    # two calls of step_multi: the same bits, weighted sums included
    model.step_multi(batch)
    tot2, ws2 = model.fetch_multi_totals(batch, weighted=True)
    assert np.array_equal(smc.bits(tot2), smc.bits(tot)) and np.array_equal(smc.bits(ws2), smc.bits(ws))
    for bad in ([1.0] * (K - 1), [-1.0] + [1.0] * (K - 1), [0.0] * K, [np.nan] + [1.0] * (K - 1),
                [np.inf] + [1.0] * (K - 1)):
        with pytest.raises(ValueError):
            model.mixture_log_likelihoods(batch, bad)
    batch.close()
    model.close()


def test_errors(contexts):
    from raoteh_amd import device, _lib
    ctx = contexts(jit=0)
    case = smc.make_case(20, 'random', 'dense', 3, seed=2, per_edge=False)
    model, batch = smc.upload(device, ctx, case)
    lib = _lib.lib()
    # no rate sets yet
    with pytest.raises(ValueError):
        model.step_multi(batch)
    with pytest.raises(ValueError):
        model.fetch_multi_log_likelihoods(batch)
    with pytest.raises(ValueError):
        model.fetch_multi_totals(batch)
    assert batch.multi_kernel_name == ''
    # K = 0 and K = 65 (the C entry point itself, past the Python helper)
    from ctypes import POINTER, c_double
    Q65 = np.zeros((65, 20, 20))
    t65 = np.zeros((65, model.tree.nnodes))
    qp, tp = Q65.ctypes.data_as(POINTER(c_double)), t65.ctypes.data_as(POINTER(c_double))
    assert lib.rt_model_set_rate_sets(model._h, 0, qp, 1, None, tp) == _lib.RT_ERR_INVALID
    assert lib.rt_model_set_rate_sets(model._h, 65, qp, 1, None, tp) == _lib.RT_ERR_INVALID
    with pytest.raises(ValueError):
        model.set_rate_sets(Q65, t=t65)
    with pytest.raises(ValueError):
        model.set_rate_sets(case.Q[:0], t=case.t[:0])
    bad_t = case.t.copy()
    bad_t[1, 3] = np.nan
    with pytest.raises(ValueError):
        model.set_rate_sets(case.Q, t=bad_t)
    # getters before any multi step of this batch
    model.set_rate_sets(case.Q, t=case.t)
    with pytest.raises(ValueError):
        model.fetch_multi_log_likelihoods(batch)
    with pytest.raises(ValueError):
        model.mixture_log_likelihoods(batch, [1.0, 1.0, 1.0])
    model.step_multi(batch)
    ll, st = model.fetch_multi_log_likelihoods(batch)
    assert ll.shape == (3, smc.NSITES)
    # K changed and no new step: the getters refuse, until the next step
    model.set_rate_sets(case.Q[:2], t=case.t[:2])
    with pytest.raises(ValueError):
        model.fetch_multi_log_likelihoods(batch)
    with pytest.raises(ValueError):
        model.fetch_multi_totals(batch)
    with pytest.raises(ValueError):
        model.mixture_log_likelihoods(batch, [1.0, 1.0])
    model.step_multi(batch)
    ll2, _ = model.fetch_multi_log_likelihoods(batch)
    assert np.array_equal(smc.bits(ll2), smc.bits(ll[:2]))
    # a batch of another model
    other, obatch = smc.upload(device, ctx, case)
    with pytest.raises(ValueError):
        model.step_multi(obatch)
    for x in (obatch, batch):
        x.close()
    other.close()
    model.close()
