"""RAOTEH_JIT_LDS_BASE (csrc/jit.hip): the team kernels whose x buffers go through base pointers,
with B operands read ahead in the text, against the interpreter kernel and
against the same form with the knob off, on the batches of test_prune_teams_gpu.py: only loads
moved, so the log-likelihoods, the statuses and the totals are the same bits."""
import os

import numpy as np
import pytest

import _step_multi_cases as smc
from test_prune_teams_gpu import CASES, FORMS, KNOBS, _tree, ctx    # noqa: F401  (ctx: fixture)

pytestmark = pytest.mark.gpu

NEW_KNOBS = ('RAOTEH_JIT_LDS_BASE', 'RAOTEH_JIT_LDS_AHEAD', 'RAOTEH_JIT_LDS_PIN')


def _upload(ctx, model, obs_nodes, dense, T, halves, env):
    """a batch on the two-team kernel of (T, halves) generated under `env`"""
    saved = {k: os.environ.pop(k) for k in NEW_KNOBS if k in os.environ}
    ctx.set_option('jit', 1)
    os.environ.update(RAOTEH_JIT_TILES=str(T), RAOTEH_JIT_HALVES='1' if halves else '0',
                      RAOTEH_JIT_TEAMS='1', **env)
    try:
        return model.upload_sites(obs_nodes, dense, kind='dense')
    finally:
        ctx.set_option('jit', -1)
        for k in KNOBS + NEW_KNOBS:
            os.environ.pop(k, None)
        os.environ.update(saved)


def _read(model, batch):
    ll, st = model.log_likelihoods(batch)
    tot = model.fetch_totals(batch)
    return smc.bits(ll), st, smc.bits(tot), tot


@pytest.mark.parametrize('T,halves', FORMS)
@pytest.mark.parametrize('n,tree', CASES)
def test_base_pointer_kernel_has_the_bits_of_the_interpreter_and_of_the_knob_off(ctx, n, tree, T, halves):
    from raoteh_amd import device
    G, root, obs_nodes = _tree(tree)
    rng = np.random.RandomState(100 * n + 10 * T + halves)
    model = device.TreeModel(G, root, n, ctx=ctx)
    w = rng.uniform(0.1, 1.0, n)
    model.set_root_distn(w / w.sum())
    model.set_rates(Q_default=smc.random_rates(n, rng))
    name = 'prune_tree_jit_mfma<%d,T%d%s,teams>' % (n, T, ',halves' if halves else '')
    for nsites in (16 * T * 2 + 5, 16, 16 * T * 2 * 3):      # a ragged last tile, one tile, three groups
        dense = rng.uniform(0.05, 1.0, size=(nsites, len(obs_nodes), n))
        dense[rng.uniform(size=dense.shape) < 0.1] = 0.0
        dense[3, 0, :] = 0.0                      # a site of probability zero
        ctx.set_option('jit', 0)
        plain = model.upload_sites(obs_nodes, dense, kind='dense')
        ctx.set_option('jit', -1)
        want = _read(model, plain)
        assert plain.kernel_name.startswith('prune_mfma'), plain.kernel_name
        assert want[1][3] != 0 and (want[1][np.arange(nsites) != 3] == 0).all()
        # the knob off, its default, the base pointers alone, the deepest reads held in place
        for env in ({'RAOTEH_JIT_LDS_BASE': '0'}, {}, {'RAOTEH_JIT_LDS_AHEAD': '0'},
                    {'RAOTEH_JIT_LDS_AHEAD': '4', 'RAOTEH_JIT_LDS_PIN': '1'}):
            if env.get('RAOTEH_JIT_LDS_AHEAD') and nsites != 16 * T * 2 + 5:
                continue                          # (the variants: one batch each)
            batch = _upload(ctx, model, obs_nodes, dense, T, halves, env)
            got = _read(model, batch)
            assert batch.kernel_name == name, (batch.kernel_name, env)
            for g, w_ in zip(got[:3], want[:3]):
                assert np.array_equal(g, w_), (name, nsites, env)
            assert got[3][1] == 1 and got[3][2] == nsites
            batch.close()
        plain.close()
    model.close()


def test_step_multi_one_launch_of_the_base_pointer_kernel(ctx):
    """K = 2 rate sets in one launch of the team kernel's multi form, knob on (the default),
    against two separate steps, bit for bit."""
    from raoteh_amd import device
    case = smc.make_case(61, 'balanced', 'dense', 2, seed=34, zero_set=False, nsites=165)
    saved = {k: os.environ.pop(k) for k in NEW_KNOBS if k in os.environ}
    ctx.set_option('jit', 1)
    os.environ.update(RAOTEH_JIT_TILES='5', RAOTEH_JIT_HALVES='1', RAOTEH_JIT_TEAMS='1')
    try:
        model, batch = smc.upload(device, ctx, case)
        batch.wait_for_kernel()
        ll, st, tot, name = smc.check_bit_identity(model, batch, case)
    finally:
        ctx.set_option('jit', -1)
        for k in KNOBS:
            os.environ.pop(k, None)
        os.environ.update(saved)
    assert name == 'prune_tree_jit_mfma<61,T5,halves,teams>,multi', name
    assert (tot[:, 2] == 165).all()
    batch.close()
    model.close()
