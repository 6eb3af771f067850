"""The two-team form of the pipelined split-M pruning kernel (csrc/jit.hip: eight waves per
workgroup, two waves per SIMD) against the interpreter kernel on the same batch: the
log-likelihoods, the statuses and the totals are the same bits.  Small trees, every split of the
chains -- (2,1), (2,2), (3,2) with root halves, (2,1) on the whole tree -- and site counts that
leave a ragged last tile, a single tile (team 1 and most of team 0 have no valid tile and must
still reach every barrier) and several workgroups."""
import os

import networkx as nx
import numpy as np
import pytest

import _step_multi_cases as smc

pytestmark = pytest.mark.gpu

KNOBS = ('RAOTEH_JIT_TILES', 'RAOTEH_JIT_HALVES', 'RAOTEH_JIT_TEAMS', 'RAOTEH_JIT_FOLD')

# (tiles per workgroup, root halves)
FORMS = [(3, True), (4, True), (5, True), (3, False)]


def _tree(kind):
    """(T, root, observed nodes)"""
    from raoteh_amd import synth
    if kind == 'three':
        # nine leaves, a root with three children
        rng = np.random.RandomState(5)
        T = nx.Graph()
        leaves = []
        for c in (1, 2, 3):
            T.add_edge(0, c, weight=0.05 + 0.1 * rng.uniform())
            for k in range(3):
                leaf = 3 * c + 1 + k
                T.add_edge(c, leaf, weight=0.05 + 0.1 * rng.uniform())
                leaves.append(leaf)
        return T, 0, leaves
    T, root, leaves = synth.balanced_tree(8, seed=17)
    return T, root, (leaves + [root] if kind == 'observed root' else leaves)


@pytest.fixture(scope='module')
def ctx():
    from raoteh_amd import device
    c = device.Context(0)
    for k, v in (('force_generic', 0), ('jit_async', 0), ('rescale', 0), ('leaf_state_kernels', 1)):
        c.set_option(k, v)
    saved = {k: os.environ.pop(k) for k in KNOBS if k in os.environ}
    yield c
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(saved)


def _batches(ctx, model, obs_nodes, dense, T, halves):
    """(interpreter batch, team batch) of the same observations"""
    ctx.set_option('jit', 0)
    plain = model.upload_sites(obs_nodes, dense, kind='dense')
    ctx.set_option('jit', 1)
    os.environ['RAOTEH_JIT_TILES'] = str(T)
    os.environ['RAOTEH_JIT_HALVES'] = '1' if halves else '0'
    os.environ['RAOTEH_JIT_TEAMS'] = '1'
    try:
        team = model.upload_sites(obs_nodes, dense, kind='dense')
    finally:
        ctx.set_option('jit', -1)
        for k in KNOBS:
            os.environ.pop(k, None)
    return plain, team


CASES = [(n, 'balanced') for n in (49, 61, 64)] + [(61, 'three'), (61, 'observed root')]


@pytest.mark.parametrize('T,halves', FORMS)
@pytest.mark.parametrize('n,tree', CASES)
def test_team_kernel_has_the_interpreters_bits(ctx, n, tree, T, halves):
    from raoteh_amd import device
    G, root, obs_nodes = _tree(tree)
    rng = np.random.RandomState(100 * n + 10 * T + halves)
    model = device.TreeModel(G, root, n, ctx=ctx)
    w = rng.uniform(0.1, 1.0, n)
    model.set_root_distn(w / w.sum())
    model.set_rates(Q_default=smc.random_rates(n, rng))
    for nsites in (16 * T * 2 + 5, 16, 16 * T * 2 * 3):
        dense = rng.uniform(0.05, 1.0, size=(nsites, len(obs_nodes), n))
        dense[rng.uniform(size=dense.shape) < 0.1] = 0.0
        dense[3, 0, :] = 0.0                      # a site of probability zero
        plain, team = _batches(ctx, model, obs_nodes, dense, T, halves)
        want, wst = model.log_likelihoods(plain)
        wtot = model.fetch_totals(plain)
        got, gst = model.log_likelihoods(team)
        gtot = model.fetch_totals(team)
        name = team.kernel_name
        assert plain.kernel_name.startswith('prune_mfma'), plain.kernel_name
        assert name == 'prune_tree_jit_mfma<%d,T%d%s,teams>' % (n, T, ',halves' if halves else ''), name
        assert wst[3] != 0 and np.isneginf(want[3]) and (wst[np.arange(nsites) != 3] == 0).all()
        assert np.array_equal(smc.bits(got), smc.bits(want)), (name, nsites)
        assert np.array_equal(gst, wst), (name, nsites)
        assert np.array_equal(smc.bits(gtot), smc.bits(wtot)), (name, nsites, gtot, wtot)
        assert gtot[1] == 1 and gtot[2] == nsites
        plain.close()
        team.close()
    model.close()


def test_the_knob_off_gives_the_one_team_kernel(ctx):
    """RAOTEH_JIT_TEAMS=0: the same batch gets the four-wave kernel, with the same bits."""
    from raoteh_amd import device
    G, root, obs_nodes = _tree('balanced')
    rng = np.random.RandomState(8)
    model = device.TreeModel(G, root, 61, ctx=ctx)
    model.set_root_distn(np.full(61, 1.0 / 61))
    model.set_rates(Q_default=smc.random_rates(61, rng))
    dense = rng.uniform(0.05, 1.0, size=(165, len(obs_nodes), 61))
    out = {}
    for teams in ('0', '1', None):
        ctx.set_option('jit', 1)
        os.environ['RAOTEH_JIT_TILES'] = '5'
        os.environ['RAOTEH_JIT_HALVES'] = '1'
        if teams is not None:
            os.environ['RAOTEH_JIT_TEAMS'] = teams
        try:
            batch = model.upload_sites(obs_nodes, dense, kind='dense')
        finally:
            ctx.set_option('jit', -1)
            for k in KNOBS:
                os.environ.pop(k, None)
        ll, st = model.log_likelihoods(batch)
        out[teams] = (smc.bits(ll), st, smc.bits(model.fetch_totals(batch)), batch.kernel_name)
        batch.close()
    model.close()
    assert out['0'][3] == 'prune_tree_jit_mfma<61,T5,halves>', out['0'][3]
    assert out['1'][3] == 'prune_tree_jit_mfma<61,T5,halves,teams>', out['1'][3]
    for k in range(3):
        assert np.array_equal(out['0'][k], out['1'][k]) and np.array_equal(out[None][k], out['1'][k])


def test_step_multi_one_launch_of_the_team_kernel(ctx):
    """K = 2 rate sets in one launch of the team kernel's multi form against two separate
    steps, bit for bit."""
    from raoteh_amd import device
    case = smc.make_case(61, 'balanced', 'dense', 2, seed=33, zero_set=False, nsites=165)
    ctx.set_option('jit', 1)
    os.environ['RAOTEH_JIT_TILES'] = '5'
    os.environ['RAOTEH_JIT_HALVES'] = '1'
    os.environ['RAOTEH_JIT_TEAMS'] = '1'
    try:
        model, batch = smc.upload(device, ctx, case)
        batch.wait_for_kernel()
        ll, st, tot, name = smc.check_bit_identity(model, batch, case)
    finally:
        ctx.set_option('jit', -1)
        for k in KNOBS:
            os.environ.pop(k, None)
    assert name == 'prune_tree_jit_mfma<61,T5,halves,teams>,multi', name
    assert (tot[:, 2] == 165).all()
    batch.close()
    model.close()


@pytest.mark.parametrize('background', [False, True])
def test_a_rejected_team_kernel_falls_back_to_the_one_team_form(background):
    """RAOTEH_JIT_REJECT_TEAMS (diagnostics): the probe verification rejects every two-team
    kernel.  The batch then runs the one-team form of the same tiling -- not the interpreter --
    with the interpreter's bits, whether the kernel was compiled at upload or in the background.
    (A context of its own: a rejection is remembered per context.)"""
    from raoteh_amd import device
    own = device.Context(0)
    for k, v in (('force_generic', 0), ('rescale', 0), ('jit_async', int(background))):
        own.set_option(k, v)
    G, root, obs_nodes = _tree('balanced')
    rng = np.random.RandomState(12)
    nsites = 1100                      # 61 states: enough work for a specialised kernel
    model = device.TreeModel(G, root, 61, ctx=own)
    model.set_root_distn(np.full(61, 1.0 / 61))
    model.set_rates(Q_default=smc.random_rates(61, rng))
    dense = rng.uniform(0.05, 1.0, size=(nsites, len(obs_nodes), 61))
    own.set_option('jit', 0)
    plain = model.upload_sites(obs_nodes, dense, kind='dense')
    want, wst = model.log_likelihoods(plain)
    own.set_option('jit', -1 if background else 1)
    os.environ.update(RAOTEH_JIT_TILES='5', RAOTEH_JIT_HALVES='1', RAOTEH_JIT_REJECT_TEAMS='1')
    try:
        batch = model.upload_sites(obs_nodes, dense, kind='dense')
        batch.wait_for_kernel()
        got, gst = model.log_likelihoods(batch)
        name = batch.kernel_name
    finally:
        for k in KNOBS + ('RAOTEH_JIT_REJECT_TEAMS',):
            os.environ.pop(k, None)
    assert name == 'prune_tree_jit_mfma<61,T5,halves>', name
    assert np.array_equal(smc.bits(got), smc.bits(want)) and np.array_equal(gst, wst)
    assert np.array_equal(smc.bits(model.fetch_totals(batch)), smc.bits(model.fetch_totals(plain)))
    plain.close()
    batch.close()
    model.close()
