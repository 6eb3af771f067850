"""The root combine of a root-halves batch carried in the idle waves of the next expm launch
(csrc/expm.hip, csrc/combine_body.inc) against the same calls with RAOTEH_CARRY_COMBINE=0, where
the combine is a launch of its own right after the pruning kernel: the log-likelihoods, the
statuses and the totals are the same bits whatever is called between a step and the read, and the
timing slot of the combine kernel counts no launch for a carried step and one per flush.

Small trees (a 9-node tree, the 8-leaf balanced tree with and without an observed root, a root
with three children), 49, 61 and 64 states, 37 and 70 sites (3 and 5 tiles, a ragged last one)
and a single tile, one impossible site, both kernel families (the interpreter's root halves
under jit = 0, a tree-specialised kernel under jit = 1); RAOTEH_JIT_HALVES=1 makes batches this
small take root halves."""
import os

import networkx as nx
import numpy as np
import pytest

import _step_multi_cases as smc

pytestmark = pytest.mark.gpu

KNOBS = ('RAOTEH_JIT_HALVES', 'RAOTEH_INTERP_HALVES', 'RAOTEH_CARRY_COMBINE', 'RAOTEH_JIT_FOLD',
         'RAOTEH_NO_DEFER_REDUCE')
RT_K_COMBINE = 3


def _tree(kind):
    """(T, root, observed nodes)"""
    from raoteh_amd import synth
    if kind == 'nine':
        return synth.random_tree(9, seed=4, max_children=3)
    if kind == 'three':
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
    os.environ['RAOTEH_JIT_HALVES'] = '1'
    yield c
    c.set_option('jit', -1)
    c.set_timing(0)
    for k in KNOBS:
        os.environ.pop(k, None)
    os.environ.update(saved)


class World(object):
    """A model with its rates and two batches of different sizes, built the same way every time."""

    def __init__(self, ctx, n, tree, jit, sizes, seed):
        from raoteh_amd import device
        self.ctx, self.n = ctx, n
        self.T, self.root, self.obs_nodes = _tree(tree)
        self.rng = np.random.RandomState(seed)
        self.model = self.new_model()
        ctx.set_option('jit', jit)
        try:
            self.batches = [self.upload(self.model, s) for s in sizes]
        finally:
            ctx.set_option('jit', -1)
        self.device = device

    def new_model(self):
        from raoteh_amd import device
        model = device.TreeModel(self.T, self.root, self.n, ctx=self.ctx)
        w = self.rng.uniform(0.1, 1.0, self.n)
        model.set_root_distn(w / w.sum())
        self.Q = smc.random_rates(self.n, self.rng)
        model.set_rates(Q_default=self.Q)
        return model

    def upload(self, model, nsites):
        dense = self.rng.uniform(0.05, 1.0, size=(nsites, len(self.obs_nodes), self.n))
        dense[self.rng.uniform(size=dense.shape) < 0.1] = 0.0
        dense[3, 0, :] = 0.0                          # a site of probability zero
        return model.upload_sites(self.obs_nodes, dense, kind='dense')

    def read(self, batch, model=None):
        model = model or self.model
        ll, st = model.fetch_log_likelihoods(batch)
        return [smc.bits(ll), st, smc.bits(model.fetch_totals(batch))]

    def close(self):
        for b in self.batches:
            b.close()
        self.model.close()


# ---- the sequences: each returns the list of arrays to compare --------------------------------

def seq_three_steps(w):
    b1, b2 = w.batches
    for b in (b1, b2, b1):
        w.model.step(b)
    return w.read(b1) + w.read(b2)


def seq_step_fetch(w):
    w.model.step(w.batches[0])
    return w.read(w.batches[0])


def seq_step_clone(w):
    b = w.batches[0]
    w.model.step(b)
    c = b.clone()
    out = w.read(c) + w.read(b)
    c.close()
    return out


def seq_set_rates_between(w):
    b = w.batches[0]
    w.model.step(b)
    w.model.set_rates(Q_default=0.7 * w.Q)
    w.model.step(b)
    return w.read(b)


def seq_step_prune(w):
    b = w.batches[0]
    w.model.step(b)
    w.model.prune(b)
    return w.read(b)


def seq_close_between(w):
    b, b2 = w.batches
    extra = w.upload(w.model, 37)
    w.model.step(extra)
    extra.close()
    w.model.step(b2)
    w.model.step(b)
    return w.read(b2) + w.read(b)


def seq_second_model(w):
    b, b2 = w.batches
    other = w.new_model()
    ob = w.upload(other, 21)
    w.model.step(b)
    other.step(ob)
    w.model.step(b2)
    out = w.read(b) + w.read(ob, other) + w.read(b2)
    ob.close()
    other.close()
    return out


def seq_same_batch_four_times(w):
    b = w.batches[0]
    out = []
    for k in range(4):
        w.model.set_rates(Q_default=(1.0 + 0.1 * k) * w.Q)
        w.model.step(b)
    out += w.read(b)
    w.model.step(b)
    w.model.step(b)
    return out + w.read(b)


def seq_root_distn_between(w):
    b = w.batches[0]
    w.model.step(b)
    w.model.set_root_distn(np.full(w.n, 1.0 / w.n))
    return w.read(b)


SEQUENCES = [seq_three_steps, seq_step_fetch, seq_step_clone, seq_set_rates_between, seq_step_prune,
             seq_close_between, seq_second_model, seq_same_batch_four_times, seq_root_distn_between]


def _both(ctx, n, tree, jit, sizes, seq, seed):
    out = {}
    for carry in ('0', None):
        if carry is None:
            os.environ.pop('RAOTEH_CARRY_COMBINE', None)
        else:
            os.environ['RAOTEH_CARRY_COMBINE'] = carry
        try:
            w = World(ctx, n, tree, jit, sizes, seed)
            out[carry] = seq(w)
            names = [b.kernel_name for b in w.batches if b.kernel_name]    # (of those that ran)
            w.close()
        finally:
            os.environ.pop('RAOTEH_CARRY_COMBINE', None)
    return out['0'], out[None], names


# (n, tree): every state count on the balanced tree, the other trees at 61 states
CASES = [(49, 'balanced'), (61, 'balanced'), (64, 'balanced'), (61, 'nine'), (61, 'three'),
         (61, 'observed root')]


@pytest.mark.parametrize('jit', [0, 1])
@pytest.mark.parametrize('n,tree', CASES)
def test_every_sequence_has_the_knob_off_bits(ctx, n, tree, jit):
    for k, seq in enumerate(SEQUENCES):
        # 37 and 70 sites: 3 and 5 tiles with a ragged last one; the single tile in turn
        sizes = (37, 70) if k % 3 else (16, 70)
        want, got, names = _both(ctx, n, tree, jit, sizes, seq, seed=1000 * n + 10 * k + jit)
        if tree != 'nine':           # (the 9-node tree's root may leave nothing to halve)
            assert all('halves' in name for name in names), names
        assert all(('jit' in name) == bool(jit) for name in names), names
        assert len(want) == len(got)
        for a, b in zip(want, got):
            assert a.shape == b.shape and np.array_equal(a, b), (seq.__name__, names, a, b)
        # the impossible site, and nothing else, is reported
        assert want[1][3] != 0 and (np.delete(want[1], 3) == 0).all()


def _combine_launches(ctx, n, jit, carry, steps):
    """(combine launches after `steps` steps of one batch and of two in turn, ... after the read)"""
    if carry:
        os.environ.pop('RAOTEH_CARRY_COMBINE', None)
    else:
        os.environ['RAOTEH_CARRY_COMBINE'] = '0'
    try:
        w = World(ctx, n, 'balanced', jit, (37, 70), seed=77 + n)
        ctx.sync()
        ctx.set_timing(1)
        ctx.reset_timing()
        for k in range(steps):
            w.model.step(w.batches[0])
        for k in range(steps):
            w.model.step(w.batches[k % 2])
        before = ctx.kernel_time(RT_K_COMBINE)[1]
        w.read(w.batches[0])
        w.read(w.batches[1])
        after = ctx.kernel_time(RT_K_COMBINE)[1]
        names = [b.kernel_name for b in w.batches]
        w.close()
    finally:
        ctx.set_timing(0)
        os.environ.pop('RAOTEH_CARRY_COMBINE', None)
    return before, after, names


@pytest.mark.parametrize('jit', [0, 1])
def test_carried_steps_launch_no_combine_kernel(ctx, jit):
    steps = 4
    off = _combine_launches(ctx, 61, jit, False, steps)
    on = _combine_launches(ctx, 61, jit, True, steps)
    assert all('halves' in name for name in on[2]), on[2]
    # knob off: one launch per step; carried: none, then the one flush of the last step's batch
    # (the other batch's combine went with the last step's expm launch)
    assert off[0] == 2 * steps and off[1] == 2 * steps, off
    assert on[0] == 0 and on[1] == 1, on


@pytest.mark.parametrize('n', [20, 122])
def test_other_state_counts_launch_what_they_launched(ctx, n):
    """Nothing is carried below 33 or above 64 states: the combine slot counts the same launches
    with the knob on and off."""
    off = _combine_launches(ctx, n, 0, False, 3)
    on = _combine_launches(ctx, n, 0, True, 3)
    assert on[:2] == off[:2], (on, off)
