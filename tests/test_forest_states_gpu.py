"""The one-word Rao-Teh forest kernels (csrc/forest.hip: the grouped forms for up to 4, 8 and 16
states and the wave-per-tree form for 17 to 64) at the state counts of _forest_states_cases.py,
against the oracle: sets exactly, pmap at the rounding bound of the two upward passes, and every
sampled state replayed against its Philox uniform and the oracle's subtree likelihoods.  Then the
grouped forms against the wave-per-tree form bit for bit, the device-resident chains at 61 and 20
states, and the closed-form stationary law at 60 and 20 states."""
import ctypes

import numpy as np
import pytest

from _forest_states_cases import (BIG_STATES, GROUPED_LIMITS, NTREES, STATES, case, check_pmap,
                                  check_sets, forest_replay_check, offsets_of)
from _forest_wide_cases import check_lumped_cycle_law, check_resident_histories

pytestmark = pytest.mark.gpu

SWEEPS = (0, 7)
SEED = 5
i64, i32, f64, u64 = ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_uint64


@pytest.fixture(scope='module')
def ra():
    import raoteh_amd
    from raoteh_amd import device, _lib, synth, pyfelscore_compat

    class NS(object):
        pass
    ns = NS()
    ns.pkg, ns.device, ns.lib, ns.synth, ns.pyf = raoteh_amd, device, _lib, synth, pyfelscore_compat
    ns.ctx = device.get_context()
    return ns


def _p(a, t):
    return a.ctypes.data_as(ctypes.POINTER(t))


def _forest_of(c):
    """(Forest, allowed masks uint64[total] with every bit at or above n set on every third node:
    the entry points ignore those bits)."""
    from raoteh_amd import _forest
    forest = _forest.Forest(c.trees)
    assert forest.total == offsets_of(c.refs)[-1] and forest.total <= 1500
    assert forest.indices.size >= forest.total - forest.ntrees
    assert forest.indptr.size == forest.total + forest.ntrees
    masks = forest.allowed_masks(c.obs, c.n)
    junk = np.uint64((2 ** 64 - 1) & ~((1 << c.n) - 1))
    masks[::3] |= junk
    return forest, masks


def _passes(ra, c, forest, masks):
    """rt_forest_passes -> (sets uint64[total], L f64[total, n])."""
    sets = masks.copy()
    L = np.full((forest.total, c.n), np.nan)
    P = np.ascontiguousarray(c.P)
    ra.lib.check(ra.lib.lib().rt_forest_passes(
        ra.ctx._h, c.n, forest.ntrees, _p(forest.node_offset, i64), _p(forest.indices, i64),
        _p(forest.indptr, i64), _p(P, f64), _p(sets, u64), _p(L, f64)))
    return sets, L


def _resample(ra, c, forest, masks, root, sweep, want_L=True):
    """rt_forest_resample_states -> (sets, L or None, states int32[total], status int32[ntrees])."""
    sets = masks.copy()
    L = np.full((forest.total, c.n), np.nan) if want_L else None
    states = np.full(forest.total, -7, dtype=np.int32)
    status = np.full(forest.ntrees, -7, dtype=np.int32)
    P = np.ascontiguousarray(c.P)
    rd = None if root is None else np.ascontiguousarray(root, dtype=np.float64)
    ra.lib.check(ra.lib.lib().rt_forest_resample_states(
        ra.ctx._h, c.n, forest.ntrees, _p(forest.node_offset, i64), _p(forest.indices, i64),
        _p(forest.indptr, i64), _p(P, f64), None if rd is None else _p(rd, f64), _p(sets, u64),
        u64(SEED), u64(sweep), _p(states, i32), _p(status, i32), None if L is None else _p(L, f64)))
    return sets, L, states, status


@pytest.mark.parametrize('n', STATES)
def test_forest_passes_match_the_oracle(ra, n):
    """_forest.get_node_to_set_and_pmap on the ragged forest of 45 trees (and, at 4, 8, 16, 33
    and 61 states, a 46th beyond the LDS image): sets equal to the oracle's, pmap within
    rtol max(1e-12, N (w + n + 2) 2^-53) at atol 0 (pmap_rtol)."""
    from raoteh_amd import _forest
    c = case(n)
    forest = _forest.Forest(c.trees)
    sets, pmaps = _forest.get_node_to_set_and_pmap(forest, c.P, c.obs, ctx=ra.ctx)
    assert len(sets) == len(c.refs) == NTREES + (n in BIG_STATES)
    masks = np.array([_forest.states_to_mask(sets[k][v], n)
                      for k, r in enumerate(c.refs) for v in r.ta.preorder_nodes], dtype=np.uint64)
    L = np.array([pmaps[k][v] for k, r in enumerate(c.refs) for v in r.ta.preorder_nodes])
    check_sets(masks, c.refs, n)
    check_pmap(L, c.refs, n, c.width)


@pytest.mark.parametrize('n', STATES)
def test_shared_matrix_entry_points_match_the_oracle(ra, n):
    """pyfelscore.mcy_get_node_to_pset and get_node_to_set with the reference's argument lists
    (the tree CSR, the matrix as a boolean CSR, the int state mask in place) on three trees,
    the largest of the forest among them: the oracle's pset and set exactly."""
    c = case(n)
    P = c.P
    tptr = np.concatenate([[0], np.cumsum((P != 0).sum(axis=1))]).astype(np.int64)
    tidx = np.nonzero(P != 0)[1].astype(np.int64)
    small = c.refs[:NTREES]
    largest = max(range(NTREES), key=lambda k: small[k].N)
    changed = 0
    for k in sorted({2, largest, len(c.refs) - 1}):
        r = c.refs[k]
        mask = r.allowed.astype(np.int64)
        ra.pyf.mcy_get_node_to_pset(r.ta.indices, r.ta.indptr, tidx, tptr, mask)
        np.testing.assert_array_equal(mask, r.pset.astype(np.int64))
        tmp = np.zeros(n, dtype=np.int64)
        ra.pyf.get_node_to_set(r.ta.indices, r.ta.indptr, tidx, tptr, mask, tmp)
        np.testing.assert_array_equal(mask, r.sets.astype(np.int64))
        changed += bool((r.sets != r.allowed).any())
    assert changed or n <= 3


@pytest.mark.parametrize('n', STATES)
def test_forest_draws_replay_against_the_oracle(ra, n):
    """rt_forest_resample_states with a subtree_probability buffer, sweeps 0 and 7: the L it
    returns is bit for bit the L of rt_forest_passes; every pick lies where its Philox uniform
    puts it in the cdf of the ORACLE's weights, at eps 1e-10 (forest_replay_check); statuses
    are 0 or 1 as the host likelihood says and zero trees carry -1; the same arguments give the
    same states and another sweep others; rt_forest_resample_states_parents (the entry of
    _sampler.HistoryBatch) gives the same states and status; without a root prior the root is
    drawn with unit weights."""
    c = case(n)
    forest, masks = _forest_of(c)
    want_sets, want_L = _passes(ra, c, forest, masks)
    full = np.uint64((1 << n) - 1)
    check_sets(want_sets, c.refs, n)
    check_pmap(want_L, c.refs, n, c.width)
    live = np.array([r.live for r in c.refs])
    off = offsets_of(c.refs)
    parent = np.concatenate([r.parent for r in c.refs]).astype(np.int32)
    P = np.ascontiguousarray(c.P)
    seen = []
    for sweep in SWEEPS:
        sets, L, states, status = _resample(ra, c, forest, masks, c.root, sweep)
        np.testing.assert_array_equal(sets & full, want_sets & full)
        assert np.array_equal(L, want_L)                                          # (i)
        checked = forest_replay_check(states, status, c.P, c.refs, c.root, n, SEED, sweep)  # (ii)
        assert checked == sum(r.N for r in c.refs if r.live)
        np.testing.assert_array_equal(status, np.where(live, 0, 1))               # (iii)
        for k in np.nonzero(~live)[0]:
            assert (states[off[k]:off[k + 1]] == -1).all()
        again = _resample(ra, c, forest, masks, c.root, sweep, want_L=False)      # (iv)
        np.testing.assert_array_equal(again[2], states)
        np.testing.assert_array_equal(again[3], status)
        sets_p = masks.copy()                                                     # (v)
        states_p = np.full(forest.total, -7, dtype=np.int32)
        status_p = np.full(forest.ntrees, -7, dtype=np.int32)
        ra.lib.check(ra.lib.lib().rt_forest_resample_states_parents(
            ra.ctx._h, n, forest.ntrees, _p(forest.node_offset, i64), _p(parent, i32), _p(P, f64),
            _p(c.root, f64), _p(sets_p, u64), u64(SEED), u64(sweep), _p(states_p, i32),
            _p(status_p, i32)))
        np.testing.assert_array_equal(states_p, states)
        np.testing.assert_array_equal(status_p, status)
        np.testing.assert_array_equal(sets_p & full, want_sets & full)
        seen.append(states)
    assert not np.array_equal(seen[0], seen[1])
    sets, L, states, status = _resample(ra, c, forest, masks, None, SWEEPS[1])    # (vi)
    assert np.array_equal(L, want_L)
    forest_replay_check(states, status, c.P, c.refs, None, n, SEED, SWEEPS[1])
    assert (status == 0).sum() >= live.sum()


@pytest.mark.parametrize('n', [n for n in STATES if n <= GROUPED_LIMITS[-1]])
def test_grouped_kernels_give_the_draws_of_the_wave_per_tree_kernels(ra, n, monkeypatch):
    """Up to 16 states RAOTEH_FOREST_WAVE_PER_TREE (read at every launch) sends the forest
    through the wave-per-tree kernels, with 2 to 16 live lanes: sets, L, states and status are
    bit for bit those of the grouped kernels -- the grouped scan adds the same terms in the same
    order and the idle lanes add exact zeros -- and pass the oracle checks themselves."""
    c = case(n)
    forest, masks = _forest_of(c)
    full = np.uint64((1 << n) - 1)
    monkeypatch.delenv('RAOTEH_FOREST_WAVE_PER_TREE', raising=False)
    grouped = [_resample(ra, c, forest, masks, c.root, sweep) for sweep in SWEEPS]
    grouped_passes = _passes(ra, c, forest, masks)
    monkeypatch.setenv('RAOTEH_FOREST_WAVE_PER_TREE', '1')
    wave = [_resample(ra, c, forest, masks, c.root, sweep) for sweep in SWEEPS]
    wave_passes = _passes(ra, c, forest, masks)
    monkeypatch.delenv('RAOTEH_FOREST_WAVE_PER_TREE')
    np.testing.assert_array_equal(wave_passes[0] & full, grouped_passes[0] & full)
    assert np.array_equal(wave_passes[1], grouped_passes[1])
    for sweep, g, w in zip(SWEEPS, grouped, wave):
        np.testing.assert_array_equal(w[0] & full, g[0] & full)
        assert np.array_equal(w[1], g[1])
        np.testing.assert_array_equal(w[2], g[2])
        np.testing.assert_array_equal(w[3], g[3])
        check_sets(w[0], c.refs, n)
        check_pmap(w[1], c.refs, n, c.width)
        forest_replay_check(w[2], w[3], c.P, c.refs, c.root, n, SEED, sweep)


@pytest.mark.parametrize('name', ['c3', 'c5'])
def test_device_resident_histories_at_61_and_20_states(ra, name):
    """rt_chains_* on the 61-state codon model (synth c3, 127 nodes) and the 20-state compound
    model (c5, 63 nodes; the rate matrix of its first edge on every edge), 100 chains with
    one-word masks from the leaf observations and every bit at or above n set on top: the
    assertions of test_wide_device_resident_histories_are_consistent_and_reproducible
    (check_resident_histories); sweep_stats_kernel<1> runs with idle lanes."""
    from raoteh_amd import _forest, _sampler
    C = 100
    cfg = ra.synth.make_config(name, nsites=C)
    T, root, n = cfg['T'], cfg['root'], cfg['nstates']
    assert n == dict(c3=61, c5=20)[name]
    Q = cfg['Q_default']
    if Q is None:
        Q = T[root][next(iter(T[root]))]['Q']
    index = _sampler.TreeArrays(T, root).node_to_index
    N = len(index)
    masks = np.empty((C, N), dtype=np.uint64)
    masks[:] = _forest.full_mask(n)
    if cfg['obs_kind'] == 'state':
        table = np.array([_forest.states_to_mask([s], n) for s in range(n)], dtype=np.uint64)
    else:
        table = np.array([_forest.states_to_mask(ss, n) for ss in cfg['leaf_allowed']],
                         dtype=np.uint64)
    cols = [index[v] for v in cfg['leaves']]
    masks[:, cols] = table[cfg['leaf_states']]
    assert (masks[:, cols] != _forest.full_mask(n)).all()
    masks |= np.uint64((2 ** 64 - 1) & ~((1 << n) - 1))       # bits at or above n are ignored
    rows_ = check_resident_histories(ra.ctx, T, root, Q, cfg['root_distn'], masks)
    assert n < 33 or ((rows_[3] >= 32).any() and (rows_[3] < 32).any())
    # a chain without a feasible history is an error at creation
    bad = masks.copy()
    bad[5, cols[0]] = np.uint64((2 ** 64 - 1) & ~((1 << n) - 1))
    with pytest.raises(ra.pkg.StructuralZeroProb):
        _sampler.DeviceHistoryBatch(T, root, Q, node_masks=bad, ctx=ra.ctx)


@pytest.mark.parametrize('where,n,lengths,factor,sweeps', [
    ('device', 60, (3.0, 2.0), 2.0, 400),
    ('device', 20, (0.9, 0.7), 2.0, 3000),
])
def test_stationary_law_on_a_lumped_cycle_is_exact(ra, where, n, lengths, factor, sweeps):
    """test_wide_stationary_law_on_a_lumped_cycle_is_exact at 60 and 20 states (n = 4 R), in
    the wave-per-tree form of the one-word kernels: the same closed form, chains and criteria
    (check_lumped_cycle_law)."""
    check_lumped_cycle_law(ra.ctx, where, n, lengths, factor, sweeps)
