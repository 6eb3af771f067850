"""Host side of rt_sites_sample_states: the numpy Philox reproduces the published known answers;
the replay check of tests/_sample_cases.py is itself checked with a numpy sampler that follows
the pinned rule (it passes, a moved pick fails, its draws follow the oracle's posterior law);
the shapes the GPU tests rely on are chosen here with the oracle; the entry point, its binding
and the Python surface exist."""
import inspect
import re

import numpy as np
import pytest

from conftest import ROOT
from _posterior_cases import oracle_pmaps, oracle_site
import _sample_cases as sc


def test_philox_known_answers():
    from raoteh_amd._philox import philox4x32, philox_uniform
    out = philox4x32((0, 0, 0, 0), (0, 0))
    assert ['%08x' % int(x) for x in out] == ['6627e8d5', 'e169c58d', 'bc57ac4c', '9b00dbd8']
    f = 0xffffffff
    out = philox4x32((f, f, f, f), (f, f))
    assert ['%08x' % int(x) for x in out] == ['408f276d', '41c83b0e', 'a20bc7c6', '6d5451fd']
    # the double: ((c0 << 21) ^ (c1 >> 11)) mod 2^53, times 2^-53; the arguments broadcast
    bits = ((0x6627e8d5 << 21) ^ (0xe169c58d >> 11)) & ((1 << 53) - 1)
    assert philox_uniform(0, 0, 0) == bits / 2.0 ** 53
    u = philox_uniform(2 ** 64 - 1, np.array([[2 ** 64 - 1]], dtype=np.uint64),
                       np.array([0, 2 ** 64 - 1], dtype=np.uint64))
    assert u.shape == (1, 2)
    bits = ((0x408f276d << 21) ^ (0x41c83b0e >> 11)) & ((1 << 53) - 1)
    assert u[0, 1] == bits / 2.0 ** 53 and 0.0 <= u[0, 0] < 1.0 and u[0, 0] != u[0, 1]


def small_case(n, kind='state', seed=3, nsites=5):
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=seed, nnodes=11)
    pre, idx, ptr, esd, parent = sc.tree_arrays(T, root, n, Q)
    if kind == 'dense':
        _, lik = sc.dense_observations(n, nsites, len(leaves), rng)
    else:
        _, lik = sc.state_observations(n, nsites, len(leaves), rng)
    L = oracle_pmaps(idx, ptr, esd, [pre.index(v) for v in leaves], lik)
    return esd, L, rd, parent


@pytest.mark.parametrize('n', [3, 20])
def test_the_numpy_sampler_passes_the_replay_check(n):
    esd, L, rd, parent = small_case(n, kind='dense')
    states, status = sc.numpy_sample(esd, L, rd, parent, seed=11, first_draw=4, ndraws=6)
    assert status.tolist() == [0, 0, 0, 0, 1]            # (the dense case zeroes its last site)
    assert (states[:, -1] == 255).all() and (states[:, :-1] < n).all()
    checked = sc.replay_check(states, status, esd, L, rd, parent, seed=11, first_draw=4)
    assert checked == 6 * 4 * L.shape[1]
    # the counter layout: a split call, another seed, another first draw
    a, _ = sc.numpy_sample(esd, L, rd, parent, seed=11, first_draw=6, ndraws=4)
    assert np.array_equal(a, states[2:])
    b, _ = sc.numpy_sample(esd, L, rd, parent, seed=12, first_draw=4, ndraws=6)
    assert not np.array_equal(b, states)
    with pytest.raises(sc.ReplayError):
        sc.replay_check(states, status, esd, L, rd, parent, seed=11, first_draw=5)
    with pytest.raises(sc.ReplayError):
        sc.replay_check(states, status, esd, L, rd, parent, seed=12, first_draw=4)


@pytest.mark.parametrize('n', [3, 20])
def test_a_moved_pick_fails_the_replay_check(n):
    """Negative control: one pick moved to a neighbouring state of positive weight."""
    esd, L, rd, parent = small_case(n)
    states, status = sc.numpy_sample(esd, L, rd, parent, seed=5, first_draw=0, ndraws=3)
    sc.replay_check(states, status, esd, L, rd, parent, seed=5)
    moved = 0
    for d, i, v in [(0, 0, 0), (1, 2, 4), (2, 4, L.shape[1] - 1)]:
        a = None if v == 0 else int(states[d, i, parent[v]])
        w = sc.weights_of(v, a, esd, L[i], rd, n)
        b = int(states[d, i, v])
        near = [s for s in (b - 1, b + 1) if 0 <= s < n and w[s] > 0]
        if not near:
            continue
        bad = states.copy()
        bad[d, i, v] = near[0]
        # (the children of v are judged given the moved state: the failure is at v itself)
        with pytest.raises(sc.ReplayError, match='node %d, draw %d, site %d' % (v, d, i)):
            sc.replay_check(bad, status, esd, L, rd, parent, seed=5)
        moved += 1
    assert moved >= 1


def test_a_wrong_status_or_a_state_at_a_dead_site_fails():
    esd, L, rd, parent = small_case(5, kind='dense')
    states, status = sc.numpy_sample(esd, L, rd, parent, seed=1, first_draw=0, ndraws=2)
    sc.replay_check(states, status, esd, L, rd, parent, seed=1)
    with pytest.raises(sc.ReplayError):
        sc.replay_check(states, np.zeros_like(status), esd, L, rd, parent, seed=1)
    bad = states.copy()
    bad[0, -1, 3] = 0
    with pytest.raises(sc.ReplayError):
        sc.replay_check(bad, status, esd, L, rd, parent, seed=1)


@pytest.mark.parametrize('n', [4, 20])
def test_the_numpy_sampler_follows_the_posterior_law(n):
    """14-node random tree, 2 sites, 8192 draws, to 5 sigma + 1e-9 per cell: at n = 4 the node
    marginals and the full joint endpoint laws of the oracle; at n = 4 and 20 the node marginals
    and the joint law summed over eight sets per edge (the cells of a 20 x 20 joint law are too
    rare for a normal bound).  LAW_SEED is chosen here so that the reference sampler alone is
    inside the bounds; the GPU test reuses seed, shapes and checks."""
    T, root, leaves, Q, rd, data, lik = sc.law_case(n)
    pre, idx, ptr, esd, parent = sc.tree_arrays(T, root, n, Q)
    assert len(pre) == sc.LAW_NNODES
    L = oracle_pmaps(idx, ptr, esd, [pre.index(v) for v in leaves], lik)
    states, status = sc.numpy_sample(esd, L, rd, parent, sc.LAW_SEED, 0, sc.LAW_DRAWS)
    assert not status.any()
    for i in range(sc.LAW_SITES):
        D, J = oracle_site(idx, ptr, esd, rd, L[i])
        if n == 4:
            assert sc.law_deviation(states[:, i], D, J, parent) <= 0.0
        esets = sc.law_edge_sets(n)
        ev = np.array([[J[v][np.ix_(A, B)].sum() if v else 0.0 for A, B in esets]
                       for v in range(len(pre))])
        assert sc.law_set_deviation(states[:, i], D, ev, esets, parent) <= 0.0
    # ... and a sampler with the wrong law is outside it (every draw shifted by one state)
    D, J = oracle_site(idx, ptr, esd, rd, L[0])
    assert sc.law_deviation((states[:, 0] + 1) % n, D, J, parent) > 0.0


@pytest.mark.parametrize('nnodes', [4096, 8192])
def test_the_big_tree_of_the_gpu_test_does_not_underflow(nnodes):
    """4096 and 8192 nodes, n = 5: the broom's root totals stay above 1e-280 and its schedule is
    one the fast kernels take (at most 16 accumulator slots)."""
    import ctypes
    from raoteh_amd import _lib
    from raoteh_amd._tree import TreeArrays
    n = 5
    T, root, leaves = sc.broom_tree(nnodes)
    assert len(T) == nnodes and len(leaves) == 64
    rng = np.random.RandomState(8)
    Q = sc.rate_matrix(n, rng)
    pre, idx, ptr, esd, parent = sc.tree_arrays(T, root, n, Q)
    _, lik = sc.state_observations(n, 17, len(leaves), rng, unobserved=0.0)
    L = oracle_pmaps(idx, ptr, esd, [pre.index(v) for v in leaves], lik)
    assert (L[:, 0].sum(axis=1) > 1e-280).all()
    ta = TreeArrays(T, root)
    ops = np.zeros((nnodes, 4), dtype=np.int32)
    depth = ctypes.c_int32(0)
    rc = _lib.lib().rt_build_schedule(
        nnodes, ta.indices.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
        ta.indptr.ctypes.data_as(ctypes.POINTER(ctypes.c_int64)),
        ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), ctypes.byref(depth))
    assert rc == 0 and depth.value <= 16


def test_host_mirror_mc0():
    """_sample_mc0_dense.resample_states: the reference's signature and errors; the draw passes
    the replay check with the seed passed in; np.random.seed governs a call without one."""
    import networkx as nx
    from raoteh_amd import _sample_mc0_dense as smc0, _sample_mcy_dense as smcy
    from raoteh_amd import StructuralZeroProb
    assert list(inspect.signature(smc0.resample_states).parameters) == [
        'T', 'root', 'node_to_pmap', 'nstates', 'root_distn', 'P_default', 'seed']
    assert list(inspect.signature(smcy.resample_states).parameters) == [
        'T', 'root', 'nstates', 'node_to_allowed_states', 'root_distn', 'P_default', 'seed']
    n = 6
    T, root, leaves, Q, rd, rng = sc.random_case(n, seed=17, nnodes=12)
    pre, idx, ptr, esd, parent = sc.tree_arrays(T, root, n, Q)
    for v in range(1, len(pre)):
        T[pre[parent[v]]][pre[v]]['P'] = esd[v]
    assert pre == list(nx.dfs_preorder_nodes(T, root))
    _, lik = sc.state_observations(n, 1, len(leaves), rng)
    L = oracle_pmaps(idx, ptr, esd, [pre.index(v) for v in leaves], lik)
    pmap = dict((v, L[0, i]) for i, v in enumerate(pre))
    got = smc0.resample_states(T, root, pmap, n, root_distn=rd, seed=77)
    assert sorted(got) == sorted(pre)
    states = np.array([[[got[v] for v in pre]]], dtype=np.uint8)
    sc.replay_check(states, [0], esd, L, rd, parent, seed=77)
    np.random.seed(4)
    a = smc0.resample_states(T, root, pmap, n, root_distn=rd)
    np.random.seed(4)
    b = smc0.resample_states(T, root, pmap, n, root_distn=rd)
    assert a == b
    dead = dict(pmap)
    dead[root] = np.zeros(n)
    with pytest.raises(StructuralZeroProb):
        smc0.resample_states(T, root, dead, n, root_distn=rd, seed=1)


def test_entry_point_is_declared_bound_and_surfaced():
    from raoteh_amd import _lib, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    assert re.search(r'\bint rt_sites_sample_states\(', header)
    m = re.search(r'#define RT_MAX_SAMPLE_NODES (\d+)\b', header)
    assert m and int(m.group(1)) == _lib.RT_MAX_SAMPLE_NODES >= 4096
    restype, argtypes = _lib.SIGNATURES['rt_sites_sample_states']
    assert len(argtypes) == 8
    assert getattr(_lib.lib(), 'rt_sites_sample_states') is not None
    assert callable(device.TreeModel.sample_states)
    assert device.SampledStates._fields == ('states', 'status', 'nodes')
    # the draw block: the tree alone decides it; no tree beyond the stated limit
    db = _lib.lib().rt_sample_states_draw_block
    assert db(14) == 16 and db(127) == 16 and db(4096) == 1 and db(_lib.RT_MAX_SAMPLE_NODES) == 1
    assert db(_lib.RT_MAX_SAMPLE_NODES + 1) == 0
    assert all(db(N) * N * 16 <= max(32 * 1024, 16 * N) for N in range(2, 3000, 7))
