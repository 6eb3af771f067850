"""Rao-Teh passes at 65 to 128 states, the part that needs no device: the fixture from the
reference against the oracle, and the two-word set masks of the package."""
import numpy as np
import networkx as nx
import pytest

from _forest_wide_cases import forest_wide_cases, lumped_cycle, rows
from oracle import oracle_numpy as orc


def test_fixture_covers_what_it_should():
    cases = forest_wide_cases()
    by_n = {}
    for c, T in cases:
        if not c.get('single') and not c['zero']:
            by_n[c['nstates']] = by_n.get(c['nstates'], 0) + 1
    assert sorted(by_n) == [65, 96, 122, 128] and min(by_n.values()) >= 2
    assert any(c.get('single') for c, _ in cases) and any(c.get('zero') for c, _ in cases)
    kinds = set()
    for c, T in cases:
        n = c['nstates']
        for ss in c['allowed'].values():
            if len(ss) == n:
                continue
            assert all(0 <= s < n for s in ss)
            if len(ss) == 1:
                kinds.add('single')
            elif max(ss) < 64:
                kinds.add('low')
            elif min(ss) >= 64:
                kinds.add('high')
            else:
                kinds.add('straddle')
        # P = I + Q / omega, a stochastic matrix with structural zeros
        np.testing.assert_allclose(c['P'], np.identity(n) + c['Q'] / c['omega'], rtol=0, atol=1e-15)
        np.testing.assert_allclose(c['P'].sum(axis=1), 1.0, rtol=1e-12)
        assert (c['P'] == 0).sum() > n * n // 2
    assert kinds == {'single', 'low', 'high', 'straddle'}


def test_fixture_agrees_with_the_oracle():
    """pset, set and pmap of the reference's un-accelerated passes against the oracle's esd
    passes with P replicated on every edge: sets exactly, pmap at rtol 1e-12."""
    from raoteh_amd._tree import TreeArrays
    done = 0
    for c, T in forest_wide_cases():
        if c.get('single'):
            continue
        n = c['nstates']
        ta = TreeArrays(T, c['root'])
        esd = np.broadcast_to(c['P'], (ta.nnodes, n, n)).copy()
        mask = np.zeros((ta.nnodes, n), dtype=np.int64)
        for i, v in enumerate(ta.preorder_nodes):
            mask[i, sorted(c['allowed'][str(v)])] = 1
        orc.mcy_esd_get_node_to_pset(ta.indices, ta.indptr, esd, mask)
        for i, v in enumerate(ta.preorder_nodes):
            assert set(np.nonzero(mask[i])[0]) == set(c['pset'][str(v)]), v
        orc.esd_get_node_to_set(ta.indices, ta.indptr, esd, mask)
        for i, v in enumerate(ta.preorder_nodes):
            assert set(np.nonzero(mask[i])[0]) == set(c['set'][str(v)]), v
        pmap = orc.mcy_esd_get_node_to_pmap(ta.indices, ta.indptr, esd, mask)
        for i, v in enumerate(ta.preorder_nodes):
            np.testing.assert_allclose(pmap[i], rows(c['pmap'], v, n), rtol=1e-12, atol=0)
        if c['zero']:
            assert not pmap[0].dot(c['root_distn']) > 0 and 'distn' not in c
        else:
            assert pmap[0].dot(c['root_distn']) == pytest.approx(c['likelihood'], rel=1e-12)
            for v in T:
                d = rows(c['distn'], v, n)
                assert d.sum() == pytest.approx(1.0, rel=1e-12)
                assert set(np.nonzero(d)[0]) <= set(c['set'][str(v)])
        done += 1
    assert done >= 9


def test_mask_shapes_and_bit_layout():
    """Forest.masks: one word per node up to 64 states, two above (state s = bit s % 64 of word
    s // 64); sets that straddle the words round-trip; 129 states are refused."""
    from raoteh_amd import _forest
    T = nx.path_graph(5)
    forest = _forest.Forest([(T, 0), (T, 2)])
    straddle = {0, 5, 63, 64, 70, 121}
    obs = [{0: straddle, 3: {64}, 4: {63}}, {2: {121}, 0: set()}]
    m = forest.masks(obs, nstates=122)
    assert m.shape == (forest.total, 2) and m.dtype == np.uint64
    got = forest.split(m)
    assert [int(x) for x in got[0][0]] == [(1 << 0) | (1 << 5) | (1 << 63), (1 << 0) | (1 << 6) | (1 << 57)]
    assert [int(x) for x in got[0][3]] == [0, 1]
    assert [int(x) for x in got[0][4]] == [1 << 63, 0]
    assert [int(x) for x in got[1][2]] == [0, 1 << 57]
    assert [int(x) for x in got[1][0]] == [0, 0]
    # unrestricted nodes: all 122 states, no bit at or above 122
    assert [int(x) for x in got[0][1]] == [2 ** 64 - 1, 2 ** 58 - 1]
    assert [int(x) for x in got[1][4]] == [2 ** 64 - 1, 2 ** 58 - 1]
    for k, d in enumerate(obs):
        for v in T:
            want = d.get(v, set(range(122)))
            assert _forest.mask_to_states(got[k][v], 122) == want
    # 128 states: both words full
    assert [int(x) for x in forest.masks(None, nstates=128)[0]] == [2 ** 64 - 1, 2 ** 64 - 1]
    assert [int(x) for x in forest.masks(None, nstates=65)[0]] == [2 ** 64 - 1, 1]
    # one word up to 64 states, as ever
    m64 = forest.masks([{0: {0, 63}}, None], nstates=64)
    assert m64.shape == (forest.total,) and m64.dtype == np.uint64
    assert int(m64[0]) == (1 << 63) | 1 and int(m64[1]) == 2 ** 64 - 1
    m4 = forest.masks(None, nstates=4)
    assert m4.shape == (forest.total,) and (m4 == 15).all()
    np.testing.assert_array_equal(forest.masks(obs[:1] + [None], 122), forest.allowed_masks(obs[:1] + [None], 122))
    with pytest.raises(ValueError):
        forest.masks(None, nstates=129)
    with pytest.raises(ValueError):
        forest.masks([{0: {122}}, None], nstates=122)


def test_lumped_cycle_lumps_onto_the_four_cycle():
    """The rate matrix of the stationary-law test: the class c = s % 4 moves as the unit-rate
    4-cycle whatever the replica, and no transition keeps the class."""
    for n in (128, 100):
        Q = lumped_cycle(n)
        cls = np.arange(n) % 4
        lump = np.zeros((n, 4))
        lump[np.arange(n), cls] = 1.0
        QL = Q.dot(lump)
        want = np.zeros((4, 4))
        for i in range(4):
            want[i, (i + 1) % 4] = 1.0
            want[i, i] = -1.0
        np.testing.assert_allclose(QL, want[cls], rtol=0, atol=1e-14)
        off = Q.copy()
        np.fill_diagonal(off, 0.0)
        assert not off[cls[:, None] == cls[None, :]].any()
