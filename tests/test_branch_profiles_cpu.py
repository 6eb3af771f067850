"""Host side of rt_sites_branch_profiles: the host reference the GPU tests compare against
(tests/_profile_cases.py: scipy expm per trial length + the oracle's pruning) reproduces a
closed form; the C ABI entry point, its binding and the Python surface exist; the argument check
of the grid of lengths."""
import re

import networkx as nx
import numpy as np
import pytest

from conftest import ROOT
from _profile_cases import make_grid, profile_from_transitions


def jc_same(alpha, t):
    """Jukes-Cantor, every off-diagonal rate alpha: P(t)[a][a]."""
    return 0.25 + 0.75 * np.exp(-4.0 * alpha * t)


def jc_diff(alpha, t):
    """... and P(t)[a][b], a != b."""
    return 0.25 - 0.25 * np.exp(-4.0 * alpha * t)


def test_host_reference_reproduces_a_closed_form():
    """Two leaves under a root with the uniform distribution: the likelihood of the leaf states
    (x, y) is P(t1 + t2)[x][y] / 4 (Chapman-Kolmogorov through the reversible root), so the
    profile of leaf 1's branch is log P(tau + t2)[x][y] - log P(t1 + t2)[x][y], with the
    Jukes-Cantor entries written out above."""
    from raoteh_amd._tree import TreeArrays
    alpha, t1, t2 = 0.3, 0.4, 0.9
    T = nx.Graph()
    T.add_edge('r', 'a', weight=t1)
    T.add_edge('r', 'b', weight=t2)
    ta = TreeArrays(T, 'r')
    va, vb = ta.node_to_index['a'], ta.node_to_index['b']
    Q = alpha * (np.ones((4, 4)) - 4.0 * np.eye(4))
    t = ta.branch_lengths()
    assert t[va] == t1 and t[vb] == t2
    esd = np.zeros((3, 4, 4))
    for v in (va, vb):
        same, diff = jc_same(alpha, t[v]), jc_diff(alpha, t[v])
        esd[v] = diff + (same - diff) * np.eye(4)
    # sites: equal states, different states, leaf a unobserved (its branch cannot matter), and
    # the pair (x, y) = (2, 3) once more
    obs = np.zeros((4, 2, 4))
    for i, (x, y) in enumerate([(1, 1), (0, 3), (None, 2), (2, 3)]):
        obs[i, 0] = 1.0 if x is None else np.eye(4)[x]
        obs[i, 1] = np.eye(4)[y]
    grid = np.array([[0.0] * 5, [0.0] * 5, [0.0] * 5])
    grid[va] = [t1, 0.0, 0.05, 1.3, 40.0]
    grid[vb] = [t2, 0.01, 0.45, 2.0, 7.5]
    values, status, loglik = profile_from_transitions(
        ta.indices, ta.indptr, esd, [va, vb], obs, np.full(4, 0.25), Q[None],
        np.zeros(3, dtype=np.int64), grid)
    assert not status.any()
    assert loglik == pytest.approx(np.log([jc_same(alpha, t1 + t2) / 4, jc_diff(alpha, t1 + t2) / 4,
                                           0.25, jc_diff(alpha, t1 + t2) / 4]), abs=1e-12)
    want = np.zeros((4, 3, 5))
    for v, other in ((va, t2), (vb, t1)):
        tot = grid[v] + other
        want[0, v] = np.log(jc_same(alpha, tot)) - np.log(jc_same(alpha, t1 + t2))
        want[1, v] = np.log(jc_diff(alpha, tot)) - np.log(jc_diff(alpha, t1 + t2))
        want[3, v] = want[1, v]
    want[2, vb] = 0.0                          # (P(tau) 1)[y] / 4 = 1 / 4 at every length
    assert np.abs(values - want).max() <= 1e-12
    assert not values[:, 0].any()                                    # the root's row
    assert np.abs(values[:, :, 0]).max() <= 1e-12                    # the resident lengths


def test_host_reference_gives_minus_infinity_and_zero_sites():
    """A branch of length 0 between two different observed states has likelihood 0: -inf at a
    live site; a site of zero likelihood at the resident lengths gives status 1 and zeros."""
    from raoteh_amd._tree import TreeArrays
    T = nx.Graph()
    T.add_edge(0, 1, weight=0.5)
    T.add_edge(0, 2, weight=0.25)
    ta = TreeArrays(T, 0)
    assert list(ta.preorder_nodes) == [0, 1, 2]
    Q = np.array([[-1.0, 1.0, 0.0], [0.5, -1.0, 0.5], [0.0, 0.0, 0.0]])   # state 2 absorbs
    import scipy.linalg
    esd = np.zeros((3, 3, 3))
    for v in (1, 2):
        esd[v] = scipy.linalg.expm(Q * ta.branch_lengths()[v])
    eye = np.eye(3)
    # the root is observed too: site 0 root 0 -> leaves (1, 0); site 1 root 2 -> leaf 0: impossible
    obs = np.array([[eye[0], eye[1], eye[0]], [eye[2], eye[0], eye[2]]])
    grid = np.array([[0.0, 0.0], [0.0, 0.5], [0.0, 0.25]])
    values, status, loglik = profile_from_transitions(
        ta.indices, ta.indptr, esd, [0, 1, 2], obs, np.full(3, 1.0 / 3), Q[None],
        np.zeros(3, dtype=np.int64), grid)
    assert status.tolist() == [0, 1] and loglik[1] == 0.0
    assert values[0, 1, 0] == -np.inf and values[0, 1, 1] == pytest.approx(0.0, abs=1e-14)
    assert values[0, 2, 0] == pytest.approx(-np.log(esd[2][0, 0]), abs=1e-14)
    assert not values[1].any()


def test_make_grid_holds_the_resident_length_and_both_sides():
    t = np.array([0.0, 0.3, 1.2, 0.05])
    for npoints in (1, 3, 8, 9, 64):
        grid, factors = make_grid(t, npoints, 5)
        assert grid.shape == (4, npoints) and not grid[0].any()
        assert len(factors) == npoints and factors.min() < 1.0
        assert npoints < 3 or (1.0 in factors and factors.max() > 1.0)
        assert np.array_equal(grid[1:], t[1:, None] * factors[None, :])


def test_entry_point_is_declared_bound_and_surfaced():
    from raoteh_amd import _lib, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    assert re.search(r'\bint rt_sites_branch_profiles\(', header)
    assert re.search(r'\bint rt_model_get_branch_lengths\(', header)
    assert re.search(r'#define RT_MAX_PROFILE_POINTS 64\b', header)
    assert 'NaN' in header                       # the zero-length caveat is documented
    assert _lib.RT_MAX_PROFILE_POINTS == 64
    restype, argtypes = _lib.SIGNATURES['rt_sites_branch_profiles']
    assert len(argtypes) == 8
    assert len(_lib.SIGNATURES['rt_model_get_branch_lengths'][1]) == 2
    assert getattr(_lib.lib(), 'rt_sites_branch_profiles') is not None
    assert getattr(_lib.lib(), 'rt_model_get_branch_lengths') is not None
    assert callable(device.TreeModel.branch_profiles)
    assert callable(device.check_profile_lengths)
    assert device.BranchProfiles._fields == ('nodes', 'lengths', 'sums', 'values', 'status')


def test_check_profile_lengths():
    from raoteh_amd import _lib, device
    from raoteh_amd._tree import TreeArrays
    check = device.check_profile_lengths
    N = 4
    resident = np.array([0.0, 0.5, 0.25, 2.0])
    # an absolute array: float64, C-contiguous, the root's row zeroed, the caller's untouched
    mine = np.arange(12, dtype=np.float32).reshape(3, 4).T + 1.0
    assert not mine.flags['C_CONTIGUOUS']
    got = check(mine, N)
    assert got.shape == (4, 3) and got.dtype == np.float64 and got.flags['C_CONTIGUOUS']
    assert not got[0].any() and np.array_equal(got[1:], mine[1:].astype(np.float64))
    assert mine[0, 0] == 1.0
    ints = check([[7], [1], [2], [3]], N)
    assert ints.dtype == np.float64 and ints[:, 0].tolist() == [0.0, 1.0, 2.0, 3.0]
    full = check(np.ones((N, _lib.RT_MAX_PROFILE_POINTS)), N)
    assert full.shape == (N, 64)
    # factors of the resident lengths
    got = check(None, N, factors=[1.0, 0.5, 2.0], resident=resident)
    assert got.shape == (4, 3) and got.dtype == np.float64 and got.flags['C_CONTIGUOUS']
    assert np.array_equal(got, resident[:, None] * np.array([1.0, 0.5, 2.0])[None, :])
    # a dict: by preorder index, or by a pair of tree nodes in either direction; edges left out
    # stay at the resident length
    T = nx.Graph()
    T.add_edge('r', 'x', weight=0.5)
    T.add_edge('x', 'y', weight=0.25)
    T.add_edge('r', 'z', weight=2.0)
    ta = TreeArrays(T, 'r')
    vx, vy, vz = (ta.node_to_index[k] for k in 'xyz')
    res = ta.branch_lengths()
    got = check({vx: [0.1, 0.2], ('y', 'x'): [0.3, 0.4]}, N, resident=res, tree=ta)
    assert got.shape == (4, 2) and got.flags['C_CONTIGUOUS'] and not got[0].any()
    assert got[vx].tolist() == [0.1, 0.2] and got[vy].tolist() == [0.3, 0.4]
    assert got[vz].tolist() == [2.0, 2.0]
    everything = check({vx: [1.0], vy: [2.0], ('r', 'z'): [3.0]}, N, tree=ta)
    assert everything[:, 0].tolist()[1:] == [{vx: 1.0, vy: 2.0, vz: 3.0}[v] for v in (1, 2, 3)]
    # refused: both or neither, shapes, counts, values
    bad_calls = [
        dict(lengths=None),                                          # neither
        dict(lengths=np.ones((N, 2)), factors=[1.0], resident=resident),      # both
        dict(lengths=None, factors=[1.0]),                           # no resident lengths
        dict(lengths=None, factors=[[1.0]], resident=resident),      # factors not 1-D
        dict(lengths=None, factors=[], resident=resident),           # G = 0
        dict(lengths=None, factors=np.ones(65), resident=resident),  # G = 65
        dict(lengths=None, factors=[-1.0], resident=resident),
        dict(lengths=np.ones((N, 0))),                               # G = 0
        dict(lengths=np.ones((N, 65))),                              # G = 65
        dict(lengths=np.ones((N + 1, 2))),
        dict(lengths=np.ones(N)),
        dict(lengths=np.ones((N, 2, 2))),
        dict(lengths='abc'),
        dict(lengths={vx: [0.1]}, tree=ta),                          # others unknown
        dict(lengths={vx: [0.1], vy: [0.1, 0.2]}, resident=res, tree=ta),
        dict(lengths={0: [0.1]}, resident=res, tree=ta),             # the root has no branch
        dict(lengths={('y', 'z'): [0.1]}, resident=res, tree=ta),    # not an edge
        dict(lengths={('x', 'y'): [0.1]}, resident=res),             # node pairs need the tree
        dict(lengths={}, resident=res, tree=ta),
    ]
    for v in (-1e-3, np.nan, np.inf, -np.inf):
        arr = np.ones((N, 3))
        arr[2, 1] = v
        bad_calls.append(dict(lengths=arr))
        bad_calls.append(dict(lengths={vy: [0.5, v]}, resident=res, tree=ta))
    for kw in bad_calls:
        lengths = kw.pop('lengths')
        with pytest.raises(ValueError):
            check(lengths, N, **kw)
    # a bad value in the root's row is ignored, as the C ABI ignores that row
    arr = np.ones((N, 2))
    arr[0] = [np.nan, -1.0]
    assert not check(arr, N)[0].any()
