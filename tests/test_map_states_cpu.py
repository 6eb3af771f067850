"""Host side of rt_sites_map_states: the numpy recursion of tests/_map_cases.py against the
enumeration of every assignment; the conditions the GPU tests rely on (the exact cases hold ties
and no dead site, the long tree underflows f64 without the scale); the entry point, its binding
and the Python surface exist."""
import os
import re

import numpy as np
import pytest

from conftest import ROOT
import _map_cases as mc
import _sample_cases as sc


@pytest.mark.parametrize('n', [3, 5])
def test_the_reference_equals_the_enumeration(n):
    T, root, leaves, Q, rd, lik = mc.small_case(n, seed=30 + n)
    pre, idx, ptr, esd, parent = sc.tree_arrays(T, root, n, Q)
    assert len(pre) == 7 and len(lik) == 20
    ta = mc.TreeArrays(T, root)
    assert ta.preorder_nodes == list(pre)
    obs = mc.full_observations(ta, leaves, lik, n)
    want, wstates, unique = mc.brute_force(esd, obs, rd, parent)
    assert np.isfinite(want).all() and unique.sum() >= 15
    for scale in (True, False):
        states, lj, _ = mc.map_reference(esd, obs, rd, parent, scale=scale)
        assert np.abs(lj - want).max() <= 1e-13
        assert np.array_equal(states[unique], wstates[unique])
        # what the reference returns is the probability of what it returns
        assert np.abs(mc.joint_log(esd, obs, rd, parent, states) - lj).max() <= 1e-13


def test_a_dead_site_and_a_tie():
    """Two leaves under a root, two states: a site that no assignment explains, and a site where
    both root states tie (the lower one wins, at the root and below it)."""
    P = np.zeros((3, 2, 2))
    P[1] = P[2] = [[0.5, 0.5], [0.5, 0.5]]
    parent = np.array([-1, 0, 0])
    obs = np.ones((2, 3, 2))
    obs[0, 1] = 0.0
    states, lj, tied = mc.map_reference(P, obs, None, parent)
    assert states.tolist() == [[255] * 3, [0, 0, 0]]
    assert lj[0] == -np.inf and abs(lj[1] - np.log(0.25)) < 1e-15
    assert tied.tolist() == [0, 3]
    assert mc.joint_log(P, obs, None, parent, states)[0] == -np.inf


@pytest.mark.parametrize('n', mc.EXACT_N)
def test_the_exact_cases_hold_ties_and_no_dead_site(n):
    c = mc.dyadic_case(n)
    assert c.ta.nnodes == 14 and c.dense.shape == (mc.EXACT_SITES, len(c.leaves), n)
    # every number is a power of two (or zero)
    for arr in (c.P[1:], c.w, c.dense):
        m, _ = np.frexp(arr)
        assert set(np.unique(m).tolist()) <= {0.0, 0.5}
    assert (c.P[1:] == 0).any() == (n > 4)
    states, lj, tied = mc.map_reference(c.P, c.obs, c.w, c.parent)
    assert np.isfinite(lj).all() and (states < n).all()
    assert (tied > 0).sum() >= 5
    # exact: the unscaled recursion gives the same states and the same probability
    s2, lj2, t2 = mc.map_reference(c.P, c.obs, c.w, c.parent, scale=False)
    assert np.array_equal(states, s2) and np.array_equal(tied, t2)
    assert np.abs(lj - lj2).max() <= 4 * 2.0 ** -52 * np.abs(lj).max()
    assert np.abs(mc.joint_log(c.P, c.obs, c.w, c.parent, states) - lj).max() <= 1e-12 * np.abs(lj).max()


@pytest.mark.parametrize('n', [4, 7])
def test_the_long_tree_underflows_without_the_scale(n):
    T, root, tips, Q, rd, data, lik = mc.long_case(n)
    pre, idx, ptr, esd, parent = sc.tree_arrays(T, root, n, Q)
    assert len(pre) == 1500 and len(tips) == 4 and data.shape == (17, 4)
    ta = mc.TreeArrays(T, root)
    obs = mc.full_observations(ta, tips, lik, n)
    _, unscaled, _ = mc.map_reference(esd, obs, rd, parent, scale=False)
    assert (unscaled == -np.inf).all()
    states, lj, _ = mc.map_reference(esd, obs, rd, parent)
    assert np.isfinite(lj).all() and (lj < -745.0).all()           # log of the smallest f64: -744.4
    jl = mc.joint_log(esd, obs, rd, parent, states)
    assert (np.abs(jl - lj) <= mc.tolerance(1500, lj)).all()


def test_the_entry_point_is_declared_and_bound():
    from raoteh_amd import _lib, device
    header = open(os.path.join(ROOT, 'include', 'raoteh_hip.h')).read()
    assert re.search(r'\bint\s+rt_sites_map_states\s*\(', header)
    restype, argtypes = _lib.SIGNATURES['rt_sites_map_states']
    assert len(argtypes) == 6
    assert device.MapStates._fields == ('states', 'log_joint', 'status', 'nodes')
    assert 'exp(log_joint' in device.TreeModel.map_states.__doc__
    src = open(os.path.join(ROOT, 'raoteh_amd', 'csrc', 'Makefile')).read()
    assert 'map_states.hip' in src
