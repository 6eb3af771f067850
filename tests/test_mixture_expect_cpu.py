"""Host side of rt_sites_branch_expectations_mixture: the entry point, its binding and the Python
surface exist and agree; rate_parameter_coefs; and the host reference the GPU tests compare
against (tests/_mixture_cases.py) -- posteriors that sum to one, equal to
_branch_cases.branch_reference when all classes are the same, the identity coefficient's closed
form, and its analytic gradients next to central differences of the oracle's mixture total."""
import re

import numpy as np
import pytest

from conftest import ROOT
import _mixture_cases as mc
import _partition_read_cases as prc
from _branch_cases import branch_reference, make_coefs

GRADIENT_H = 1e-5            # the step of test_partition_reads_cpu.py's gradient_gap


def test_entry_point_is_declared_bound_and_surfaced():
    from raoteh_amd import _lib, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    m = re.search(r'\bint rt_sites_branch_expectations_mixture\(([^;]*)\);', header)
    assert m, 'the header does not declare the entry point'
    params = [' '.join(a.split()) for a in m.group(1).split(',')]
    kinds = []
    for a in params:
        if '*' not in a:
            kinds.append(a.rsplit(' ', 1)[0])
        else:
            kinds.append(a[:a.rindex('*') + 1].replace('const ', '').replace(' ', ''))
    assert kinds == ['rt_model*', 'rt_sites*', 'int', 'double*', 'int64_t', 'int', 'double*',
                     'double*', 'double*', 'double*', 'double*', 'double*', 'double*', 'int32_t*']
    restype, argtypes = _lib.SIGNATURES['rt_sites_branch_expectations_mixture']
    import ctypes
    p_f64, p_i32 = ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_int32)
    assert restype is ctypes.c_int
    assert list(argtypes) == [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int, p_f64, ctypes.c_int64,
                              ctypes.c_int, p_f64, p_f64, p_f64, p_f64, p_f64, p_f64, p_f64, p_i32]
    assert getattr(_lib.lib(), 'rt_sites_branch_expectations_mixture') is not None
    for name in ('branch_expectations_mixture', 'class_posteriors', 'branch_length_gradient_mixture'):
        assert callable(getattr(device.TreeModel, name))
    assert device.MixtureBranchExpectations._fields == (
        'values', 'edge_sums', 'set_edge_sums', 'class_posteriors', 'class_sums',
        'log_likelihoods', 'status')
    assert '2d. site-class mixtures' in header
    refusals = header[header.index('Everything else refuses a partitioned batch'):]
    assert 'rt_sites_branch_expectations_mixture,' in refusals[:600]


def test_rate_parameter_coefs():
    from raoteh_amd import device
    Q = np.array([[-3.0, 1.0, 2.0], [0.5, -0.5, 0.0], [4.0, 1.0, -5.0]])
    dQ = np.array([[-1.0, 1.0, 0.0], [0.25, -0.25, 0.0], [0.0, -2.0, 2.0]])
    E = device.rate_parameter_coefs(Q, dQ)
    np.testing.assert_array_equal(
        E, [[-1.0, 1.0, 0.0], [0.5, -0.25, 0.0], [0.0, -2.0, 2.0]])
    # the direction the device forms from E is dQ itself
    C = E * Q
    np.fill_diagonal(C, np.diag(E))
    np.testing.assert_array_equal(C, dQ)
    bad = dQ.copy()
    bad[1, 2] = 0.1                      # Q[1, 2] == 0: a structural mismatch
    with pytest.raises(ValueError, match='zero'):
        device.rate_parameter_coefs(Q, bad)
    for wrong in ((Q, dQ[:2]), (Q[0], dQ[0]), (np.zeros((2, 3)), np.zeros((2, 3)))):
        with pytest.raises(ValueError):
            device.rate_parameter_coefs(*wrong)


@pytest.mark.parametrize('n,tree,kind', [(4, 'balanced', 'state'), (5, 'random', 'dense')])
def test_reference_posteriors_and_skipped_sets(n, tree, kind):
    """K = 3 with the zero set (P = I) and per-edge Q: the posteriors sum to one on the live
    sites; a site whose leaves disagree has posterior exactly 0 for the zero set; a class of
    weight 0 has a column of zeros and changes nothing else."""
    case = mc.make_case(n, tree, kind, 3, seed=8400 + n, nsites=30)
    ta = mc.tree_arrays(case)
    coefs = make_coefs(n, 2, 8400 + n)
    c = np.array([0.5, 0.2, 0.3])
    ref = mc.mixture_reference(ta, case, coefs, c)
    assert not ref.status.any()
    np.testing.assert_allclose(ref.post.sum(axis=1), 1.0, rtol=1e-14)
    dead_in_zero_set = ~(ref.L[2] > 0)
    assert dead_in_zero_set.sum() >= (5 if kind == 'state' else 1) and (~dead_in_zero_set).sum() >= 3
    assert not ref.post[dead_in_zero_set, 2].any() and ref.post[~dead_in_zero_set, 2].all()
    np.testing.assert_allclose(ref.class_sums.sum(), 30.0, rtol=1e-13)
    np.testing.assert_allclose(ref.edge_sums, ref.values.sum(axis=0), rtol=1e-12, atol=1e-14)
    off = mc.mixture_reference(ta, case, coefs, np.array([0.5, 0.0, 0.3]), check=0)
    assert not off.post[:, 1].any() and not off.set_edge_sums[1].any() and off.class_sums[1] == 0
    two = case._replace(Q=case.Q[[0, 2]], t=case.t[[0, 2]])
    want = mc.mixture_reference(ta, two, coefs, np.array([0.5, 0.3]), check=0)
    np.testing.assert_array_equal(off.values, want.values)
    np.testing.assert_array_equal(off.loglik, want.loglik)
    np.testing.assert_array_equal(off.post[:, [0, 2]], want.post)


def test_reference_dead_site():
    case = mc.make_case(4, 'balanced', 'dense', 2, seed=8450, nsites=12, dead_site=3)
    ta = mc.tree_arrays(case)
    ref = mc.mixture_reference(ta, case, make_coefs(4, 1, 8450), np.array([0.4, 0.6]))
    assert ref.status[3] == 1 and ref.status.sum() == 1
    assert ref.loglik[3] == -np.inf and not ref.post[3].any() and not ref.values[3].any()
    assert np.isfinite(np.delete(ref.loglik, 3)).all() and np.isfinite(ref.values).all()


@pytest.mark.parametrize('n,kind', [(4, 'state'), (5, 'dense')])
def test_equal_sets_are_the_ordinary_reference(n, kind):
    """K equal sets: whatever the class weights, the mixture is that one set."""
    case = mc.make_case(n, 'balanced', kind, 1, seed=8500 + n, nsites=21)
    ta = mc.tree_arrays(case)
    three = case._replace(Q=np.repeat(case.Q, 3, axis=0), t=np.repeat(case.t, 3, axis=0))
    coefs = make_coefs(n, 3, 8500 + n)
    model, sub = prc.set_case(ta, case, 0, np.arange(21))
    want, wstatus = branch_reference(model, sub, coefs, check_sites=[0, 20])
    c = np.array([0.2, 0.5, 0.3])
    ref = mc.mixture_reference(ta, three, coefs, c)
    np.testing.assert_array_equal(ref.status, wstatus)
    np.testing.assert_allclose(ref.values, want, rtol=1e-14, atol=1e-16 * np.abs(want).max())
    np.testing.assert_allclose(ref.post, np.broadcast_to(c, (21, 3)), rtol=1e-14)
    np.testing.assert_allclose(ref.loglik, np.log(ref.L[0]), rtol=1e-14)


def test_identity_coefficient_gives_the_posterior_mean_branch_length():
    """E = I: the direction is the identity, the statistic is the time spent anywhere on the
    branch, t[k][v] under set k -- so values[i][v] = sum_k post[i][k] t[k][v]."""
    n = 4
    case = mc.make_case(n, 'random', 'mask', 3, seed=8600, zero_set=False, nsites=25)
    ta = mc.tree_arrays(case)
    c = np.array([0.1, 0.6, 0.3])
    ref = mc.mixture_reference(ta, case, np.eye(n), c)
    np.testing.assert_allclose(ref.values[:, :, 0], ref.post @ case.t, rtol=1e-11)
    assert ref.post.min() > 0 and ref.post.max() < 1


@pytest.mark.parametrize('n', [4, 5])
def test_reference_gradients_against_the_oracles_central_difference(n):
    """g_t[k][v], g_c[k] and one kappa-style rate parameter (rate_parameter_coefs) from the host
    reference next to central differences of the oracle's mixture total, step and tolerance of
    test_partition_reads_cpu.py's gradient test: h = 1e-5, gap <= 1e-5 max |analytic|.  A wrong
    posterior, table or factor would be of order one."""
    case = mc.gradient_case(n, 8700 + n, nsites=40)
    ta = mc.tree_arrays(case)
    c = np.array([0.5, 0.3, 0.2])
    gaps = mc.gradient_gaps(ta, case, c, GRADIENT_H)
    for name, (analytic, gap) in sorted(gaps.items()):
        print('n=%d d/d%s: oracle central difference vs host analytic: max gap %.2e (max |g| %.2e)'
              % (n, name, gap, np.abs(analytic).max()))
        assert np.abs(analytic).max() > 0
        assert gap <= 1e-5 * np.abs(analytic).max()
    assert not gaps['t'][0][:, 0].any()
