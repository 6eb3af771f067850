"""Host side of rt_sites_branch_expectations: the host reference the GPU tests compare against
(tests/_branch_cases.py: oracle passes + scipy expm_frechet) reproduces the reference's own
record of examples/code2x3/run.py (tests/golden/branch_expectations.json); the C ABI entry
point, its binding and the Python surface exist; the argument check of the coefficients."""
import inspect
import re

import numpy as np
import pytest

from conftest import ROOT
from _branch_cases import load_golden, one_site_reference


def test_host_reference_reproduces_the_reference():
    fix, calls = load_golden()
    assert 'get_expected_ntransitions' in fix['provenance']
    # eight call sites of run.py's main(): the pure primary process at two data levels, the
    # switching and the blinking process at three each
    assert len(calls) == 23
    assert sorted(set(c['nstates'] for c in calls)) == [6, 48, 54]
    for c in calls:
        got = one_site_reference(c['T'], c['root'], c['nstates'], c['allowed'], c['root_distn'],
                                 c['Q'], c['E'])
        assert set(got) == set(c['expectations'])
        for edge, want in c['expectations'].items():
            assert got[edge] == pytest.approx(want, rel=1e-10, abs=1e-13), edge


def test_no_data_gives_the_branch_length_at_rate_one():
    """The pure primary process without data: expected rate 1, every expectation is the branch
    length (run.py's first call)."""
    _, calls = load_golden()
    c = calls[0]
    assert c['nstates'] == 6 and all(len(s) == 6 for s in c['allowed'].values())
    for (a, b), x in c['expectations'].items():
        assert x == pytest.approx(c['T'][a][b]['weight'], rel=1e-12)


def test_entry_point_is_declared_bound_and_surfaced():
    from raoteh_amd import _lib, _mjp_dense, device
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    assert re.search(r'\bint rt_sites_branch_expectations\(', header)
    assert re.search(r'#define RT_MAX_BRANCH_COEFS 8\b', header)
    assert _lib.RT_MAX_BRANCH_COEFS == 8
    restype, argtypes = _lib.SIGNATURES['rt_sites_branch_expectations']
    assert len(argtypes) == 8
    assert getattr(_lib.lib(), 'rt_sites_branch_expectations') is not None
    assert callable(device.TreeModel.branch_expectations)
    assert callable(device.TreeModel.branch_length_gradient)
    args = list(inspect.signature(_mjp_dense.get_expected_ntransitions).parameters)
    assert args == ['T', 'node_to_allowed_states', 'root', 'nstates', 'root_distn', 'Q_default',
                    'E']
    assert callable(_mjp_dense.get_expected_ntransitions_batch)


def test_check_branch_coefs():
    from raoteh_amd import _lib, device
    one = device.check_branch_coefs(np.eye(3), 3)
    assert one.shape == (1, 3, 3) and one.dtype == np.float64 and one.flags['C_CONTIGUOUS']
    many = device.check_branch_coefs([np.eye(3), -np.ones((3, 3))], 3)
    assert many.shape == (2, 3, 3) and many[1, 0, 1] == -1.0
    full = device.check_branch_coefs(np.zeros((_lib.RT_MAX_BRANCH_COEFS, 5, 5)), 5)
    assert full.shape == (8, 5, 5)
    nan = np.eye(3)
    nan[0, 1] = np.nan
    inf = np.eye(3)
    inf[2, 2] = np.inf
    for bad in (np.eye(4), np.zeros((3, 4)), np.zeros(9), np.zeros((2, 2, 3, 3)), [],
                np.zeros((_lib.RT_MAX_BRANCH_COEFS + 1, 3, 3)), nan, inf,
                [np.eye(3), np.eye(4)]):
        with pytest.raises(ValueError):
            device.check_branch_coefs(bad, 3)
