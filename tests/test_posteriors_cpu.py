"""Host side of rt_sites_posteriors: the oracle restated over state sets reproduces the
reference's record of the switching model (tests/golden/switching_posteriors.json), which pins
the oracle the GPU tests compare against; the set-to-mask helper; the C ABI entry point."""
import re

import numpy as np
import pytest

from conftest import GOLDEN, ROOT, load_golden, switching_cases
from oracle import oracle_numpy as orc
from _posterior_cases import oracle_pmaps, oracle_site, sums_over_sets


def test_oracle_over_sets_reproduces_the_reference():
    fx, cases = switching_cases()
    ref = load_golden('switching_posteriors')
    n1, n2 = fx['nstates'], fx['ncompound']
    assert (ref['nstates'], ref['ncompound']) == (n1, n2)
    lo, hi = list(range(n1)), list(range(n1, n2))
    zeros = 0
    for c, want in zip(cases, ref['sites']):
        pre, idx, ptr, esd = orc.get_expm_augmented_transitions(c['T'], c['root'], n2,
                                                                Q_default=c['Q_compound'])
        obs = [v for v in pre if len(c['allowed'][v]) < n2]
        lik = np.zeros((1, len(obs), n2))
        for k, v in enumerate(obs):
            lik[0, k, sorted(c['allowed'][v])] = 1.0
        L = oracle_pmaps(idx, ptr, esd, [pre.index(v) for v in obs], lik)
        got = oracle_site(idx, ptr, esd, c['compound_distn'], L[0])
        if want['structural_zero']:
            assert got is None
            zeros += 1
            continue
        D, J = got
        nv, ev = sums_over_sets(D, J, [lo], [(lo, hi), (hi, lo)])
        for v, p in want['p_primary'].items():
            assert nv[pre.index(int(v)), 0] == pytest.approx(p, rel=1e-10, abs=1e-13)
        for v, p in want['switch'].items():
            assert ev[pre.index(int(v)), 0] == pytest.approx(p, rel=1e-10, abs=1e-13)
        for v, p in want['switch_back'].items():
            assert ev[pre.index(int(v)), 1] == pytest.approx(p, rel=1e-10, abs=1e-13)
        np.testing.assert_allclose(D[pre.index(ref['original_root'])], want['original_root_distn'],
                                   rtol=1e-10, atol=1e-13)
        np.testing.assert_allclose(D[pre.index(ref['leaf_node'])], want['leaf_distn'],
                                   rtol=1e-10, atol=1e-13)
    assert zeros == 1


def test_states_to_mask():
    from raoteh_amd import device
    m = device.states_to_mask([0, 5, 63, 64, 127], 128)
    assert m.dtype == np.uint64 and m.shape == (2,)
    assert int(m[0]) == (1 << 0) | (1 << 5) | (1 << 63)
    assert int(m[1]) == (1 << 0) | (1 << 63)
    assert device.states_to_mask([], 4).tolist() == [0, 0]
    assert device.states_to_mask(np.array([1, 2]), 4).tolist() == [6, 0]
    for bad in ([4], [-1], [1.5]):
        with pytest.raises(ValueError):
            device.states_to_mask(bad, 4)


def test_rt_sites_posteriors_is_declared_and_exported():
    from raoteh_amd import _lib
    with open(f'{ROOT}/include/raoteh_hip.h') as f:
        header = f.read()
    assert re.search(r'\bint rt_sites_posteriors\(', header)
    assert re.search(r'#define RT_MAX_POSTERIOR_SETS 8\b', header)
    assert _lib.RT_MAX_POSTERIOR_SETS == 8
    assert 'rt_sites_posteriors' in _lib.SIGNATURES
    assert getattr(_lib.lib(), 'rt_sites_posteriors') is not None
