"""csrc/expm.hip, 33 <= n <= 64: the eight-wave Taylor kernel (two waves per SIMD, the left
operand of every product in registers) against the four-wave kernel it replaces, which
RAOTEH_EXPM_WAVES=4 selects.  Every accumulator tile sees the same seed and the same k-steps
in the same order, whichever wave holds it, so the results are the same bits: transition
matrices, order / squarings words, and -- through the A fragments the pruning kernels read --
the per-site log-likelihoods of one rt_step.  (Pquad exists for n <= 32 only: not reached.)"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ORDERS = [33, 47, 48, 49, 61, 64]
# ||Q t||_1 against theta = 1.39e-5, 9.07e-3, 8.96e-2, 0.300, 0.641: the five degrees, then one
# squaring per doubling of the norm beyond theta_15 (1.0, 2.0, 4.0: 1, 2, 3 squarings)
NORMS = [1e-6, 5e-3, 0.05, 0.2, 0.5, 1.0, 2.0, 4.0]


@pytest.fixture(scope='module')
def ra():
    from raoteh_amd import device, _lib, synth

    class NS(object):
        pass
    ns = NS()
    ns.device, ns.lib, ns.synth = device, _lib, synth
    ns.ctx = device.get_context()
    _lib.check(_lib.lib().rt_set_option(b'jit_async', 0))
    return ns


def rate_matrix(n, rng):
    """A random sparse rate matrix with ||Q||_1 = 1, so that t is the 1-norm of Q t."""
    Q = rng.exponential(size=(n, n)) * (rng.uniform(size=(n, n)) < 0.4)
    np.fill_diagonal(Q, 0.0)
    Q -= np.diag(Q.sum(axis=1))
    return Q / np.abs(Q).sum(axis=0).max()


def raw_expm(ra, Q, t, qidx):
    """rt_expm as Context.expm calls it, without raising: (return code, P, info).  The call
    fills P and info before it reports a non-finite matrix (RT_ERR_SINGULAR)."""
    from ctypes import c_double, c_int32, c_int64
    from raoteh_amd.device import _f64, _i64, _ptr
    Q, t, qi = _f64(Q), _f64(t), _i64(qidx)
    n, count = Q.shape[1], t.shape[0]
    P = np.empty((count, n, n), dtype=np.float64)
    info = np.zeros((count, 2), dtype=np.int32)
    rc = ra.lib.lib().rt_expm(ra.ctx._h, n, count, _ptr(Q, c_double), Q.shape[0],
                              _ptr(qi, c_int64), _ptr(t, c_double), _ptr(P, c_double),
                              _ptr(info, c_int32))
    return rc, P, info


def check_orders_and_squarings(info):
    assert set(info[:, 0]) >= {3, 6, 9, 12, 15}, sorted(set(info[:, 0]))
    assert set(info[:, 1]) >= {0, 1, 2, 3}, sorted(set(info[:, 1]))


@pytest.mark.parametrize('count', [8, 200])
@pytest.mark.parametrize('n', ORDERS)
def test_transition_matrices_and_info_are_the_same_bits(ra, n, count, monkeypatch):
    """rt_expm: few matrices (n >= 49: two workgroups per matrix) and more than half as many as
    the device has compute units (one workgroup each); two rate matrices, so that both the
    speculative fetch of matrix 0 and the second fetch run, and a third one with an infinite
    entry (info -1, P all NaN; rt_expm fills its outputs and then reports that matrix)."""
    rng = np.random.RandomState(1000 + n)
    Q = np.stack([rate_matrix(n, rng), rate_matrix(n, rng), rate_matrix(n, rng)])
    Q[2, 3, 5] = np.inf
    t = np.tile(NORMS, (count + len(NORMS) - 1) // len(NORMS))[:count]
    qidx = np.arange(count) % 2
    qidx[count // 2] = 2
    pair = n >= 49 and count == 8
    out = {}
    for waves in ('4', '8'):
        monkeypatch.setenv('RAOTEH_EXPM_WAVES', waves)
        rc, P, info = raw_expm(ra, Q, t, qidx)
        assert rc == ra.lib.RT_ERR_SINGULAR, rc
        out[waves] = (P, info)
        ra.ctx.set_timing(True)
        ra.ctx.expm(Q[:2], t, q_index=np.arange(count) % 2)
        name = ra.ctx.kernel_time(0)[2]
        ra.ctx.set_timing(False)
        assert name == ('expm_taylor_ps_mfma_split2' if pair else 'expm_taylor_ps_mfma'), name
    (P4, info4), (P8, info8) = out['4'], out['8']
    bad = count // 2
    assert tuple(info4[bad]) == (-1, 0) and np.isnan(P4[bad]).all()
    check_orders_and_squarings(np.delete(info4, bad, axis=0))
    np.testing.assert_array_equal(info8, info4)
    np.testing.assert_array_equal(P8, P4)
    good = np.delete(P4, bad, axis=0)
    assert np.abs(good.sum(axis=2) - 1).max() < 1e-12


@pytest.mark.parametrize('split', ['0', '1'])
@pytest.mark.parametrize('n', ORDERS)
def test_tree_step_log_likelihoods_are_the_same_bits(ra, n, split, monkeypatch):
    """rt_model_set_rates and rt_step on a 31-node tree (the root's slot is all zeros), one and
    two workgroups per matrix: transitions, info words and the per-site log-likelihoods, which
    the pruning kernel computes from the A fragments the expm epilogue writes."""
    rng = np.random.RandomState(2000 + n)
    T, root, leaves = ra.synth.balanced_tree(16)
    Q = rate_matrix(n, rng)
    for k, (a, b) in enumerate(T.edges()):
        T[a][b]['weight'] = NORMS[k % len(NORMS)]
    dense = rng.uniform(0.1, 1.0, size=(40, len(leaves), n))
    monkeypatch.setenv('RAOTEH_EXPM_SPLIT', split)
    out = {}
    for waves in ('4', '8'):
        monkeypatch.setenv('RAOTEH_EXPM_WAVES', waves)
        model = ra.device.TreeModel(T, root, n)
        model.set_rates(Q_default=Q)
        batch = model.upload_sites(leaves, dense, kind='dense')
        ll, st = model.log_likelihoods(batch)
        model.step(batch)
        ll2, st2 = model.fetch_log_likelihoods(batch)
        out[waves] = (model.get_transitions(), model.expm_info(), ll, st, ll2, st2)
    a, b = out['4'], out['8']
    assert (a[0][0] == 0).all() and tuple(a[1][0]) == (0, 0)          # the root slot
    check_orders_and_squarings(a[1][1:])
    assert np.isfinite(a[2]).all()
    for x, y in zip(a, b):
        np.testing.assert_array_equal(y, x)
    np.testing.assert_array_equal(b[4], b[2])
