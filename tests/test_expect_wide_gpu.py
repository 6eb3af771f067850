"""Expected history statistics on a resident batch for 65 to 128 states (rt_expect_step above
RT_MAX_EXPECT_STATES): the pair-recurrence Frechet kernel (csrc/frechet_wide.hip), the site
sums with a row tile per wave and the downward pass / root sums for five to eight row tiles.
Every check compares with a host reference that no device path enters: scipy expm of the
order-2n block (tests/_resident_cases.py), the oracle, and the reference's own numbers
(tests/golden/expectations_wide.json)."""
import numpy as np
import pytest
import scipy.linalg

from _expect_wide_cases import wide_cases
from _resident_cases import expectation_reference, make_case, rate_matrix, set_rates

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}


@pytest.fixture(scope='module')
def ra():
    from raoteh_amd import device, _lib

    class NS(object):
        pass
    ns = NS()
    ns.device, ns.lib = device, _lib
    return ns


def open_context(ra, opts):
    ctx = ra.device.Context(0)
    for k, v in dict(DEFAULTS, **opts).items():
        ctx.set_option(k, v)
    return ctx


def build(ra, ctx, case, weights=None):
    model = ra.device.TreeModel(case.T, case.root, case.n, ctx=ctx)
    set_rates(model, case)
    model.set_root_distn(case.root_distn)
    batch = model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
    if weights is not None:
        batch.set_weights(weights)
    return model, batch


def weighted_reference(model, case, weights, Qs=None):
    """expectation_reference takes every site once: with weights, the sites are repeated
    (integer multiplicities), which is what a weight means."""
    if weights is None:
        return expectation_reference(model, case, Qs=Qs, check_sites=[0, len(case.obs_lik) // 2])
    rep = np.repeat(np.arange(len(weights)), weights.astype(int))
    return expectation_reference(model, case._replace(obs_lik=case.obs_lik[rep]), Qs=Qs,
                                 check_sites=[0])


def check_step(model, batch, case, weights=None, Qs=None, recompute=True):
    """check_expectations of test_resident_reads_gpu.py (its tolerances), with weights."""
    dwell, rootp, trans, status = model.expected_history_statistics(
        batch, recompute_transitions=recompute, return_status=True)
    want = weighted_reference(model, case, weights, Qs=Qs)
    bad = np.zeros(batch.nsites, dtype=np.int32)
    if case.zero_site is not None:
        bad[case.zero_site] = 2                    # a zero denominator (likelihood 0)
    np.testing.assert_array_equal(status, bad)
    scale = np.abs(want[0]).max()
    print('n=%d %s: max |dwell - ref| / scale %.2e, max |trans - ref| / scale %.2e'
          % (case.n, case.kind, np.abs(dwell - want[0]).max() / scale,
             np.abs(trans - want[2]).max() / scale))
    np.testing.assert_allclose(dwell, want[0], rtol=1e-9, atol=1e-13 * scale)
    np.testing.assert_allclose(rootp, want[1], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(trans, want[2], rtol=1e-9, atol=1e-13 * scale)
    # the invariants the n <= 64 test asserts
    wsum = float(batch.nsites if weights is None else weights.sum())
    live = wsum - (0.0 if case.zero_site is None else
                   (1.0 if weights is None else float(weights[case.zero_site])))
    total = float(np.sum(model.tree.branch_lengths()[1:]))
    assert dwell.sum() == pytest.approx(total * live, rel=1e-10)
    assert rootp.sum() == pytest.approx(live, rel=1e-11)
    return dwell, rootp, trans, status


# one per number of row tiles 5 .. 8 plus both ends; every observation kind, the interpreter
# and the tree-specialised pruning kernel, weights, site counts that are no multiple of 16
STEP_CASES = [
    # n, kind, sites, tree nodes, jit, weights
    (65, 'state', 17, 9, 0, False),
    (80, 'dense', 37, 11, 1, True),
    (97, 'mask', 50, 10, 0, True),
    (112, 'state', 33, 12, 1, False),
    (122, 'mask', 45, 9, 1, False),
    (128, 'dense', 19, 8, 0, True),
]


@pytest.mark.parametrize('n,kind,nsites,nnodes,jit,weighted', STEP_CASES,
                         ids=['n%d-%s-jit%d' % (c[0], c[1], c[4]) for c in STEP_CASES])
def test_step_against_the_host_reference(ra, n, kind, nsites, nnodes, jit, weighted):
    seed = 5000 + n
    case = make_case(n, nnodes, nsites, kind, seed, internal=True, per_edge=True)
    weights = None
    if weighted:
        weights = np.random.RandomState(seed).randint(1, 4, size=nsites).astype(np.float64)
    ctx = open_context(ra, {'jit': jit})
    try:
        model, batch = build(ra, ctx, case, weights)
        check_step(model, batch, case, weights)
    finally:
        ctx.close()


def test_unweighted_sums_are_the_site_and_tree_totals(ra):
    """dwell.sum() == total branch length x sites, rootp.sum() == sites (no zero site here)."""
    case = make_case(122, 9, 21, 'mask', 77, internal=False, per_edge=True)
    assert case.zero_site is None
    ctx = open_context(ra, {'jit': 0})
    try:
        model, batch = build(ra, ctx, case)
        dwell, rootp, trans, status = check_step(model, batch, case)
        assert not status.any()
    finally:
        ctx.close()


def _table(case):
    n = case['n']
    dwell = case['dwell']
    return n, np.abs(dwell).max()


@pytest.mark.parametrize('k', [0, 1])
def test_reference_numbers_through_the_python_surface(ra, k):
    """expectations_wide.json through get_expected_history_statistics and its batch form (site
    dicts: the two-word mask route), at test_gpu_parity.py's tolerances for expectations.json."""
    from raoteh_amd import _mjp_dense
    case = wide_cases()[k]
    n, scale = _table(case)
    T, root = case['T'], case['root']
    dwell, init, trans = _mjp_dense.get_expected_history_statistics(
        T, case['allowed'], root, n, root_distn=case['root_distn'], Q_default=case['Q_default'])
    got_dwell = np.array([dwell[c] for c in range(n)])
    got_trans = np.zeros((n, n))
    for c, d, dat in trans.edges(data=True):
        got_trans[c, d] = dat['weight']
    off = case['live'] & ~np.eye(n, dtype=bool)
    print('%s: max |dwell - ref| / scale %.2e, max |trans - ref| / scale %.2e' % (
        case['name'], np.abs(got_dwell - case['dwell']).max() / scale,
        np.abs(got_trans - case['trans'])[off].max() / scale))
    np.testing.assert_allclose(got_dwell, case['dwell'], rtol=1e-10, atol=1e-13 * scale)
    np.testing.assert_allclose(init, case['init'], rtol=1e-12, atol=1e-15)
    np.testing.assert_allclose(got_trans[off], case['trans'][off], rtol=1e-10, atol=1e-13 * scale)
    # every nonzero rate has its edge in the graph, as in the reference
    assert set((c, d) for c, d in trans.edges()) >= set(zip(*np.nonzero(off)))
    # the batch form: the site twice with weights 1 and 2 = three times the numbers
    bd, br, bt = _mjp_dense.get_expected_history_statistics_batch(
        T, root, n, sites=[case['allowed'], case['allowed']], root_distn=case['root_distn'],
        Q_default=case['Q_default'], weights=[1.0, 2.0])
    np.testing.assert_allclose(bd, 3 * case['dwell'], rtol=1e-10, atol=3e-13 * scale)
    np.testing.assert_allclose(br, 3 * case['init'], rtol=1e-12, atol=3e-15)
    np.testing.assert_allclose(bt[off], 3 * case['trans'][off], rtol=1e-10, atol=3e-13 * scale)


def test_python_surface_flags_a_zero_site(ra):
    from raoteh_amd import _mjp_dense, _util
    case = wide_cases()[0]
    n = case['n']
    Q = case['Q_default']
    allowed = dict(case['allowed'])
    # a root prior on one state that cannot reach the leaves' states in zero time: every
    # branch length 0 makes P the identity
    T = case['T'].copy()
    for a, b in T.edges():
        T[a][b]['weight'] = 0.0
        T[a][b].pop('Q', None)
    leaves = [v for v in T if T.degree(v) == 1]
    allowed[leaves[0]] = {0}
    allowed[leaves[1]] = {1}
    with pytest.raises(_util.NumericalZeroProb):
        _mjp_dense.get_expected_history_statistics_batch(T, case['root'], n, sites=[allowed],
                                                         root_distn=case['root_distn'], Q_default=Q)


# ---- the Frechet entry alone ---------------------------------------------------------------

def frechet_inputs(n, seed):
    """Five edges, two rate matrices (edges 1 and 3 carry the second), branch lengths from no
    squaring (|tQ| <= 0.64) to six, W >= 0 with entries over sixteen orders of magnitude,
    one edge with W = 0."""
    rng = np.random.RandomState(seed)
    Qs = np.stack([rate_matrix(n, rng), rate_matrix(n, rng)])
    qi = np.array([0, 1, 0, 1, 0])
    big = max(np.abs(np.diag(Q)).max() for Q in Qs)
    t = np.array([0.25, 1.0, 4.0, 10.0, 20.0]) / big       # |tQ|_1 = 2 t max|q_ii| = 0.5 .. 40
    W = rng.uniform(0.0, 1.0, (5, n, n)) * 10.0 ** rng.randint(-8, 9, (5, n, n))
    W[2] = 0.0
    return Qs, qi, t, W


def frechet_host(Qs, qi, t, W):
    n = Qs.shape[1]
    dwell, trans = np.zeros(n), np.zeros((n, n))
    for e in range(len(t)):
        Q = Qs[qi[e]]
        B = np.zeros((2 * n, 2 * n))
        B[:n, :n] = B[n:, n:] = t[e] * Q.T
        B[:n, n:] = W[e]
        M = scipy.linalg.expm(B)[:n, n:]
        dwell += t[e] * np.diag(M)
        trans += np.where(Q != 0, t[e] * Q * M, 0.0)
    return dwell, trans


def gap(got, want):
    """The smallest rtol at which (got, want) pass with atol = 1e-13 x the largest entry."""
    worst = 0.0
    for g, w in zip(got, want):
        atol = 1e-13 * np.abs(w).max()
        excess = np.abs(g - w) - atol
        nz = w != 0
        assert np.all(excess[~nz] <= 0)
        worst = max(worst, float(np.max(excess[nz] / np.abs(w[nz]), initial=0.0)))
    return worst


def test_frechet_entry_alone(ra):
    """ctx.frechet_statistics above 64 states against scipy expm of the order-2n block: rtol
    1e-10, atol 1e-13 x the largest entry.  The yardstick on the long branches is today's
    order-2n block route: the same draw at n = 64 goes through it here, and where that route
    itself is further than 1e-10 from scipy the pair kernel gets ten times its gap (another
    summation order over twice the dimension).  Both figures are printed.  Measured on the
    MI355X: the block route at n = 64 is 1.3e-12 from scipy, so the bound is 1e-10; the pair
    kernel 3.2e-13 (n = 65), 1.9e-13 (96), 4.6e-14 (122), 1.8e-12 (128), squarings 0, 2, 4, 5, 6."""
    from raoteh_amd.device import get_context
    ctx = get_context()
    from oracle import oracle_numpy as orc
    base = frechet_inputs(64, 640)
    gap64 = gap(ctx.frechet_statistics(*base), frechet_host(*base))
    bound = 1e-10 if gap64 <= 1e-10 else 10.0 * gap64
    print('order-2n block route at n = 64: gap %.3e -> bound %.3e' % (gap64, bound))
    for n in (65, 96, 122, 128):
        Qs, qi, t, W = frechet_inputs(n, 10 * n)
        sq = [orc.device_expm_order_and_squarings(n, 2 * tt * np.abs(np.diag(Qs[k])).max())[1]
              for tt, k in zip(t, qi)]
        assert sq[0] == 0 and max(sq) >= 3, sq
        got = ctx.frechet_statistics(Qs, qi, t, W)
        g = gap(got, frechet_host(Qs, qi, t, W))
        print('pair kernel at n = %d: squarings %s, gap %.3e' % (n, sq, g))
        assert g <= bound, (n, g, bound)
        # shared Q and an all-zero W
        d0, t0 = ctx.frechet_statistics(Qs[0], np.zeros(5, dtype=np.int64), t, np.zeros_like(W))
        assert not d0.any() and not t0.any()
        one = ctx.frechet_statistics(Qs[0], np.zeros(2, dtype=np.int64), t[:2], W[:2])
        assert gap(one, frechet_host(Qs[:1], np.zeros(2, dtype=int), t[:2], W[:2])) <= bound


# ---- unchanged behaviour -------------------------------------------------------------------

def test_the_step_leaves_the_batch_alone_and_repeats_its_bits(ra):
    case = make_case(122, 10, 40, 'mask', 1220, internal=True, per_edge=True)
    ctx = open_context(ra, {'jit': 1})
    try:
        model, batch = build(ra, ctx, case)
        model.prune(batch)
        ll, st = model.fetch_log_likelihoods(batch)
        tot, name = model.fetch_totals(batch), batch.kernel_name
        a = check_step(model, batch, case)
        b = model.expected_history_statistics(batch, return_status=True)
        for x, y in zip(a, b):
            np.testing.assert_array_equal(x, y)            # fixed-order sums
        ll2, st2 = model.fetch_log_likelihoods(batch)
        np.testing.assert_array_equal(ll, ll2)
        np.testing.assert_array_equal(st, st2)
        np.testing.assert_array_equal(tot, model.fetch_totals(batch))
        assert batch.kernel_name == name
        # new rates on the same batch, the transitions not recomputed by the step
        rng = np.random.RandomState(3)
        Q1 = np.stack([rate_matrix(case.n, rng) for _ in range(len(case.Qs))])
        set_rates(model, case, Q1)
        model.step(batch)
        check_step(model, batch, case, Qs=Q1, recompute=False)
    finally:
        ctx.close()


@pytest.mark.parametrize('opt', ['rescale', 'force_generic'])
def test_refusals_stay(ra, opt):
    case = make_case(122, 8, 20, 'state', 9, internal=False)
    ctx = open_context(ra, {opt: 1})
    try:
        model, batch = build(ra, ctx, case)
        model.prune(batch)
        with pytest.raises(ra.lib.RaotehHipError) as e:
            model.expected_history_statistics(batch)
        assert e.value.code == ra.lib.RT_ERR_UNSUPPORTED
    finally:
        ctx.close()


def test_129_states_are_refused_where_the_model_is_created(ra):
    case = make_case(128, 6, 4, 'state', 1)
    with pytest.raises((ValueError, ra.lib.RaotehHipError)):
        ra.device.TreeModel(case.T, case.root, 129)
