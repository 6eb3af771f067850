"""A long-lived model and batch read like fresh ones: the walk of tests/_history_cases.py -- every
ordered pair (operation, read) adjacent at least once -- on a TreeModel / SiteBatch that live through
all of it, every read compared BIT FOR BIT (returned arrays, statuses, error codes) with the same
read on a fresh pair in a second context that was told the current parameters alone.

One case per row of the layout table (and per piece of its walk where SEGMENTS cuts it); the kernel
name proves the row.  Two more tests: the comparison sees a twin that missed the last change of any
parameter a read depends on, and the twin at the end of a walk is tied to the host oracle.  The
mismatches the walk found are named regression tests at the end of the file."""
import collections

import numpy as np
import pytest

import _history_cases as hc

pytestmark = pytest.mark.gpu

RTOL = 1e-10               # a log-likelihood against the oracle (test_resident_reads_gpu.RTOL)


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
    for k, v in dict(hc.DEFAULTS, **opts).items():
        ctx.set_option(k, v)
    return ctx


def check_name(row, name):
    assert name.startswith(row.prefix), (row.name, name)
    for part in row.need:
        assert part in name, (row.name, name)


def matches(expected, got):
    """The attempt on the long-lived pair is what the shadow state predicts from the header."""
    return got[0] == 'ok' if expected == 'ok' else got == ('refused', expected)


def walk(ra, row, piece, ctx, ctx2):
    """Runs the operations on one long-lived pair; -> (the pair, the mismatches)."""
    live = hc.LongLived(ra.device, ra.lib, ctx, row)
    bad = []
    for step, op in enumerate(piece):
        tail = piece[max(0, step - 4):step + 1]
        try:
            expected, got, read, flag = live.run(op)
        except ra.lib.RaotehHipError as e:
            raise AssertionError('step %d of %d (... %s): %s' % (step, len(piece), ' -> '.join(tail), e))
        if not matches(expected, got):
            bad.append((step, tail, 'the header says %r, the call gave %r'
                        % (expected, got if got[0] == 'refused' else 'ok')))
        if read is None:
            continue
        try:
            twin = hc.Twin(ra.device, ctx2, live.state, read)
            try:
                want = twin.read(ra.lib, row, read, flag)
            finally:
                twin.close()
        except ra.lib.RaotehHipError as e:
            raise AssertionError('the twin of step %d of %d (... %s): %s'
                                 % (step, len(piece), ' -> '.join(tail), e))
        diff = hc.differences(got, want, hc.tolerance(live.state, read))
        if diff:
            bad.append((step, tail, '%s differs from the fresh twin in %s' % (read, diff)))
    return live, bad


GPU_ROWS = hc.ROWS
CASES = [(row, i) for row in GPU_ROWS for i in range(hc.SEGMENTS.get(row.name, 1))]


@pytest.mark.parametrize('row,piece', CASES, ids=['%s-%d' % (r.name, i) for r, i in CASES])
def test_reads_of_a_long_lived_pair_equal_those_of_a_fresh_one(ra, row, piece, tmp_path, monkeypatch):
    if row.background:
        # a cold code-object cache: the walk begins on the interpreter kernel and the batch
        # switches (and packs its sites again) at a pruning launch or at wait_for_kernel
        monkeypatch.setenv('RAOTEH_JIT_CACHE_DIR', str(tmp_path / 'jit'))
    ops = hc.build_segments(row)[piece]
    ctx, ctx2 = open_context(ra, row.opts), open_context(ra, row.opts)
    try:
        live, bad = walk(ra, row, ops, ctx, ctx2)
        assert not bad, '%d mismatches, the first: %r' % (len(bad), bad[:3])
        # the kernel the row is about ran
        if row.partitioned:
            if live.state.cur.sets is None:
                live.run('set_rate_sets_same')
            live.run('step_partitioned_true')
        else:
            live.run('wait_for_kernel')
            live.run('prune')
        check_name(row, live.batch.kernel_name)
    finally:
        ctx.close()
        ctx2.close()


AnchorCase = collections.namedtuple('AnchorCase', 'T root n obs_nodes leaves kind data obs_lik '
                                                  'root_distn Q node_q t site_sets nsets')


def host_transitions(row, p, a):
    """The transition matrices of snapshot p from the shadow state alone (scipy)."""
    import scipy.linalg
    if p.mode == 'direct':
        return a['esd']
    N = row.nnodes
    esd = np.zeros((N, row.n, row.n))
    for v in range(1, N):
        Q = a['Qspec'] if p.mode == 'spectral' else a['Q'][0 if a['node_q'] is None else a['node_q'][v]]
        esd[v] = scipy.linalg.expm(a['t'][v] * Q)
    return esd


@pytest.mark.parametrize('row', GPU_ROWS, ids=[r.name for r in GPU_ROWS])
def test_the_twin_at_the_end_of_the_walk_agrees_with_the_host_oracle(ra, row):
    """Ties the SHADOW STATE to the host oracle.  No walk runs here: the state the row's walk ends in
    is simulated on the host, one fresh twin is built from it, and its log-likelihoods, statuses
    and totals are checked against loglik_reference / totals_reference on the device's own
    transition matrices and against the oracle on matrices computed from the shadow state alone
    (scipy); the partitioned row has one oracle, _partition_cases.oracle, which is already of the
    second kind."""
    from oracle import oracle_numpy as orc
    from _resident_cases import loglik_reference, totals_reference
    import _partition_cases
    fx = hc.fixed_of(row)
    state = hc.simulate(row, hc.build_segments(row)[-1])[-1][2]
    tail = ['set_rate_sets_same', 'step_partitioned_true'] if row.partitioned else ['prune']
    state = hc.simulate(row, tail, state)[-1][2]
    read = 'partition_loglik' if row.partitioned else 'loglik'
    ctx = open_context(ra, row.opts)
    try:
        twin = hc.Twin(ra.device, ctx, state, read)
        got = hc.call_read(twin.model, twin.batch, row, read, twin.call_arrays)
        ll, st, tot = got['loglik'], got['status'], got['totals']
        snap = state.part if row.partitioned else state.pruned
        a = hc.materialise(row, snap)
        root = a['root'] if a['root'] is not None else np.ones(row.n)
        ta = twin.model.tree
        cols = [ta.node_to_index[v] for v in fx.obs_nodes]
        if row.partitioned:
            Q, node_q, t = a['sets']
            case = AnchorCase(fx.T, fx.root, row.n, fx.obs_nodes, fx.obs_nodes, row.kind, fx.data,
                              fx.obs_lik, root, Q, node_q if node_q is not None else
                              np.zeros(row.nnodes, dtype=np.int64), t, fx.site_sets, hc.PART_NSETS)
            want, wst = _partition_cases.oracle(twin.model, case)
            references = [(want, wst)]
        else:
            case = AnchorCase(fx.T, fx.root, row.n, fx.obs_nodes, fx.obs_nodes, row.kind, fx.data,
                              fx.obs_lik, root, None, None, None, None, 0)
            want, wst = loglik_reference(twin.model, case)
            shadow_ll, shadow_st = orc.batch_log_likelihoods(
                ta.indices, ta.indptr, host_transitions(row, snap, a), cols, fx.obs_lik, root)
            references = [(want, wst), (shadow_ll, shadow_st)]
        for w, ws in references:
            np.testing.assert_array_equal(st, ws)
            ok = ws == 0
            np.testing.assert_allclose(ll[ok], w[ok], rtol=RTOL)
            assert np.all(np.isneginf(ll[~ok]))
        # (other sites may have likelihood 0 too: an edge of length 0 between two observed nodes)
        assert st[fx.zero_site] == 1 and not st.all()
        ref = totals_reference(ll, st)
        assert tot[1] == ref[1] >= 1 and tot[2] == ref[2] == row.nsites
        assert abs(tot[0] - ref[0]) <= 1e-12 * abs(ref[0]) + 1e-300, (tot, ref)
        assert abs(tot[0] - totals_reference(want, wst)[0]) <= RTOL * abs(ref[0])
        twin.close()
    finally:
        ctx.close()


@pytest.mark.parametrize('row', GPU_ROWS, ids=[r.name for r in GPU_ROWS])
def test_the_comparison_sees_a_stale_parameter(ra, row):
    """For every read and every parameter of its dependency set: a twin that missed the last change
    of that parameter differs from the fresh twin.  (Valid calls only.)"""
    ctx = open_context(ra, row.opts)
    blind = []
    try:
        for read, param in hc.stale_cases(row):
            state, old = hc.stale_states(row, read, param)
            out = []
            for stale in (None, (param, old)):
                twin = hc.Twin(ra.device, ctx, state, read, stale=stale)
                try:
                    out.append(twin.read(ra.lib, row, read))
                finally:
                    twin.close()
            assert out[0][0] == out[1][0] == 'ok', (read, param, out[0][:1], out[1][:1])
            if not hc.differences(out[1], out[0]):
                blind.append((read, param))
    finally:
        ctx.close()
    assert not blind, blind


# ---- what the walk found -----------------------------------------------------------------------

def test_rate_reads_refuse_transitions_set_directly_after_the_rates(ra):
    """set_rates -> set_transitions -> branch_expectations / expected_history_statistics /
    sample_mappings without recompute_transitions: the rate matrices of the earlier set_rates were
    still resident, so the calls ran and combined derivatives of the OLD rates with the NEW matrices
    (rates_current was not consulted, unlike in branch_profiles, nni_scores, spr_scores and
    place_queries).  The header refuses "transitions set directly"; a fresh model with the same
    matrices does.  With recompute_transitions they answer as a fresh model under the rates."""
    row = hc.ROW['mfma-one-wave-n20-dense-33']
    fx = hc.fixed_of(row)
    Q, t, esd = hc.gen_Q(row, 1, 1), hc.gen_t(row, 1), hc.gen_esd(row, 1)
    ctx = open_context(ra, row.opts)
    try:
        model = ra.device.TreeModel(fx.T, fx.root, row.n, ctx=ctx)
        model.set_rates(Q=Q, t=t)
        batch = hc.upload(model, row)
        fresh = ra.device.TreeModel(fx.T, fx.root, row.n, ctx=ctx)
        fresh.set_rates(Q=Q, t=t)
        fbatch = hc.upload(fresh, row)
        calls = [lambda m, b, **kw: m.branch_expectations(b, fx.coefs, **kw),
                 lambda m, b, **kw: m.branch_length_gradient(b, **kw),
                 lambda m, b, **kw: m.sample_mappings(b, fx.coefs[:1], ndraws=2, seed=5, **kw),
                 lambda m, b, **kw: m.expected_history_statistics(
                     b, recompute_transitions=kw.get('recompute_transitions', False))]
        for call in calls:
            want = hc.attempt(ra.lib, lambda: call(fresh, fbatch))
            assert want[0] == 'ok'
            model.set_transitions(esd)
            assert hc.attempt(ra.lib, lambda: call(model, batch)) == ('refused', hc.INVALID)
            np.testing.assert_array_equal(model.get_transitions(), esd)      # nothing was touched
            got = hc.attempt(ra.lib, lambda: call(model, batch, recompute_transitions=True))
            assert not hc.differences(got, want)
            assert hc.attempt(ra.lib, lambda: call(model, batch)) == got
    finally:
        ctx.close()


@pytest.mark.parametrize('n', [5, 8])
def test_expectation_step_at_5_to_8_states_loads_no_pair_behind_the_observation_image(ra, n):
    """What the n = 8 walk met as "an illegal memory access": with 5 .. 8 states a site tile holds ONE
    pair of k-steps per observed node (1 KB), but in expect_wsum_kernel the lanes of the padding
    states 8 .. 15 addressed pair 1 of an observed leaf -- the next slot of the image, and for the
    last slot of the last tile the kilobyte behind the end of the batch's observations.  The loaded
    values were discarded (the results were right), so the read showed only where that kilobyte
    was not mapped: a fault that depended on what the process had allocated before.  The lanes
    now load pair 0.  Here: the path itself, two tiles, the last observed leaf in the last tile,
    against the host reference at the tolerances of test_resident_reads_gpu.check_expectations."""
    from _resident_cases import expectation_reference, make_case, set_rates
    case = make_case(n, 10, 17, 'dense', 40 + n)
    ctx = open_context(ra, {'jit': 0})
    try:
        model = ra.device.TreeModel(case.T, case.root, n, ctx=ctx)
        set_rates(model, case)
        model.set_root_distn(case.root_distn)
        batch = model.upload_sites(case.obs_nodes, case.data, kind='dense')
        dwell, rootp, trans, status = model.expected_history_statistics(batch, return_status=True)
        want = expectation_reference(model, case)
        assert status[case.zero_site] == 2 and not status[:case.zero_site].any()
        scale = np.abs(want[0]).max()
        np.testing.assert_allclose(dwell, want[0], rtol=1e-9, atol=1e-13 * scale)
        np.testing.assert_allclose(rootp, want[1], rtol=1e-9, atol=1e-15)
        np.testing.assert_allclose(trans, want[2], rtol=1e-9, atol=1e-13 * scale)
    finally:
        ctx.close()
