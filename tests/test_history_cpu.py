"""The history-independence walk on the host (tests/_history_cases.py): the walk is deterministic,
every ordered pair (operation, read) of every row is adjacent in it, what is never live is exactly
the set of refusals the header documents, the shadow state makes the transitions the header
describes, and the dependency table covers every read.  No device."""
import itertools

import numpy as np
import pytest

import _history_cases as hc

ROWS = hc.ROWS
IDS = [r.name for r in ROWS]


def walk_of(row):
    return hc.build_segments(row)


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_the_walk_is_deterministic(row):
    a, b = hc.build_segments(row), hc.build_segments(row)
    assert a == b
    assert hc.euler_circuit(row, 1) != hc.euler_circuit(row, 2)          # (the seed is used)
    ta = [(op, res, s.cur.key()) for piece in a for op, res, s in hc.simulate(row, piece)]
    tb = [(op, res, s.cur.key()) for piece in b for op, res, s in hc.simulate(row, piece)]
    assert ta == tb


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_the_circuit_takes_every_pair_once(row):
    """The Euler circuit alone: |ops| * |reads| pairs (operation, read) and |reads| * |mutators|
    pairs (read, mutator), each adjacent exactly once -- no shorter walk has them all."""
    ops, reads, muts = hc.ops_of(row), hc.reads_of(row), hc.mutators_of(row)
    circuit = hc.euler_circuit(row, row.seed)
    pairs = list(zip(circuit, circuit[1:]))
    assert len(pairs) == len(set(pairs)) == len(ops) * len(reads) + len(reads) * len(muts)
    assert set(p for p in pairs if p[1] in reads) == set(itertools.product(ops, reads))
    assert not any(a in muts and b in muts for a, b in pairs)


@pytest.mark.parametrize('row', ROWS, ids=IDS)
def test_pair_coverage_is_complete_apart_from_documented_refusals(row):
    ops, reads = hc.ops_of(row), hc.reads_of(row)
    every = set(itertools.product(ops, reads))
    assert len(every) == len(ops) * len(reads)
    pieces = walk_of(row)
    assert len(pieces) == hc.SEGMENTS.get(row.name, 1)
    adjacent, live = set(), set()
    for piece in pieces:
        assert set(piece) <= set(ops)
        adjacent |= hc.adjacent_pairs(row, piece)
        live |= hc.live_pairs(row, hc.simulate(row, piece))
    assert adjacent == every                       # refused pairs stay in the walk
    assert len(live) == len(every) - len(hc.documented_refusals(row))
    assert every - live == hc.documented_refusals(row)


def test_documented_refusals_are_what_the_table_says():
    row = hc.ROW['mfma-one-wave-n20-dense-33']
    ref = hc.documented_refusals(row)
    for r in hc.READS:
        if 'o' not in r.kinds:
            continue
        assert (('set_transitions', r.name) in ref) == r.needs.startswith('rate'), r.name
        assert (('set_rates_spectral', r.name) in ref) == (r.needs in ('rateq', 'rateq1')), r.name
        assert (('set_rate_sets_other', r.name) in ref) == (r.snapshot == 'multi'), r.name
        assert (('set_rate_sets_per_edge', r.name) in ref) == (r.needs == 'sets1'), r.name
        assert (('clone', r.name) in ref) == (r.snapshot == 'multi'), r.name
        for x in ('prune', 'step_true', 'wait_for_kernel', 'recompute:posteriors', 'set_rates_Q',
                  'posteriors', r.name):
            assert (x, r.name) not in ref
    # above 64 states there are no spectral rates: the call is refused and changes nothing
    wide = hc.ROW['wide-n70-mask-17']
    assert not any(x == 'set_rates_spectral' for x, _ in hc.documented_refusals(wide))
    assert hc.mutator_outcome(hc.initial_state(wide), 'set_rates_spectral') == hc.UNSUPPORTED
    # a partitioned batch: the reads of section 2c and nothing else
    part = hc.ROW['partitioned-n20-dense-4sets']
    ref = hc.documented_refusals(part)
    for r in hc.PART_REFUSED_READS:
        assert all((x, r) in ref for x in hc.ops_of(part))
        assert hc.read_outcome(hc.initial_state(part), r) == hc.UNSUPPORTED


def run(row, ops, state=None):
    trace = hc.simulate(row, ops, state)
    return trace[-1][2], [res for _, res, _ in trace]


def test_rates_current_after_set_transitions_and_after_a_recomputing_read():
    row = hc.ROW['mfma-one-wave-n20-dense-33']
    s = hc.initial_state(row)
    assert s.rates_current
    s, res = run(row, ['set_transitions'], s)
    assert not s.rates_current and s.cur.mode == 'direct' and s.cur.rates_kind == 'rates'
    for name in ('branch_profiles', 'nni_scores', 'spr_scores', 'place_queries',
                 'branch_expectations', 'branch_length_gradient', 'sample_mappings',
                 'expected_history_statistics'):
        assert hc.read_outcome(s, name) == hc.INVALID, name
        assert hc.read_outcome(s, name, recompute=True) == 'ok', name
    for name in ('posteriors', 'sample_states', 'map_states'):
        assert hc.read_outcome(s, name) == 'ok'
    # a refused read leaves the state as it was
    t, res = run(row, ['branch_profiles'], s)
    assert res == [hc.INVALID] and t.cur.key() == s.cur.key() and not t.rates_current
    # a read with recompute_transitions=True is a mutator: it makes the rates current
    flagged = hc.flagged_reads(row)
    assert 'loglik' not in flagged and 'multi' not in flagged and len(flagged) == 14
    assert all(hc.RECOMPUTE + r in hc.mutators_of(row) for r in flagged)
    for r in ('posteriors', 'branch_expectations', 'spr_scores', 'map_states'):
        t, res = run(row, [hc.RECOMPUTE + r], s)
        assert res == ['ok'] and t.rates_current and t.cur.mode == 'rates', r
    # ... a rate-set read rebuilds the tables of the sets, not the model's own matrices
    u, res = run(row, ['set_rate_sets_same', 'recompute:class_posteriors'], s)
    assert res == ['ok', 'ok'] and not u.rates_current
    # ... and one that is refused (per-edge rate matrices) changes nothing
    u, res = run(row, ['set_rates_per_edge', 'set_transitions', 'recompute:branch_length_gradient'])
    assert res[-1] == hc.INVALID and not u.rates_current
    # recompute_transitions, step(True) and the set_rates calls do; step(False) and prune do not
    for op, want in (('recompute_transitions', True), ('step_true', True), ('set_rates_t', True),
                     ('set_rates_Q', True), ('set_rates_spectral', True), ('step_false', False),
                     ('prune', False), ('set_root_w', False)):
        assert run(row, [op], s)[0].rates_current == want, op
    # spectral rates: the matrices are current, but there is no rate matrix
    t, _ = run(row, ['set_rates_spectral'], s)
    assert hc.read_outcome(t, 'branch_profiles') == 'ok'
    assert hc.read_outcome(t, 'branch_expectations', recompute=True) == hc.INVALID
    t, _ = run(row, ['set_transitions', 'recompute_transitions'], t)
    assert t.cur.mode == 'spectral'


def test_the_epoch_after_the_number_of_rate_sets_changed():
    row = hc.ROW['mfma-one-wave-n20-dense-33']
    s, res = run(row, ['multi', 'step_multi', 'set_rate_sets_same', 'multi', 'step_multi', 'multi'])
    assert res == [hc.INVALID, hc.INVALID, 'ok', hc.INVALID, 'ok', 'ok']
    K = s.cur.K
    kept = s.multi.sets
    s, res = run(row, ['set_rate_sets_same', 'multi', 'mixture_log_likelihoods'], s)
    assert res == ['ok'] * 3 and s.multi_ok and s.multi.sets == kept != s.cur.sets
    t, res = run(row, ['set_rate_sets_other', 'multi', 'mixture_log_likelihoods',
                       'class_posteriors'], s)
    assert res == ['ok', hc.INVALID, hc.INVALID, 'ok'] and t.cur.K != K and not t.multi_ok
    t, res = run(row, ['set_rate_sets_same', 'multi', 'step_multi', 'multi'], t)
    assert res == ['ok', hc.INVALID, 'ok', 'ok'] and t.multi.K == t.cur.K != K
    # a clone carries the log-likelihoods, not the step_multi results and not the weights
    u, res = run(row, ['set_weights_w', 'prune', 'clone', 'loglik', 'multi'], s)
    assert res == ['ok', 'ok', 'ok', 'ok', hc.INVALID] and u.cur.weights is None
    # the partitioned batch
    part = hc.ROW['partitioned-n20-dense-4sets']
    p, res = run(part, ['partition_loglik', 'set_rate_sets_same', 'step_partitioned_true',
                        'partition_loglik', 'set_rate_sets_other', 'partition_loglik',
                        'branch_expectations_partitioned', 'step_partitioned_false',
                        'partition_loglik', 'prune', 'posteriors'])
    assert res == [hc.INVALID, 'ok', 'ok', 'ok', 'ok', hc.INVALID, 'ok', 'ok', 'ok',
                   hc.UNSUPPORTED, hc.UNSUPPORTED]
    assert p.cur.K == hc.PART_NSETS + 1


def test_snapshot_selection_per_read():
    row = hc.ROW['mfma-one-wave-n20-dense-33']
    s, _ = run(row, ['set_rate_sets_same', 'set_weights_w', 'prune', 'step_multi'])
    at_launch = s.cur.key()
    s, _ = run(row, ['set_rates_Q', 'set_root_w', 'set_weights_w', 'set_rate_sets_same'], s)
    assert s.pruned.key() == at_launch == s.multi.key() != s.cur.key()
    for r in hc.READS:
        if 'o' not in r.kinds:
            continue
        snap = s.cur if r.snapshot == 'cur' else getattr(s, r.snapshot)
        assert (snap.key() == at_launch) == (r.name in ('loglik', 'multi', 'mixture_log_likelihoods'))
    # step(True) launches with recomputed matrices, step(False) with what is there
    s, _ = run(row, ['set_transitions', 'step_false'], s)
    assert s.pruned.mode == 'direct'
    s, _ = run(row, ['step_true'], s)
    assert s.pruned.mode == 'rates' and s.pruned.Q == s.cur.Q


def test_the_dependency_table_covers_every_read():
    params = set(hc.PARAM_TOKENS)
    assert params == {'Q', 't', 'root', 'weights', 'sets', 'cw'}
    names = [r.name for r in hc.READS]
    assert len(names) == len(set(names)) == 20
    for r in hc.READS:
        assert r.deps and set(r.deps) <= params, r.name
        assert 'root' in r.deps
        assert ('sets' in r.deps) != ('Q' in r.deps and 't' in r.deps), r.name
        assert r.cite and ('rt_' in r.cite or 'section 2' in r.cite or 'device.py' in r.cite), r.name
        assert r.snapshot in ('cur', 'pruned', 'multi', 'part')
        assert (r.needs == 'launch') == (r.snapshot != 'cur') or r.name == 'mixture_log_likelihoods'
    for row in ROWS:
        reads = hc.reads_of(row)
        assert len(reads) == len(set(reads))
        assert all(r in hc.READ for r in reads)
        cases = hc.stale_cases(row)
        live = [r for r in reads if not (row.partitioned and r in hc.PART_REFUSED_READS)]
        assert sorted(set(r for r, _ in cases)) == sorted(live)
        assert len(cases) == sum(len(hc.READ[r].deps) for r in live)
        for read, param in cases:
            state, old = hc.stale_states(row, read, param)
            assert hc.read_outcome(state, read) == 'ok'
            snap = state.cur if hc.READ[read].snapshot == 'cur' else getattr(state, hc.READ[read].snapshot)
            token = hc.PARAM_TOKENS[param][0]
            assert getattr(snap, token) != getattr(old, token), (read, param)
    # every read of the catalogue is in some row
    assert set(names) == set(r for row in ROWS for r in hc.reads_of(row))
    for key, (fields, cite, tol) in hc.EXCEPTIONS.items():
        assert key[0] in hc.ROW and key[1] in hc.READ and fields
        assert 'DESIGN.md' in cite or 'section' in cite          # (no exception without a citation)
        assert tol <= 1e-12


def test_generated_parameters():
    for row in ROWS:
        fx = hc.fixed_of(row)
        assert 9 <= row.nnodes <= 13 and fx.T.number_of_nodes() == row.nnodes
        deg = dict(fx.T.degree())
        assert deg[fx.root] == 3                                   # a multifurcation
        assert sum(1 for v, d in deg.items() if d == 2 and v != fx.root) >= 1     # a single child
        assert (len(fx.obs_nodes) > len(fx.leaves)) == (not row.leaves_only)
        assert 0 < fx.zero_site < row.nsites - 1 and fx.zero_weight_site != fx.zero_site
        for tok in (0, 1, 5):
            Q = hc.gen_Q(row, tok, 2)
            assert not Q[:, 0, :].any() and not Q[:, :, 0].any()
            assert np.allclose(Q.sum(axis=2), 0.0, atol=1e-12)
            t = hc.gen_t(row, tok)
            assert (t[1:] == 0).sum() == 1 and t[0] == 0 and (t >= 0).all()
            w = hc.gen_weights(row, tok)
            assert (w == 0).sum() == 1 and w[fx.zero_weight_site] == 0
            P = hc.gen_esd(row, tok)
            assert np.allclose(P[1:].sum(axis=2), 1.0) and not P[1:, 1:, 0].any()
        assert not np.array_equal(hc.gen_Q(row, 1, 1), hc.gen_Q(row, 2, 1))
        if row.wide:
            assert fx.data.shape[2] == 2 and fx.data[:, :, 1].any() and fx.data[:, :, 0].any()
    per_edge = [row for row in ROWS if 'set_rates_per_edge' in hc.mutators_of(row)]
    assert len(per_edge) >= 2


def test_exceptions_hold_only_for_launches_before_the_kernel_wait():
    row = hc.ROW['lane-background-n4-mask-38']
    s, _ = run(row, ['set_rate_sets_same', 'prune', 'step_multi'])
    assert hc.tolerance(s, 'loglik') == (('totals',), 1e-12)
    assert hc.tolerance(s, 'multi') == (('totals', 'weighted_sums'), 1e-12)
    assert hc.tolerance(s, 'posteriors') is None and hc.tolerance(s, 'mixture_log_likelihoods') is None
    # the results of a launch from before the wait stay what the earlier kernel made of them
    s, _ = run(row, ['wait_for_kernel'], s)
    assert hc.tolerance(s, 'loglik') is not None and hc.tolerance(s, 'multi') is not None
    t, _ = run(row, ['clone'], s)                       # (a clone carries them, and waits)
    assert t.waited and hc.tolerance(t, 'loglik') is not None
    s, _ = run(row, ['prune', 'step_multi'], s)
    assert hc.tolerance(s, 'loglik') is None and hc.tolerance(s, 'multi') is None
    for other in ROWS:
        if not other.background:
            u, _ = run(other, ['prune'])
            assert hc.tolerance(u, 'loglik') is None


def test_a_change_of_the_number_of_rate_sets_leaves_the_gradients_live():
    for name, grad in (('mfma-one-wave-n20-dense-33', 'branch_length_gradient_mixture'),
                       ('partitioned-n20-dense-4sets', 'branch_length_gradient_partitioned')):
        row = hc.ROW[name]
        s, res = run(row, ['set_rate_sets_same', 'set_rate_sets_other', grad])
        assert res == ['ok'] * 3 and s.cur.set_nq == 1
        assert ('set_rate_sets_other', grad) not in hc.documented_refusals(row)
        s, res = run(row, ['set_rate_sets_per_edge', grad], s)
        assert res == ['ok', hc.INVALID] and s.cur.set_nq == 2
        assert ('set_rate_sets_per_edge', grad) in hc.documented_refusals(row)
