"""Every state-count instance of the reads of a resident batch against the host, on the GPU.

Above four states every read is a template stamped out per KS = ceil(n / 4) (2..32) or per
NT = ceil(n / 16) (1..8); the other GPU modules reach a handful of those instances.  Here one small
case per n (tests/_state_sweep_cases.py: every KS, every NT, every tail of the last k-step and of
the last row tile, three sites pinned to the tail states) runs every read -- the plain forms over
PLAIN (64 values), the mixture and partitioned forms over FORMS (33) -- each against the reference
and at the tolerance of its own parity test, whose check function is imported from that test's
module or restated beside its name.  Then the tree-specialised pruning kernel at four n, bit for
bit against the interpreter's results, and a descending walk over n in one context per form, bit
for bit against the fresh contexts: the only way, from outside, to put a larger n's data behind
the rows a smaller n assumes to be zero.

One context per (form, n), opened by a module-scoped parametrised fixture (pytest groups the
tests of one n together) and closed when the n is done; jit = 0 and jit_async = 0 throughout
except in the spot checks."""
import numpy as np
import pytest

import _mapping_cases as mpc
import _partition_cases as pc
import _sample_cases as sc
import _state_sweep_cases as sw
import _step_multi_cases as smc
from _resident_cases import expectation_reference, posterior_reference
# the check functions (and with them the tolerances) of the parity tests
import test_branch_expect_gpu as t_branch
import test_branch_profiles_gpu as t_profile
import test_map_states_gpu as t_map
import test_mixture_expect_gpu as t_mix_branch
import test_mixture_search2_gpu as t_mix_search2
import test_mixture_search_gpu as t_mix_search
import test_nni_gpu as t_nni
import test_partition_reads_gpu as t_part_branch
import test_partition_search2_gpu as t_part_search2
import test_partition_search_gpu as t_part_search
import test_place_gpu as t_place
import test_resident_reads_gpu as t_reads
import test_sample_mappings_gpu as t_mappings
import test_spr_gpu as t_spr

pytestmark = pytest.mark.gpu

DEFAULTS = {'jit': 0, 'force_generic': 0, 'jit_block_sites': 0, 'jit_async': 0, 'rescale': 0,
            'leaf_state_kernels': 1}
W = sw.site_weights()
PINNED = list(sw.PINNED_SITES)
ZERO_PROB = 1                                   # RT_SITE_ZERO_PROB
SAMPLE_SEED, SAMPLE_FIRST, NDRAWS = 77, 2 ** 40 + 5, 2


def nid(n):
    return 'n%d' % n


# ---- building a case on the device -----------------------------------------------------------

class State(object):
    pass


def open_context(opts=None):
    from raoteh_amd import device
    ctx = device.Context(0)
    for k, v in dict(DEFAULTS, **(opts or {})).items():
        ctx.set_option(k, v)
    return ctx


def build(form, ctx, case):
    """(model, batch) of a case on the context, as the parity tests of the form build theirs."""
    from raoteh_amd import device
    if form == 'plain':
        model = device.TreeModel(case.T, case.root, case.n, ctx=ctx)
        model.set_rates(Q=case.Qs, node_q=case.node_q)
        model.set_root_distn(case.root_distn)
        return model, model.upload_sites(case.obs_nodes, case.data, kind=case.kind)
    model, batch = (smc if form == 'mix' else pc).upload(device, ctx, case)
    model.set_rate_sets(case.Q, t=case.t, node_q=case.node_q)
    return model, batch


def open_state(form, n, opts=None, ctx=None):
    s = State()
    s.form, s.n, s.case = form, n, sw.case_of(form, n)
    s.own_ctx = ctx is None
    s.ctx = open_context(opts) if ctx is None else ctx
    s.model, s.batch = build(form, s.ctx, s.case)
    s.ta = s.model.tree
    s.c = sw.class_weights_of(n)
    s.factors = sw.factors_of(s.ta)
    return s


def place_reference_of(s):
    """The placement reference of the state's case, shared by the dense and the state query."""
    if not hasattr(s, 'place_ref'):
        s.place_ref = (sw.place_ref(s.model, s.case) if s.form == 'plain'
                       else (sw.mix_refs if s.form == 'mix' else sw.part_refs)(s.case, 'place'))
    return s.place_ref


def close_state(s):
    s.batch.close()
    s.model.close()
    if s.own_ctx:
        s.ctx.close()


def _state_fixture(form, ns):
    @pytest.fixture(scope='module', params=ns, ids=nid)
    def fixture(request):
        s = open_state(form, request.param)
        yield s
        close_state(s)
    return fixture


plain = _state_fixture('plain', sw.PLAIN)
mix = _state_fixture('mix', sw.FORMS)
part = _state_fixture('part', sw.FORMS)


# ---- the reads the walk and the spot checks repeat -------------------------------------------

def read_nni(s):
    s.batch.set_weights(W)
    if s.form == 'plain':
        return s.model.nni_scores(s.batch, lengths=sw.grid_of(s.model), per_site=True)
    if s.form == 'mix':
        return s.model.nni_scores_mixture(s.batch, s.c, s.factors, per_site=True)
    return s.model.nni_scores_partitioned(s.batch, s.factors, per_site=True)


def read_place(s, qkind):
    s.batch.set_weights(W)
    dense, states = sw.form_queries(s.n)
    q = dense if qkind == 'dense' else states
    kw = dict(kind=qkind, fractions=sw.FRACTIONS, pendant=sw.PENDANT, per_site=True)
    if s.form == 'plain':
        return s.model.place_queries(s.batch, q, **kw)
    if s.form == 'mix':
        return s.model.place_queries_mixture(s.batch, s.c, q, **kw)
    return s.model.place_queries_partitioned(s.batch, q, **kw)


def read_branch(s):
    s.batch.set_weights(W)
    if s.form == 'plain':
        return s.model.branch_expectations(s.batch, sw.coefs_of(s.n))
    if s.form == 'mix':
        return s.model.branch_expectations_mixture(s.batch, sw.form_coefs(s.n), s.c)
    return s.model.branch_expectations_partitioned(s.batch, sw.form_coefs(s.n))


def read_posteriors(s):
    node_sets, edge_sets = t_reads.sets_of(s.n, np.random.RandomState(12000 + s.n))
    return s.model.posteriors(s.batch, node_sets=node_sets, edge_sets=edge_sets, marginals=True), \
        node_sets, edge_sets


READS = {'nni': read_nni, 'place-dense': lambda s: read_place(s, 'dense'),
         'place-state': lambda s: read_place(s, 'state'), 'branch': read_branch,
         'posteriors': lambda s: read_posteriors(s)[0]}
WALKED = ('nni', 'place-dense', 'place-state', 'branch')
SPOTTED = ('posteriors', 'nni', 'place-dense', 'place-state')


def bits_of(got):
    """Every array of a result tuple, by name, as bytes."""
    return dict((name, (x.shape, x.dtype.str, x.tobytes())) for name, x in zip(got._fields, got)
                if isinstance(x, np.ndarray))


FRESH = {}                                       # (form, n, read) -> bits_of, from a fresh context


def keep(s, read, got):
    FRESH[s.form, s.n, read] = bits_of(got)
    return got


def fresh_bits(form, n, read):
    """The bits the read gave in the fresh context of section 1..3 (computed here, in a context
    of its own, when that test did not run in this session)."""
    if (form, n, read) not in FRESH:
        s = open_state(form, n)
        try:
            keep(s, read, READS[read](s))
        finally:
            close_state(s)
    return FRESH[form, n, read]


def assert_same_bits(got, want, label):
    got = bits_of(got)
    assert sorted(got) == sorted(want), label
    for name in sorted(want):
        assert got[name][:2] == want[name][:2], (label, name)
        if got[name][2] != want[name][2]:
            size = np.dtype(got[name][1]).itemsize
            a = np.frombuffer(got[name][2], dtype=np.uint8).reshape(-1, size)
            b = np.frombuffer(want[name][2], dtype=np.uint8).reshape(-1, size)
            at = np.flatnonzero((a != b).any(axis=1))
            x = np.frombuffer(got[name][2], dtype=got[name][1])[at[:3]]
            y = np.frombuffer(want[name][2], dtype=want[name][1])[at[:3]]
            raise AssertionError('%s: %s differs in %d of %d entries, the first %r against %r'
                                 % (label, name, len(at), len(a), x.tolist(), y.tolist()))


def live_and_pinned(status, zero_site=None):
    assert not np.asarray(status)[PINNED].any()           # the pinned sites are live
    if zero_site is not None:
        assert status[zero_site] == ZERO_PROB and np.count_nonzero(status) == 1


# ---- 1. the plain forms ----------------------------------------------------------------------

def label_of(s, family):
    return 'sweep %s %s n=%d (KS %d, NT %d, %s)' % (s.form, family, s.n, sw.ks_of(s.n),
                                                   sw.nt_of(s.n), s.case.kind)


def test_plain_posteriors(plain):
    """check_posteriors of test_resident_reads_gpu.py, restated so that the gap is printed: RTOL
    1e-10 with atol 1e-15 on the set sums and the marginals, the status exactly; the node set
    [0, n - 1] and edge sets over both halves of the states are among sets_of's."""
    s = plain
    post, node_sets, edge_sets = read_posteriors(s)
    keep(s, 'posteriors', post)
    nv, ev, D, status = posterior_reference(s.model, s.case, node_sets, edge_sets, [0, 1, 17, 32])
    np.testing.assert_array_equal(post.status, status)
    live_and_pinned(post.status, s.case.zero_site)
    gap = max(np.abs(post.node_values - nv).max(), np.abs(post.edge_values - ev).max(),
              np.abs(post.marginals - D).max())
    print('%s: max |value - ref| / scale %.2e (probabilities: scale 1; bound %.0e relative)'
          % (label_of(s, 'posteriors'), gap, t_reads.RTOL))
    for got, want in ((post.node_values, nv), (post.edge_values, ev), (post.marginals, D)):
        np.testing.assert_allclose(got, want, rtol=t_reads.RTOL, atol=1e-15)
    assert not post.marginals[s.case.zero_site].any()
    # the pinned leaves sit in their pinned state with posterior one
    for site, col, state in sw.pins_of(s.case):
        v = s.ta.node_to_index[s.case.obs_nodes[col]]
        assert abs(post.marginals[site, v, state] - 1.0) <= 1e-12
        assert not np.delete(post.marginals[site, v], state).any()


def test_plain_expected_history_statistics(plain):
    """check_expectations of test_resident_reads_gpu.py / check_step of test_expect_wide_gpu.py
    (the expectation step up to 64 states and from 65 to 128), restated so that the gap is
    printed: rtol 1e-9 with atol 1e-13 of the largest dwell time, 1e-15 for the root sums; the
    status exactly (2 at the zero-likelihood site)."""
    s = plain
    s.batch.set_weights(None)
    dwell, rootp, trans, status = s.model.expected_history_statistics(
        s.batch, recompute_transitions=True, return_status=True)
    want = expectation_reference(s.model, s.case, check_sites=[0, 17])
    bad = np.zeros(sw.NSITES, dtype=np.int32)
    bad[s.case.zero_site] = 2
    np.testing.assert_array_equal(status, bad)
    scale = np.abs(want[0]).max()
    gap = max(np.abs(dwell - want[0]).max(), np.abs(trans - want[2]).max()) / scale
    print('%s: max |value - ref| / scale %.2e (scale %.3g; bound 1e-9 relative, 1e-13 of the '
          'scale absolute)' % (label_of(s, 'expectations'), gap, scale))
    np.testing.assert_allclose(dwell, want[0], rtol=1e-9, atol=1e-13 * scale)
    np.testing.assert_allclose(rootp, want[1], rtol=1e-9, atol=1e-15)
    np.testing.assert_allclose(trans, want[2], rtol=1e-9, atol=1e-13 * scale)
    assert dwell[s.n - 1] > 0 and trans[s.n - 1].any()       # the last state is lived in and left


def test_plain_branch_expectations(plain):
    """test_branch_expect_gpu.py::test_against_the_host_reference: check_values (rtol 1e-9, atol
    1e-13 of the scale) on the values and the weighted edge sums, the status, the zeros."""
    s = plain
    got = keep(s, 'branch', read_branch(s))
    want, wstatus = sw.branch_ref(s.model, s.case)
    np.testing.assert_array_equal(got.status, wstatus)
    live_and_pinned(got.status, s.case.zero_site)
    assert got.values.shape == (sw.NSITES, s.ta.nnodes, 2)
    assert not got.values[:, 0].any() and not got.values[s.case.zero_site].any()
    t_branch.check_values(got.values, want, label_of(s, 'branch') + ' values')
    t_branch.check_values(got.edge_sums, np.einsum('i,ivk->vk', W, want),
                          label_of(s, 'branch') + ' edge sums')


def test_plain_branch_length_gradient(plain):
    """test_branch_expect_gpu.py::test_branch_length_gradient, the direct hold of the device's
    analytic gradient to the host's (rtol 1e-9, atol 1e-13 of the largest entry), on the case
    under its first rate matrix alone (the call wants one Q for all edges) and with the branch
    lengths of _state_sweep_cases.gradient_case, which says why."""
    from raoteh_amd import device
    s = plain
    one, t = sw.gradient_case(s.n)
    model = device.TreeModel(one.T, one.root, s.n, ctx=s.ctx)
    model.set_rates(Q=one.Qs, node_q=one.node_q, t=t)
    model.set_root_distn(one.root_distn)
    batch = model.upload_sites(one.obs_nodes, one.data, kind=one.kind)
    try:
        assert np.array_equal(model.branch_lengths()[1:], t[1:])
        grad = model.branch_length_gradient(batch)
        analytic, status = sw.gradient_ref(s.n)
        live_and_pinned(status, one.zero_site)
        scale = np.abs(analytic).max()
        print('%s: max |value - ref| / scale %.2e (scale %.3g)'
              % (label_of(s, 'gradient'), np.abs(grad - analytic).max() / scale, scale))
        assert grad.shape == analytic.shape and grad[0] == 0.0
        np.testing.assert_allclose(grad, analytic, rtol=1e-9, atol=1e-13 * scale)
    finally:
        batch.close()
        model.close()


def test_plain_branch_profiles(plain):
    """test_branch_profiles_gpu.py::test_against_the_host_reference: check_profile (1e-10 of
    max(1, |log L|) per site and of the weighted sum)."""
    s = plain
    s.batch.set_weights(W)
    grid = sw.grid_of(s.model)
    got = s.model.branch_profiles(s.batch, lengths=grid, per_site=True)
    want, wstatus, loglik = sw.profile_ref(s.model, s.case)
    live_and_pinned(got.status, s.case.zero_site)
    assert got.values.shape == (sw.NSITES, s.ta.nnodes, 2) and got.sums.shape == (s.ta.nnodes, 2)
    assert got.lengths.tobytes() == grid.tobytes()
    assert not got.values[:, 0].any() and not got.values[s.case.zero_site].any()
    assert not got.sums[0].any()
    t_profile.check_profile(got, want, wstatus, loglik, W, label_of(s, 'profile'))
    # (the first grid point is the resident length: 1e-12, the bound of
    # test_the_resident_length_gives_zero)
    assert np.abs(got.values[:, :, 0]).max() <= 1e-12


def test_plain_nni_scores(plain):
    """test_nni_gpu.py::test_against_the_host_reference: check_scores (the moves, the status and
    -inf exactly; 1e-10 of max(1, |log L|) per site and of the weighted sum)."""
    s = plain
    got = keep(s, 'nni', read_nni(s))
    wmoves, want, wstatus, loglik = sw.nni_ref(s.model, s.case)
    live_and_pinned(got.status, s.case.zero_site)
    assert len(wmoves) >= 2 and not got.values[s.case.zero_site].any()
    t_nni.check_scores(got, wmoves, want, wstatus, loglik, W, label_of(s, 'nni'))


def test_plain_spr_scores(plain):
    """test_spr_gpu.py::test_against_the_host_reference: check_scores; every move up to 64 states,
    radius 1 above."""
    s = plain
    s.batch.set_weights(W)
    radius = sw.radius_of(s.n)
    got = s.model.spr_scores(s.batch, radius=radius, fractions=sw.FRACTIONS, per_site=True)
    wmoves, want, wstatus, loglik = sw.spr_ref(s.model, s.case)
    live_and_pinned(got.status, s.case.zero_site)
    assert len(wmoves) >= 4 and got.fractions.tolist() == list(sw.FRACTIONS)
    t_spr.check_scores(got, wmoves, want, wstatus, loglik, W, label_of(s, 'spr'))


@pytest.mark.parametrize('qkind', ['dense', 'state'])
def test_plain_placements(plain, qkind):
    """test_place_gpu.py::test_against_the_host_reference: check_placements; a dense query with
    exact zeros and a state query with state n - 1 at the pinned sites and an unobserved entry."""
    s = plain
    got = keep(s, 'place-' + qkind, read_place(s, qkind))
    want, wstatus, loglik = place_reference_of(s)
    live_and_pinned(got.status, s.case.zero_site)
    row = slice(0, 1) if qkind == 'dense' else slice(1, 2)
    assert np.isfinite(want[wstatus == 0][:, row]).any()
    t_place.check_placements(got, want[:, row], wstatus, loglik, W,
                             label_of(s, 'place') + ', %s query' % qkind)


def test_plain_map_states(plain):
    """test_map_states_gpu.py: check_optimal with the device's own P (test_optimal_on_real_models),
    and the states exactly those of map_reference's recursion and tie rule (test_exact_cases)."""
    s = plain
    got = s.model.map_states(s.batch)
    assert got.nodes == list(s.ta.preorder_nodes)
    want, live = t_map.check_optimal(s.model, got, s.case.obs_nodes, s.case.obs_lik,
                                     s.case.root_distn, label_of(s, 'map_states'))
    live_and_pinned(got.status, s.case.zero_site)
    states, log_joint, tied = sw.map_ref(s.model, s.case)
    assert not tied[live].any()
    wrong = np.nonzero((got.states != states).any(axis=1))[0]
    assert not len(wrong), (wrong.tolist(), got.states[wrong[0]].tolist(),
                            states[wrong[0]].tolist())
    for site, col, state in sw.pins_of(s.case):
        assert got.states[site, s.ta.node_to_index[s.case.obs_nodes[col]]] == state


def test_plain_sample_states(plain):
    """test_sample_states_gpu.py::sample_and_replay: the replay of _sample_cases (every pick of
    every draw inside the interval of its uniform number, eps 1e-10 of the total), the status."""
    s = plain
    got = s.model.sample_states(s.batch, ndraws=NDRAWS, seed=SAMPLE_SEED, first_draw=SAMPLE_FIRST)
    N = s.ta.nnodes
    assert got.states.shape == (NDRAWS, sw.NSITES, N) and got.nodes == list(s.ta.preorder_nodes)
    live_and_pinned(got.status, s.case.zero_site)
    esd = s.model.get_transitions()                            # the device's own P
    _, _, L = sw.sample_ref(s.model, s.case, SAMPLE_SEED, SAMPLE_FIRST, 1)
    checked = sc.replay_check(got.states, got.status, esd, L, s.case.root_distn, s.ta.parent,
                              SAMPLE_SEED, SAMPLE_FIRST)
    assert checked == NDRAWS * (sw.NSITES - 1) * N
    assert (got.states[:, s.case.zero_site] == 255).all()
    for site, col, state in sw.pins_of(s.case):
        assert (got.states[:, site, s.ta.node_to_index[s.case.obs_nodes[col]]] == state).all()


def test_plain_sample_mappings(plain):
    """test_sample_mappings_gpu.py: the states are those of sample_states
    (test_states_are_those_of_sample_states), the counts exactly and the values to rtol 1e-9 those
    of the mirror of _mapping_cases (check_parity), under per-edge rate matrices."""
    s = plain
    coefs = mpc.parity_coefs(s.n, 12000 + s.n)
    got = s.model.sample_mappings(s.batch, coefs, ndraws=NDRAWS, seed=SAMPLE_SEED,
                                  first_draw=SAMPLE_FIRST)
    want = s.model.sample_states(s.batch, ndraws=NDRAWS, seed=SAMPLE_SEED, first_draw=SAMPLE_FIRST)
    assert np.array_equal(got.states, want.states)
    assert np.array_equal(got.status & 1, want.status & 1)
    live_and_pinned(got.status & 1, s.case.zero_site)
    rates = (s.case.Qs, s.case.node_q, s.ta.branch_lengths())
    mir = t_mappings.check_parity(s.model, got, rates, coefs, SAMPLE_SEED, SAMPLE_FIRST)
    assert mir['picks'] >= NDRAWS * (sw.NSITES - 1)
    assert got.counts[..., 1].max() >= 1


# ---- 2. the mixture forms --------------------------------------------------------------------

def rows_of(ref, r):
    """The reference of one query of a placement reference."""
    kw = dict(values=ref.values[:, r:r + 1], sums=ref.sums[r:r + 1])
    if hasattr(ref, 'set_sums'):
        kw['set_sums'] = ref.set_sums[:, r:r + 1]
    return ref._replace(**kw)


def test_mix_branch_profiles(mix):
    """test_mixture_search_gpu.py::test_profiles_against_the_host_reference: check_against."""
    s = mix
    s.batch.set_weights(W)
    got = s.model.branch_profiles_mixture(s.batch, s.c, s.factors, per_site=True)
    ref = sw.mix_refs(s.case, 'profile')
    live_and_pinned(got.status)
    t_mix_search.check_against(got.values, got.sums, got.loglik, got.status, ref, W,
                               label_of(s, 'profile'))


def test_mix_nni_scores(mix):
    """test_mixture_search_gpu.py::test_nni_scores_against_the_host_reference: check_against."""
    s = mix
    got = keep(s, 'nni', read_nni(s))
    ref = sw.mix_refs(s.case, 'nni')
    live_and_pinned(got.status)
    assert np.array_equal(got.moves, ref.moves) and len(ref.moves) > 0
    t_mix_search.check_against(got.values, got.sums, got.loglik, got.status, ref, W,
                               label_of(s, 'nni'))


def test_mix_spr_scores(mix):
    """test_mixture_search2_gpu.py::test_spr_scores_against_the_host_reference: check_against."""
    s = mix
    s.batch.set_weights(W)
    got = s.model.spr_scores_mixture(s.batch, s.c, radius=sw.radius_of(s.n),
                                     fractions=sw.FRACTIONS, per_site=True)
    ref = sw.mix_refs(s.case, 'spr')
    live_and_pinned(got.status)
    assert np.array_equal(got.moves, ref.moves) and len(ref.moves) > 0
    t_mix_search2.check_against(got.values, got.sums, got.loglik, got.status, ref, W,
                                label_of(s, 'spr'))


@pytest.mark.parametrize('qkind', ['dense', 'state'])
def test_mix_placements(mix, qkind):
    """test_mixture_search2_gpu.py::test_placements_against_the_host_reference: check_against."""
    s = mix
    got = keep(s, 'place-' + qkind, read_place(s, qkind))
    ref = rows_of(place_reference_of(s), 0 if qkind == 'dense' else 1)
    live_and_pinned(got.status)
    assert (got.values[:, :, 0] == 0).all() and (got.sums[:, 0] == 0).all()
    t_mix_search2.check_against(got.values, got.sums, got.loglik, got.status, ref, W,
                                label_of(s, 'place') + ', %s query' % qkind)


def test_mix_branch_expectations(mix):
    """test_mixture_expect_gpu.py::test_against_the_host_reference: check_values (rtol 1e-9, atol
    1e-13 of the scale) on every output, the status, the zero set's posteriors."""
    s = mix
    got = keep(s, 'branch', read_branch(s))
    want = sw.mix_refs(s.case, 'branch')
    np.testing.assert_array_equal(got.status, want.status)
    live_and_pinned(got.status)
    assert not got.values[:, 0].any()
    dead = ~(want.L[sw.K_MIX - 1] > 0)                     # under the zero set, P = I
    assert dead.any() and not got.class_posteriors[dead, sw.K_MIX - 1].any()
    assert not got.class_posteriors[:, 1].any()            # the set of weight zero
    label = label_of(s, 'branch')
    t_mix_branch.check_values(got.values, want.values, label + ' values')
    t_mix_branch.check_values(got.set_edge_sums, want.set_edge_sums, label + ' per-set sums')
    t_mix_branch.check_values(got.edge_sums, want.edge_sums, label + ' edge sums')
    t_mix_branch.check_values(got.class_posteriors, want.post, label + ' posteriors')
    t_mix_branch.check_values(got.class_sums, want.class_sums, label + ' class sums')
    t_mix_branch.check_values(got.log_likelihoods, want.loglik, label + ' log-likelihoods')


def test_mix_branch_length_gradient(mix):
    """test_mixture_expect_gpu.py::test_gradients_against_the_host_reference: check_values on g_t
    and g_c, with one rate matrix per set (the call wants that)."""
    s = mix
    one = s.case._replace(Q=s.case.Q[:, :1].copy(), node_q=np.zeros_like(s.case.node_q))
    model, batch = build('mix', s.ctx, one)
    try:
        batch.set_weights(W)
        g_t, g_c, total = model.branch_length_gradient_mixture(batch, s.c)
        ref = sw.mix_refs(s.case, 'gradient')
        want_t = np.zeros_like(one.t)
        want_t[:, 1:] = ref.set_edge_sums[:, 1:, 0] / one.t[:, 1:]
        want_c = np.where(s.c > 0, ref.class_sums / np.where(s.c > 0, s.c, 1.0), 0.0)
        label = label_of(s, 'gradient')
        t_mix_branch.check_values(g_t, want_t, label + ' g_t')
        t_mix_branch.check_values(g_c, want_c, label + ' g_c')
        live = ref.status == 0
        assert abs(total - np.dot(W[live], ref.loglik[live])) <= 1e-10 * abs(total)
    finally:
        batch.close()
        model.close()


# ---- 3. the partitioned forms ----------------------------------------------------------------

def test_part_step_partitioned_totals(part):
    """test_partition_gpu.py: the log-likelihoods of step_partitioned against the oracle, each
    site under its own set (RTOL_LL = 1e-10, test_log_likelihoods); the per-set totals against
    numpy sums of the per-site values (1e-12 relative) and the counts exactly
    (test_totals_weights_and_repeatability)."""
    s = part
    s.batch.set_weights(W)
    s.model.step_partitioned(s.batch)
    ll, st = s.model.fetch_log_likelihoods(s.batch)
    want, wst = sw.part_refs(s.case, 'totals')
    assert np.array_equal(st & 1, wst)
    live_and_pinned(st & 1)
    live = wst == 0
    err = np.max(np.abs(ll[live] - want[live]) / np.abs(want[live]))
    print('%s: max rel err %.2e (bound 1e-10)' % (label_of(s, 'totals'), err))
    assert err < 1e-10 and np.isneginf(ll[~live]).all()
    ptot, ws = s.model.fetch_partition_totals(s.batch, weighted=True)
    assert ptot.shape == (sw.NSETS, 3) and ws.shape == (sw.NSETS,)
    for k in range(sw.NSETS):
        mine = s.case.site_sets == k
        assert ptot[k, 1] == (mine & ~live).sum() and ptot[k, 2] == mine.sum()
        for got, ref in ((ptot[k, 0], ll[mine & live].sum()),
                         (ws[k], np.dot(W[mine & live], ll[mine & live]))):
            assert abs(got - ref) <= 1e-12 * abs(ref)


def test_part_branch_profiles(part):
    """test_partition_search_gpu.py::test_profiles_against_the_host_reference: check_against."""
    s = part
    s.batch.set_weights(W)
    got = s.model.branch_profiles_partitioned(s.batch, s.factors, per_site=True)
    live_and_pinned(got.status)
    assert not got.values[:, 0].any() and not got.sums[0].any()
    t_part_search.check_against(got, sw.part_refs(s.case, 'profile'), s.case, W,
                                label_of(s, 'profile'))


def test_part_nni_scores(part):
    """test_partition_search_gpu.py::test_nni_scores_against_the_host_reference: check_against."""
    s = part
    got = keep(s, 'nni', read_nni(s))
    ref = sw.part_refs(s.case, 'nni')
    live_and_pinned(got.status)
    np.testing.assert_array_equal(got.moves, ref.moves)
    t_part_search.check_against(got, ref, s.case, W, label_of(s, 'nni'))


def test_part_spr_scores(part):
    """test_partition_search2_gpu.py::test_spr_scores_against_the_host_reference: check_against."""
    s = part
    s.batch.set_weights(W)
    got = s.model.spr_scores_partitioned(s.batch, radius=sw.radius_of(s.n),
                                         fractions=sw.FRACTIONS, per_site=True)
    ref = sw.part_refs(s.case, 'spr')
    live_and_pinned(got.status)
    np.testing.assert_array_equal(got.moves, ref.moves)
    t_part_search2.check_against(got, ref, s.case, W, label_of(s, 'spr'))


@pytest.mark.parametrize('qkind', ['dense', 'state'])
def test_part_placements(part, qkind):
    """test_partition_search2_gpu.py::test_placements_against_the_host_reference: check_against."""
    s = part
    got = keep(s, 'place-' + qkind, read_place(s, qkind))
    ref = rows_of(place_reference_of(s), 0 if qkind == 'dense' else 1)
    live_and_pinned(got.status)
    assert not got.values[:, :, 0].any() and not got.sums[:, 0].any()
    t_part_search2.check_against(got, ref, s.case, W, label_of(s, 'place') + ', %s query' % qkind)


def test_part_branch_expectations(part):
    """test_partition_reads_gpu.py::test_against_the_host_reference: check_values on the values,
    the per-set sums and the edge sums; the status."""
    s = part
    got = keep(s, 'branch', read_branch(s))
    want, wstatus, want_sets, want_sums = sw.part_refs(s.case, 'branch')
    np.testing.assert_array_equal(got.status, wstatus)
    live_and_pinned(got.status)
    assert not got.values[:, 0].any()
    label = label_of(s, 'branch')
    t_part_branch.check_values(got.values, want, label + ' values')
    t_part_branch.check_values(got.set_edge_sums, want_sets, label + ' per-set sums')
    t_part_branch.check_values(got.edge_sums, want_sums, label + ' edge sums')


def test_part_branch_length_gradient(part):
    """test_partition_reads_gpu.py::test_branch_length_gradient_partitioned, the direct hold of
    the device's analytic gradient to the host's (rtol 1e-9, atol 1e-13 of the largest entry), with
    one rate matrix per set."""
    s = part
    one = s.case._replace(Q=s.case.Q[:, :1].copy(), node_q=np.zeros_like(s.case.node_q))
    model, batch = build('part', s.ctx, one)
    try:
        batch.set_weights(W)
        grad = model.branch_length_gradient_partitioned(batch)
        _, status, set_sums, _ = sw.part_refs(s.case, 'gradient')
        analytic = np.zeros((sw.NSETS, s.ta.nnodes))
        analytic[:, 1:] = set_sums[:, 1:, 0] / one.t[:, 1:]
        scale = np.abs(analytic).max()
        print('%s: max |value - ref| / scale %.2e (scale %.3g)'
              % (label_of(s, 'gradient'), np.abs(grad - analytic).max() / scale, scale))
        assert grad.shape == analytic.shape and not grad[:, 0].any()
        np.testing.assert_allclose(grad, analytic, rtol=1e-9, atol=1e-13 * scale)
    finally:
        batch.close()
        model.close()


# ---- 4. the tree-specialised pruning kernel --------------------------------------------------

@pytest.mark.parametrize('n', sw.SPOT, ids=nid)
def test_reads_after_the_tree_specialised_kernel_give_the_same_bits(n):
    """jit = 1: the batch runs the tree-specialised pruning kernel, and posteriors, NNI scores and
    placements take their L and M from that upward pass -- the bits of the jit = 0 contexts."""
    s = open_state('plain', n, {'jit': 1})
    try:
        ll, st = s.model.log_likelihoods(s.batch)
        assert s.batch.kernel_name.startswith('prune_tree_jit'), s.batch.kernel_name
        live_and_pinned(st & 1, s.case.zero_site)
        for read in SPOTTED:
            got = READS[read](s)
            assert_same_bits(got, fresh_bits('plain', n, read), 'jit = 1, n = %d, %s' % (n, read))
    finally:
        close_state(s)


# ---- 5. a larger n's data behind a smaller n's rows ------------------------------------------

@pytest.mark.parametrize('form', ['plain', 'mix', 'part'])
def test_a_descending_walk_in_one_context_gives_the_bits_of_fresh_contexts(form):
    """One context, n from 128 down to 6: the context's scratch and the LDS of a resident
    workgroup hold the larger n's data behind the smaller n's rows, where the kernels assume
    zeros.  NNI scores, placements and branch expectations at every n, bit for bit those of the
    fresh contexts above."""
    ctx = open_context()
    try:
        for n in sorted(sw.FORMS, reverse=True):
            s = open_state(form, n, ctx=ctx)
            try:
                for read in WALKED:
                    assert_same_bits(READS[read](s), fresh_bits(form, n, read),
                                     'walk %s, n = %d, %s' % (form, n, read))
            finally:
                close_state(s)
    finally:
        ctx.close()
