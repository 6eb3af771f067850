"""The state-count sweep without a GPU (tests/_state_sweep_cases.py): the lists of state counts
reach every KS, every NT and every tail; the pinned observations are in the data that is uploaded
and the references see them as live sites, at every n and in every form; every reference the GPU
module compares with runs on the host, and each of them loses the pinned sites when the pinned
state is made unobservable -- the sweep has teeth only if the references depend on the last row,
the last k-step and the first state of the last k-step."""
import numpy as np
import pytest

import _state_sweep_cases as sw

FORMS = ('plain', 'mix', 'part')
NS = {'plain': sw.PLAIN, 'mix': sw.FORMS, 'part': sw.FORMS}
ALL = [(form, n) for form in FORMS for n in NS[form]]
HOST = [(form, n) for form in FORMS for n in sw.HOST]


def ids(pairs):
    return ['%s-n%d' % p for p in pairs]


# ---- 1. the lists ----------------------------------------------------------------------------

def test_the_lists_reach_every_instance_and_every_tail():
    assert len(sw.ROTATING) == len(sw.THIN) == 31
    assert set(sw.PLAIN) == set(sw.ROTATING) | set(sw.THIN) | {6, 127} and len(sw.PLAIN) == 64
    assert set(sw.FORMS) == set(sw.ROTATING) | {6, 127}
    assert sw.ROTATING[0] == 7 and sw.ROTATING[-1] == 128
    assert not set(sw.ROTATING) & set(sw.THIN)
    for ns in (sw.ROTATING, sw.THIN):
        assert sorted(sw.ks_of(n) for n in ns) == list(range(2, 33))       # post_dispatch<2, 32>
        assert 5 <= min(ns) and max(ns) <= 128
    assert set(sw.nt_of(n) for n in sw.ROTATING) == set(range(1, 9))        # post_dispatch<1, 8>
    assert set(sw.ks_of(n) for n in sw.ROTATING if n <= 64) == set(range(2, 17))
    # every (NT, n % 4): a full last k-step and 3, 2, 1 live columns in it, per row-tile count
    # (NT = 1 has three KS only, 2..4: its fourth residue comes from n = 6, see EXTRA)
    every = set((nt, r) for nt in range(1, 9) for r in range(4))
    assert set((sw.nt_of(n), n % 4) for n in sw.ROTATING) == every - {(1, 2)}
    assert set((sw.nt_of(n), n % 4) for n in sw.FORMS) == every
    assert set((sw.nt_of(n), n % 4) for n in sw.PLAIN) == every
    # the last row tile: full, one row, and the residues between
    assert set(n % 16 for n in sw.ROTATING if n > 16) == {0, 3, 6, 9}
    assert set(n % 16 for n in sw.THIN if n > 16) == {1, 5, 11, 13}
    assert {1, 15} <= set(n % 16 for n in sw.PLAIN)                         # (15: 127, see EXTRA)
    assert 15 in set(n % 16 for n in sw.FORMS)
    # THIN: one live column in the last k-step, three where ROTATING has the one already
    for n, r in zip(sw.THIN, sw.ROTATING):
        assert sw.ks_of(n) == sw.ks_of(r) and n % 4 == (3 if r % 4 == 1 else 1)
    # the spot checks: NT = 1, 3, 6, 7, each a value of the sweep
    assert [sw.nt_of(n) for n in sw.SPOT] == [1, 3, 6, 7] and set(sw.HOST) <= set(sw.PLAIN)
    assert set(sw.HOST) <= set(sw.ROTATING)
    # the observation kinds rotate: each occurs in each list, on either side of 64 states
    for ns in (sw.ROTATING, sw.THIN):
        for part in ([n for n in ns if n <= 64], [n for n in ns if n > 64]):
            assert set(sw.kind_of(n) for n in part) == set(sw.KINDS)


def test_the_shapes_of_the_cases():
    """The plain tree: 9 nodes, a multifurcation, a single-child node, an observed internal node,
    two distinct rate matrices both in use; 33 sites; three sets over three granules."""
    for n in (7, 64, 128):
        case = sw.plain_case(n)
        ta = sw.tree_of(case)
        kids = np.diff(ta.indptr)
        assert ta.nnodes == 9 and kids.max() >= 3 and (kids == 1).any()
        assert any(kids[ta.node_to_index[v]] > 0 for v in case.obs_nodes)
        assert len(case.Qs) == 2 and set(case.node_q[1:]) == {0, 1}
        assert not np.array_equal(case.Qs[0], case.Qs[1])
        assert case.obs_lik.shape[0] == sw.NSITES == 33 and case.zero_site == 32
        mix = sw.mix_case(n)
        assert mix.Q.shape[:2] == (3, 2) and not mix.Q[2].any()             # (the zero set)
        c = sw.class_weights_of(n)
        assert c[1] == 0.0 and c[0] > 0 and c[2] > 0 and abs(c.sum() - 1.0) < 1e-15
        assert np.diff(sw.tree_of(mix).indptr).max() >= 3
        part = sw.part_case(n)
        assert part.nsets == 3 and np.bincount(part.site_sets).tolist() == [11, 11, 11]
        assert [int(part.site_sets[i]) for i in sw.PINNED_SITES] == [0, 2, 1]


# ---- 2. the pins, at every n and in every form -----------------------------------------------

def host_liveness(form, case):
    """(log-likelihoods or log Lambda, status) of every site from the form's own likelihood
    reference at the resident lengths."""
    if form == 'plain':
        return sw.loglik_ref(sw.HostModel(case), case)
    if form == 'part':
        return sw.part_refs(case, 'totals')
    import _mixture_cases as mc
    ta = sw.tree_of(case)
    L = np.array([mc.set_likelihoods(ta, case, k) for k in range(sw.K_MIX)])
    _, loglik, dead = mc.combine(L, sw.class_weights_of(case.n))
    return loglik, dead.astype(np.int32)


@pytest.mark.parametrize('form,n', ALL, ids=ids(ALL))
def test_pins_are_uploaded_and_live(form, n):
    case = sw.case_of(form, n)
    assert case.kind == sw.kind_of(n) and case.n == n
    up = sw.uploaded_likelihoods(case)
    assert up.shape == case.obs_lik.shape
    assert np.array_equal(up != 0, case.obs_lik != 0)          # the upload is the reference's data
    pins = sw.pins_of(case)
    assert [p[0] for p in pins] == list(sw.PINNED_SITES)
    assert len(set(p[1] for p in pins)) == 3                   # three different leaves
    assert [p[2] for p in pins] == [n - 1, n - 1, 4 * (sw.ks_of(n) - 1)]
    nodes = case.obs_nodes if form == 'plain' else case.leaves
    kids = np.diff(sw.tree_of(case).indptr)
    for site, col, state in pins:
        assert kids[sw.tree_of(case).node_to_index[nodes[col]]] == 0        # a leaf
        want = np.zeros(n)
        want[state] = 1.0
        assert np.array_equal(up[site, col], want)
        if case.kind == 'state':
            assert case.data[site, col] == state
    ll, status = host_liveness(form, case)
    for site in sw.PINNED_SITES:
        assert status[site] == 0 and np.isfinite(ll[site])
    if form == 'plain':
        assert status[case.zero_site] == 1 and status.sum() == 1


# ---- 3. every reference runs; 4. and depends on the pinned states -----------------------------

def plain_statuses(case, cheap=False):
    """{family: status} of every reference of the plain form, each from its own code path; the
    shapes and the finiteness of the full references are checked on the way unless `cheap`
    (then the branch reference gets no coefficient matrix: its status alone)."""
    from _branch_cases import branch_reference
    from _resident_cases import expectation_reference, posterior_reference
    model = sw.HostModel(case)
    n, S, N = case.n, sw.NSITES, model.tree.nnodes
    out = {}
    moves, values, out['nni'], ll = sw.nni_ref(model, case)
    assert values.shape == (S, len(moves), 2) and len(moves) >= 2 and not np.isnan(values).any()
    values, out['profile'], _ = sw.profile_ref(model, case)
    assert values.shape == (S, N, 2) and not np.isnan(values).any()
    moves, values, out['spr'], _ = sw.spr_ref(model, case)
    assert values.shape == (S, len(moves), 2) and len(moves) >= 4 and not np.isnan(values).any()
    values, out['place'], _ = sw.place_ref(model, case)
    assert values.shape == (S, 2, N, 2, 1) and not np.isnan(values).any()
    if cheap:
        out['branch'] = branch_reference(model, case, np.zeros((0, n, n)))[1]
    else:
        values, out['branch'] = sw.branch_ref(model, case)
        assert values.shape == (S, N, 2) and np.isfinite(values).all()
        analytic, out['gradient'] = sw.gradient_ref(n)
        assert analytic.shape == (N,) and np.isfinite(analytic).all() and analytic[1:].all()
        dwell, rootp, trans = expectation_reference(model, case)
        assert dwell.shape == (n,) and trans.shape == (n, n)
        assert np.isfinite(dwell).all() and np.isfinite(trans).all()
        assert abs(rootp.sum() - (S - 1)) < 1e-9               # one posterior per live site
    nv, ev, D, out['posteriors'] = posterior_reference(
        model, case, [[0, n - 1]], [([n - 1], list(range(n)))], [0, 17])
    assert D.shape == (S, N, n) and np.isfinite(D).all()
    states, log_joint, _ = sw.map_ref(model, case)
    out['map'] = np.where(np.isfinite(log_joint), 0, 1)
    assert states.shape == (S, N) and (states[out['map'] == 0] < n).all()
    states, out['sample'], _ = sw.sample_ref(model, case, 3, 0, 2)
    assert states.shape == (2, S, N)
    if not cheap:
        import _mapping_cases as mpc
        live = out['sample'] == 0
        mir = mpc.numpy_mappings(case.Qs, model.branch_lengths(), case.node_q, model.tree.parent,
                                 states[:, live], mpc.parity_coefs(n, 5), 3, 0)
        assert mir['values'].shape == (2, live.sum(), N, 3) and np.isfinite(mir['values']).all()
    return out


def form_statuses(form, case, cheap=False):
    refs = sw.mix_refs if form == 'mix' else sw.part_refs
    out = {}
    for family in ('profile', 'nni', 'spr', 'place'):
        ref = refs(case, family)
        assert ref.values.shape[0] == sw.NSITES and not np.isnan(ref.values).any()
        assert ref.sums.shape == ref.values.shape[1:]
        out[family] = ref.status
    if form == 'part':
        out['totals'] = refs(case, 'totals')[1]
    if cheap:
        ta, none = sw.tree_of(case), np.zeros((0, case.n, case.n))
        if form == 'mix':
            import _mixture_cases as mc
            out['branch'] = mc.mixture_reference(ta, case, none, sw.class_weights_of(case.n),
                                                 check=0).status
        else:
            import _partition_read_cases as prc
            out['branch'] = prc.partition_reference(ta, case, none, check=0)[1]
        return out
    for family in ('branch', 'gradient'):
        ref = refs(case, family)
        values, status = (ref.values, ref.status) if form == 'mix' else ref[:2]
        assert values.shape[0] == sw.NSITES and np.isfinite(values).all()
        out[family] = status
    return out


def statuses(form, case, cheap=False):
    return plain_statuses(case, cheap) if form == 'plain' else form_statuses(form, case, cheap)


@pytest.mark.parametrize('form,n', HOST, ids=ids(HOST))
def test_every_reference_runs_and_keeps_the_pinned_sites(form, n):
    out = statuses(form, sw.case_of(form, n))
    assert len(out) >= 6
    for family, status in out.items():
        assert status.shape == (sw.NSITES,), family
        assert not status[list(sw.PINNED_SITES)].any(), family


@pytest.mark.parametrize('form,n', HOST, ids=ids(HOST))
def test_every_reference_loses_a_pinned_site_with_its_state(form, n):
    """State n - 1 unobservable: the sites 0 and 17 turn zero-likelihood in every reference; the
    first state of the last k-step unobservable: site 1 turns (at n % 4 == 1 the two are one
    state).  (What the other sites do is not asserted: another leaf of theirs may observe the
    state too.)"""
    case = sw.case_of(form, n)
    first = 4 * (sw.ks_of(n) - 1)
    assert (first == n - 1) == (n % 4 == 1)
    before = statuses(form, case, cheap=True)
    for family, status in statuses(form, sw.without_state(case, n - 1), cheap=True).items():
        assert before[family][0] == 0 and before[family][17] == 0, family
        assert status[0] != 0 and status[17] != 0, family
    for family, status in statuses(form, sw.without_state(case, first), cheap=True).items():
        assert before[family][1] == 0 and status[1] != 0, family
