"""The cases and checks of test_forest_states_gpu.py, the part that needs no device: the cases
cover what they should, the numpy sampler that states the kernels' rule passes the replay check
exactly and follows the exact posterior, and the checks reject kernels that are subtly wrong."""
import numpy as np
import pytest

from _forest_states_cases import (BIG_NODES, BIG_STATES, FAMILY_LIMITS, FOREST_CAP, NTREES, STATES,
                                  ForestCheckError, case, check_pmap, check_sets, family_of,
                                  forest_replay_check, numpy_forest_sample, offsets_of, pmap_rtol,
                                  rule_pick)
from _forest_wide_cases import chi_square

SWEEPS = (0, 7)
SEED = 5


def test_state_counts_cover_every_kernel_form():
    """Each form of the one-word kernels gets at least three state counts, its largest among
    them; the wave-per-tree form runs on both sides of lane 32, at 61, 63 and 64."""
    assert FAMILY_LIMITS == (4, 8, 16, 64)
    by_family = {}
    for n in STATES:
        by_family.setdefault(family_of(n), []).append(n)
    assert sorted(by_family) == list(FAMILY_LIMITS)
    for limit, counts in by_family.items():
        assert len(counts) >= 3 and limit in counts, (limit, counts)
    lo = dict((limit, min(counts)) for limit, counts in by_family.items())
    assert lo[8] == 5 and lo[16] == 9 and lo[64] == 17           # the thin tails
    assert {31, 32, 33, 61, 63, 64} <= set(by_family[64])
    assert set(BIG_STATES) <= set(STATES)
    assert sorted(set(family_of(n) for n in BIG_STATES)) == list(FAMILY_LIMITS)
    assert BIG_NODES > FOREST_CAP


@pytest.mark.parametrize('n', STATES)
def test_case_covers_what_it_should(n):
    c = case(n)
    big = n in BIG_STATES
    assert len(c.trees) == NTREES + big and NTREES % 16 and NTREES % 8 and NTREES % 4
    sizes = [r.N for r in c.refs]
    assert sizes[:3] == [1, 2, 3]
    assert all(2 <= s <= 13 for s in sizes[3:NTREES]) and len(set(sizes[:NTREES])) >= 8
    assert offsets_of(c.refs)[-1] <= 1500
    # P = I + Q / omega: stochastic, sparse, the cycle in its support; one zero in the prior
    np.testing.assert_allclose(c.P.sum(axis=1), 1.0, rtol=1e-12)
    assert (c.P >= 0).all() and (c.P[np.arange(n), (np.arange(n) + 1) % n] > 0).all()
    assert n < 16 or (c.P == 0).sum() > n * n // 2
    assert n <= 3 or (c.P == 0).any()
    assert c.width == (c.P != 0).sum(axis=1).max() and 2 <= c.width <= n
    assert (c.root == 0).sum() == 1 and (c.root >= 0).all() and c.root[n - 1] > 0
    # about a third of the nodes restricted, every kind of restriction
    small = sum(sizes[:NTREES])
    restricted = sum(len(d) for d in c.obs[:NTREES])
    assert 0.2 * small <= restricted <= 0.5 * small
    kinds = set(min(len(ss), 3) for d in c.obs for ss in d.values())
    assert kinds == ({1, 2} if n < 6 else {1, 2, 3})
    if n >= 34:
        assert any({31, 32} <= ss for d in c.obs for ss in d.values())
    # at least 30 feasible trees, state n - 1 live in at least 20 trees
    live = [r.live for r in c.refs[:NTREES]]
    assert sum(live) >= 30, sum(live)
    assert sum(bool(r.sets[:, n - 1].any()) for r in c.refs[:NTREES]) >= 20
    for r in c.refs:
        assert not r.live or r.sets.any(axis=1).all()
    if big:
        r = c.refs[-1]
        assert r.N == BIG_NODES and r.live and len(c.obs[-1]) == 10
        assert not r.sets.all() and (r.sets != r.allowed).any()


def test_every_family_has_a_zero_likelihood_tree():
    zero = dict((limit, 0) for limit in FAMILY_LIMITS)
    for n in STATES:
        zero[family_of(n)] += sum(not r.live for r in case(n).refs)
    assert min(zero.values()) >= 1, zero


@pytest.mark.parametrize('n', STATES)
def test_numpy_sampler_passes_the_replay_check_exactly(n):
    """eps = 0: the sampler's pick is the state the check asks for, to the last bit; with a
    root prior and with unit root weights; the zero-likelihood trees carry status 1 and -1."""
    c = case(n)
    total = offsets_of(c.refs)[-1]
    for root in (c.root, None):
        seen = None
        for sweep in SWEEPS:
            states, status = numpy_forest_sample(c.P, c.refs, root, n, SEED, sweep)
            checked = forest_replay_check(states, status, c.P, c.refs, root, n, SEED, sweep, eps=0.0)
            live = np.array([r.live for r in c.refs])
            if root is not None:
                np.testing.assert_array_equal(status, np.where(live, 0, 1))
                assert checked == sum(r.N for r in c.refs if r.live)
            assert checked <= total
            for k, r in enumerate(c.refs):                       # inside the oracle's sets
                st = states[offsets_of(c.refs)[k]:offsets_of(c.refs)[k + 1]]
                if status[k] == 0:
                    assert r.sets[np.arange(r.N), st].all()
            assert seen is None or not np.array_equal(seen, states)
            seen = states


@pytest.mark.parametrize('n', [17, 33, 61, 64])
def test_numpy_sampler_follows_the_exact_posterior(n):
    """Three feasible trees of six nodes or more, 4 000 copies of each in one forest: the node
    marginals of the numpy sampler against mc0_esd_get_node_to_distn with the pooled chi-square
    (cells expecting 8 or more on their own, the rest pooled; stat < dof + 6 sqrt(2 dof) + 10
    per node), and never a state outside the support.  Draws that pass the replay check at
    1e-10 are this sampler's draws, so the device needs no law test of its own."""
    c = case(n)
    reps = 4000
    chosen = [r for r in c.refs[:NTREES] if r.live and r.N >= 6][:3]
    assert len(chosen) == 3
    refs = [r for r in chosen for _ in range(reps)]
    states, status = numpy_forest_sample(c.P, refs, c.root, n, 99, 3)
    assert not status.any()
    off = offsets_of(refs)
    margin = np.inf
    for j, r in enumerate(chosen):
        st = np.stack([states[off[k]:off[k + 1]] for k in range(j * reps, (j + 1) * reps)])
        want = r.distn(c.root)
        for v in range(r.N):
            got = np.bincount(st[:, v], minlength=n)
            assert not got[want[v] == 0].any(), (j, v)
            law = dict(((s, 0), want[v, s]) for s in range(n) if want[v, s] > 0)
            stat, dof = chi_square(st[:, v], np.zeros(reps, dtype=np.int64), law, reps)
            bound = dof + 6.0 * np.sqrt(2.0 * dof) + 10.0
            assert stat < bound, (j, v, stat, dof)
            margin = min(margin, bound - stat)
    print('n = %d: smallest margin of the pooled chi-square %.1f' % (n, margin))


# ---------------------------------------------------------------------------
# sensitivity: what a subtly wrong kernel would return is rejected
# ---------------------------------------------------------------------------

def _rejected(n, **wrong):
    """The replay check of the GPU test (eps = 1e-10, the oracle's L) on the draws of a wrong
    sampler, at the sweeps the GPU test runs: the sweeps at which it is rejected."""
    c = case(n)
    out = []
    for sweep in SWEEPS:
        states, status = numpy_forest_sample(c.P, c.refs, c.root, n, SEED, sweep, **wrong)
        try:
            forest_replay_check(states, status, c.P, c.refs, c.root, n, SEED, sweep)
        except ForestCheckError:
            out.append(sweep)
    return out


@pytest.mark.parametrize('n', STATES)
def test_replay_check_rejects_wrong_samplers(n):
    def never_last(w):                                   # (a) state n - 1 is never picked
        w = w.copy()
        w[:, n - 1] = 0.0
        return w

    def next_lane(w, cdf, target):                       # (d) the cdf is off by one lane
        return np.minimum(rule_pick(w, cdf, target) + 1, n - 1)

    assert _rejected(n) == []
    assert _rejected(n, weights=never_last) == list(SWEEPS)
    assert _rejected(n, tree_counter=True) == list(SWEEPS)           # (c)
    assert _rejected(n, pick=next_lane) == list(SWEEPS)
    if n > 32:                                           # (b) the total stops at lane 31
        assert _rejected(n, total_of=lambda cdf: cdf[:, 31]) == list(SWEEPS)


def _device_like_passes(c, r, skip_last_child=False, drop_last_column=False):
    """The boolean passes and the ELL upward pass as csrc/forest.hip runs them, in numpy
    -> (uint64[N] sets, f64[N, n] pmap); the keywords break them."""
    n, nz = c.n, c.P != 0
    idx, ptr = r.ta.indices, r.ta.indptr
    S = r.allowed.copy()
    for v in range(r.N - 1, -1, -1):
        kids = idx[ptr[v]:ptr[v + 1]]
        for ch in (kids[:-1] if skip_last_child else kids):
            S[v] &= nz[:, S[ch]].any(axis=1)
    for v in range(r.N):
        for ch in idx[ptr[v]:ptr[v + 1]]:
            S[ch] &= nz[S[v], :].any(axis=0)
    col = np.tile(np.arange(n)[:, None], (1, c.width))
    val = np.zeros((n, c.width))
    for s in range(n):
        at = np.nonzero(nz[s])[0]
        col[s, :len(at)] = at
        val[s, :len(at)] = c.P[s, at]
    if drop_last_column:
        val[:, c.width - 1] = 0.0
    L = S.astype(float)
    for v in range(r.N - 1, 0, -1):
        L[r.parent[v]] *= (val * L[v][col]).sum(axis=1)
    masks = (S.astype(np.uint64) << np.arange(n, dtype=np.uint64)[None, :]).sum(axis=1)
    return masks.astype(np.uint64), L


@pytest.mark.parametrize('n', STATES)
def test_set_and_pmap_checks_reject_wrong_passes(n):
    """(e) a backward boolean pass that ignores the last child of every node fails the set
    check; (f) an upward pass that loses the last ELL column of each row fails the pmap check
    (and only that: its sets are right).  The same passes unbroken pass both."""
    c = case(n)

    def run(**wrong):
        parts = [_device_like_passes(c, r, **wrong) for r in c.refs]
        return np.concatenate([m for m, _ in parts]), np.concatenate([L for _, L in parts])

    masks, L = run()
    check_sets(masks, c.refs, n)
    check_pmap(L, c.refs, n, c.width)
    masks, _ = run(skip_last_child=True)
    if (c.P == 0).any():
        with pytest.raises(ForestCheckError):
            check_sets(masks, c.refs, n)
    else:
        # 2 and 3 states: the cycle and the diagonal fill P, and a full matrix leaves the boolean
        # passes nothing to remove from a non-empty set -- there is no wrong answer to give
        assert n <= 3
        check_sets(masks, c.refs, n)
    masks, L = run(drop_last_column=True)
    check_sets(masks, c.refs, n)
    with pytest.raises(ForestCheckError):
        check_pmap(L, c.refs, n, c.width)


def test_pmap_tolerance():
    """1e-12 for the small trees, about 9e-12 for the tree of 1 100 nodes at 61 states."""
    assert pmap_rtol(13, 64, 64) == 1e-12
    assert 8e-12 < pmap_rtol(BIG_NODES, case(61).width, 61) < 1e-11
