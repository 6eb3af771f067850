"""tests/golden/forest_wide.json (tools/gen_golden_forest_wide.py) decoded once for the CPU and
the GPU tests of the Rao-Teh passes at 65 to 128 states, and the helpers those tests share with
the tests of the one-word kernels (test_forest_states_*.py): the sparse uniformized matrix, the
pooled chi-square, the closed-form law on a lumped cycle and the consistency of device-resident
histories."""
import functools
from math import exp, factorial

import networkx as nx
import numpy as np

from conftest import load_golden


def dense(entries, n):
    M = np.zeros((n, n))
    for i, j, x in entries:
        M[i, j] = x
    return M


def rows(d, v, n):
    """A node's sparse [state, value] list -> f64[n]."""
    out = np.zeros(n)
    for s, x in d[str(v)]:
        out[s] = x
    return out


@functools.lru_cache(maxsize=None)
def forest_wide_cases():
    """-> list of (case dict with dense 'P' and 'Q' and 'omega', chunk tree)."""
    fx = load_golden('forest_wide')
    assert 'gen_golden_forest_wide.py' in fx['provenance']
    out = []
    for c in fx['cases']:
        c = dict(c)
        n = c['nstates']
        m = fx['matrices'][c['matrix']]
        assert m['nstates'] == n
        c['P'], c['Q'], c['omega'] = dense(m['P'], n), dense(m['Q'], n), m['omega']
        # the file lists the restricted chunk nodes only
        c['allowed'] = dict((str(v), c['allowed'].get(str(v), list(range(n))))
                            for v in c['chunk_nodes'])
        T = nx.Graph()
        T.add_nodes_from(c['chunk_nodes'])
        T.add_edges_from((a, b) for a, b in c['chunk_edges'])
        out.append((c, T))
    return out


def lumped_cycle(n):
    """n = 4 R states s = 4 r + c: rate 1 / R from (c, r) to (c + 1 mod 4, r') for every r'.
    Lumps exactly onto the unit-rate 4-cycle on c = s % 4; every transition changes c."""
    assert n % 4 == 0
    R = n // 4
    Q = np.zeros((n, n))
    s = np.arange(n)
    Q[(s[None, :] % 4) == ((s[:, None] + 1) % 4)] = 1.0 / R
    Q -= np.diag(Q.sum(axis=1))
    return Q


def sparse_uniformized(rng, n, extras=3.0):
    """P = I + Q / omega of a sparse random rate matrix whose support holds a cycle."""
    Q = np.zeros((n, n))
    for i in range(n):
        Q[i, (i + 1) % n] = rng.exponential() + 0.1
    Q += (rng.uniform(size=(n, n)) < extras / n) * rng.exponential(size=(n, n))
    np.fill_diagonal(Q, 0.0)
    Q -= np.diag(Q.sum(axis=1))
    return Q, np.identity(n) + Q / (2.0 * (-np.diag(Q)).max())


def cycle_law(ta, tb, kmax=40):
    law = {}
    for s in range(4):
        for ka in range((-s) % 4, kmax, 4):
            for kb in range((-s) % 4, kmax, 4):
                w = 0.25 * exp(-ta) * ta ** ka / factorial(ka) * exp(-tb) * tb ** kb / factorial(kb)
                law[(s, ka + kb)] = law.get((s, ka + kb), 0.0) + w
    z = sum(law.values())
    return dict((k, v / z) for k, v in law.items())


def chi_square(root, total, law, C):
    """Pooled chi-square of C observations (root[i], total[i]) against law {(a, b): p}: cells
    with an expected count of at least 8 enter on their own, the rest (and every observation
    outside the law's support) as one pooled cell if that expects at least 8.
    -> (statistic, degrees of freedom)."""
    cells = sorted(law, key=lambda k: -law[k])
    stat, dof, rest_e, rest_o = 0.0, -1, 0.0, 0
    seen = 0
    for key in cells:
        e = law[key] * C
        o = int(((root == key[0]) & (total == key[1])).sum())
        seen += o
        if e >= 8.0:
            stat += (o - e) ** 2 / e
            dof += 1
        else:
            rest_e += e
            rest_o += o
    rest_o += C - seen
    if rest_e >= 8.0:
        stat += (rest_o - rest_e) ** 2 / rest_e
        dof += 1
    return stat, dof


def check_lumped_cycle_law(ctx, where, n, lengths, factor, sweeps):
    """n = 4 R states s = 4 r + c with rate 1 / R from (c, r) to (c + 1 mod 4, r') for every r':
    the class c = s % 4 is the unit-rate 4-cycle of
    test_rao_teh_stationary_law_on_a_pure_cycle_is_exact and every transition changes it.  On
    the 3-node tree with both leaves allowed {s : s % 4 == 0} (R states) and a uniform root,
    the law of (root class, total number of transitions) is that test's closed form; same
    chains, settings and criteria.  The number of transitions of a chain is its rows minus its
    two edges (the int64[C][n][n] count array would be 2.6 GB at 128 states)."""
    from raoteh_amd import _sampler
    Q = lumped_cycle(n)
    device = where == 'device'
    cls = _sampler.DeviceHistoryBatch if device else _sampler.HistoryBatch
    C = 20000 if device else 3000
    ta, tb = lengths
    T = nx.Graph()
    T.add_edge(0, 1, weight=ta)
    T.add_edge(0, 2, weight=tb)
    law = cycle_law(ta, tb)
    base = lambda st: 2 * ((-st) % 4)
    turned = sum(p for (st, k), p in law.items() if k >= base(st) + 4)
    zero_class = set(s for s in range(n) if s % 4 == 0)
    b = cls(T, 0, Q, node_to_allowed_states={1: zero_class, 2: zero_class}, nchains=C,
            root_distn=np.full(n, 1.0 / n), uniformization_factor=factor, seed=11, ctx=ctx)

    def run(k):
        if device:
            b.sweep(k)
        else:
            for _ in range(k):
                b.sweep()

    def observed():
        chain = b.rows()[0] if device else b.chain
        states = b.node_states
        assert (states[:, 1:] % 4 == 0).all()
        return states[:, 0] % 4, np.bincount(chain, minlength=C) - 2

    if (ta, factor) == (0.9, 2.0):
        run(3)
        root, total = observed()
        early = float((total >= 2 * ((-root) % 4) + 4).mean())
        assert early <= turned + 4.0 * np.sqrt(turned / C), (early, turned)
        run(sweeps - 3)
    else:
        run(sweeps)
    root, total = observed()
    assert ((total + 2 * root) % 4 == 0).all()
    stat, dof = chi_square(root, total, law, C)
    print('lumped cycle %s n=%d t=%s factor=%g: chi-square %.1f, dof %d' % (
        where, n, lengths, factor, stat, dof))
    assert stat < dof + 6.0 * np.sqrt(2.0 * dof) + 10.0, (ta, tb, factor, stat, dof)
    late = float((total >= 2 * ((-root) % 4) + 4).mean())
    assert abs(late - turned) < 6.0 * np.sqrt(turned * (1 - turned) / C) + 1e-3, \
        (ta, tb, factor, late, turned)
    # the replicas of a class are exchangeable: the root's replica is uniform
    replica = np.bincount(b.node_states[:, 0] // 4, minlength=n // 4)
    e = C / float(n // 4)
    assert ((replica - e) ** 2 / e).sum() < (n // 4 - 1) + 6.0 * np.sqrt(2.0 * (n // 4 - 1)) + 10.0


def histories_consistent(batch, rows_, masks, Q):
    """The rows of a device-resident batch: sorted by (chain, edge), adding up to the branch
    lengths at 1e-12, neighbouring rows of an edge in different states joined by a transition
    of Q; the node states are the states of the rows at the edge ends and lie in `masks`
    (uint64[C][N] up to 64 states, uint64[C][N][2] above; bits at or above n may be set).
    -> bool[rows - 1]: the row and its predecessor lie on one edge."""
    chain, edge, length, state = rows_
    C, N = masks.shape[:2]
    n = Q.shape[0]
    key = chain * N + edge
    assert (np.diff(key) >= 0).all()
    per_edge = np.bincount(key, weights=length, minlength=C * N).reshape(C, N)
    np.testing.assert_allclose(per_edge[:, 1:], np.broadcast_to(batch.branch[1:], (C, N - 1)),
                               rtol=1e-12)
    assert (length > 0).all() and ((state >= 0) & (state < n)).all()
    same_edge = key[1:] == key[:-1]
    assert (state[1:][same_edge] != state[:-1][same_edge]).all()
    assert (Q[state[:-1][same_edge], state[1:][same_edge]] > 0).all()
    ns = batch.node_states
    assert ((ns >= 0) & (ns < n)).all()
    last = np.ones(chain.shape[0], dtype=bool)
    last[:-1] = ~same_edge
    first = np.ones(chain.shape[0], dtype=bool)
    first[1:] = ~same_edge
    np.testing.assert_array_equal(ns[chain[last], edge[last]], state[last])
    np.testing.assert_array_equal(ns[chain[first], batch.parent[edge[first]]], state[first])
    word = np.take_along_axis(masks.reshape(C, N, -1), (ns // 64)[:, :, None], axis=2)[:, :, 0]
    assert ((word >> (ns % 64).astype(np.uint64)) & np.uint64(1)).all()
    return same_edge


def check_resident_histories(ctx, T, root, Q, root_distn, masks, sweeps=5):
    """rt_chains_* on one tree and rate matrix: (seed, batch) fixes the rows; the rows pass
    histories_consistent; the statistics kernels agree with numpy on the rows; another seed
    gives other histories; snapshot / restore returns rejected chains to their snapshot.
    -> the rows (chain, edge, length, state) after `sweeps` sweeps."""
    from raoteh_amd import _sampler
    C = masks.shape[0]
    n = Q.shape[0]
    batches = [_sampler.DeviceHistoryBatch(T, root, Q, node_masks=masks, root_distn=root_distn,
                                           seed=21, ctx=ctx) for _ in range(2)]
    for b in batches:
        b.sweep(sweeps)
    a, b = batches
    rows_a, rows_b = a.rows(), b.rows()
    for x, y in zip(rows_a, rows_b):
        np.testing.assert_array_equal(x, y)
    same_edge = histories_consistent(a, rows_a, masks, Q)
    chain, edge, length, state = rows_a
    assert a.sizes()[0] == chain.shape[0] and a.sizes()[1] >= C
    dwell = np.bincount(chain * n + state, weights=length, minlength=C * n).reshape(C, n)
    np.testing.assert_allclose(a.dwell_times(), dwell, rtol=1e-13)
    at = np.nonzero(same_edge)[0] + 1
    trans = np.bincount((chain[at] * n + state[at - 1]) * n + state[at],
                        minlength=C * n * n).reshape(C, n, n)
    np.testing.assert_array_equal(a.transition_counts(), trans)
    # another seed: other histories
    c = _sampler.DeviceHistoryBatch(T, root, Q, node_masks=masks, root_distn=root_distn, seed=22,
                                    ctx=ctx)
    c.sweep(sweeps)
    assert c.rows()[2].shape != length.shape or not np.array_equal(c.rows()[2], length)

    # snapshot / restore: the rejected chains are back at their snapshot, the others moved on
    def per_chain(rows_):
        ch = rows_[0]
        cut = np.searchsorted(ch, np.arange(C + 1))
        return [tuple(x[cut[k]:cut[k + 1]].tolist() for x in rows_[1:]) for k in range(C)]

    before, ns_before = per_chain(rows_a), a.node_states
    a.snapshot()
    a.sweep(1)
    after, ns_after = per_chain(a.rows()), a.node_states
    reject = np.arange(C) % 3 == 0
    a.restore(reject)
    rows_r = a.rows()
    histories_consistent(a, rows_r, masks, Q)
    now, ns_now = per_chain(rows_r), a.node_states
    moved = 0
    for k in range(C):
        assert now[k] == (before[k] if reject[k] else after[k]), k
        np.testing.assert_array_equal(ns_now[k], ns_before[k] if reject[k] else ns_after[k])
        moved += before[k] != after[k]
    assert moved >= C // 2
    return rows_a
