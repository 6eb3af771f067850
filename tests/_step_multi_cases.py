"""Cases of the rate-set tests (test_step_multi_gpu.py): a tree, observations of one kind at
every leaf and K rate sets that differ in their rate matrices and branch lengths; and the
comparison of one step_multi with K separate set_rates + step on the same batch, bit for bit.

Run as a program (a fresh child process of the RAOTEH_MULTI=loop test) it checks one 61-state
case and prints the batch's multi kernel name."""
import collections
import os
import sys

import numpy as np

NSITES = 83          # six tiles of 16 sites, the last one partial; 2 lane blocks

Case = collections.namedtuple('Case', 'T root n leaves kind data obs_lik root_distn Q node_q t')


def _encode_mask(n, lik):
    words = np.zeros(lik.shape[:2] + ((n + 63) // 64,), dtype=np.uint64)
    for s in range(n):
        words[:, :, s >> 6] |= (lik[:, :, s] != 0).astype(np.uint64) << np.uint64(s & 63)
    return words[:, :, 0].copy() if n <= 64 else words


def observations(kind, n, nsites, nleaves, rng):
    """(upload data, likelihoods f64[S, L, n]).  'state': one state per leaf; 'mask': one or two;
    every 7th site has the same single state at every leaf (likelihood > 0 under P = I, where
    the sites with differing leaves have likelihood 0)."""
    if kind == 'dense':
        lik = rng.uniform(0.0, 1.0, size=(nsites, nleaves, n))
        lik[rng.uniform(size=lik.shape) < 0.2] = 0.0
        lik[:, :, 1] += 0.05
        lik[::7] = 0.0
        lik[::7, :, 2 % n] = 0.5           # one live state, the same at every leaf
        lik[5] = 0.0
        lik[5, 0::2, 0] = 1.0              # leaves in different states: zero under P = I only
        lik[5, 1::2, 1] = 1.0
        return lik, lik
    st = rng.randint(0, n, size=(nsites, nleaves))
    st[::7] = st[::7, :1]
    st[5, 0], st[5, 1] = 0, 1
    lik = np.zeros((nsites, nleaves, n))
    ii, kk = np.indices(st.shape)
    lik[ii, kk, st] = 1.0
    if kind == 'state':
        return st.astype(np.uint8), lik
    second = rng.randint(0, n, size=(nsites, nleaves))
    second[::7] = st[::7]
    second[5] = st[5]
    lik[ii, kk, second] = 1.0
    return _encode_mask(n, lik), lik


def random_rates(n, rng):
    R = rng.uniform(0.1, 1.0, (n, n))
    np.fill_diagonal(R, 0.0)
    Q = R - np.diag(R.sum(axis=1))
    return Q / R.sum(axis=1).mean()


def make_case(n, tree, kind, K, seed, per_edge=True, zero_set=True, nsites=NSITES):
    """K rate sets on the 8-leaf balanced tree or a random non-binary tree of 12 nodes.  per_edge:
    Q is [K, 2, n, n] with a node_q, and set 0 is the one whose two matrices differ (the others
    repeat their matrix); else [K, n, n].  zero_set (K >= 2): the last set has Q = 0, P = I."""
    from raoteh_amd import synth, _tree
    rng = np.random.RandomState(seed)
    if tree == 'balanced':
        T, root, leaves = synth.balanced_tree(8, seed=seed)
    else:
        T, root, leaves = synth.random_tree(12, seed=seed, max_children=3)
    ta = _tree.TreeArrays(T, root)
    data, lik = observations(kind, n, nsites, len(leaves), rng)
    root_distn = rng.uniform(0.1, 1.0, n)
    root_distn /= root_distn.sum()
    Q = np.zeros((K, 2 if per_edge else 1, n, n))
    t = np.zeros((K, ta.nnodes))
    for k in range(K):
        Q[k, :] = random_rates(n, rng) * rng.uniform(0.5, 2.0)
        t[k] = ta.branch_lengths() * rng.uniform(0.5, 1.5, ta.nnodes)
    if per_edge:
        Q[0, 1] = random_rates(n, rng)
    if zero_set and K >= 2:
        Q[K - 1] = 0.0
    node_q = None
    if per_edge:
        node_q = np.zeros(ta.nnodes, dtype=np.int64)
        node_q[1::3] = 1
    t[:, 0] = 0.0
    return Case(T, root, n, leaves, kind, data, lik, root_distn,
                Q if per_edge else Q[:, 0], node_q, t)


def upload(device, ctx, case):
    model = device.TreeModel(case.T, case.root, case.n, ctx=ctx)
    model.set_root_distn(case.root_distn)
    batch = model.upload_sites(case.leaves, case.data, kind=case.kind)
    return model, batch


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def separate_steps(model, batch, case, sets=None):
    """(loglik [K, S], status [K, S], totals [K, 3]) of set_rates + step + fetch per set."""
    K = case.Q.shape[0]
    ll, st, tot = [], [], []
    for k in (range(K) if sets is None else sets):
        model.set_rates(Q=case.Q[k], node_q=case.node_q, t=case.t[k])
        model.step(batch)
        a, b = model.fetch_log_likelihoods(batch)
        ll.append(a)
        st.append(b)
        tot.append(model.fetch_totals(batch))
    return np.array(ll), np.array(st), np.array(tot)


def check_bit_identity(model, batch, case, sets=None):
    """One set_rate_sets + step_multi against the separate steps of the same sets."""
    sel = list(range(case.Q.shape[0]) if sets is None else sets)
    model.set_rate_sets(case.Q[sel], t=case.t[sel], node_q=case.node_q)
    model.step_multi(batch)
    ll, st = model.fetch_multi_log_likelihoods(batch)
    tot = model.fetch_multi_totals(batch)
    name = batch.multi_kernel_name
    wll, wst, wtot = separate_steps(model, batch, case, sel)
    assert ll.shape == wll.shape and st.shape == wst.shape and tot.shape == wtot.shape
    assert np.array_equal(bits(ll), bits(wll)), (name, np.argwhere(bits(ll) != bits(wll))[:4])
    assert np.array_equal(st, wst), name
    assert np.array_equal(bits(tot), bits(wtot)), (name, tot, wtot)
    return ll, st, tot, name


def main():
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    from raoteh_amd import device
    ctx = device.Context(0)
    ctx.set_option('jit', 1)
    case = make_case(61, 'balanced', 'state', 3, seed=7)
    model, batch = upload(device, ctx, case)
    batch.wait_for_kernel()
    ll, st, tot, name = check_bit_identity(model, batch, case)
    assert (st[-1] & 1).any() and not (st[0] & 1).any()
    print('MULTI_KERNEL %s' % name)


if __name__ == '__main__':
    main()
