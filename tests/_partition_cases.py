"""Cases of the partitioned-likelihood tests (test_partition_gpu.py): an 8-leaf random binary
tree, observations of one kind at every leaf, K rate sets that differ in their rate matrices and
branch lengths, and one rate-set index per site."""
import collections

import networkx as nx
import numpy as np

import _step_multi_cases as smc

Case = collections.namedtuple(
    'Case', 'T root n leaves kind data obs_lik root_distn Q node_q t site_sets nsets')


def random_binary_tree(nleaves, seed):
    """Random topology (random joins of the remaining subtrees), random branch lengths in
    [0.05, 0.35].  -> (T, root, leaves)."""
    rng = np.random.RandomState(seed)
    T = nx.Graph()
    live = list(range(nleaves))
    leaves = list(live)
    nxt = nleaves
    while len(live) > 1:
        a, b = (live.pop(rng.randint(len(live))) for _ in range(2))
        T.add_edge(nxt, a, weight=float(rng.uniform(0.05, 0.35)))
        T.add_edge(nxt, b, weight=float(rng.uniform(0.05, 0.35)))
        live.append(nxt)
        nxt += 1
    return T, live[0], leaves


def granule(n):
    """Sites that share one copy of the tables: a 16-site tile above four states, else the
    256 sites of a lane-kernel workgroup (on this tree the P table is staged in LDS)."""
    return 16 if n > 4 else 256


def make_case(n, kind, seed, nsets=4, nsites=None, site_sets=None, zero_set=None):
    """nsets rate sets with two rate matrices each and a node_q; by default site i is in set
    i % 3 (set 3 empty) and there are 3 G + 5 sites.  zero_set: that set has Q = 0 (P = I)."""
    from raoteh_amd import _tree
    rng = np.random.RandomState(seed)
    T, root, leaves = random_binary_tree(8, seed)
    ta = _tree.TreeArrays(T, root)
    if nsites is None:
        nsites = 3 * granule(n) + 5
    data, lik = smc.observations(kind, n, nsites, len(leaves), rng)
    root_distn = rng.uniform(0.1, 1.0, n)
    root_distn /= root_distn.sum()
    Q = np.zeros((nsets, 2, n, n))
    t = np.zeros((nsets, ta.nnodes))
    for k in range(nsets):
        Q[k, 0] = smc.random_rates(n, rng) * rng.uniform(0.5, 2.0)
        Q[k, 1] = smc.random_rates(n, rng) * rng.uniform(0.5, 2.0)
        t[k] = ta.branch_lengths() * rng.uniform(0.5, 1.5, ta.nnodes)
    if zero_set is not None:
        Q[zero_set] = 0.0
    node_q = np.zeros(ta.nnodes, dtype=np.int64)
    node_q[1::3] = 1
    t[:, 0] = 0.0
    if site_sets is None:
        site_sets = np.arange(nsites) % 3
    return Case(T, root, n, leaves, kind, data, lik, root_distn, Q, node_q, t,
                np.asarray(site_sets), nsets)


def upload(device, ctx, case, partitioned=True):
    model = device.TreeModel(case.T, case.root, case.n, ctx=ctx)
    model.set_root_distn(case.root_distn)
    if partitioned:
        batch = model.upload_sites(case.leaves, case.data, kind=case.kind,
                                   site_sets=case.site_sets, nsets=case.nsets)
    else:
        batch = model.upload_sites(case.leaves, case.data, kind=case.kind)
    return model, batch


def oracle(model, case):
    """(loglik, status) per site from scipy exponentials of the site's own rate set and the
    numpy oracle's pruning."""
    import scipy.linalg
    from oracle import oracle_numpy as orc
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.leaves]
    ll = np.zeros(len(case.site_sets))
    st = np.zeros(len(case.site_sets), dtype=np.int32)
    for k in np.unique(case.site_sets):
        esd = np.zeros((ta.nnodes, case.n, case.n))
        for v in range(1, ta.nnodes):
            esd[v] = scipy.linalg.expm(case.t[k, v] * case.Q[k, case.node_q[v]])
        mine = np.flatnonzero(case.site_sets == k)
        ll[mine], st[mine] = orc.batch_log_likelihoods(ta.indices, ta.indptr, esd, cols,
                                                       case.obs_lik[mine], case.root_distn)
    return ll, st
