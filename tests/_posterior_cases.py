"""The oracle (oracle/oracle_numpy.py) restated over state sets: what rt_sites_posteriors
returns, computed per site from mc0_esd_get_node_to_distn / mc0_esd_get_joint_endpoint_distn
(test_posteriors_gpu.py, test_posteriors_cpu.py)."""
import numpy as np

from oracle import oracle_numpy as orc


def oracle_pmaps(indices, indptr, esd, obs_cols, obs_lik):
    """Subtree likelihoods of every node, f64[nsites, N, n] (batch_upward keeping all L)."""
    N, n = len(indptr) - 1, esd.shape[1]
    S = obs_lik.shape[0]
    slot = dict((int(v), k) for k, v in enumerate(obs_cols))
    L = np.ones((S, N, n))
    for v in range(N - 1, -1, -1):
        for c in indices[indptr[v]:indptr[v + 1]]:
            L[:, v] *= L[:, c] @ esd[c].T
        if v in slot:
            L[:, v] *= obs_lik[:, slot[v], :]
    return L


def oracle_site(indices, indptr, esd, root_distn, pmap):
    """(D f64[N, n], J f64[N, n, n]) of one site from the oracle, or None (zero likelihood)."""
    w = pmap[0] * (1.0 if root_distn is None else root_distn)
    if not w.sum() > 0:
        return None
    D = orc.mc0_esd_get_node_to_distn(indices, indptr, esd, root_distn, pmap)
    J = orc.mc0_esd_get_joint_endpoint_distn(indices, indptr, esd, pmap, D)
    return D, J


def sums_over_sets(D, J, node_sets, edge_sets):
    nv = np.array([[D[v, sorted(S)].sum() for S in node_sets] for v in range(D.shape[0])])
    ev = np.array([[J[v][np.ix_(sorted(A), sorted(B))].sum() for A, B in edge_sets]
                   for v in range(D.shape[0])])
    return nv.reshape(D.shape[0], len(node_sets)), ev.reshape(D.shape[0], len(edge_sets))


