"""Host reference of rt_sites_branch_expectations_mixture (test_mixture_expect_cpu.py,
test_mixture_expect_gpu.py): per rate set k, _branch_cases.branch_reference over all sites with
t[k] and Q[k][node_q] (scipy expm and expm_frechet, the oracle's passes: the wrapper
_partition_read_cases.set_case), the site likelihoods L_ik from oracle_numpy.batch_log_likelihoods,
and the definitions of include/raoteh_hip.h section 2d combined in numpy -- never from a device
path.  The cases are _step_multi_cases.make_case's: an ordinary batch and K rate sets."""
import collections

import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc
from _branch_cases import branch_reference
import _partition_read_cases as prc
import _step_multi_cases as smc

NSITES = smc.NSITES          # 83: six tiles of 16 sites, the last one partial

Reference = collections.namedtuple(
    'Reference', 'values edge_sums set_edge_sums post class_sums loglik status x L')


def tree_arrays(case):
    from raoteh_amd import _tree
    return _tree.TreeArrays(case.T, case.root)


def normalised(case):
    """The case with Q as [K, nq, n, n] and a node_q (what set_case indexes)."""
    if case.Q.ndim == 4:
        return case
    nnodes = case.t.shape[1]
    return case._replace(Q=case.Q[:, None].copy(), node_q=np.zeros(nnodes, dtype=np.int64))


def make_case(n, tree, kind, K, seed, per_edge=True, zero_set=True, nsites=NSITES, dead_site=None):
    """_step_multi_cases.make_case, normalised.  dead_site (dense data only): that site's first
    leaf observes nothing -- likelihood zero under every set."""
    case = normalised(smc.make_case(n, tree, kind, K, seed, per_edge=per_edge, zero_set=zero_set,
                                    nsites=nsites))
    if dead_site is not None:
        assert kind == 'dense'
        lik = case.obs_lik.copy()
        lik[dead_site, 0, :] = 0.0
        case = case._replace(data=lik, obs_lik=lik)
    return case


def set_transitions(ta, case, k, t=None, Q=None):
    t = case.t[k] if t is None else t
    Q = case.Q[k] if Q is None else Q
    esd = np.zeros((ta.nnodes, case.n, case.n))
    for v in range(1, ta.nnodes):
        esd[v] = scipy.linalg.expm(t[v] * Q[case.node_q[v]])
    return esd


def set_likelihoods(ta, case, k, t=None, Q=None):
    """L_ik f64[S] from the oracle (0 where the oracle reports zero likelihood)."""
    cols = [ta.node_to_index[v] for v in case.leaves]
    ll, st = orc.batch_log_likelihoods(ta.indices, ta.indptr, set_transitions(ta, case, k, t, Q),
                                       cols, case.obs_lik, case.root_distn)
    return np.where(st == 0, np.exp(np.where(st == 0, ll, 0.0)), 0.0)


def combine(L, c):
    """(post [S, K], loglik [S], dead [S]) of the definitions: set k live at site i when c_k > 0
    and L_ik > 0; sums over k in set order."""
    K, S = L.shape
    live = (np.asarray(c)[:, None] > 0) & (L > 0)
    mix = np.zeros(S)
    for k in range(K):
        mix = mix + np.where(live[k], c[k] * L[k], 0.0)
    dead = ~(mix > 0)
    post = np.zeros((S, K))
    for k in range(K):
        post[:, k] = np.where(live[k] & ~dead, c[k] * L[k] / np.where(dead, 1.0, mix), 0.0)
    with np.errstate(divide='ignore'):
        loglik = np.where(dead, -np.inf, np.log(np.where(dead, 1.0, mix)))
    return post, loglik, dead


def mixture_reference(ta, case, coefs, class_weights, weights=None, check=2):
    """The Reference of a case: x [K, S, N, C] the unweighted per-set values, L [K, S] the site
    likelihoods, and every output of the call.  `check`: sites on which branch_reference checks
    its site-axis restatement against the oracle's own passes, per set."""
    case = normalised(case)
    n, K = case.n, case.Q.shape[0]
    S, N = case.obs_lik.shape[0], ta.nnodes
    c = np.asarray(class_weights, dtype=float)
    w = np.ones(S) if weights is None else np.asarray(weights, dtype=float)
    C = prc.coefs_of_set(coefs, n, 0).shape[0]
    x = np.zeros((K, S, N, C))
    L = np.zeros((K, S))
    picks = sorted(set(np.linspace(0, S - 1, check).astype(int))) if check else ()
    for k in range(K):
        model, sub = prc.set_case(ta, case, k, np.arange(S))
        x[k], zero = branch_reference(model, sub, prc.coefs_of_set(coefs, n, k), check_sites=picks)
        L[k] = set_likelihoods(ta, case, k)
        assert np.array_equal(zero != 0, ~(L[k] > 0)), k     # (the two oracles agree on the zeros)
    post, loglik, dead = combine(L, c)
    values = np.zeros((S, N, C))
    set_sums = np.zeros((K, N, C))
    for k in range(K):
        live = post[:, k] != 0
        values[live] += post[live, k][:, None, None] * x[k][live]
        set_sums[k] = np.einsum('i,ivc->vc', (w * post[:, k])[live], x[k][live])
    edge_sums = np.zeros((N, C))
    for k in range(K):
        edge_sums = edge_sums + set_sums[k]
    status = np.where(dead, 1, 0).astype(np.int32)
    return Reference(values, edge_sums, set_sums, post, (w[:, None] * post).sum(axis=0), loglik,
                     status, x, L)


# ---- gradients ------------------------------------------------------------------------------

def gradient_coefs(Q):
    """Per-set coefficients of the branch-length gradient for Q [K, 1, n, n]."""
    return prc.gradient_coefs(Q)


def kappa_mask(n):
    """The off-diagonal entries a kappa-style parameter multiplies: a <-> b with a + b even."""
    a, b = np.indices((n, n))
    return ((a + b) % 2 == 0) & (a != b)


def kappa_rates(Q0, kappa):
    """Q(kappa): the masked off-diagonal entries of Q0 times kappa, rows summing to zero (Q(1) =
    Q0 for a Q0 whose rows do), and dQ / d kappa."""
    n = Q0.shape[-1]
    m = kappa_mask(n)
    off = Q0 * ~np.eye(n, dtype=bool)
    Q = np.where(m, kappa * off, off)
    Q = Q - np.diag(Q.sum(axis=1))
    dQ = np.where(m, off, 0.0)
    dQ = dQ - np.diag(dQ.sum(axis=1))
    return Q, dQ


def kappa_coefs(case):
    """Per-set coefficients [K, 1, n, n] for d / d kappa at kappa = 1 (one shared kappa that
    scales the masked entries of every set's one rate matrix)."""
    from raoteh_amd import device
    K = case.Q.shape[0]
    return np.array([[device.rate_parameter_coefs(case.Q[k, 0], kappa_rates(case.Q[k, 0], 1.0)[1])]
                     for k in range(K)])


def reference_gradients(ta, case, c, weights=None):
    """(g_t [K, N], g_c [K], g_kappa, total) of f = sum_i w_i log sum_k c_k L_ik from the host
    reference, for a case with one rate matrix per set and no dead site."""
    case = normalised(case)
    assert case.Q.shape[1] == 1
    c = np.asarray(c, dtype=float)
    ref = mixture_reference(ta, case, gradient_coefs(case.Q), c, weights, check=0)
    assert not ref.status.any()
    g_t = np.zeros_like(case.t)
    g_t[:, 1:] = ref.set_edge_sums[:, 1:, 0] / case.t[:, 1:]
    g_c = np.where(c > 0, ref.class_sums / np.where(c > 0, c, 1.0), 0.0)
    kap = mixture_reference(ta, case, kappa_coefs(case), c, weights, check=0)
    w = np.ones(len(ref.loglik)) if weights is None else np.asarray(weights, dtype=float)
    return g_t, g_c, float(kap.edge_sums[:, 0].sum()), float((w * ref.loglik).sum())


def oracle_total(ta, case, c, L):
    post, loglik, dead = combine(L, np.asarray(c, dtype=float))
    assert not dead.any()
    return float(loglik.sum())


def gradient_gaps(ta, case, c, h):
    """The host reference's analytic gradients next to central differences (step h) of the
    oracle's mixture total -> dict name -> (analytic, max |central difference - analytic|)."""
    case = normalised(case)
    c = np.asarray(c, dtype=float)
    K, N = case.t.shape
    g_t, g_c, g_kappa, _ = reference_gradients(ta, case, c)
    L = np.array([set_likelihoods(ta, case, k) for k in range(K)])
    fd_t = np.zeros_like(g_t)
    for k in range(K):
        for v in range(1, N):
            f = []
            for sign in (1.0, -1.0):
                t = case.t[k].copy()
                t[v] += sign * h
                Lk = L.copy()
                Lk[k] = set_likelihoods(ta, case, k, t=t)
                f.append(oracle_total(ta, case, c, Lk))
            fd_t[k, v] = (f[0] - f[1]) / (2 * h)
    fd_c = np.zeros(K)
    for k in range(K):
        f = []
        for sign in (1.0, -1.0):
            ck = c.copy()
            ck[k] += sign * h
            f.append(oracle_total(ta, case, ck, L))
        fd_c[k] = (f[0] - f[1]) / (2 * h)
    f = []
    for sign in (1.0, -1.0):
        Lk = np.array([set_likelihoods(ta, case, k, Q=kappa_rates(case.Q[k, 0], 1.0 + sign * h)[0][None])
                       for k in range(K)])
        f.append(oracle_total(ta, case, c, Lk))
    fd_kappa = (f[0] - f[1]) / (2 * h)
    return {'t': (g_t, float(np.abs(fd_t - g_t).max())),
            'c': (g_c, float(np.abs(fd_c - g_c).max())),
            'kappa': (np.array([g_kappa]), float(abs(fd_kappa - g_kappa)))}


def gradient_case(n, seed, nsites=60, K=3):
    """'state' data on the balanced tree, one rate matrix per set, no zero set: no dead site."""
    return make_case(n, 'balanced', 'state', K, seed, per_edge=False, zero_set=False, nsites=nsites)
