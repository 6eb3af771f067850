"""Host reference of rt_sites_branch_profiles (test_branch_profiles_cpu.py,
test_branch_profiles_gpu.py): for every edge v and every trial length tau of its grid, that
edge's matrix in the model's transition matrices is replaced by scipy.linalg.expm(Q_v tau), the
per-site likelihoods are recomputed with the oracle's pruning (oracle/oracle_numpy.py), and
    value = log L(tau) - log L(t)
is taken -- (nnodes - 1) G whole-tree evaluations, never a device path."""
import numpy as np
import scipy.linalg

from oracle import oracle_numpy as orc


def _one_blas_thread():
    """(nnodes - 1) G small exponentials: a threaded BLAS spends far longer handing each of their
    products to its pool than computing it -- one thread where threadpoolctl is there to ask."""
    try:
        from threadpoolctl import threadpool_limits
    except ImportError:
        import contextlib
        return contextlib.nullcontext()
    return threadpool_limits(limits=1, user_api='blas')


def make_grid(t, npoints, seed):
    """([nnodes, npoints] trial lengths, the factors): every branch's resident length t_v times
    the same factors -- 1 (the resident length itself), one below it and one above, the rest
    log-uniform in [1/4, 4], in a shuffled order.  Fewer than three points cannot hold all
    three: then the factor below (and the one above) only, the resident length has a test of
    its own.  Row 0 is zero."""
    rng = np.random.RandomState(seed)
    head = [1.0, 0.5, 1.75] if npoints >= 3 else [0.5, 1.75]
    factors = np.concatenate([head, np.exp(rng.uniform(-np.log(4), np.log(4), 64))])
    factors = factors[:npoints][rng.permutation(npoints)]
    grid = np.asarray(t, dtype=float)[:, None] * factors[None, :]
    grid[0] = 0.0
    return np.ascontiguousarray(grid), factors


def profile_from_transitions(indices, indptr, esd, cols, obs_lik, root_distn, Qs, node_q, grid):
    """(values f64[S, N, G], status int32[S], log-likelihoods f64[S]) from the transition
    matrices `esd` [N, n, n] of the resident lengths: zero-likelihood sites give zeros, a trial
    length at which a live site has likelihood 0 gives -inf."""
    esd = np.asarray(esd, dtype=float)
    grid = np.asarray(grid, dtype=float)
    N, G = grid.shape
    base, status = orc.batch_log_likelihoods(indices, indptr, esd, cols, obs_lik, root_distn)
    live = status == 0
    values = np.zeros((len(base), N, G))
    with _one_blas_thread():
        trials = [[scipy.linalg.expm(Qs[node_q[v]] * grid[v, g]) for g in range(G)]
                  for v in range(1, N)]
    for v in range(1, N):
        for g in range(G):
            trial = esd.copy()
            trial[v] = trials[v - 1][g]
            ll, st = orc.batch_log_likelihoods(indices, indptr, trial, cols, obs_lik, root_distn)
            values[live, v, g] = np.where(st[live] == 0, ll[live], -np.inf) - base[live]
    return values, status.astype(np.int32), np.where(live, base, 0.0)


def profile_reference(model, case, grid, Qs=None, node_q=None):
    """profile_from_transitions of a _resident_cases.Case on model.get_transitions() (Qs,
    node_q: the case's unless given, as for a model with spectral rates)."""
    ta = model.tree
    cols = [ta.node_to_index[v] for v in case.obs_nodes]
    return profile_from_transitions(
        ta.indices, ta.indptr, model.get_transitions(), cols, case.obs_lik, case.root_distn,
        case.Qs if Qs is None else Qs, case.node_q if node_q is None else node_q, grid)


def site_bounds(loglik, weights=None, tol=1e-10):
    """The tolerances of the comparison: tol * max(1, |log L_i|) per site and tol * max(1,
    sum_i w_i |log L_i|) for the weighted sums (both sides are differences of log-likelihoods:
    the error scales with |log L_i|, not with the difference).  tol = 1e-10 is the project's
    tolerance for log-likelihoods against the oracle (test_config_fixtures_batched)."""
    per_site = tol * np.maximum(1.0, np.abs(loglik))
    w = np.ones(len(loglik)) if weights is None else np.asarray(weights, dtype=float)
    return per_site, tol * max(1.0, float((w * np.abs(loglik)).sum()))
