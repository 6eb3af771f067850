"""The state-count sweep (test_state_sweep_cpu.py, test_state_sweep_gpu.py): one small case per
state count n, chosen so that every instance of the reads of a resident batch runs once against
its host reference -- every KS = ceil(n / 4) in 2..32 (the k-steps of the f64 16x16x4 product) and
every NT = ceil(n / 16) in 1..8 (the row-tile waves), with every tail of the last k-step and of
the last row tile.  The cases come from the existing builders (_resident_cases.make_case, the
mixture's and the partition's); three sites are then pinned to
the tail states, so that a kernel which loses the last row, the last k-step or the second half of
an odd pair turns a pinned site into a zero, a -inf or a visibly different number."""
import functools

import numpy as np
import scipy.linalg

from _map_cases import EXACT_SITES
from _resident_cases import _encode, make_case

# ---- 1. the state counts ---------------------------------------------------------------------

KS_RANGE = range(2, 33)


def ks_of(n):
    return (n + 3) // 4


def nt_of(n):
    return (n + 15) // 16


# one n per KS: within every NT the four KS get the four residues of n % 4, the last row tile
# 16, 1, 6 or 9 live rows; KS = 2 takes 7, the smallest n with n % 4 == 3 (the formula gives 6)
ROTATING = [7 if ks == 2 else 4 * ks - ks % 4 for ks in KS_RANGE]
# the thinnest tail of every KS, one live column in the last k-step -- three where ROTATING has
# that value already
THIN = [4 * ks - 3 if 4 * ks - 3 != r else 4 * ks - 1 for ks, r in zip(KS_RANGE, ROTATING)]
# two tails the two lists leave out.  NT = 1 holds three KS only (KS = 1 is the lane kernels'), so
# its tail n % 4 == 2 is missing: 6, the formula's own value for KS = 2.  No value has 15 live rows
# in the last row tile (n % 16 == 15): 127, at the largest NT and KS
EXTRA = [6, 127]
PLAIN = sorted(set(ROTATING) | set(THIN) | set(EXTRA))      # the plain forms
FORMS = sorted(set(ROTATING) | set(EXTRA))                  # the mixture and partitioned forms
SPOT = [7, 41, 86, 105]                    # NT = 1, 3, 6, 7: the tree-specialised pruning kernel
HOST = SPOT + [121]                        # the references' smoke and sensitivity checks (CPU)

NSITES = EXACT_SITES                       # 33: two full 16-site tiles and one lane of a third
NNODES = 9
KINDS = ('state', 'mask', 'dense')
FACTORS = (1.0, 0.5)                       # the resident length and one trial length
FRACTIONS = (0.0, 0.6)                     # two cuts of the regraft / attachment edge
PENDANT = (0.2,)
PINNED_SITES = (0, 17, 1)                  # state n - 1 (first tile), n - 1 (second tile), 4 (KS - 1)


def site_weights():
    """1, 2 or 3 per site and one site of weight 0 -- not a pinned site, not the last."""
    w = np.random.RandomState(12000).randint(1, 4, size=NSITES).astype(np.float64)
    w[9] = 0.0
    return w


def kind_of(n):
    return KINDS[n % 3]


def radius_of(n):
    """SPR: every move up to 64 states, radius 1 above (the host reference's cost)."""
    return None if n <= 64 else 1


# ---- 2. the cases ----------------------------------------------------------------------------

def _tree_is_fit(seed):
    """A multifurcation, a single-child node and an observed internal node (make_case observes
    every second internal node) in synth.random_tree(NNODES, seed)."""
    from raoteh_amd import synth, _tree
    T, root, leaves = synth.random_tree(NNODES, seed=seed, max_children=3)
    kids = np.diff(_tree.TreeArrays(T, root).indptr)
    return kids.max() >= 3 and (kids == 1).any() and len(T) - len(leaves) >= 1


@functools.lru_cache(maxsize=None)
def seed_of(n):
    seed = 12000 + n
    while not _tree_is_fit(seed):
        seed += 1000
    return seed


def pins_of(case):
    """[(site, column of obs_nodes, state)]: three different leaves."""
    n = case.n
    return [(0, 0, n - 1), (17, 1, n - 1), (1, 2, 4 * (ks_of(n) - 1))]


def pin(case, pins=None):
    """The case with the pinned observations written over the builder's: one-hot likelihoods,
    through the module's own _encode (state data: the state itself)."""
    lik = case.obs_lik.copy()
    data = case.data.copy()
    for site, col, state in pins_of(case) if pins is None else pins:
        lik[site, col] = 0.0
        lik[site, col, state] = 1.0
        if case.kind == 'state':
            data[site, col] = state
    if case.kind != 'state':
        # (_step_multi_cases._encode_mask, the mixture and partition builders' own, is the same
        # packing)
        data = _encode(case.kind, case.n, lik)
        if case.kind == 'mask':
            assert data.shape == case.data.shape and data.dtype == case.data.dtype
    return case._replace(obs_lik=lik, data=data)


@functools.lru_cache(maxsize=None)
def plain_case(n):
    """make_case: a 9-node tree, 33 sites, per-edge rate matrices (two distinct ones), an observed
    internal node, the zero-likelihood last site; then the pins."""
    case = make_case(n, NNODES, NSITES, kind_of(n), seed_of(n), internal=True, per_edge=True)
    assert case.zero_site == NSITES - 1
    return pin(case)


K_MIX = 3
NSETS = 3


def class_weights_of(n):
    """_mixture_search_cases.class_weights with the middle set at weight zero (the last set is
    the builder's zero set, Q = 0 and P = I, and stays in)."""
    from _mixture_search_cases import class_weights
    c = class_weights(K_MIX, 12000 + n)
    c[1] = 0.0
    return c / c.sum()


@functools.lru_cache(maxsize=None)
def mix_case(n):
    """_mixture_cases.make_case: the 12-node non-binary tree (multifurcations; this builder
    observes the leaves only), 33 sites, K = 3 rate sets with two rate matrices per set and
    lengths of their own; then the pins."""
    import _mixture_cases as mc
    return pin(mc.make_case(n, 'random', kind_of(n), K_MIX, 12000 + n, nsites=NSITES))


@functools.lru_cache(maxsize=None)
def part_case(n):
    """_partition_cases.make_case: the 8-leaf binary tree, 33 sites, three rate sets, site i in
    set i % 3 -- three granules of 16 slots, the fewest that hold three sets; the pinned sites
    0, 17 and 1 lie in the sets 0, 2 and 1; then the pins."""
    import _partition_cases as pc
    return pin(pc.make_case(n, kind_of(n), 12000 + n, nsets=NSETS, nsites=NSITES,
                            site_sets=np.arange(NSITES) % NSETS))


def case_of(form, n):
    return {'plain': plain_case, 'mix': mix_case, 'part': part_case}[form](n)


def shared_q(case):
    """The case under its first rate matrix alone (branch_length_gradient wants one Q)."""
    return case._replace(Qs=case.Qs[:1], node_q=np.zeros_like(case.node_q))


def without_state(case, state):
    """`state` made unobservable: its observation likelihood zeroed at every observed node."""
    lik = case.obs_lik.copy()
    lik[:, :, state] = 0.0
    return case._replace(obs_lik=lik)


def uploaded_likelihoods(case):
    """f64[S, K, n] decoded from case.data, the array that goes to the device."""
    n = case.n
    if case.kind == 'dense':
        return np.asarray(case.data, dtype=float)
    S, K = case.data.shape[:2]
    lik = np.ones((S, K, n))
    if case.kind == 'state':
        seen = case.data != 255
        lik[seen] = 0.0
        ii, kk = np.nonzero(seen)
        lik[ii, kk, case.data[ii, kk]] = 1.0
        return lik
    words = case.data.reshape(S, K, -1)
    for s in range(n):
        lik[:, :, s] = (words[:, :, s >> 6] >> np.uint64(s & 63)) & np.uint64(1)
    return lik


def make_queries(n, seed):
    """(dense f64[1, S, n] with exact zeros and the last state live, states uint8[1, S] with
    state n - 1 at the pinned sites and an unobserved entry)."""
    rng = np.random.RandomState(seed)
    dense = rng.uniform(0.0, 1.0, size=(1, NSITES, n))
    dense[rng.uniform(size=dense.shape) < 0.2] = 0.0
    dense[:, :, 0] = 0.0
    dense[:, :, n - 1] += 0.05
    states = rng.randint(1, n, size=(1, NSITES)).astype(np.uint8)
    states[0, [0, 17]] = n - 1
    states[0, 5] = 255
    return dense, states


# ---- 3. a host stand-in for the device model -------------------------------------------------

class ExpmCache(object):
    """scipy.linalg.expm per (matrix, tau) within a case: the references of one case ask for the
    same halves and trial lengths again and again."""

    def __init__(self, Qs, node_q):
        self.Qs, self.node_q, self.memo = Qs, node_q, {}

    def __call__(self, v, tau):
        key = (int(self.node_q[v]), float(tau))
        if key not in self.memo:
            self.memo[key] = scipy.linalg.expm(self.Qs[key[0]] * key[1])
        return self.memo[key]


class HostModel(object):
    """What the references ask of a TreeModel -- tree, get_transitions(), branch_lengths() --
    with scipy's exponentials in place of the device's."""

    def __init__(self, case):
        from raoteh_amd import _tree
        self.tree = _tree.TreeArrays(case.T, case.root)
        self.nstates = case.n
        self.expm = ExpmCache(case.Qs, case.node_q)
        t = self.branch_lengths()
        self._esd = np.zeros((self.tree.nnodes, case.n, case.n))
        for v in range(1, self.tree.nnodes):
            self._esd[v] = self.expm(v, t[v])

    def branch_lengths(self):
        return self.tree.branch_lengths()

    def get_transitions(self):
        return self._esd.copy()


def grid_of(model):
    """[N, 2] trial lengths: the resident length of every edge and half of it; row 0 is zero."""
    grid = np.asarray(model.branch_lengths(), dtype=float)[:, None] * np.array(FACTORS)[None, :]
    grid[0] = 0.0
    return np.ascontiguousarray(grid)


# ---- 4. the references, each the one its own parity test uses --------------------------------

def _cols(model, case):
    return [model.tree.node_to_index[v] for v in case.obs_nodes]


def coefs_of(n):
    from _branch_cases import make_coefs
    return make_coefs(n, 2, 12000 + n)


def queries_of(n):
    """f64[2, S, n]: the dense query and the state query as likelihoods (test_place_gpu.py)."""
    from _place_cases import query_likelihoods
    dense, states = make_queries(n, 12000 + n)
    return np.concatenate([dense, query_likelihoods(states, 'state', n)])


def loglik_ref(model, case):
    from oracle import oracle_numpy as orc
    ta = model.tree
    return orc.batch_log_likelihoods(ta.indices, ta.indptr, model.get_transitions(),
                                     _cols(model, case), case.obs_lik, case.root_distn)


def nni_ref(model, case):
    """(moves, values [S, M, 2], status, loglik): _nni_cases.nni_reference on grid_of(model)."""
    from _nni_cases import nni_reference
    return nni_reference(model, case, grid_of(model), trial_matrix=ExpmCache(case.Qs, case.node_q))


def profile_ref(model, case):
    """(values [S, N, 2], status, loglik): _profile_cases.profile_reference on grid_of(model)."""
    from _profile_cases import profile_reference
    return profile_reference(model, case, grid_of(model))


def spr_ref(model, case):
    """(moves, values [S, M, 2], status, loglik): _spr_cases.spr_reference."""
    from _spr_cases import spr_reference
    return spr_reference(model, case, FRACTIONS, radius_of(case.n),
                         trial_matrix=ExpmCache(case.Qs, case.node_q))


def place_ref(model, case):
    """(values [S, 2, N, 2, 1], status, loglik): _place_cases.place_reference, the dense query
    first, the state query second."""
    from _place_cases import place_reference
    return place_reference(model, case, queries_of(case.n), 'dense', FRACTIONS, PENDANT,
                           trial_matrix=ExpmCache(case.Qs, case.node_q))


def branch_ref(model, case):
    """(values [S, N, 2], status): _branch_cases.branch_reference."""
    from _branch_cases import branch_reference
    return branch_reference(model, case, coefs_of(case.n), check_sites=[0, 17])


def map_ref(model, case):
    """(states, log_joint, tied): _map_cases.map_reference on the model's transitions."""
    from _map_cases import full_observations, map_reference
    obs = full_observations(model.tree, case.obs_nodes, case.obs_lik, case.n)
    return map_reference(model.get_transitions(), obs, case.root_distn, model.tree.parent)


def sample_ref(model, case, seed, first_draw, ndraws):
    """(states, status, L): _sample_cases.numpy_sample on the oracle's L (the host's draw)."""
    from _posterior_cases import oracle_pmaps
    from _sample_cases import numpy_sample
    ta = model.tree
    esd = model.get_transitions()
    L = oracle_pmaps(ta.indices, ta.indptr, esd, _cols(model, case), case.obs_lik)
    states, status = numpy_sample(esd, L, case.root_distn, ta.parent, seed, first_draw, ndraws)
    return states, status, L


# ---- 5. the mixture and the partitioned forms ------------------------------------------------

def tree_of(case):
    from raoteh_amd import _tree
    return _tree.TreeArrays(case.T, case.root)


def factors_of(ta):
    """[N, 2] factors of every set's own lengths (row 0 zero): FACTORS on every branch."""
    from _partition_search_cases import device_factors
    return device_factors(FACTORS, ta.nnodes)


def form_queries(n):
    """(dense f64[1, S, n], states uint8[1, S]) of make_queries."""
    return make_queries(n, 12000 + n)


def form_coefs(n):
    """One coefficient matrix for the mixture and partitioned forms: their references take one
    expm_frechet per set, edge and matrix, a second at 128 states apiece."""
    return coefs_of(n)[:1]


def mix_refs(case, family):
    """The reference of `family` for a mix_case under site_weights(), from the module its own parity test uses
    (test_mixture_search_gpu.py, test_mixture_search2_gpu.py, test_mixture_expect_gpu.py)."""
    import _mixture_cases as mc
    import _mixture_search_cases as msc
    import _mixture_search2_cases as m2
    ta, c, w = tree_of(case), class_weights_of(case.n), site_weights()
    if family == 'profile':
        return msc.profile_reference(ta, case, c, factors_of(ta), w)
    if family == 'nni':
        return msc.nni_reference(ta, case, c, factors_of(ta), w)
    if family == 'spr':
        return m2.spr_reference(ta, case, c, FRACTIONS, radius_of(case.n), w)
    if family == 'place':
        return m2.place_reference(ta, case, c, queries_of(case.n), 'dense', FRACTIONS, PENDANT,
                                  weights=w)
    if family == 'branch':
        return mc.mixture_reference(ta, case, form_coefs(case.n), c, w, check=2)
    if family == 'gradient':
        one = case._replace(Q=case.Q[:, :1].copy(), node_q=np.zeros_like(case.node_q))
        return mc.mixture_reference(ta, one, mc.gradient_coefs(one.Q), c, w, check=0)
    raise KeyError(family)


def part_refs(case, family):
    """The reference of `family` for a part_case under site_weights() (test_partition_search_gpu.py,
    test_partition_search2_gpu.py, test_partition_reads_gpu.py, test_partition_gpu.py)."""
    import _partition_cases as pc
    import _partition_read_cases as prc
    import _partition_search_cases as psc
    import _partition_search2_cases as p2
    ta, w = tree_of(case), site_weights()
    if family == 'profile':
        return psc.profile_reference(ta, case, factors_of(ta), w)
    if family == 'nni':
        return psc.nni_reference(ta, case, factors_of(ta), w)
    if family == 'spr':
        return p2.spr_reference(ta, case, FRACTIONS, radius_of(case.n), w)
    if family == 'place':
        return p2.place_reference(ta, case, queries_of(case.n), 'dense', FRACTIONS, PENDANT,
                                  weights=w)
    if family == 'branch':
        return prc.partition_reference(ta, case, form_coefs(case.n), w, check=2)
    if family == 'gradient':
        one = case._replace(Q=case.Q[:, :1].copy(), node_q=np.zeros_like(case.node_q))
        return prc.partition_reference(ta, one, prc.gradient_coefs(one.Q), w, check=0)
    if family == 'totals':
        import types
        return pc.oracle(types.SimpleNamespace(tree=ta), case)
    raise KeyError(family)



# ---- 6. the plain form's branch-length gradient ----------------------------------------------

def gradient_case(n):
    """(case under its first rate matrix alone, branch lengths f64[N]) for branch_length_gradient,
    which wants one Q for all edges.  make_case's rate matrices are not normalised -- the mean exit
    rate is about 0.4 n -- so at the builder's branch lengths the tree is saturated above some
    60 states: the likelihood hardly depends on a length, the gradient is near zero (0.02 at
    n = 107), and the parity test's bound, 1e-13 of the largest entry of the gradient, falls below
    what f64 gives either side: scipy's expm_frechet route and t Q P in extended precision differ
    by 1.2e-13 there, absolute, with a bound of 2.2e-15.  The gradient is therefore taken with
    the builder's lengths read as expected numbers of changes, t_v / mean exit rate: gradients of
    250 to 5700 at n = 21 .. 128, the same two host routes 1e-13 to 1e-12 apart, a hundred times
    under the bound."""
    case = shared_q(plain_case(n))
    t = tree_of(case).branch_lengths() / (-np.diag(case.Qs[0]).mean())
    return case, t


def gradient_ref(n):
    """(analytic gradient f64[N], status) of _branch_cases.branch_reference with the gradient's
    coefficient matrix (ones off the diagonal, diag(Q) on it: the direction is Q itself), as
    test_branch_expect_gpu.py::test_branch_length_gradient builds its analytic value."""
    import types
    from _branch_cases import branch_reference
    from _partition_read_cases import _TreeWithLengths
    case, t = gradient_case(n)
    E = np.ones((n, n))
    np.fill_diagonal(E, np.diag(case.Qs[0]))
    model = types.SimpleNamespace(tree=_TreeWithLengths(tree_of(case), t))
    values, status = branch_reference(model, case, E[None])
    analytic = np.zeros(len(t))
    analytic[1:] = values[:, 1:, 0].sum(axis=0) / t[1:]
    return analytic, status
