"""
Generate tests/golden/forest_wide.json: the Rao-Teh sweep core on chunk trees with ONE shared
matrix at 65 to 128 states -- the recipe of gen_golden.fixture_forest (random trees with random
event nodes cut into the reference's chunk tree, _graph_transform.get_chunk_tree_type_b; a
uniformized P = I + Q / omega of a sparse random rate matrix with a cyclic support; allowed sets
on some chunk nodes; a random root distribution, sometimes with a zero) above the 64 states one
mask word holds.

Per case the reference gives pset (_mcy.unaccelerated_get_node_to_pset), set
(_mc0.get_node_to_set_unaccelerated), pmap (_mcy.unaccelerated_get_node_to_pmap), the
likelihood or the zero flag, and the exact node marginals (_mc0.get_node_to_distn).

State counts 65, 96, 122, 128, two cases of positive likelihood each (a draw whose sets leave
no history is drawn again: with a sparse P most random restrictions do), one more case at 96
states that is a structural zero by construction (two neighbouring chunks pinned to states
without a transition between them) and one single-chunk case at 122.  The allowed sets are
single states, sets inside the low word (states < 64), sets inside the high word (states >= 64)
and sets that straddle both.

To keep the file small, the rate matrix of a state count is drawn once and shared by its cases
(``matrices``; a case refers to it by index, as branch_expectations.json does), and the inputs
are binary fractions: rates are multiples of 1/16, omega is the power of two at or above twice
the largest total rate (so P = I + Q / omega is exact and its entries print short), the root
distribution is counts out of 1024.  P and Q are stored as lists of their non-zero entries
[row, column, value], pmap and distn as lists of [state, value] per node.  Floats are written by
repr (they round-trip).

    python tools/gen_golden_forest_wide.py [--out tests/golden/forest_wide.json]
"""
import argparse
import importlib
import json
import os
import sys

import networkx as nx
import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden                                   # noqa: E402  (helpers; no fixture is touched)

PROVENANCE = (
    "reference raoteh/sampler: _graph_transform.get_chunk_tree_type_b, "
    "_mcy.unaccelerated_get_node_to_pset, _mc0.get_node_to_set_unaccelerated, "
    "_mcy.unaccelerated_get_node_to_pmap, _mc0.get_likelihood, _mc0.get_node_to_distn with "
    "P_default = I + Q / omega on every edge, run unmodified on random inputs (numpy "
    "RandomState(6512)); tools/gen_golden_forest_wide.py")

STATE_COUNTS = (65, 96, 122, 128)
CASES_PER_COUNT = 2


def sparse_matrix(M):
    return [[int(i), int(j), float(M[i, j])] for i, j in zip(*np.nonzero(M))]


def sparse_rows(d):
    return dict((str(int(v)), [[int(s), float(x)] for s, x in sorted(m.items()) if x])
                for v, m in d.items())


def random_allowed(rng, n):
    """One restricted set: a single state, a set in the low word, in the high word, or across."""
    kind = rng.randint(4)
    if kind == 0:
        return {int(rng.randint(n))}
    if kind == 1:
        return set(int(x) for x in rng.choice(64, size=int(rng.randint(2, 33)), replace=False))
    if kind == 2:
        k = int(rng.randint(1, min(32, n - 64) + 1))
        return set(64 + int(x) for x in rng.choice(n - 64, size=k, replace=False))
    low = set(int(x) for x in rng.choice(64, size=int(rng.randint(1, 25)), replace=False))
    k = int(rng.randint(1, min(24, n - 64) + 1))
    return low | set(64 + int(x) for x in rng.choice(n - 64, size=k, replace=False))


def rate_matrix(rng, n):
    """Sparse rate matrix with a connected support (a cycle) plus about one random extra a row,
    rates in sixteenths; -> (Q, omega, P = I + Q / omega), all exact."""
    Q = np.zeros((n, n))
    for i in range(n):
        Q[i, (i + 1) % n] = rng.randint(2, 33) / 16.0
    extra = rng.uniform(size=(n, n)) < 1.0 / n
    Q += extra * (rng.randint(1, 33, size=(n, n)) / 16.0)
    np.fill_diagonal(Q, 0.0)
    Q -= np.diag(Q.sum(axis=1))
    omega = 2.0 ** np.ceil(np.log2(2.0 * (-np.diag(Q)).max()))
    return Q, float(omega), np.identity(n) + Q / omega


def one_case(mods, _gt, rng, n, matrix, P, single=False, zero=False):
    _mc0, _mcy, _util = mods['_mc0'], mods['_mcy'], mods['_util']
    P_nx = gen_golden.dense_to_nx(P)
    nnodes = int(rng.randint(3, 12))
    T = nx.Graph()
    T.add_node(0)
    for k in range(1, nnodes):
        T.add_edge(int(rng.randint(k)), k)
    events = set() if single else set(int(v) for v in range(1, nnodes) if rng.uniform() < 0.6)
    if zero and not events:
        events = {1}
    chunk_tree, edge_to_chunk, event_to_edge = _gt.get_chunk_tree_type_b(T, 0, events)
    root = 0
    nodes = list(chunk_tree)
    allowed = dict((v, set(range(n))) for v in nodes)
    for v in nodes:
        if rng.uniform() < 0.4:
            allowed[v] = random_allowed(rng, n)
    if zero:
        a, b = next(iter(nx.bfs_edges(chunk_tree, root)))
        sa = int(rng.randint(n))
        sb = int(rng.choice(np.nonzero(P[sa] == 0)[0]))
        allowed[a], allowed[b] = {sa}, {sb}
    w = rng.exponential(size=n)
    if rng.uniform() < 0.3:
        w[rng.randint(n)] = 0.0
    distn = rng.multinomial(1024, w / w.sum()) / 1024.0
    distn_dict = dict((i, float(p)) for i, p in enumerate(distn) if p)
    rec = dict(nstates=n, matrix=matrix,
               tree_edges=[[int(a), int(b)] for a, b in T.edges()],
               event_nodes=sorted(events),
               chunk_nodes=[int(v) for v in nodes],
               chunk_edges=[[int(a), int(b)] for a, b in nx.bfs_edges(chunk_tree, root)]
               if len(nodes) > 1 else [],
               root=root, root_distn=distn.tolist(),
               # (a chunk node that is not listed is unrestricted)
               allowed=gen_golden.set_json(dict((v, ss) for v, ss in allowed.items()
                                                if len(ss) < n)))
    if len(nodes) == 1:
        rec['single'] = True            # the reference's passes need at least one edge
        return rec
    pset = _mcy.unaccelerated_get_node_to_pset(
        chunk_tree, root, node_to_allowed_states=allowed, P_default=P_nx)
    nset = _mc0.get_node_to_set_unaccelerated(chunk_tree, root, pset, P_default=P_nx)
    pmap = _mcy.unaccelerated_get_node_to_pmap(
        chunk_tree, root, node_to_allowed_states=allowed, node_to_set=nset, P_default=P_nx)
    rec['pset'] = gen_golden.set_json(pset)
    rec['set'] = gen_golden.set_json(nset)
    rec['pmap'] = sparse_rows(pmap)
    try:
        rec['likelihood'] = _mc0.get_likelihood(pmap[root], root_distn=distn_dict)
        rec['zero'] = False
        nd = _mc0.get_node_to_distn(chunk_tree, root, pmap, root_distn=distn_dict,
                                    P_default=P_nx)
        rec['distn'] = sparse_rows(nd)
    except _util.StructuralZeroProb:
        rec['likelihood'] = 0.0
        rec['zero'] = True
    return rec


def build():
    mods = gen_golden.import_reference()
    _gt = importlib.import_module('raoteh.sampler._graph_transform')
    rng = np.random.RandomState(6512)
    cases, matrices, dense = [], [], {}
    for n in STATE_COUNTS:
        Q, omega, P = rate_matrix(rng, n)
        dense[n] = (len(matrices), P)
        matrices.append(dict(nstates=n, omega=omega, Q=sparse_matrix(Q), P=sparse_matrix(P)))
        for k in range(CASES_PER_COUNT):
            rec = one_case(mods, _gt, rng, n, *dense[n])
            while rec.get('single') or rec['zero']:
                rec = one_case(mods, _gt, rng, n, *dense[n])
            cases.append(rec)
    cases.append(one_case(mods, _gt, rng, 96, *dense[96], zero=True))
    cases.append(one_case(mods, _gt, rng, 122, *dense[122], single=True))
    assert any(c.get('single') for c in cases)
    assert any(c.get('zero') for c in cases)
    assert any(not c.get('single') and not c['zero'] for c in cases)
    return dict(provenance=PROVENANCE, matrices=matrices, cases=cases)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'tests', 'golden',
                                                  'forest_wide.json'))
    args = ap.parse_args()
    fix = build()
    with open(args.out, 'w') as f:
        json.dump(fix, f, separators=(',', ':'))
        f.write('\n')
    print('%d cases, states %s, %d zero, %d single, %d bytes -> %s' % (
        len(fix['cases']), sorted(set(c['nstates'] for c in fix['cases'])),
        sum(1 for c in fix['cases'] if c.get('zero')),
        sum(1 for c in fix['cases'] if c.get('single')), os.path.getsize(args.out), args.out))


if __name__ == '__main__':
    main()
