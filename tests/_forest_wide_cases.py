"""tests/golden/forest_wide.json (tools/gen_golden_forest_wide.py) decoded once for the CPU and
the GPU tests of the Rao-Teh passes at 65 to 128 states."""
import functools

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
