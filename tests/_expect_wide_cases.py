"""tests/golden/expectations_wide.json (tools/gen_golden.py, fixture_expectations_wide) rebuilt
into trees, dense rate matrices and allowed-state sets (test_expect_wide_cpu.py,
test_expect_wide_gpu.py)."""
import networkx as nx
import numpy as np

from conftest import load_golden


def wide_cases():
    """-> list of dict(name, T, root, n, mats, Q_default, allowed, root_distn, dwell, init,
    trans f64[n, n], live bool[n, n] (the nonzero rates the reference reports), seconds)."""
    out = []
    for c in load_golden('expectations_wide')['cases']:
        n = c['nstates']
        mats = []
        for triples in c['Q_offdiagonal']:
            R = np.zeros((n, n))
            for a, b, v in triples:
                R[a, b] = v
            mats.append(R - np.diag(R.sum(axis=1)))
        T = nx.Graph()
        for a, b, w, q in c['edges']:
            T.add_edge(int(a), int(b), weight=float(w))
            if q:
                T[int(a)][int(b)]['Q'] = mats[q]
        allowed = dict((int(v), set(ss)) for v, ss in c['allowed'].items())
        trans = np.zeros((n, n))
        live = np.zeros((n, n), dtype=bool)
        for a, b, v in c['trans']:
            trans[a, b] = v
            live[a, b] = True
        out.append(dict(name=c['name'], T=T, root=c['root'], n=n, mats=mats, Q_default=mats[0],
                        allowed=allowed, root_distn=np.array(c['root_distn']),
                        dwell=np.array(c['dwell']), init=np.array(c['init']), trans=trans,
                        live=live, seconds=c['reference_seconds']))
    return out
