"""
Generate tests/golden/branch_expectations.json: every call that the REFERENCE's own worked
example (examples/code2x3/run.py, main()) makes to the reference's own
extras.get_expected_ntransitions (examples/code2x3/extras.py:19-132), with its arguments and the
dict of per-edge expectations it returned.

run.py and extras.py are imported from the reference tree at run time and run unmodified;
get_expected_ntransitions is wrapped by a recorder.  The reference's dense modules import the
Cython extension ``pyfelscore``, which is not installed: a stand-in module supplies only the pass
functions those modules call, delegating to oracle/oracle_numpy.py (which tests/golden/ pins to
the reference's pure-Python twins).  Everything above that layer -- the model builders of run.py,
_mjp_dense.get_expm_augmented_tree, _mcy_dense.get_node_to_pmap, _mc0_dense.get_node_to_distn /
get_joint_endpoint_distn, scipy.linalg.expm_frechet and the sum over the endpoint states -- is
the reference's code.

Per call the file holds nstates, the tree edges with lengths, root_distn, the allowed sets, E as
a list of its non-zero entries and the expectation per edge; each process's rate matrix is
stored once (``Q``) and referred to by index.  Floats are written by repr (they round-trip).

    python tools/gen_golden_branch.py [--out tests/golden/branch_expectations.json]
"""
import argparse
import contextlib
import importlib
import importlib.util
import io
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import gen_golden                                   # noqa: E402  (helpers; no fixture is touched)
from oracle import oracle_numpy as orc              # noqa: E402

REF = gen_golden.REF

PROVENANCE = (
    "reference examples/code2x3/run.py main() run unmodified with the reference's own "
    "examples/code2x3/extras.get_expected_ntransitions (wrapped to record arguments and return "
    "value); the absent Cython extension pyfelscore replaced by a stand-in module whose pass "
    "functions (mcy_esd_get_node_to_pset, esd_get_node_to_set, mcy_esd_get_node_to_pmap, "
    "mc0_esd_get_node_to_distn, mc0_esd_get_joint_endpoint_distn) delegate to "
    "oracle/oracle_numpy.py; tools/gen_golden_branch.py")


def pyfelscore_stand_in():
    """Only the layer below the reference's dense modules: the passes, from the oracle."""
    mod = types.ModuleType('pyfelscore')

    def mcy_esd_get_node_to_pset(indices, indptr, esd, state_mask):
        orc.mcy_esd_get_node_to_pset(indices, indptr, esd, state_mask)

    def esd_get_node_to_set(indices, indptr, esd, state_mask):
        orc.esd_get_node_to_set(indices, indptr, esd, state_mask)

    def mcy_esd_get_node_to_pmap(indices, indptr, esd, state_mask, out):
        out[...] = orc.mcy_esd_get_node_to_pmap(indices, indptr, esd, state_mask)

    def mc0_esd_get_node_to_distn(indices, indptr, esd, root_distn, pmap, out):
        out[...] = orc.mc0_esd_get_node_to_distn(indices, indptr, esd, root_distn, pmap)

    def mc0_esd_get_joint_endpoint_distn(indices, indptr, esd, pmap, distn, out):
        out[...] = orc.mc0_esd_get_joint_endpoint_distn(indices, indptr, esd, pmap, distn)

    for f in (mcy_esd_get_node_to_pset, esd_get_node_to_set, mcy_esd_get_node_to_pmap,
              mc0_esd_get_node_to_distn, mc0_esd_get_joint_endpoint_distn):
        setattr(mod, f.__name__, f)
    return mod


def record_calls():
    gen_golden.import_reference()
    sys.modules['pyfelscore'] = pyfelscore_stand_in()
    for name in list(sys.modules):                  # (modules that bound the empty stand-in)
        if name.startswith('raoteh.sampler.') and getattr(sys.modules[name], 'pyfelscore', None):
            sys.modules[name].pyfelscore = sys.modules['pyfelscore']
    example = REF + '/examples/code2x3'
    sys.path.insert(0, example)
    try:
        extras = importlib.import_module('extras')
        original = extras.get_expected_ntransitions
        calls = []

        def recorder(T, node_to_allowed_states, root, nstates, root_distn=None, Q_default=None,
                     E=None):
            out = original(T, node_to_allowed_states, root, nstates, root_distn=root_distn,
                           Q_default=Q_default, E=E)
            calls.append(dict(T=T, allowed=node_to_allowed_states, root=root, nstates=nstates,
                              root_distn=root_distn, Q=Q_default, E=E, out=out))
            return out
        extras.get_expected_ntransitions = recorder
        spec = importlib.util.spec_from_file_location('code2x3_run', example + '/run.py')
        run = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(run)
        with contextlib.redirect_stdout(io.StringIO()):
            run.main()
    finally:
        sys.path.remove(example)
    return calls


def to_fixture(calls):
    mats, rows = [], []
    for c in calls:
        n = int(c['nstates'])
        T = c['T']
        for a, b in T.edges():
            assert 'Q' not in T[a][b], 'run.py puts no rate matrix on an edge'
        Q = np.asarray(c['Q'], dtype=float)
        for qi, M in enumerate(mats):
            if M.shape == Q.shape and np.array_equal(M, Q):
                break
        else:
            qi = len(mats)
            mats.append(Q)
        E = c['E']
        if E is not None:
            E = np.asarray(E, dtype=float)
            E = [[int(i), int(j), float(E[i, j])] for i, j in zip(*np.nonzero(E))]
        rows.append(dict(
            nstates=n, root=int(c['root']), q=qi,
            edges=[[int(a), int(b), float(T[a][b]['weight'])] for a, b in T.edges()],
            root_distn=None if c['root_distn'] is None else
            [float(x) for x in np.asarray(c['root_distn'])],
            allowed=dict((str(v), sorted(int(s) for s in ss)) for v, ss in c['allowed'].items()),
            E=E,
            expectations=[[int(a), int(b), float(x)] for (a, b), x in c['out'].items()]))
    return dict(provenance=PROVENANCE, Q=[M.tolist() for M in mats], calls=rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(os.path.dirname(HERE), 'tests', 'golden',
                                                  'branch_expectations.json'))
    args = ap.parse_args()
    calls = record_calls()
    fix = to_fixture(calls)
    with open(args.out, 'w') as f:
        json.dump(fix, f, separators=(',', ':'))
        f.write('\n')
    print('%d calls, states %s, %d rate matrices, %d bytes -> %s' % (
        len(calls), sorted(set(c['nstates'] for c in fix['calls'])), len(fix['Q']),
        os.path.getsize(args.out), args.out))


if __name__ == '__main__':
    main()
