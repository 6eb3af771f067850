"""Rate sets (TreeModel.set_rate_sets): what can be checked without a device -- the shape
checks of the Python helpers and the new entry points of the library."""
import numpy as np
import pytest

from raoteh_amd import device, _lib


def test_the_library_exports_the_rate_set_entry_points():
    lib = _lib.lib()
    for name in ('rt_model_set_rate_sets', 'rt_step_multi', 'rt_sites_get_multi_logliks',
                 'rt_sites_get_multi_totals', 'rt_sites_multi_mixture',
                 'rt_sites_multi_kernel_name'):
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    assert _lib.RT_MAX_RATE_SETS == 64
    assert lib.rt_sites_multi_kernel_name(None) == b''
    # argument checks that come before any device call
    assert lib.rt_model_set_rate_sets(None, 1, None, 1, None, None) == _lib.RT_ERR_INVALID
    assert lib.rt_step_multi(None, None, 1) == _lib.RT_ERR_INVALID
    assert lib.rt_sites_get_multi_logliks(None, None, None) == _lib.RT_ERR_INVALID
    assert lib.rt_sites_get_multi_totals(None, None, None) == _lib.RT_ERR_INVALID
    assert lib.rt_sites_multi_mixture(None, None, None, None, None) == _lib.RT_ERR_INVALID


def test_check_rate_sets_shapes():
    n, N = 5, 9
    Q3, Q4 = np.zeros((3, n, n)), np.zeros((3, 2, n, n))
    t1, t2 = np.arange(N, dtype=float), np.ones((3, N))
    nodeq = np.zeros(N, dtype=np.int64)
    Q, t, q = device.check_rate_sets(Q3, t1, None, n, N)
    assert Q.shape == (3, 1, n, n) and t.shape == (3, N) and q is None
    assert Q.flags.c_contiguous and t.flags.c_contiguous and (t == t1).all()
    Q, t, q = device.check_rate_sets(Q4, t2, nodeq, n, N)
    assert Q.shape == (3, 2, n, n) and t.shape == (3, N) and q.dtype == np.int64
    # (the root's entry of node_q is not an edge: anything goes there)
    rootq = nodeq.copy()
    rootq[0] = -1
    device.check_rate_sets(Q4, t2, rootq, n, N)
    bad = [
        (np.zeros((n, n)), t1, None),                  # no set axis
        (np.zeros((3, n, n + 1)), t1, None),           # not square
        (np.zeros((3, n + 1, n + 1)), t1, None),       # another number of states
        (np.zeros((3, 2, 2, n, n)), t1, None),         # too many axes
        (np.zeros((0, n, n)), np.zeros((0, N)), None),          # K = 0
        (np.zeros((65, n, n)), np.zeros((65, N)), None),        # K = 65
        (Q3, np.ones(N + 1), None),                    # t of another tree
        (Q3, np.ones((2, N)), None),                   # t for another K
        (Q3, np.ones((3, N, 1)), None),
        (Q4, t2, None),                                # two matrices per set, no node_q
        (Q4, t2, np.zeros(N + 1, dtype=np.int64)),     # node_q of another tree
        (Q4, t2, np.full(N, 2, dtype=np.int64)),       # node_q out of range
        (Q4, t2, np.full(N, -1, dtype=np.int64)),
    ]
    for Qb, tb, qb in bad:
        with pytest.raises(ValueError):
            device.check_rate_sets(Qb, tb, qb, n, N)
    device.check_rate_sets(np.zeros((64, n, n)), t1, None, n, N)


def test_check_class_weights():
    c = device.check_class_weights([0.0, 0.5, 2.0], 3)
    assert c.dtype == np.float64 and c.shape == (3,)
    for bad in ([0.5, 0.5], [[0.5, 0.5, 0.0]], [0.0, 0.0, 0.0], [-0.1, 1.0, 1.0],
                [np.nan, 1.0, 1.0], [np.inf, 1.0, 1.0]):
        with pytest.raises(ValueError):
            device.check_class_weights(bad, 3)


KNOBS = ('RAOTEH_JIT_TILES', 'RAOTEH_JIT_QUAD', 'RAOTEH_JIT_HALVES', 'RAOTEH_JIT_FOLD',
         'RAOTEH_JIT_SOURCE_SPARSE', 'RAOTEH_JIT_SOURCE_STATES', 'RAOTEH_JIT_SOURCE_MULTI',
         'RAOTEH_JIT_SPLIT')

# (states, environment, has a combine kernel): (61, T2), (61, T3, halves), (48, halves, fold),
# (61, halves, pipelined leaf-state)
MULTI_FORMS = [
    (61, {'RAOTEH_JIT_TILES': '2'}, False),
    (61, {'RAOTEH_JIT_TILES': '3', 'RAOTEH_JIT_HALVES': '1'}, True),
    (48, {'RAOTEH_JIT_TILES': '2', 'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_FOLD': '1'}, True),
    (61, {'RAOTEH_JIT_TILES': '2', 'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_SOURCE_SPARSE': 'pipe'},
     True),
]


def _source(n, env, monkeypatch, seed):
    import ctypes
    from raoteh_amd import synth
    from raoteh_amd._tree import TreeArrays
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    p64 = ctypes.POINTER(ctypes.c_int64)
    buf = ctypes.create_string_buffer(1 << 24)
    T, root, leaves = synth.balanced_tree(8, seed=seed)
    ta = TreeArrays(T, root)
    obs = np.array(sorted(ta.node_to_index[v] for v in leaves), dtype=np.int64)
    _lib.check(_lib.lib().rt_jit_source(
        ta.nnodes, ta.indices.ctypes.data_as(p64), ta.indptr.ctypes.data_as(p64), n, len(obs),
        obs.ctypes.data_as(p64), 2, buf, len(buf)))
    return buf.value


@pytest.mark.parametrize('k', range(len(MULTI_FORMS)))
def test_multi_form_source_compiles_for_gfx950(k, tmp_path, monkeypatch):
    """RAOTEH_JIT_SOURCE_MULTI=1: the split-M family's one-launch form goes through hiprtc for
    gfx950 with the product's options: no scratch, no spills, the kernels the library looks up;
    the prologue costs no vector register; and without the knob the text is what it was."""
    import re
    import subprocess
    from test_host_cpu import _hiprtc_compile
    n, env, combine = MULTI_FORMS[k]
    readelf = '/opt/rocm/lib/llvm/bin/llvm-readelf'
    plain = _source(n, env, monkeypatch, k)
    multi = _source(n, dict(env, RAOTEH_JIT_SOURCE_MULTI='1'), monkeypatch, k)
    for word in (b'blockIdx.y', b'ms_table', b'ms_site', b'rset'):
        assert word not in plain and word in multi, word
    # the multi form is the plain form plus the strides and the prologue, nothing else
    text = re.sub(br',\n\s+long ms_table[^)]*', b'', multi)
    kept = [l for l in text.split(b'\n')
            if b'rset' not in l and b'rate set of this workgroup' not in l]
    assert b'\n'.join(kept) == plain
    stats = {}
    for label, src in (('plain', plain), ('multi', multi)):
        path = tmp_path / ('%s.co' % label)
        path.write_bytes(_hiprtc_compile(src, vgpr_form=True))
        notes = subprocess.run([readelf, '--notes', str(path)], stdout=subprocess.PIPE,
                               check=True).stdout.decode()
        names = re.findall(r'\.name:\s+(\S+)', notes)
        assert 'rt_jit_prune' in names and ('rt_jit_combine' in names) == combine, names
        scratch = [int(v) for v in re.findall(r'\.private_segment_fixed_size:\s+(\d+)', notes)]
        spills = [int(v) for v in re.findall(r'\.vgpr_spill_count:\s+(\d+)', notes)]
        assert scratch and max(scratch) == 0 and max(spills + [0]) == 0, (label, scratch, spills)
        stats[label] = [int(v) for v in re.findall(r'\.vgpr_count:\s+(\d+)', notes)]
    print('vgpr counts', stats)
    assert stats['multi'] == stats['plain'], stats
