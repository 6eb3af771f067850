"""The two-team form of the pipelined split-M pruning kernel (csrc/jit.hip: eight waves per
workgroup, chains split (2,1), (2,2) or (3,2) over two four-wave teams): what can be checked
without a device.  Its text goes through hiprtc for gfx950 with the product's options and must
fit two waves per SIMD -- at most 256 registers, no scratch, no spills -- and without the knob
the generator's text holds none of the team code."""
import ctypes
import re
import subprocess

import numpy as np
import pytest

from raoteh_amd import _lib

KNOBS = ('RAOTEH_JIT_TILES', 'RAOTEH_JIT_QUAD', 'RAOTEH_JIT_HALVES', 'RAOTEH_JIT_FOLD',
         'RAOTEH_JIT_SOURCE_SPARSE', 'RAOTEH_JIT_SOURCE_STATES', 'RAOTEH_JIT_SOURCE_MULTI',
         'RAOTEH_JIT_SPLIT', 'RAOTEH_JIT_TEAMS', 'RAOTEH_JIT_TRACE', 'RAOTEH_JIT_GATHER_AHEAD')
READELF = '/opt/rocm/lib/llvm/bin/llvm-readelf'

# (label, environment, has a combine kernel)
FORMS = [
    ('halves T3', {'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '3'}, True),
    ('halves T4', {'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '4'}, True),
    ('halves T5', {'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '5'}, True),
    ('whole tree T3', {'RAOTEH_JIT_TILES': '3'}, False),
    ('halves T5 multi', {'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '5',
                         'RAOTEH_JIT_SOURCE_MULTI': '1'}, True),
]


def _source(env, monkeypatch, n=61, levels=6):
    """The generator's text for the balanced tree of 2**levels leaves, n states."""
    from raoteh_amd import synth
    from raoteh_amd._tree import TreeArrays
    for name in KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    p64 = ctypes.POINTER(ctypes.c_int64)
    buf = ctypes.create_string_buffer(1 << 25)
    T, root, leaves = synth.balanced_tree(2 ** levels, seed=3)
    ta = TreeArrays(T, root)
    obs = np.array(sorted(ta.node_to_index[v] for v in leaves), dtype=np.int64)
    _lib.check(_lib.lib().rt_jit_source(
        ta.nnodes, ta.indices.ctypes.data_as(p64), ta.indptr.ctypes.data_as(p64), n, len(obs),
        obs.ctypes.data_as(p64), 2, buf, len(buf)))
    return buf.value


def _kernels(code, tmp_path, label):
    """{kernel name: its metadata as a dict of ints} from the notes of a code object."""
    path = tmp_path / ('%s.co' % label.replace(' ', '_'))
    path.write_bytes(code)
    notes = subprocess.run([READELF, '--notes', str(path)], stdout=subprocess.PIPE,
                           check=True).stdout.decode()
    out = {}
    for block in notes.split('- .agpr_count:')[1:]:
        block = '.agpr_count:' + block
        name = re.search(r'\.name:\s+(\S+)', block).group(1)
        out[name] = {k: int(v) for k, v in re.findall(r'\.(\w+):\s+(\d+)\s*$', block, re.M)}
    return out


@pytest.mark.parametrize('k', range(len(FORMS)))
def test_team_form_fits_two_waves_per_simd(k, tmp_path, monkeypatch):
    """64-leaf balanced tree, 61 states: root halves at 3, 4 and 5 tiles, the whole tree at 3,
    and the one-launch (multi) form at 5: rt_jit_prune (and rt_jit_combine with halves) are
    there; VGPR + AGPR <= 256, scratch 0, spills 0, static LDS <= 160 KB."""
    from test_host_cpu import _hiprtc_compile
    label, env, combine = FORMS[k]
    src = _source(dict(env, RAOTEH_JIT_TEAMS='1'), monkeypatch)
    assert b'team' in src and b'__launch_bounds__(512)' in src, label
    assert b'amdgpu_waves_per_eu(2, 2)' in src, label
    kern = _kernels(_hiprtc_compile(src, vgpr_form=True), tmp_path, label)
    assert 'rt_jit_prune' in kern and ('rt_jit_combine' in kern) == combine, sorted(kern)
    for name, md in kern.items():
        print(label, name, {key: md.get(key) for key in (
            'vgpr_count', 'agpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
            'private_segment_fixed_size', 'group_segment_fixed_size', 'max_flat_workgroup_size')})
        assert md['private_segment_fixed_size'] == 0, (label, name, md)
        assert md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, (label, name, md)
        assert md['group_segment_fixed_size'] <= 160 * 1024, (label, name, md)
    md = kern['rt_jit_prune']
    # VGPR + AGPR <= 256: .vgpr_count is the unified file's total on gfx950 (the accumulation
    # registers, placed behind the vector registers, are part of it)
    assert md['agpr_count'] <= md['vgpr_count'] <= 256, (label, md)
    assert md['max_flat_workgroup_size'] == 512, (label, md)


@pytest.mark.parametrize('k', range(len(FORMS)))
def test_without_the_knob_the_text_holds_no_team_code(k, monkeypatch):
    label, env, _ = FORMS[k]
    for off in ({'RAOTEH_JIT_TEAMS': '0'}, {}):
        src = _source(dict(env, **off), monkeypatch)
        assert b'team' not in src and b'__launch_bounds__(512)' not in src, label
        assert b'__launch_bounds__(256)' in src, label


def test_team_bodies_are_the_one_team_chains(monkeypatch):
    """Every chain's products are those of the one-team form, statement for statement, and each
    body holds the barriers of the one-team program (the workgroup's barriers are shared by the
    two teams, so both bodies must execute the same number)."""
    env = {'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '5'}
    one = _source(env, monkeypatch).decode()
    two = _source(dict(env, RAOTEH_JIT_TEAMS='1'), monkeypatch).decode()
    one, two = one[:one.index('rt_jit_combine')], two[:two.index('rt_jit_combine')]
    mfma = lambda text: sorted(l for l in text.split('\n') if '__builtin_amdgcn_mfma_f64' in l)
    assert len(mfma(one)) == 2 * 63 * 16 * 5 and mfma(one) == mfma(two)
    publish = lambda text: sorted(l for l in text.split('\n') if l.startswith('    xb'))
    assert publish(one) == publish(two)
    assert two.count('__syncthreads()') == 2 * one.count('__syncthreads()') > 100
    assert two.count('if (team == 0) {') == 2


def test_forms_without_teams_return_nothing(monkeypatch):
    """Two tiles per workgroup already run two workgroups per CU, and fewer than 49 states are
    fewer than four waves: no team form; the caller falls back on the empty text."""
    for env, n in (({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '2'}, 61),
                   ({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '3'}, 48),
                   ({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '3', 'RAOTEH_JIT_FOLD': '1'}, 61)):
        assert _source(dict(env, RAOTEH_JIT_TEAMS='1'), monkeypatch, n=n, levels=3) == b''
