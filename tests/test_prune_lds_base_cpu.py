"""RAOTEH_JIT_LDS_BASE (csrc/jit.hip, rt_jit_mfma_split_pipelined_source): the x buffers of the
pipelined NT = 4 forms at three or more tiles per workgroup through six opaque base pointers per
body, B operands as named values read ahead in the text -- what can be checked without a device.
With the knob off the generator's text is the text it was before the knob existed (hashes recorded from that commit, over the knob matrix of test_prune_teams_cpu.py); with
it on, the team forms compile for gfx950 without scratch into at most 256 registers, both bodies
of a program hold the same number of barriers, and no body addresses LDS through more than 12
distinct registers (before: 55 and 83 in the two bodies of the 64-leaf tree at T = 5)."""
import hashlib
import re
import subprocess

import pytest

from test_prune_teams_cpu import FORMS, _kernels, _source

OBJDUMP = '/opt/rocm/lib/llvm/bin/llvm-objdump'

# sha256 of rt_jit_source's text at the commit before this knob: 64-leaf balanced tree (seed 3),
# 61 states; label of test_prune_teams_cpu.FORMS -> RAOTEH_JIT_TEAMS = '1' / ('0' or unset)
BEFORE = {
    'halves T3': ('83243566f5ea78b9dae9f2a0740d6142bf54769650751fc20386c9a5ad0717a8',
                  '2b1ecc2856d2ca9e170c3ef321d75b8e3c32c124d961e85acb4fbe6ddcfdf15d'),
    'halves T4': ('173f3cb14370f2569fd79f7734db045075a920cf6407d95e64ee2a3da66ef034',
                  '9e9b373be80d3c1c58e9b2a4ea1db263bde737560a7a4736395036c0bb22a966'),
    'halves T5': ('25ef2461ff4959e4ecb873199b2b9bbb67e94d1c5f3428de3585469b0395222b',
                  '730890ed1d42d7730e0404f3c86449746ac62ffe1bcb1a64aa8c96a63e1f1113'),
    'whole tree T3': ('62744140aa71f47c3b5fc5347d0d991d4454bc7d366f9316c2ff78d43b9ca88d',
                      '6319d54e43cee0a24038f0eacb7b1ea89bb6a85502c00591c9a02d2c006590ce'),
    'halves T5 multi': ('df45f8c9759fdd03f70045c429e474715156f7c90b88054f9a5ddcf70c4e4815',
                        '74190abad58561aebbb5a6ffdcea6a2bc181828f0beee526aaf4897f7a26404e'),
}
NEW_KNOBS = ('RAOTEH_JIT_LDS_BASE', 'RAOTEH_JIT_LDS_AHEAD', 'RAOTEH_JIT_LDS_PIN')


def _text(env, monkeypatch, **kw):
    for name in NEW_KNOBS:
        monkeypatch.delenv(name, raising=False)
    return _source(env, monkeypatch, **kw)


@pytest.mark.parametrize('k', range(len(FORMS)))
def test_knob_off_is_the_text_before_the_knob(k, monkeypatch):
    label, env, _ = FORMS[k]
    for teams, want in (('1', BEFORE[label][0]), ('0', BEFORE[label][1]), (None, BEFORE[label][1])):
        e = dict(env, RAOTEH_JIT_LDS_BASE='0')
        if teams is not None:
            e['RAOTEH_JIT_TEAMS'] = teams
        src = _text(e, monkeypatch)
        assert hashlib.sha256(src).hexdigest() == want, (label, teams)
        on = _text({k2: v for k2, v in e.items() if k2 != 'RAOTEH_JIT_LDS_BASE'}, monkeypatch)
        assert on != src and b'rt_lds rb0' in on and b'rt_lds' not in src, (label, teams)


def test_forms_with_a_small_x_image_keep_their_text(monkeypatch):
    """Two tiles per workgroup (48 KB of x) and three waves (48 states): the knob changes nothing."""
    for env, n in (({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '2'}, 61),
                   ({'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '3'}, 48)):
        off = _text(dict(env, RAOTEH_JIT_LDS_BASE='0'), monkeypatch, n=n, levels=3)
        assert off and off == _text(env, monkeypatch, n=n, levels=3) and b'rt_lds' not in off


def _bodies(dis):
    """The straight-line pieces of rt_jit_prune that hold the chains: (MFMAs, barriers, the
    registers its LDS instructions take their address from) of each."""
    text = dis[dis.index('<rt_jit_prune>:'):]
    nxt = re.search(r'^[0-9a-f]+ <\w+>:', text[20:], re.M)
    if nxt:
        text = text[:20 + nxt.start()]
    out = []
    for piece in re.split(r'\n\s+s_c?branch\w*[^\n]*', text):
        mfma = len(re.findall(r'v_mfma_f64', piece))
        if mfma < 100:
            continue
        regs = set(re.findall(r'\bds_read\w*\s+(?:v\[\d+:\d+\]|v\d+),\s*(v\d+)', piece))
        regs |= set(re.findall(r'\bds_write\w*\s+(v\d+),', piece))
        out.append((mfma, len(re.findall(r's_barrier', piece)), sorted(regs)))
    return out


# (label, environment, bodies: root programs x teams, chains of team 0 / team 1)
COMPILED = [
    ('halves T5', {'RAOTEH_JIT_HALVES': '1', 'RAOTEH_JIT_TILES': '5'}, 4, (3, 2)),
    ('whole tree T3', {'RAOTEH_JIT_TILES': '3'}, 2, (2, 1)),
]


@pytest.mark.parametrize('k', range(len(COMPILED)))
def test_base_pointer_form_compiles_into_two_waves_per_simd(k, tmp_path, monkeypatch):
    """8-leaf balanced tree, 61 states, the knob on (its default): no scratch, at most 256
    registers, equal barrier counts in the two bodies of a program, at most 12 LDS address
    registers per body, and every B operand a named value read ahead of its MFMA."""
    from test_host_cpu import _hiprtc_compile
    label, env, nbodies, chains = COMPILED[k]
    src = _text(dict(env, RAOTEH_JIT_TEAMS='1'), monkeypatch, levels=3)
    assert b'rt_lds rb0' in src and b'B operands 2 k-steps ahead' in src
    head = src[:src.index(b'rt_jit_combine')] if b'rt_jit_combine' in src else src
    assert not re.search(rb'mfma_f64_16x16x4f64\(A\w+\.[xy], (?!b\d+_\d+_\d+,)', head), label
    code = _hiprtc_compile(src, vgpr_form=True)
    md = _kernels(code, tmp_path, label)['rt_jit_prune']
    print(label, {key: md.get(key) for key in ('vgpr_count', 'agpr_count', 'vgpr_spill_count',
                                               'private_segment_fixed_size')})
    assert md['private_segment_fixed_size'] == 0, (label, md)
    assert md.get('vgpr_spill_count', 0) == 0 and md.get('sgpr_spill_count', 0) == 0, (label, md)
    assert md['agpr_count'] <= md['vgpr_count'] <= 256, (label, md)
    path = tmp_path / ('%s.co' % label.replace(' ', '_'))
    dis = subprocess.run([OBJDUMP, '-d', str(path)], stdout=subprocess.PIPE, check=True).stdout.decode()
    bodies = _bodies(dis)
    print(label, [(m, b, len(r)) for m, b, r in bodies])
    assert len(bodies) == nbodies, (label, [(m, b) for m, b, _ in bodies])
    for team0, team1 in zip(bodies[0::2], bodies[1::2]):
        assert team0[1] == team1[1] > 0, (label, team0[:2], team1[:2])           # barriers
        lo, hi = sorted((team0[0], team1[0]))                                    # MFMAs: 2 : 3, 1 : 2
        assert lo * max(chains) == hi * min(chains), (label, team0[0], team1[0])
    for mfma, _, regs in bodies:
        assert 0 < len(regs) <= 12, (label, mfma, regs)
