"""The host rule of the carried root combine (csrc/common.h: rt_carry_combine_plan and
rt_carry_tile, exported as rt_carry_combine_deal): which pending batch an expm launch of G matrix
workgroups carries, and which tile each of its idle waves finishes.  No device needed."""
import ctypes

import numpy as np
import pytest

from raoteh_amd import _lib


def _deal(nt, nblocks, G, halves=1, rescale=0, part=0, multi=0, table=True):
    out = np.full(4 * max(G, 1), -7, dtype=np.int64)
    ok = _lib.lib().rt_carry_combine_deal(nt, nblocks, G, halves, rescale, part, multi,
                                          out.ctypes.data_as(ctypes.POINTER(ctypes.c_int64))
                                          if table else None)
    return ok, out


# (tiles, matrix workgroups): the 10 000-site batch on the 64-leaf tree's two-workgroup launch,
# fewer tiles than workgroups, exactly one and exactly four rounds' worth, a single workgroup
@pytest.mark.parametrize('nblocks,G', [(625, 252), (3, 18), (1, 18), (18, 18), (72, 18), (71, 18),
                                       (4, 1), (1, 1), (1008, 252)])
def test_every_tile_is_dealt_exactly_once(nblocks, G):
    ok, out = _deal(4, nblocks, G)
    assert ok == 1
    dealt = out[out >= 0]
    assert sorted(dealt.tolist()) == list(range(nblocks))
    assert (out[out < 0] == -1).all()
    # wave k of workgroup g: tile g + k G
    for g in range(G):
        for k in range(4):
            t = g + k * G
            assert out[4 * g + k] == (t if t < nblocks else -1)


@pytest.mark.parametrize('nblocks,G', [(1009, 252), (73, 18), (5, 1), (2500, 252)])
def test_more_than_one_round_is_refused(nblocks, G):
    ok, out = _deal(4, nblocks, G)
    assert ok == 0
    assert (out == -7).all()                 # (nothing is dealt on a refusal)


@pytest.mark.parametrize('nt', [1, 2, 3, 5, 8])
def test_other_row_tile_counts_are_refused(nt):
    assert _deal(nt, 10, 18)[0] == 0


def test_only_plain_root_halves_are_carried():
    assert _deal(4, 10, 18, table=False)[0] == 1
    assert _deal(4, 10, 18, halves=0)[0] == 0
    assert _deal(4, 10, 18, rescale=1)[0] == 0
    assert _deal(4, 10, 18, part=1)[0] == 0
    assert _deal(4, 10, 18, multi=1)[0] == 0
    assert _deal(4, 10, 0)[0] == 0           # a launch that is not the carrying kernel
    assert _deal(4, 0, 18)[0] == 0
