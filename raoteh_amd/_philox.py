"""
Philox4x32-10 (Salmon et al. 2011) in numpy: the counter-based generator of the device's
sampling kernels (csrc/philox.h), restated on the host.  ``philox_uniform(seed, draw, index)``
gives the uniform the device uses for draw number `draw` (a sweep of rt_forest_resample_states,
first_draw + d of rt_sites_sample_states) and counter index `index` (site * nnodes + node),
bit for bit; the arguments broadcast.
"""
from __future__ import annotations

import numpy as np

__all__ = ['philox4x32', 'philox_uniform']

_M0, _M1 = np.uint64(0xD2511F53), np.uint64(0xCD9E8D57)
_W0, _W1 = 0x9E3779B9, 0xBB67AE85
_LO = np.uint64(0xFFFFFFFF)
_S32 = np.uint64(32)


def philox4x32(counter, key, rounds=10):
    """counter (c0, c1, c2, c3) and key (k0, k1): 32-bit words (arrays broadcast) -> the four
    output words as uint64 arrays holding 32-bit values."""
    c0, c1, c2, c3 = [np.asarray(c, dtype=np.uint64) & _LO for c in counter]
    k0, k1 = [np.asarray(k, dtype=np.uint64) & _LO for k in key]
    for r in range(rounds):
        p0, p1 = _M0 * c0, _M1 * c2          # 32 x 32 -> 64 bits: no overflow in uint64
        c0, c1, c2, c3 = (p1 >> _S32) ^ c1 ^ k0, p1 & _LO, (p0 >> _S32) ^ c3 ^ k1, p0 & _LO
        k0 = (k0 + np.uint64(_W0)) & _LO
        k1 = (k1 + np.uint64(_W1)) & _LO
    return c0, c1, c2, c3


def _words(x):
    if isinstance(x, int):
        x = np.uint64(x % (1 << 64))
    x = np.asarray(x)
    if x.dtype != np.uint64:
        x = x.astype(np.int64).astype(np.uint64)
    return x & _LO, x >> _S32


def philox_uniform(seed, draw, index):
    """f64 in [0, 1) with 53 random bits: counter {index low, index high, draw low, draw high},
    key {seed low, seed high}; ((c0 << 21) ^ (c1 >> 11)) mod 2^53 times 2^-53."""
    i0, i1 = _words(index)
    d0, d1 = _words(draw)
    k0, k1 = _words(seed)
    c0, c1, _, _ = philox4x32((i0, i1, d0, d1), (k0, k1))
    bits = ((c0 << np.uint64(21)) ^ (c1 >> np.uint64(11))) & np.uint64((1 << 53) - 1)
    return bits.astype(np.float64) * (1.0 / 9007199254740992.0)
