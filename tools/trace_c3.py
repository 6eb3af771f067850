#!/usr/bin/env python
"""
Where does a step of the split-M tree-specialised kernel (config 3) spend its time?
Run on a GPU box:   RAOTEH_JIT_TRACE=<workgroup> python tools/trace_c3.py [sites] [tiles] [dense]
The waves of that workgroup stamp the shader clock at the start of every step (t0), after
the x-exchange barrier (t1) and after the last MFMA of the step has been issued (t2).
Prints, per wave, the mean prelude (t1 - t0), chain (t2 - t1) and tail (t0' - t2) in
cycles, split into leaf steps and internal steps.
`dense`: dense leaf vectors, as bench.py uploads them (default: leaf states).  The pipelined
generator's kernels (root halves, one or two teams) get the summary of `pipelined()`: clocks per
step in issue order, per wave -- for the two-team form with the team of each wave and the wait
at the barrier -- and the core clock from the constant 100 MHz clock.
"""
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
os.environ.setdefault('RAOTEH_JIT_TRACE', '0')
os.environ.setdefault('RAOTEH_JIT_NO_VERIFY', '1')     # the trace global changes nothing, skip

from raoteh_amd import _lib, device, synth             # noqa: E402


def pipelined(batch, nrec):
    """Stamps of a kernel of the pipelined generator: rows are steps in issue order of the
    workgroup's program (a root half: at most nrec rows, the unused ones stay zero)."""
    teams = ',teams' in batch.kernel_name
    nwaves, width = (8, 4) if teams else (4, 3)
    tr = np.zeros((nwaves, nrec + 1, width), dtype=np.uint64)
    # (a root half has fewer steps than the schedule: the array is as long as the longer half)
    for rows in range(nrec + 1, 1, -1):
        tr = np.zeros((nwaves, rows, width), dtype=np.uint64)
        if _lib.lib().rt_debug_jit_global(batch._h, b'rt_trace', tr.ctypes.data_as(ctypes.c_void_p),
                                          tr.nbytes) == 0:
            break
    tr = tr.astype(np.int64)
    out = dict(kernel=batch.kernel_name, workgroup=int(os.environ['RAOTEH_JIT_TRACE']), waves=[])
    for w in range(nwaves):
        t0 = tr[w, :, 0]
        last = int(np.nonzero(t0)[0].max())            # the stamp behind the last step
        steps = np.arange(1, last - 1)                 # (not the first step, not the root's)
        real = int(tr[w, -1, 2] - tr[w, -1, 1])        # ticks of the constant 100 MHz clock
        total = int(t0[last] - t0[0])
        row = dict(wave=w % 4, steps=int(last), total_clocks=total,
                   clocks_per_step=float(np.mean(np.diff(t0[:last + 1])[1:-1])),
                   start_to_last_mfma=float(np.mean((tr[w, steps, 2] - t0[steps]))),
                   kernel_100mhz_ticks=real)
        if real > 0:
            row['core_ghz_at_least'] = round(total / (real * 10.0), 3)   # (the ticks span a little more)
        if teams:
            row['team'] = w // 4
            # the barrier that ends step i stands in the chain of step i (stamps of row i + 1)
            # (no barrier, and no stamps, in front of the root's step)
            ends = steps[tr[w, steps + 1, 3] != 0]
            row['wait_at_barrier'] = float(np.mean(tr[w, ends + 1, 1] - tr[w, ends + 1, 3]))
            row['start_to_barrier'] = float(np.mean(tr[w, ends + 1, 3] - t0[ends]))
        out['waves'].append(row)
    print(json.dumps(out, indent=1))


def main():
    nsites = int(sys.argv[1]) if len(sys.argv) > 1 else 10000
    if len(sys.argv) > 2:
        os.environ['RAOTEH_JIT_TILES'] = sys.argv[2]
    dense = len(sys.argv) > 3 and sys.argv[3] == 'dense'
    cfg = synth.make_config('c3', nsites=nsites)
    ctx = device.get_context(0)
    model = device.TreeModel(cfg['T'], cfg['root'], cfg['nstates'], ctx=ctx)
    model.set_rates(Q_default=cfg['Q_default'])
    model.set_root_distn(cfg['root_distn'])
    if dense:
        batch = model.upload_sites(cfg['leaves'], synth.leaf_likelihoods(cfg), kind='dense')
    else:
        batch = model.upload_sites(cfg['leaves'], cfg['leaf_states'].astype(np.uint8), kind='state')
    batch.wait_for_kernel()              # (a background compile: the stamps are the kernel's)
    for _ in range(5):
        model.prune(batch)
    ctx.sync()
    nops = ctypes.c_int64(0)
    _lib.check(_lib.lib().rt_model_get_schedule(model._h, None, 0, ctypes.byref(nops)))
    nrec = nops.value
    if dense:
        return pipelined(batch, nrec)
    ops = np.zeros((nrec, 4), dtype=np.int32)
    _lib.check(_lib.lib().rt_model_get_schedule(
        model._h, ops.ctypes.data_as(ctypes.POINTER(ctypes.c_int32)), nrec, ctypes.byref(nops)))
    NT = 4
    tr = np.zeros((NT, nrec + 1, 3), dtype=np.uint64)
    _lib.check(_lib.lib().rt_debug_jit_global(batch._h, b'rt_trace', tr.ctypes.data_as(ctypes.c_void_p),
                                              tr.nbytes))
    tr = tr.astype(np.int64)
    leaf = ops[:, 2] < 0                 # pop < 0
    root = ops[:, 3] < 0
    out = dict(kernel=batch.kernel_name, workgroup=int(os.environ['RAOTEH_JIT_TRACE']), waves=[])
    for w in range(NT):
        t0, t1, t2 = tr[w, :nrec, 0], tr[w, :nrec, 1], tr[w, :nrec, 2]
        nxt = tr[w, 1:, 0]
        ok = ~root
        rows = {}
        for name, sel in (('leaf', leaf & ok), ('internal', ~leaf & ok)):
            rows[name] = dict(steps=int(sel.sum()),
                              prelude=float(np.mean((t1 - t0)[sel])),
                              chain=float(np.mean((t2 - t1)[sel])),
                              tail=float(np.mean((nxt - t2)[sel])),
                              step=float(np.mean((nxt - t0)[sel])))
        # the pipelined generator has no separate prelude: "issue" = step start to last
        # MFMA issued (chain + everything in its shadow), "sync" = from there to the next
        # step's start (barrier + whatever ran serially)
        rows['issue_to_last_mfma'] = float(np.mean((t2 - t0)[ok]))
        rows['sync_after_last_mfma'] = float(np.mean((nxt - t2)[ok]))
        rows['total_cycles'] = int(tr[w, nrec, 0] - tr[w, 0, 0])
        out['waves'].append(rows)
    print(json.dumps(out, indent=1))
    w0 = tr[0]
    print('first 12 steps of wave 0: (leaf?, prelude, chain, tail)')
    for i in range(12):
        print(i, bool(leaf[i]), int(w0[i, 1] - w0[i, 0]), int(w0[i, 2] - w0[i, 1]),
              int(w0[i + 1, 0] - w0[i, 2]))


if __name__ == '__main__':
    main()
