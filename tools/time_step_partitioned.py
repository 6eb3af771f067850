#!/usr/bin/env python
"""
Each site under its own rate set (site i in set i % K): microseconds per evaluation of the
whole alignment under K fresh parameter vectors, by

  partitioned       set_rate_sets + step_partitioned + one fetch of the per-set totals
  step_only         step_partitioned (exponentials again from the resident sets) + that fetch
  subbatch_jit      K x (set_rates + step) over K ordinary sub-batches holding the sites of one
                    set each, with tree-specialised kernels ("jit" = 1), + a fetch of the totals
  subbatch_interp   the same with the interpreter kernels ("jit" = 0)
  step_multi        set_rate_sets + step_multi of the whole batch ("jit" = 0: K times the
                    arithmetic) + one fetch of the K totals

each the median of nine windows, with the window minimum and maximum.  The last three use
nothing the partitioned likelihood added, so `--baseline-only` runs on a checkout without it.

    python tools/time_step_partitioned.py --workload c3 --K 4,64 [--baseline-only]
        [--out profiles/step_partitioned_c3.json] [--kernel-times K] [--once K]

`--kernel-times K`: no windows; device time of the pruning launch (the runtime's own begin / end
stamps of the kernel, rt_ctx_set_timing) of the partitioned step next to an ordinary "jit" = 0
step of the whole batch, nine groups of launches each.  `--once K`: warm up, then twenty steps
of each of those two (the program to put behind `rocprofv3 --kernel-trace --stats --`).
"""
import argparse
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

from raoteh_amd import device, synth          # noqa: E402

WINDOWS = 9


def rate_sets(cfg, K, model):
    """K parameter vectors around the configuration's own (kappa, omega, tree scale)."""
    if cfg['name'] != 'c3':
        raise SystemExit('workload %s: only c3 (the codon configuration) is set up here' % cfg['name'])
    t0 = model.tree.branch_lengths()
    Q = np.empty((K, cfg['nstates'], cfg['nstates']))
    t = np.empty((K, len(t0)))
    for k in range(K):
        Q[k] = synth.mg94(kappa=3.17632 * (1.0 + 0.01 * k), omega=0.21925 * (1.0 + 0.02 * k))[0]
        t[k] = t0 * (1.0 + 0.005 * k)
    return Q, t


def windows(fn, reps):
    out = []
    for _ in range(WINDOWS):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return out


def summary(us):
    us = np.array(us)
    return dict(median_us=float(np.median(us)), min_us=float(us.min()), max_us=float(us.max()),
                windows=len(us))


def new_model(cfg, jit):
    ctx = device.Context(0)
    ctx.set_option('jit', jit)
    ctx.set_option('jit_async', 0)
    model = device.TreeModel(cfg['T'], cfg['root'], cfg['nstates'], ctx=ctx)
    model.set_root_distn(cfg['root_distn'])
    model.set_rates(Q_default=cfg['Q_default'])
    return ctx, model


def subbatch_loop(cfg, dense, site_sets, K, Q, t, jit):
    """-> (fn, kernel name): K x (set_rates + step) over the K sub-batches, then the totals."""
    ctx, model = new_model(cfg, jit)
    subs = [model.upload_sites(cfg['leaves'], np.ascontiguousarray(dense[site_sets == k]),
                               kind='dense') for k in range(K)]
    for b in subs:
        b.wait_for_kernel()

    def fn():
        for k in range(K):
            model.set_rates(Q=Q[k], t=t[k])
            model.step(subs[k])
        return np.array([model.fetch_totals(b) for b in subs])
    fn()
    return fn, subs[0].kernel_name, (ctx, model, subs)


def kernel_ms(ctx, fn, groups=WINDOWS, reps=20):
    """Device time per pruning launch (ms; the combine kernel of a root-halves launch added),
    one figure per group of `reps` calls."""
    out = []
    ctx.set_timing(1)
    for _ in range(groups):
        ctx.reset_timing()
        for _ in range(reps):
            fn()
        ctx.sync()
        ms, launches, name = ctx.kernel_time(device._lib.RT_K_PRUNE)
        cms, claunches, _ = ctx.kernel_time(device._lib.RT_K_COMBINE)
        out.append((ms + cms) / max(launches, 1))
    ctx.set_timing(0)
    return out, name


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--workload', default='c3')
    ap.add_argument('--K', default='4,64')
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--baseline-only', action='store_true')
    ap.add_argument('--out', default=None)
    ap.add_argument('--kernel-times', type=int, default=0)
    ap.add_argument('--once', type=int, default=0)
    args = ap.parse_args()
    single = args.kernel_times or args.once
    Ks = [single] if single else [int(k) for k in args.K.split(',')]
    cfg = synth.make_config(args.workload)
    dense = synth.leaf_likelihoods(cfg)
    nsites = dense.shape[0]
    result = dict(workload=args.workload, kind='dense', nsites=nsites, reps_per_window=args.reps,
                  assignment='site i in set i % K', rows=[])
    for K in Ks:
        site_sets = np.arange(nsites) % K
        ctx, model = new_model(cfg, 0)
        Q, t = rate_sets(cfg, K, model)
        whole = model.upload_sites(cfg['leaves'], dense, kind='dense')
        row = dict(K=K)

        if single:
            part = model.upload_sites(cfg['leaves'], dense, kind='dense', site_sets=site_sets,
                                      nsets=K)
            model.set_rate_sets(Q, t=t)

            def pstep():
                model.step_partitioned(part, recompute_transitions=False)

            def ostep():
                model.step(whole, recompute_transitions=False)
            for _ in range(3):
                pstep()
                ostep()
            ctx.sync()
            if args.once:
                for _ in range(20):
                    pstep()
                    ostep()
                ctx.sync()
                print('twenty steps each: %s | %s' % (part.kernel_name, whole.kernel_name))
                return
            pms, pname = kernel_ms(ctx, pstep)
            oms, oname = kernel_ms(ctx, ostep)
            row['partitioned_kernel'] = dict(name=pname, slots=int(_padded(part)),
                                             **summary(np.array(pms) * 1e3))
            row['ordinary_kernel'] = dict(name=oname, slots=nsites, **summary(np.array(oms) * 1e3))
            result['rows'].append(row)
            print(json.dumps(row))
            continue

        def multi():
            model.set_rate_sets(Q, t=t)
            model.step_multi(whole)
            return model.fetch_multi_totals(whole)
        for _ in range(3):
            mtot = multi()
        row['step_multi'] = dict(kernel=whole.multi_kernel_name, **summary(windows(multi, args.reps)))
        for label, jit in (('subbatch_jit', 1), ('subbatch_interp', 0)):
            fn, name, keep = subbatch_loop(cfg, dense, site_sets, K, Q, t, jit)
            for _ in range(3):
                btot = fn()
            row[label] = dict(kernel=name, **summary(windows(fn, args.reps)))
            del keep
        if not args.baseline_only:
            part = model.upload_sites(cfg['leaves'], dense, kind='dense', site_sets=site_sets,
                                      nsets=K)

            def partitioned():
                model.set_rate_sets(Q, t=t)
                model.step_partitioned(part, recompute_transitions=False)
                return model.fetch_partition_totals(part)

            def step_only():
                model.step_partitioned(part)
                return model.fetch_partition_totals(part)
            for _ in range(3):
                ptot = partitioned()
            # the per-set sums are those of the sub-batch loop (another summation order only)
            assert np.array_equal(ptot[:, 1:], btot[:, 1:]), (ptot, btot)
            assert np.allclose(ptot[:, 0], btot[:, 0], rtol=1e-12, atol=0), (ptot, btot)
            row['partitioned'] = dict(kernel=part.kernel_name, slots=int(_padded(part)),
                                      **summary(windows(partitioned, args.reps)))
            row['step_only'] = summary(windows(step_only, args.reps))
            for base in ('subbatch_jit', 'subbatch_interp', 'step_multi'):
                row['ratio_%s_over_partitioned' % base] = (row[base]['median_us'] /
                                                           row['partitioned']['median_us'])
        result['rows'].append(row)
        print(json.dumps(row))
    if args.out:
        with open(args.out, 'w') as f:
            json.dump(result, f, indent=1)
            f.write('\n')


def _padded(batch):
    import ctypes
    v = ctypes.c_int64(0)
    device._lib.check(device._lib.lib().rt_sites_partition_info(batch._h, None, None, ctypes.byref(v)))
    return v.value


if __name__ == '__main__':
    main()
