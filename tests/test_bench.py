"""
bench.py itself: the options that decide what a plain run does (--steps, --full,
--dump-outputs) and the arrays --dump-outputs writes.
"""
import importlib.util
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT


def _bench_module():
    spec = importlib.util.spec_from_file_location('bench', os.path.join(ROOT, 'bench.py'))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    return bench


def _run_bench(*args, timeout=600):
    return subprocess.run([sys.executable, os.path.join(ROOT, 'bench.py')] + list(args),
                          cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                          timeout=timeout)


def test_bench_refuses_bad_arguments_before_touching_a_device():
    for args in (['--steps', '0'], ['--warmup', '-1'], ['--also', 'c2']):
        proc = _run_bench(*args, timeout=120)
        assert proc.returncode != 0, args
        assert proc.stdout == b'', args
    proc = _run_bench('--also', 'c2', timeout=120)
    assert b'--full' in proc.stderr


def test_bench_inputs_depend_only_on_the_arguments():
    bench = _bench_module()
    for name in ('c2', 'c3', 'c5'):
        a, ta = bench.shard_config(name, 0, 1, 500)
        b, tb = bench.shard_config(name, 0, 1, 500)
        assert ta == tb == 500
        np.testing.assert_array_equal(a['leaf_states'], b['leaf_states'])
        np.testing.assert_array_equal(a['Q_default'], b['Q_default'])
        np.testing.assert_array_equal(a['root_distn'], b['root_distn'])


def test_dump_outputs_float64_and_within_the_budget(tmp_path, monkeypatch):
    bench = _bench_module()
    rng = np.random.default_rng(5)
    ll = -rng.random(1000) * 100
    st = np.zeros(1000, dtype=np.int32)
    st[7] = 1
    totals = np.array([ll.sum(), 1.0, 1000.0])
    bench.dump_outputs(str(tmp_path / 'small'), ll, st, totals)
    got = dict((f[:-4], np.load(str(tmp_path / 'small' / f)))
               for f in os.listdir(str(tmp_path / 'small')))
    assert sorted(got) == ['log_likelihoods', 'status', 'totals']
    assert all(a.dtype == np.float64 for a in got.values())
    np.testing.assert_array_equal(got['log_likelihoods'], ll)
    np.testing.assert_array_equal(got['status'], st)
    np.testing.assert_array_equal(got['totals'], totals)
    # a block above the budget: a fixed, seeded sample of its sites, the same every time
    monkeypatch.setattr(bench, 'DUMP_LIMIT_BYTES', 2 ** 16 + 24 * 300)
    for k in range(2):
        bench.dump_outputs(str(tmp_path / ('big%d' % k)), ll, st, totals)
    idx = np.load(str(tmp_path / 'big0' / 'site_index.npy'))
    assert idx.dtype == np.float64 and len(idx) == 300 and np.all(np.diff(idx) > 0)
    for name in ('site_index', 'log_likelihoods', 'status', 'totals'):
        np.testing.assert_array_equal(np.load(str(tmp_path / 'big0' / (name + '.npy'))),
                                      np.load(str(tmp_path / 'big1' / (name + '.npy'))))
    np.testing.assert_array_equal(np.load(str(tmp_path / 'big0' / 'log_likelihoods.npy')),
                                  ll[idx.astype(np.int64)])
    total = sum(os.path.getsize(str(tmp_path / 'big0' / f))
                for f in os.listdir(str(tmp_path / 'big0')))
    assert total <= bench.DUMP_LIMIT_BYTES


@pytest.mark.gpu
def test_plain_bench_run_times_k_steps_and_dumps_what_the_oracle_computes(tmp_path):
    """A plain run: exactly --steps timed steps in one window, the headline fields only, and
    the log-likelihoods of the last timed step equal to the oracle's for the same sites."""
    from oracle import oracle_numpy as orc
    from raoteh_amd import synth
    out = tmp_path / 'out'
    proc = _run_bench('--gpus', '1', '--steps', '3', '--warmup', '1', '--dump-outputs', str(out))
    assert proc.returncode == 0, proc.stderr.decode()[-3000:]
    line = json.loads(proc.stdout.decode().strip().splitlines()[-1])
    for key in ('metric', 'value', 'unit', 'higher_is_better', 'dtype', 'ms_per_step'):
        assert key in line, key
    assert line['steps'] == 3 and line['warmup'] == 1 and line['timed_windows'] == 1
    assert line['unit'] == 'sites/s' and line['higher_is_better'] is True
    assert line['dtype'] == 'f64' and line['ms_per_step'] > 0
    assert not ({'workloads', 'roofline', 'kernels_us', 'cpu_baseline', 'next_rows'} & set(line))
    ll = np.load(str(out / 'log_likelihoods.npy'))
    st = np.load(str(out / 'status.npy'))
    totals = np.load(str(out / 'totals.npy'))
    assert ll.dtype == st.dtype == totals.dtype == np.float64
    assert ll.shape == (10000,) and not st.any()
    assert totals[1] == 0 and totals[2] == 10000
    np.testing.assert_allclose(totals[0], ll.sum(), rtol=1e-12)
    np.testing.assert_allclose(line['total_log_likelihood'], totals[0], rtol=0)
    cfg = synth.make_config('c3', nsites=10000)
    m = 100
    dense = synth.leaf_likelihoods(dict(cfg, leaf_states=cfg['leaf_states'][:m]))
    pre, idx, ptr, esd = orc.get_expm_augmented_transitions(
        cfg['T'], cfg['root'], cfg['nstates'], Q_default=cfg['Q_default'])
    want, _ = orc.batch_log_likelihoods(idx, ptr, esd, [pre.index(v) for v in cfg['leaves']],
                                        dense, cfg['root_distn'])
    np.testing.assert_allclose(ll[:m], want, rtol=1e-10)
