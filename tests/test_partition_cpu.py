"""The host side of the partitioned likelihood (no GPU): the planner rt_partition_plan against
a numpy restatement, the same planner (csrc/partition_plan.h) in a stand-alone program under
AddressSanitizer + UBSan, and the argument checks of check_site_sets."""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

from conftest import ROOT

RT_ERR_INVALID = -1


def plan_cases():
    """(label, site_set, K, G).  Random assignments at the three granules, K = 1, empty sets, runs
    of exactly G, G - 1, G + 1 and 1, a single site."""
    rng = np.random.RandomState(5)
    cases = []
    for G in (16, 64, 256):
        cases.append(('random G=%d' % G, rng.randint(0, 5, size=3 * G + 5), 5, G))
        cases.append(('K=1 G=%d' % G, np.zeros(2 * G + 3, dtype=np.int64), 1, G))
        cases.append(('empty sets G=%d' % G, rng.choice([1, 4], size=G + 7), 6, G))
        runs = np.concatenate([np.full(G, 0), np.full(G - 1, 1), np.full(G + 1, 2), np.full(1, 3)])
        cases.append(('runs G, G-1, G+1, 1 G=%d' % G, rng.permutation(runs), 4, G))
        cases.append(('nsites=1 G=%d' % G, np.array([2]), 3, G))
    cases.append(('i %% 3 of 53, set 3 empty', np.arange(53) % 3, 4, 16))
    return cases


def numpy_plan(site_set, K, G):
    """The plan restated: stable sort by set, every run padded to a multiple of G with copies of
    its last real site."""
    site_set = np.asarray(site_set)
    order, is_pad, gset, run_begin = [], [], [], [0]
    for k in range(K):
        mine = np.flatnonzero(site_set == k)            # ascending: stable
        pads = (-len(mine)) % G
        order += list(mine) + [mine[-1]] * pads if len(mine) else []
        is_pad += [0] * len(mine) + [1] * pads
        gset += [k] * ((len(mine) + pads) // G)
        run_begin.append(len(order))
    order = np.array(order, dtype=np.int64)
    slot_of_site = np.empty(len(site_set), dtype=np.int64)
    real = np.flatnonzero(np.array(is_pad) == 0)
    slot_of_site[order[real]] = real
    return (order, slot_of_site, np.array(is_pad, dtype=np.uint8), np.array(gset, dtype=np.int32),
            np.array(run_begin, dtype=np.int64))


def c_plan(lib, site_set, K, G):
    """rt_partition_plan through ctypes -> (rc, arrays or None)."""
    ss = np.ascontiguousarray(site_set, dtype=np.int32)
    n = len(ss)
    i64p, i32p = ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int32)
    fn = lib.rt_partition_plan
    fn.restype = ctypes.c_int
    fn.argtypes = [i32p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64, i64p, i64p,
                   ctypes.POINTER(ctypes.c_ubyte), i32p, i64p, i64p]
    padded = ctypes.c_int64(-1)
    rc = fn(ss.ctypes.data_as(i32p), n, K, G, 0, None, None, None, None, None, ctypes.byref(padded))
    if rc != 0:
        return rc, None
    cap = n + K * (G - 1)
    assert 0 < padded.value <= cap and padded.value % G == 0
    order = np.full(cap, -7, dtype=np.int64)
    slot = np.full(n, -7, dtype=np.int64)
    pad = np.full(cap, 9, dtype=np.uint8)
    gset = np.full(cap // G + 1, -7, dtype=np.int32)
    rb = np.full(K + 1, -7, dtype=np.int64)
    p2 = ctypes.c_int64(-1)
    rc = fn(ss.ctypes.data_as(i32p), n, K, G, cap, order.ctypes.data_as(i64p),
            slot.ctypes.data_as(i64p), pad.ctypes.data_as(ctypes.POINTER(ctypes.c_ubyte)),
            gset.ctypes.data_as(i32p), rb.ctypes.data_as(i64p), ctypes.byref(p2))
    assert rc == 0 and p2.value == padded.value
    P = padded.value
    # nothing written past the plan
    assert (order[P:] == -7).all() and (pad[P:] == 9).all() and (gset[P // G:] == -7).all()
    return 0, (order[:P], slot, pad[:P], gset[:P // G], rb)


@pytest.fixture(scope='module')
def lib():
    path = os.environ.get('RAOTEH_HIP_LIB', os.path.join(ROOT, 'raoteh_amd', 'libraoteh_hip.so'))
    if not os.path.exists(path):
        pytest.fail('libraoteh_hip.so has not been built')
    return ctypes.CDLL(path)


@pytest.mark.parametrize('label,site_set,K,G', plan_cases(), ids=[c[0] for c in plan_cases()])
def test_plan_against_numpy(lib, label, site_set, K, G):
    rc, got = c_plan(lib, site_set, K, G)
    assert rc == 0
    order, slot, pad, gset, rb = got
    want = numpy_plan(site_set, K, G)
    for g, w in zip(got, want):
        assert g.shape == w.shape and np.array_equal(g, w), label
    site_set = np.asarray(site_set)
    real = pad == 0
    # every site exactly once among the real slots; slot_of_site inverts order there
    assert np.array_equal(np.sort(order[real]), np.arange(len(site_set)))
    assert np.array_equal(order[slot], np.arange(len(site_set))) and real[slot].all()
    for k in range(K):
        lo, hi = rb[k], rb[k + 1]
        assert (hi - lo) % G == 0 and (gset[lo // G:hi // G] == k).all()
        mine = order[lo:hi][real[lo:hi]]
        assert np.array_equal(mine, np.flatnonzero(site_set == k))       # stable within the set
        # a pad repeats a real site of its own run (the last), and pads come after the real slots
        pads = order[lo:hi][~real[lo:hi]]
        assert len(pads) < G and (len(mine) > 0 or len(pads) == 0)
        if len(pads):
            assert (pads == mine[-1]).all() and not real[lo + len(mine):hi].any()
    assert (site_set[order] == np.repeat(gset, G)).all()      # every granule homogeneous


@pytest.mark.parametrize('bad', [-1, 3])
def test_plan_refuses_a_set_index_out_of_range(lib, bad):
    ss = np.array([0, 1, 2, bad, 1])
    rc, _ = c_plan(lib, ss, 3, 16)
    assert rc == RT_ERR_INVALID
    fn = lib.rt_last_error
    fn.restype = ctypes.c_char_p
    assert b'site_set[3]' in fn()


def test_plan_refuses_a_capacity_too_small(lib):
    ss = np.zeros(5, dtype=np.int32)
    order = np.zeros(15, dtype=np.int64)
    padded = ctypes.c_int64(0)
    i32p, i64p = ctypes.POINTER(ctypes.c_int32), ctypes.POINTER(ctypes.c_int64)
    lib.rt_partition_plan.restype = ctypes.c_int
    lib.rt_partition_plan.argtypes = [i32p, ctypes.c_int64, ctypes.c_int64, ctypes.c_int64,
                                      ctypes.c_int64, i64p, i64p, ctypes.POINTER(ctypes.c_ubyte),
                                      i32p, i64p, i64p]
    rc = lib.rt_partition_plan(ss.ctypes.data_as(i32p), 5, 1, 16, 15, order.ctypes.data_as(i64p),
                               None, None, None, None, ctypes.byref(padded))
    assert rc == RT_ERR_INVALID and padded.value == 16 and (order == 0).all()


PROGRAM = r'''
#include "partition_plan.h"
#include <cstdio>
#include <cstdlib>
// reads cases "K G nsites s0 s1 ..." from the file argv[1]; prints per case the return code and,
// on success, padded, order, slot_of_site, is_pad, granule_set, run_begin, one line each
int main(int argc, char **argv)
{
    if (argc < 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long K, G, n;
    while (fscanf(f, "%lld %lld %lld", &K, &G, &n) == 3) {
        std::vector<int32_t> ss((size_t)n);
        for (long long i = 0; i < n; ++i) {
            int v;
            if (fscanf(f, "%d", &v) != 1) return 2;
            ss[(size_t)i] = v;
        }
        rt_partition_layout plan;
        int64_t bad = -1;
        const int rc = rt_partition_plan_build(ss.data(), n, K, G, &plan, &bad);
        printf("rc %d %lld\n", rc, rc ? (long long)bad : (long long)plan.padded);
        if (rc) continue;
        for (int64_t v : plan.order) printf("%lld ", (long long)v);
        printf("\n");
        for (int64_t v : plan.slot_of_site) printf("%lld ", (long long)v);
        printf("\n");
        for (uint8_t v : plan.is_pad) printf("%d ", (int)v);
        printf("\n");
        for (int32_t v : plan.granule_set) printf("%d ", (int)v);
        printf("\n");
        for (int64_t v : plan.run_begin) printf("%lld ", (long long)v);
        printf("\n");
    }
    fclose(f);
    return 0;
}
'''


def test_planner_header_in_a_sanitized_program(tmp_path):
    """csrc/partition_plan.h in a program of its own, built with -fsanitize=address,undefined and
    run on the cases above plus the two refused ones: the same plans, no sanitizer report."""
    cxx = next((c for c in ('c++', 'g++', 'clang++') if shutil.which(c)), None)
    if cxx is None:
        pytest.skip('no C++ compiler')
    src = tmp_path / 'plan_main.cpp'
    src.write_text(PROGRAM)
    exe = tmp_path / 'plan_main'
    # (the sanitizer runtimes linked statically, which clang does by itself: the program then
    # does not care what else the environment has the loader bring in)
    probe = subprocess.run([cxx, '--version'], stdout=subprocess.PIPE, stderr=subprocess.STDOUT,
                           universal_newlines=True, timeout=60)
    static = [] if 'clang' in probe.stdout else ['-static-libasan', '-static-libubsan']
    build = subprocess.run([cxx, '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined',
                            '-fno-sanitize-recover=all'] + static +
                           ['-I', os.path.join(ROOT, 'raoteh_amd', 'csrc'),
                            str(src), '-o', str(exe)], stdout=subprocess.PIPE,
                           stderr=subprocess.STDOUT, universal_newlines=True, timeout=300)
    if build.returncode != 0 and 'cannot find' in build.stdout and 'san' in build.stdout.lower():
        pytest.skip('the compiler has no sanitizer runtime')
    assert build.returncode == 0, build.stdout[-3000:]
    cases = [(np.asarray(ss), K, G) for _, ss, K, G in plan_cases()]
    cases += [(np.array([0, 1, 2, -1, 1]), 3, 16), (np.array([0, 1, 2, 3, 1]), 3, 16)]
    inp = tmp_path / 'cases.txt'
    inp.write_text(''.join('%d %d %d %s\n' % (K, G, len(ss), ' '.join(str(int(v)) for v in ss))
                           for ss, K, G in cases))
    env = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:halt_on_error=1',
               UBSAN_OPTIONS='halt_on_error=1:print_stacktrace=1')
    run = subprocess.run([str(exe), str(inp)], stdout=subprocess.PIPE, stderr=subprocess.PIPE,
                         universal_newlines=True, timeout=300, env=env)
    assert run.returncode == 0, (run.stdout[-1000:], run.stderr[-3000:])
    assert 'Sanitizer' not in run.stderr and 'runtime error' not in run.stderr, run.stderr[-3000:]
    lines = run.stdout.splitlines()
    at = 0
    for ss, K, G in cases:
        head = lines[at].split()
        at += 1
        if ((ss < 0) | (ss >= K)).any():
            assert head == ['rc', '-1', str(int(np.flatnonzero((ss < 0) | (ss >= K))[0]))]
            continue
        want = numpy_plan(ss, K, G)
        assert head == ['rc', '0', str(len(want[0]))]
        for w in want:
            got = np.array(lines[at].split(), dtype=np.int64)
            at += 1
            assert np.array_equal(got, w.astype(np.int64))
    assert at == len(lines)


def test_check_site_sets():
    from raoteh_amd.device import check_site_sets
    sets, K = check_site_sets([0, 2, 1, 2], 4)
    assert sets.dtype == np.int32 and sets.flags.c_contiguous and K == 3
    assert np.array_equal(sets, [0, 2, 1, 2])
    assert check_site_sets(np.array([0, 0], dtype=np.uint8), 2, nsets=4)[1] == 4
    assert check_site_sets(np.zeros(3, dtype=np.int64), 3, nsets=64)[1] == 64
    for bad, nsites, nsets in (([0, 1], 3, None),               # one entry per site
                               ([[0, 1]], 2, None),             # shape
                               ([0.0, 1.0], 2, None),           # not integers
                               ([True, False], 2, None),
                               ([0, -1], 2, None),              # out of range
                               ([0, 3], 2, 3),
                               ([0, 1], 2, 0),                  # nsets out of range
                               ([0, 1], 2, 65),
                               ([0, 64], 2, None),
                               ([0, 1], 2, 2.5),
                               ([], 0, None)):
        with pytest.raises(ValueError):
            check_site_sets(bad, nsites, nsets)
