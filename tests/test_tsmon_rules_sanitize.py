"""csrc/tsmon_rules.h under ASan + UBSan: tests/cpp/tsmon_rules_san.cpp, a stand-alone program that includes nothing but the rules,
run directly on files written by the generator of tests/tsmon_ref.py; what it prints and writes must be the model's."""
import os
import subprocess

import numpy as np
import pytest

import tsmon_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'tsmon_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'tsmon_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


@pytest.mark.parametrize('per_call,flt', [(0, dict()), (1, dict(mode=1, pids=[0x100, 0x1FFF])), (7, dict(mode=2, pids=[0x11], drop_null=True, drop_tei=True, drop_bad_sync=True)),
                                          (64, dict(drop_tei=True))])
def test_rules_under_sanitizers_equal_the_model(exe, tmp_path, per_call, flt):
    rng = np.random.default_rng(per_call)
    ts, info = T.make_mux(rng, 250, [0, 0x11, 0x100, 0x1FFE])
    for inject in T.INJECTORS:
        ts, info, _ = inject(rng, ts, info)
    ts.tofile(tmp_path / 'ts.bin')
    m = T.Monitor()
    m.set_filter(**flt)
    step = per_call or len(ts)
    want = np.concatenate([m.process(ts[a:a + step]) for a in range(0, len(ts), step)])
    args = [str(tmp_path / 'ts.bin'), str(tmp_path / 'out.bin'), str(per_call), str(flt.get('mode', 0))] + \
           [str(int(flt.get(k, False))) for k in ('drop_null', 'drop_tei', 'drop_bad_sync')] + [str(p) for p in flt.get('pids', [])]
    r = subprocess.run([exe] + args, capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and 'tsmon rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    lines = r.stdout.splitlines()
    assert [int(v) for v in lines[0].split()[1:]] == [m.stats()[k] for k in T.STAT_KEYS]
    assert [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith('row ')] == m.table
    assert np.array_equal(np.fromfile(tmp_path / 'out.bin', np.uint8), want)


def test_rules_on_an_empty_file(exe, tmp_path):
    (tmp_path / 'ts.bin').write_bytes(b'')
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(tmp_path / 'out.bin'), '0', '0', '0', '0', '0'], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and r.stdout.splitlines()[0] == 'stats' + ' 0' * 10, (r.stdout, r.stderr[-2000:])
