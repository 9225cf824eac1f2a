"""csrc/aud_rules.h under ASan + UBSan: tests/cpp/aud_rules_san.cpp, a stand-alone program that includes nothing but the rules, run
directly (its own process) on the faulty multiplex of tests/aud_cases.py, where what it prints must be the model's, and on seeded
random packets."""
import os
import subprocess

import pytest

import aud_cases as K
import aud_ref as A

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'aud_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'aud_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _clean(r):
    assert r.returncode == 0 and 'aud rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def _line(r, head):
    return [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith(head)][0].split()[1:]]


@pytest.mark.parametrize('per_call', [0, 1, 37])
def test_the_faulty_multiplex_under_sanitizers_equals_the_model(exe, tmp_path, per_call):
    ts = K.mux()[:1000]
    ts.tofile(tmp_path / 'ts.bin')
    watches = sorted(K.WATCHES)                                      # slots 0, 3, 5, 11: the program watches in slots 0, 1, 2, 3
    m = K.model(watches=[(s, pid, codec) for s, (_, pid, codec) in enumerate(watches)])
    rows, step = [], per_call or len(ts)
    for c, a in enumerate(range(0, len(ts), step)):
        m.process(ts[a:a + step])
        rows += [(c,) + tuple(r[k] for k in A.ROW_KEYS) for r in m.table]
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(per_call)] + ['%d,%d' % (pid, codec) for _, pid, codec in watches], capture_output=True, text=True,
                       timeout=120, env=ENV)
    _clean(r)
    assert [tuple(int(v) for v in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith('row ')] == rows and len(rows) > 200
    assert _line(r, 'stats') == [m.stats()[k] for k in A.STAT_KEYS]
    assert _line(r, 'stream') == [1000, 0, len(rows)]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_packets_under_sanitizers(exe, seed):
    r = subprocess.run([exe, 'random', str(seed), '6000'], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    st = dict(zip(A.STAT_KEYS, _line(r, 'stats')))
    assert st['packets'] > 3000 and st['pes_starts'] > 300 and st['frames'] > 300 and min(st.values()) > 0, st
    packets, dropped, rows = _line(r, 'stream')
    assert packets == 6000 and dropped > 0 and rows > st['pes_starts']
