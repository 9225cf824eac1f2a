"""csrc/pes_rules.h under ASan + UBSan: tests/cpp/pes_rules_san.cpp, a stand-alone program that includes nothing but the rules, run
directly (its own process) on the constructed cases of tests/pes_cases.py, where what it prints must be the model's, and on seeded
random packets."""
import os
import subprocess

import pytest

import pes_cases as K
import pes_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'pes_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'pes_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _clean(r):
    assert r.returncode == 0 and 'pes rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def _line(r, head):
    return [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith(head)][0].split()[1:]]


@pytest.mark.parametrize('per_call', [0, 1, 7])
def test_constructed_cases_under_sanitizers_equal_the_model(exe, tmp_path, per_call):
    ts = K.whole_stream()
    ts.tofile(tmp_path / 'ts.bin')
    m = P.Pes()
    m.set_watch(0, K.PID), m.set_rate(K.TPP_Q24)
    rows, step = [], per_call or len(ts)
    for c, a in enumerate(range(0, len(ts), step)):
        m.process(ts[a:a + step])
        rows += [(c,) + tuple(r[k] for k in P.ROW_KEYS) for r in m.table]
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(per_call), str(K.PID), str(K.TPP_Q24)], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    assert [tuple(int(v) for v in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith('row ')] == rows and len(rows) == 85
    assert _line(r, 'stats') == [m.stats()[k] for k in P.STAT_KEYS]
    assert _line(r, 'stream') == [m.stream_stats()['packets'], 0, 85]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_packets_under_sanitizers(exe, seed):
    r = subprocess.run([exe, 'random', str(seed), '6000'], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    st = dict(zip(P.STAT_KEYS, _line(r, 'stats')))
    assert st['packets'] > 3000 and st['starts'] > 500 and min(v for k, v in st.items() if k != 'closed_ok') > 0, st     # (no random length is ever met)
    packets, dropped, starts = _line(r, 'stream')
    assert packets == 6000 and dropped > 0 and starts == st['starts']
