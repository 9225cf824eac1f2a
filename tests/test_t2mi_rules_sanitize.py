"""csrc/t2mi_rules.h under ASan + UBSan: tests/cpp/t2mi_rules_san.cpp, a stand-alone program that includes nothing but the rules, run
directly (its own process) on the constructed cases of tests/t2mi_cases.py, where what it prints must be the model's, and on seeded
random packets."""
import os
import subprocess

import pytest

import t2mi_cases as K
import t2mi_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 't2mi_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 't2mi_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _clean(r):
    assert r.returncode == 0 and 't2mi rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def _line(r, head):
    return [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith(head)][0].split()[1:]]


@pytest.mark.parametrize('per_call', [0, 1, 7])
def test_constructed_cases_under_sanitizers_equal_the_model(exe, tmp_path, per_call):
    ts = K.whole_stream()
    ts.tofile(tmp_path / 'ts.bin')
    m = T.Slot(K.PID, 2)
    rows, step, h = [], per_call or len(ts), 0
    for c, a in enumerate(range(0, len(ts), step)):
        for b in m.process(ts[a:a + step]):
            h = (h * 131 + int(b)) % 1000000007
        rows += [(c,) + tuple(r[k] for k in T.ROW_KEYS) for r in m.table]
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(per_call), str(K.PID), '2'], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    assert [tuple(int(v) for v in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith('row ')] == rows and len(rows) == sum(len(v) for v in K.ROWS.values())
    assert _line(r, 'stats') == [m.st[k] for k in T.STAT_KEYS] and m.st['bbframes_delivered'] == 11
    assert _line(r, 'bytes') == [h, len(m.buf)]


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_packets_under_sanitizers(exe, seed):
    r = subprocess.run([exe, 'random', str(seed), '8000'], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    st = dict(zip(T.STAT_KEYS, _line(r, 'stats')))
    assert st['packets'] > 4000 and st['t2mi_packets'] > 500 and st['crc_errors'] > 100, st
    assert min(st[k] for k in ('dropped_packets', 'malformed_packets', 'scrambled_packets', 'pointer_slack')) > 0, st
