"""csrc/ule_rules.h (and csrc/ip_rules.h behind it) under ASan + UBSan: tests/cpp/ule_rules_san.cpp, a stand-alone program with its own
main that includes nothing but the rules, run directly (its own process; nothing is preloaded, nothing is loaded into Python) on the
constructed cases of tests/ule_cases.py and on three seeded random feeds, where what it prints must be the model's."""
import os
import subprocess

import pytest

import ule_cases as K
import ule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'ule_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'ule_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _clean(r):
    assert r.returncode == 0 and 'ule rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def _line(r, head):
    return [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith(head)][0].split()[1:]]


def _run_both(exe, tmp_path, ts, per_call, pid, mac, mask, accept=True):
    """the program and the model on the same calls -> the model's slot; rows, counters, byte hash and open bytes are compared"""
    ts.tofile(tmp_path / 'ts.bin')
    m = R.Slot(pid, mac, mask, accept)
    rows, step, h = [], per_call or len(ts), 0
    for c, a in enumerate(range(0, len(ts), step)):
        for b in m.process(ts[a:a + step]):
            h = (h * 131 + int(b)) % 1000000007
        rows += [(c,) + tuple(r[k] if k != 'mac' else int(r[k].hex(), 16) for k in R.ROW_KEYS) for r in m.table]
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(per_call), str(pid), mac.hex(), mask.hex(), str(int(accept))], capture_output=True, text=True, timeout=120, env=ENV)
    _clean(r)
    got = [l.split()[1:] for l in r.stdout.splitlines() if l.startswith('row ')]
    assert [tuple(int(v, 16) if i == 4 else int(v) for i, v in enumerate(l)) for l in got] == rows
    assert _line(r, 'stats') == [m.st[k] for k in R.STAT_KEYS]
    assert _line(r, 'bytes') == [h, len(m.buf)]
    return m, len(rows)


@pytest.mark.parametrize('per_call', [0, 1, 7, 64])
def test_constructed_cases_under_sanitizers_equal_the_model(exe, tmp_path, per_call):
    m, rows = _run_both(exe, tmp_path, K.whole_stream(), per_call, K.PID, K.NPA, K.MASK)
    assert rows == sum(len(v) for v in K.ROWS.values()) and m.st == K.STATS
    m, _ = _run_both(exe, tmp_path, K.whole_stream(), per_call, K.PID, K.NPA, K.MASK, accept=False)
    assert m.st == K.STATS_NO_ACCEPT


@pytest.mark.parametrize('seed', [1, 3, 4])
def test_random_packets_under_sanitizers(exe, tmp_path, seed):
    ts = K.wild_packets(seed, 1500)
    probe = R.Slot(0x40, K.NPA, K.MASK, True)                        # the floors, on the model alone, before anything is compared
    probe.process(ts)
    st = probe.st
    assert st['packets'] > 1000 and st['sndus'] > 200 and st['datagrams'] > 30, st
    assert min(st[k] for k in ('crc_errors', 'filtered', 'no_address', 'test', 'bridged', 'extension', 'other_protocol', 'bad_ip', 'datagrams',
                               'datagrams_delivered', 'bytes_delivered', 'dropped_sndus', 'malformed_sndus', 'slack', 'malformed_packets',
                               'scrambled_packets')) > 0, st
    m, _ = _run_both(exe, tmp_path, ts, 5 + 13 * seed, 0x40, K.NPA, K.MASK)
    assert m.st == st
