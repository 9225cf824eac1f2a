"""csrc/ipts_rules.h under ASan + UBSan: tests/cpp/ipts_rules_san.cpp, a stand-alone program that includes nothing but the rules, run
directly (its own process) on the constructed cases of tests/ipts_cases.py and on seeded random tables, where what it prints must be
the model's."""
import os
import subprocess

import pytest

import ipts_cases as K
import ipts_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
FLOW_ARGS = ['%d:%s:%d' % (fam, bytes(addr).hex(), port) for fam, addr, port in K.FLOWS]


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'ipts_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'ipts_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _clean(r):
    assert r.returncode == 0 and 'ipts rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]


def _line(r, head):
    return [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith(head)][0].split()[1:]]


def _run_both(exe, tmp_path, data, table, per_call, kind):
    """the program and the model on the same calls -> the model; rows, counters, byte hashes and the slots' states are compared"""
    data.tofile(tmp_path / 'data.bin'), table.tofile(tmp_path / 'table.bin')
    m = R.Stream()
    K.set_flows(m)
    rows, h = [], [0] * 4
    for c, part in enumerate(K.calls_of(table, per_call)):
        for k, out in enumerate(m.process(data, part, kind)):
            for b in out:
                h[k] = (h[k] * 131 + int(b)) % 1000000007
        rows += [(c,) + tuple(r[k] for k in R.ROW_KEYS) for r in m.table]
    r = subprocess.run([exe, str(tmp_path / 'data.bin'), str(tmp_path / 'table.bin'), str(per_call), str(kind)] + FLOW_ARGS, capture_output=True, text=True,
                       timeout=120, env=ENV)
    _clean(r)
    assert [tuple(int(v) for v in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith('row ')] == rows
    assert _line(r, 'stats') == [m.st[k] for k in R.STREAM_KEYS] + [s[k] for s in m.slot_st for k in R.SLOT_KEYS]
    assert _line(r, 'bytes') == h
    assert _line(r, 'state') == [v for q in m.seq for v in ((0, 0, 0) if q is None else (1, q[0], q[1]))]
    return m


@pytest.mark.parametrize('per_call', [0, 1, 7])
@pytest.mark.parametrize('kind', [R.RAW_IP, R.GRE])
def test_constructed_cases_under_sanitizers_equal_the_model(exe, tmp_path, kind, per_call):
    cases = K.cases() if kind == R.RAW_IP else K.gre_cases()
    m = _run_both(exe, tmp_path, *K.table_of(cases, shift=1), per_call, kind)
    assert m.stats() == K.expected_stats(cases)


@pytest.mark.parametrize('seed,kind', [(1, R.RAW_IP), (2, R.RAW_IP), (3, R.GRE)])
def test_random_tables_under_sanitizers(exe, tmp_path, seed, kind):
    m = _run_both(exe, tmp_path, *K.random_table(seed, 700, kind), 5 + 13 * seed, kind)
    st = m.stats()                                                   # the floors, on the model alone: the run has met every rule
    assert min(st.values()) > 0 and st['ts'] > 200, st
