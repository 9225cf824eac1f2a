"""csrc/ipout_rules.h under ASan + UBSan: tests/cpp/ipout_rules_san.cpp, a stand-alone program that includes nothing but the rules, run
directly (its own process) on the constructed cases of tests/ipout_cases.py and on seeded random packets, where what it prints must
be the model's."""
import os
import subprocess

import numpy as np
import pytest

import ipout_cases as K
import ipout_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD = os.path.join(ROOT, 'tests', 'cpp', 'build')
SAN = ['-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-fno-omit-frame-pointer', '-g', '-O1']
ENV = dict(os.environ, ASAN_OPTIONS='detect_leaks=1:abort_on_error=0:exitcode=23', UBSAN_OPTIONS='print_stacktrace=1:halt_on_error=1')
CASES = K.cases()


@pytest.fixture(scope='module')
def exe():
    os.makedirs(BUILD, exist_ok=True)
    out = os.path.join(BUILD, 'ipout_rules_san')
    r = subprocess.run(['g++', '-std=c++17', '-Wall', '-Wextra', '-Werror'] + SAN + [os.path.join(ROOT, 'tests', 'cpp', 'ipout_rules_san.cpp'), '-o', out],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    return out


def _flow_line(slot, f):
    f = dict(R.FLOW_DEFAULTS, **f)
    pids = sorted(f['pids'])
    nums = [f[k] for k in ('src_port', 'dst_port', 'ttl', 'dscp', 'mode', 'packets_per_datagram', 'ssrc', 'timestamp_base', 'seq_base', 'pid_mode')]
    return 'flow %d %d %s %s ' % (slot, f['family'], f['src'].hex(), f['dst'].hex()) + ' '.join(str(int(v)) for v in nums + [bool(f['drop_null']), len(pids)] + pids)


def _run_both(exe, tmp_path, flows, calls):
    """the program and the model on the same calls [(rate or None, packets, flush)] -> the model; rows, counters and byte hashes are compared"""
    m = R.Stream()
    script, rows, h, at, parts = [], [], [0] * 4, 0, []
    for slot, f in flows.items():
        m.set_flow(slot, **f)
        script.append(_flow_line(slot, f))
    for c, (rate, ts, flush) in enumerate(calls):
        if rate is not None:
            m.set_rate(rate)
            script.append('rate %d' % rate)
        script.append('call %d %d %d' % (at, ts.size // 188, flush))
        at += ts.size // 188
        parts.append(ts)
        for k, out in enumerate(m.process(ts, flush)):
            for b in out:
                h[k] = (h[k] * 131 + b) % 1000000007
            rows += [(c, k) + tuple(r[key] for key in R.ROW_KEYS) for r in m.table[k]]
    np.concatenate(parts + [np.zeros(0, np.uint8)]).tofile(tmp_path / 'ts.bin')
    (tmp_path / 'script.txt').write_text('\n'.join(script) + '\n')
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(tmp_path / 'script.txt')], capture_output=True, text=True, timeout=120, env=ENV)
    assert r.returncode == 0 and 'ipout rules run ok' in r.stdout, (r.returncode, r.stdout[-500:], r.stderr[-3000:])
    assert 'runtime error' not in r.stderr and 'AddressSanitizer' not in r.stderr, r.stderr[-3000:]
    line = lambda head: [int(v) for v in [l for l in r.stdout.splitlines() if l.startswith(head)][0].split()[1:]]
    assert [tuple(int(v) for v in l.split()[1:]) for l in r.stdout.splitlines() if l.startswith('row ')] == rows
    assert line('stats') == [m.st[k] for k in R.STREAM_KEYS] + [s[k] for s in m.slot_st for k in R.SLOT_KEYS]
    assert line('bytes') == h
    return m


@pytest.mark.parametrize('cut', [None, 1, 7])
def test_constructed_cases_under_sanitizers_equal_the_model(exe, tmp_path, cut):
    for case in CASES:
        _run_both(exe, tmp_path, case[1], K.calls(case, cut))


@pytest.mark.parametrize('seed', [1, 2, 3])
def test_random_packets_under_sanitizers(exe, tmp_path, seed):
    rng = np.random.default_rng(seed)
    pids = [0x100, 0x101, 0x102, 0x1FFF, 0x33]
    flows = {0: K.flow(4, R.RTP_MODE, 7, port=5600, seq_base=65000 + seed), 1: K.flow(6, R.RAW, 1 + seed, port=5601, pid_mode=1, pids=(0x100, 0x33)),
             2: K.flow(6, R.RTP_MODE, 3, port=5602, pid_mode=2, pids=(0x101,), drop_null=True, timestamp_base=2 ** 32 - 1000),
             3: K.flow(4, R.RAW, 2 * seed, port=5603, drop_null=True)}
    calls = []
    for c in range(40):
        n = int(rng.integers(0, 60))
        ts = K.packets([pids[i] for i in rng.integers(0, len(pids), n)], seed=100 * seed + c, bad=tuple(int(b) for b in rng.integers(0, 200, 2)))
        calls.append((K.RATE * (1 + c // 10) if c % 10 == 0 else None, ts, c % 9 == 8))
    m = _run_both(exe, tmp_path, flows, calls)
    st = m.stats()                                                   # the floors, on the model alone: the run has met every counter
    assert min(st[k] for k in R.STAT_KEYS if k != 'held') > 0 and st['datagrams'] > 300, st
