"""The C++ host class of the IP-TS bank (include/dvbs2gpu_host.hpp: IpTsBank) over host banks, driven by tests/cpp/ipts_host.cpp
behind an MpeBank: it compiles warning-free, the inner TS that comes out is the one that went in, and its rows and counters are the
models' (tests/mpe_ref.py, then tests/ipts_ref.py) and the values written out below."""
import os
import subprocess

import numpy as np
import pytest

import ipts_ref as R
import mpe_ref as MP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'ipts_host')
PID, PORT = 0x0300, 1234


@pytest.fixture(scope='module')
def ipts_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'ipts_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_ipts_bank_behind_an_mpe_bank(ipts_host, tmp_path):
    inner = [R.ts_packets(2, 0x100 + i, 2 * i, seed=i) for i in range(6)]
    ds = [R.datagram(R.rtp(inner[0], seq=10, timestamp=1000, ssrc=0x0A0B0C0D)), R.datagram(R.rtp(inner[1], seq=11, timestamp=2000, ssrc=0x0A0B0C0D)),
          R.datagram(R.rtp(inner[2], seq=13, timestamp=3000, ssrc=0x0A0B0C0D)), R.datagram(R.rtp(inner[3], seq=12, ssrc=0x0A0B0C0D)),
          R.datagram(inner[4], dport=PORT + 1), R.datagram(inner[5])]
    secs = [MP.section(d) for d in ds]
    secs.insert(2, MP.raw_section(0x3B, bytes(30)))                  # another table: a row without a datagram
    ts = MP.Packetiser(PID).lay(secs)
    ts.tofile(tmp_path / 'ts.bin')
    per_call = 5
    m1, m2 = MP.Slot(PID), R.Stream()
    m2.set_flow(1, 4, R.V4_DST, PORT)
    want_rows, want_ts, want_calls, sizes = [], b'', [], []
    for c, a in enumerate(range(0, len(ts), per_call)):
        ip = m1.process(ts[a:a + per_call])
        out = m2.process(ip, [(r['offset'], r['bytes']) for r in m1.table])
        want_rows += ['row %d ' % c + ' '.join(str(r[k]) for k in R.ROW_KEYS) for r in m2.table]
        want_calls.append('call %d bytes 0 %d 0 0' % (c, out[1].size))
        want_ts += out[1].tobytes()
        sizes.append(out[1].size)
    args = [str(tmp_path / 'ts.bin'), str(per_call), str(PID), R.V4_DST.hex(), str(PORT)]
    r = subprocess.run([ipts_host] + args + ['4096', str(tmp_path / 'inner.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == want_calls and [l for l in lines if l.startswith('row ')] == want_rows
    stats = lambda s: ' '.join(str(m2.stats(s)[k]) for k in R.STAT_KEYS)
    assert lines[-3:] == ['stats -1 ' + stats(-1), 'stats 0 ' + stats(0), 'stats 1 ' + stats(1)]
    assert (tmp_path / 'inner.bin').read_bytes() == want_ts == inner[0] + inner[1] + inner[2] + inner[5]
    # written out: flags, slot, packets, lost of the seven rows, and the counters of slot 1
    assert [tuple(int(v) for v in (l.split()[2], l.split()[3], l.split()[12], l.split()[13])) for l in lines if l.startswith('row ')] == [
        (R.RTP | R.TS_ROW, 1, 2, 0), (R.RTP | R.TS_ROW, 1, 2, 0), (R.NOT_DELIVERED, -1, 0, 0), (R.RTP | R.LOSS | R.TS_ROW, 1, 2, 1), (R.RTP | R.LATE, 1, 0, 0),
        (R.UNWATCHED, -1, 0, 0), (R.RAW | R.TS_ROW, 1, 2, 0)]
    # rows .. unwatched | matched, bad_checksum, no_checksum, bad_payload, other_payload, raw, rtp, new_source, loss_events, late, ts, ts_packets, bytes, lost
    assert lines[-3] == 'stats -1 7 1 0 0 0 0 0 1 5 0 0 0 0 1 4 0 1 1 4 8 1504 1'
    r = subprocess.run([ipts_host] + args + ['375', str(tmp_path / 'again.bin')], capture_output=True, text=True, timeout=120)      # a buffer of one packet short
    assert r.returncode == 0, r.stderr
    again, cap, refused = r.stdout.splitlines(), 375, []
    for c, n in enumerate(sizes):                                    # every call that needs more than the buffer holds says so, and is repeated
        if n > cap:
            refused.append('call %d capacity %d' % (c, n))
            cap = n
    assert refused and [l for l in again if 'capacity' in l] == refused and [l for l in again if 'capacity' not in l] == lines
    assert (tmp_path / 'again.bin').read_bytes() == want_ts
