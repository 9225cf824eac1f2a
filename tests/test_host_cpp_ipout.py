"""The C++ host class of the IP output bank (include/dvbs2gpu_host.hpp: IpOutBank) over host banks, driven by tests/cpp/ipout_host.cpp
in front of an IpTsBank: it compiles warning-free, its rows and counters are the model's (tests/ipout_ref.py), the IP-TS bank reads
every datagram back without a complaint, the inner TS that comes out is the one that went in, and a capacity refusal is repeated with a
larger buffer."""
import os
import subprocess

import numpy as np
import pytest

import ipout_cases as K
import ipout_ref as R
import ipts_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'ipout_host')
PID = 0x155


@pytest.fixture(scope='module')
def ipout_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'ipout_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


@pytest.mark.parametrize('P,mode', [(7, R.RTP_MODE), (3, R.RAW)])
def test_cpp_ipout_bank_in_front_of_an_ipts_bank(ipout_host, tmp_path, P, mode):
    rng = np.random.default_rng(P)
    pids = [int(p) for p in rng.choice([PID, PID, 0x1FFF, 0x200], 61)]
    ts = K.packets(pids, seed=P, bad=(17,))
    ts.tofile(tmp_path / 'ts.bin')
    per_call = 9
    m = R.Stream()
    m.set_flow(2, family=4, src=bytes([10, 0, 0, 1]), dst=bytes([239, 9, 9, 9]), src_port=4000, dst_port=5500, ttl=5, dscp=34, mode=mode, ssrc=0xA1B2C3D4,
               seq_base=65534, timestamp_base=90000, packets_per_datagram=P, pid_mode=1, pids=(PID, 0x1FFF), drop_null=True)
    m.set_rate(1000 << 24)
    want, sizes, nrows = [], [], 0
    for c, a in enumerate(range(0, ts.size, per_call * 188)):
        out = m.process(ts[a:a + per_call * 188], a + per_call * 188 >= ts.size)[2]
        want.append('call %d bytes 0 0 %d 0' % (c, len(out)))
        want += ['row %d ' % c + ' '.join(str(r[k]) for k in R.ROW_KEYS) for r in m.table[2]]
        flags = (T.RTP if mode == R.RTP_MODE else T.RAW) | T.TS_ROW
        want += ['back %d %d %d %d' % (c, flags, r['packets'], r['rtp_seq']) for r in m.table[2]]
        sizes.append(len(out))
        nrows += len(m.table[2])
    st = m.stats(2)
    want.append('stats %d %d ' % (m.stats()['packets'], m.stats()['bad_sync']) + ' '.join(str(st[k]) for k in R.SLOT_KEYS))
    want.append('back stats %d %d %d 0 0' % (nrows, nrows, st['ts_packets']))
    sent = ts.reshape(-1, 188)
    sent = sent[(sent[:, 0] == 0x47) & ((sent[:, 1] & 31).astype(int) * 256 + sent[:, 2] == PID)].tobytes()
    assert st['held'] == 0 and st['short_datagrams'] == (len(sent) // 188 % P != 0) and m.stats()['bad_sync'] == 1 and nrows >= 3
    args = [str(tmp_path / 'ts.bin'), str(per_call), str(P), str(mode), str(PID)]
    r = subprocess.run([ipout_host] + args + ['8192', str(tmp_path / 'inner.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == want
    assert (tmp_path / 'inner.bin').read_bytes() == sent
    cap = min(s for s in sizes if s) - 1                             # a buffer one byte short of the smallest call
    r = subprocess.run([ipout_host] + args + [str(cap), str(tmp_path / 'again.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    again, refused = r.stdout.splitlines(), []
    for c, n in enumerate(sizes):                                    # every call that needs more than the buffer holds says so, and is repeated
        if n > cap:
            refused.append('call %d capacity %d' % (c, n))
            cap = n
    assert refused and [l for l in again if 'capacity' in l] == refused and [l for l in again if 'capacity' not in l] == want
    assert (tmp_path / 'again.bin').read_bytes() == sent
