"""The C++ host class of the ULE bank (include/dvbs2gpu_host.hpp: UleBank) over a host bank, driven by tests/cpp/ule_host.cpp: it
compiles warning-free, the datagrams that come out are the ones that went in to the filtered address, and its rows and counters are
the values written out below."""
import os
import subprocess

import numpy as np
import pytest

import psi_ref as S
import ule_cases as K
import ule_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'ule_host')


@pytest.fixture(scope='module')
def ule_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'ule_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_ule_bank_over_a_host_bank(ule_host, tmp_path):
    rng = np.random.default_rng(4)
    other = bytes.fromhex('02aabbccdd02')
    sent = [K.dgram(60, 1), K.dgram(700, 2, sport=7), K.dgram(90, 3), K.dgram(300, 4), K.dgram(44, 5), K.dgram(50, 6)]
    sndus = [R.sndu(0x0800, sent[0], npa=K.GROUP), R.sndu(0x0800, sent[1], npa=K.GROUP), R.sndu(0x0800, sent[2], npa=other),
             R.sndu(*R.extended([(2, 0x11, b'\x01\x02')], *R.bridged(0x0800, sent[3])), npa=K.GROUP), R.sndu(0x0000, bytes(20), npa=K.GROUP),
             R.sndu(0x0800, sent[4] + bytes(3), npa=K.GROUP), R.sndu(0x0800, sent[5])]
    ule = R.Packetiser(K.PID).lay(sndus, pad=True)
    ule[2, 60] ^= 1                                                  # a bit error in the 700-byte datagram
    ts = np.concatenate([ule[:3], S.filler(0x31, 2, rng), ule[3:]])
    assert len(ts) == 10
    ts.tofile(tmp_path / 'ts.bin')
    args = [str(tmp_path / 'ts.bin'), '4', str(K.PID), K.NPA.hex(), K.MASK.hex()]
    r = subprocess.run([ule_host] + args + ['8', str(tmp_path / 'out.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == ['call 0 bytes 60', 'call 1 bytes 0', 'call 2 bytes 344']
    A, B = 3232235521, 3758096645
    assert [l for l in lines if l.startswith('row ')] == [
        'row 0 512 4 17 01005e000105 10 0 5004 1234 %d %d 74 0 60 0 0 2048 0' % (A, B),
        'row 1 2 0 0 000000000000 0 0 0 0 0 0 714 -1 0 -1 2 0 0',
        'row 1 4 0 0 02aabbccdd02 0 0 0 0 0 0 104 -1 0 2 2 0 0',       # (it starts and ends inside the fifth ULE packet)
        'row 2 544 4 17 01005e000105 28 4 5004 1234 %d %d 332 0 300 -1 0 2048 0' % (A, B),
        'row 2 16 0 0 01005e000105 0 0 0 0 0 0 34 -1 0 0 0 0 0',
        'row 2 512 4 17 01005e000105 10 0 5004 1234 %d %d 61 300 44 0 1 2048 3' % (A, B),
        'row 2 12 0 0 000000000000 0 0 0 0 0 0 58 -1 0 1 1 0 0']
    # packets, sndus, crc_errors, filtered, no_address, test, bridged, extension, other_protocol, bad_ip, datagrams, datagrams_delivered, bytes_delivered,
    # dropped_sndus, malformed_sndus, slack, malformed_packets, scrambled_packets
    assert lines[-2:] == ['stats 0 8 7 1 2 1 1 1 0 0 0 3 3 404 0 0 0 0 0', 'stats 1 8 7 1 0 1 1 1 0 0 0 5 0 0 0 0 0 0 0']
    assert (tmp_path / 'out.bin').read_bytes() == sent[0] + sent[3] + sent[4]
    args[1] = '10'                                                   # one call and a table of two rows: it fails for capacity, says 7 rows, and is repeated
    r = subprocess.run([ule_host] + args + ['2', str(tmp_path / 'again.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines()[:2] == ['call 0 capacity -1 7', 'call 0 bytes 404'] and r.stdout.splitlines()[-2:] == lines[-2:]
    assert (tmp_path / 'again.bin').read_bytes() == sent[0] + sent[3] + sent[4]
