"""The C++ host class of the T2-MI bank (include/dvbs2gpu_host.hpp: T2miBank) over a host bank, driven by tests/cpp/t2mi_host.cpp in
front of a host mode-adaptation bank: it compiles warning-free, the inner transport stream is what went into the BBFRAMEs, and its
rows and counters are the values written out below."""
import os
import subprocess

import numpy as np
import pytest

import ma_ref as M
import psi_ref as S
import t2mi_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 't2mi_host')


@pytest.fixture(scope='module')
def t2mi_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 't2mi_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_t2mi_bank_in_front_of_the_mode_adaptation_bank(t2mi_host, tmp_path):
    rng = np.random.default_rng(4)
    inner = M.make_ts(12, rng, null_runs=False)
    frames = [f for f, _ in M.frames_of_stream(M.slot_stream(inner)[0], 188, [7032], sis=True)]
    assert len(frames) == 3
    other = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    pk = [T.bb_packet(10, 3, bytes(frames[0]), frame_idx=0, start=1), T.t2mi_packet(0x10, 11, bytes(40)), T.bb_packet(12, 5, other, frame_idx=1),
          T.bb_packet(14, 3, bytes(frames[1]), frame_idx=2), T.t2mi_packet(0x20, 15, bytes(11), payload_bits=88), T.bb_packet(16, 3, bytes(frames[2]), frame_idx=3)]
    t2 = T.Packetiser(0x1000).lay(pk)
    t2[9, 60] ^= 1                                                   # a bit error in the second BBFRAME of PLP 3
    ts = np.concatenate([t2[:7], S.filler(0x31, 2, rng), t2[7:]])
    assert len(ts) == 19
    ts.tofile(tmp_path / 'ts.bin')
    r = subprocess.run([t2mi_host, str(tmp_path / 'ts.bin'), '8', str(0x1000), '3', '8', str(tmp_path / 'inner.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == ['call 0 bytes 879 frames 879', 'call 1 bytes 0 frames', 'call 2 bytes 879 frames 879']
    B, I, C, N = T.BBFRAME, T.INTL_FRAME_START, T.CRC_ERROR, T.COUNT_ERROR
    assert [l for l in lines if l.startswith('row ')] == [
        'row 0 0 10 0 0 %d 3 0 7056 892 0 879 0 4' % (B | I),
        'row 0 16 11 0 0 0 0 0 320 50 -1 0 4 5',
        'row 0 0 12 0 0 %d 5 1 2424 313 -1 300 5 6' % B,
        'row 1 0 14 0 0 %d 0 0 7056 892 -1 0 -1 5' % C,
        'row 1 32 15 0 0 %d 0 0 88 21 -1 0 5 5' % N,
        'row 2 0 16 0 0 %d 3 3 7056 892 0 879 -1 2' % B]
    assert lines[-2:] == ['stats 0 17 6 1 1 3 0 2 1758 0 0 0 0', 'stats 1 17 6 1 1 3 0 0 0 0 0 0 0']
    got = np.fromfile(tmp_path / 'inner.bin', np.uint8)
    rx = M.Receiver((0,))
    want = np.concatenate([rx.process([frames[0]])[0], rx.process([frames[2]])[0]])
    assert np.array_equal(got, want) and got.size >= 4 * 188       # two data fields of 869 bytes
    r = subprocess.run([t2mi_host, str(tmp_path / 'ts.bin'), '8', str(0x1000), '3', '2', str(tmp_path / 'inner.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr                               # a table of two rows: the call fails for capacity, says 3 rows, and is repeated
    assert r.stdout.splitlines()[0] == 'call 0 capacity -1 3' and r.stdout.splitlines()[-2:] == lines[-2:]
