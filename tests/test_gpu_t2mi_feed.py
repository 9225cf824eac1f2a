"""T2miBank::feed of the C++ host class (include/dvbs2gpu_host.hpp) on the device: tests/cpp/t2mi_feed.cpp runs a device T2-MI bank in
front of a dvbs2::BBFrameTSParser in mode-adaptation mode and hands every call's BBFRAMEs over with feed().  The inner transport stream is
what went into the BBFRAMEs, a feed() into too small a buffer says false, names the size and consumes nothing.  (The host-bank program
tests/cpp/t2mi_host.cpp cannot call feed(): the parser class has no host form.)"""
import os
import subprocess

import numpy as np
import pytest

import ma_ref as M
import psi_ref as S
import t2mi_ref as T

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 't2mi_feed')


@pytest.fixture(scope='module')
def t2mi_feed(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 't2mi_feed.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_feed_hands_a_device_banks_bbframes_to_the_parser(t2mi_feed, tmp_path):
    rng = np.random.default_rng(4)
    inner = M.make_ts(12, rng, null_runs=False)
    frames = [f for f, _ in M.frames_of_stream(M.slot_stream(inner)[0], 188, [7032], sis=True)]
    assert len(frames) == 3
    other = bytes(rng.integers(0, 256, 300, dtype=np.uint8))
    pk = [T.bb_packet(10, 3, bytes(frames[0]), frame_idx=0, start=1), T.t2mi_packet(0x10, 11, bytes(40)), T.bb_packet(12, 5, other, frame_idx=1),
          T.bb_packet(14, 3, bytes(frames[1]), frame_idx=2), T.t2mi_packet(0x20, 15, bytes(11), payload_bits=88), T.bb_packet(16, 3, bytes(frames[2]), frame_idx=3)]
    t2 = T.Packetiser(0x1000).lay(pk)
    t2[9, 60] ^= 1                                                   # a bit error in the second BBFRAME of PLP 3: it is not delivered
    ts = np.concatenate([t2[:7], S.filler(0x31, 2, rng), t2[7:]])
    assert len(ts) == 19
    ts.tofile(tmp_path / 'ts.bin')
    rx = M.Receiver((0,))
    want = [rx.process([frames[0]])[0], rx.process([frames[2]])[0]]
    assert all(w.size >= 188 for w in want)                          # so 187 bytes are too few for either call
    r = subprocess.run([t2mi_feed, str(tmp_path / 'ts.bin'), '8', str(0x1000), '3', '8', str(tmp_path / 'inner.bin')], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    assert r.stdout.splitlines() == ['call 0 bytes 879 frames 1 refused %d inner %d' % (want[0].size, want[0].size), 'call 1 bytes 0 frames 0 refused 0 inner 0',
                                     'call 2 bytes 879 frames 1 refused %d inner %d' % (want[1].size, want[1].size),
                                     'parser packets %d rejected 0 skipped 0' % rx.stats(0)['packets']]
    assert np.array_equal(np.fromfile(tmp_path / 'inner.bin', np.uint8), np.concatenate(want))
