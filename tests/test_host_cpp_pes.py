"""The C++ host class of the PES bank (include/dvbs2gpu_host.hpp: PesBank) over a host bank, driven by tests/cpp/pes_host.cpp beside a
PsiBank on one multiplex written by the builders of tests/psi_ref.py and tests/pes_ref.py: it compiles warning-free, its watches
come from the decoded PMT, and its rows and counters are the values written out below."""
import os
import subprocess

import numpy as np
import pytest

import pes_ref as P
import psi_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'pes_host')
NO = (1 << 64) - 1


@pytest.fixture(scope='module')
def pes_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'pes_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_pes_bank_beside_the_psi_bank(pes_host, tmp_path):
    rng = np.random.default_rng(4)
    fill = S.filler(0x202, 16, rng)
    V, A = 0x200, 0x201
    video = lambda cc, **kw: P.pes_packet(V, cc, 0xE0, **kw).reshape(1, -1)
    audio = lambda cc, **kw: P.pes_packet(A, cc, 0xC0, **kw).reshape(1, -1)
    body = lambda cc: P.body_packet(V, cc).reshape(1, -1)
    ts = np.concatenate([
        S.Packetiser(0).lay([S.pat(0x77, [(0, 0x10), (1, 0x100)])]), video(0, pts=1), fill[0:2],                        # call 0: the PAT; nothing watched
        S.Packetiser(0x100).lay([S.pmt(1, V, [(0x1b, V), (0x0f, A), (0x05, 0x203)])]), fill[2:3], video(1, pts=2), fill[3:4],   # call 1: the PMT names 0x200, 0x201
        video(2, pts=90000, declared=362), body(3), audio(0, pts=90000), video(4, pts=93600),                           # call 2: two firsts; a whole PES packet closed
        body(5), audio(1, pts=160000), video(6, pts=97200, dts=95400), fill[4:5]])                                      # call 3: a gap of the audio timestamps; T is the DTS
    assert len(ts) == 16
    ts.tofile(tmp_path / 'ts.bin')
    r = subprocess.run([pes_host, str(tmp_path / 'ts.bin'), '4', '8'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == ['call 0 starts 0', 'call 1 starts 0', 'call 2 starts 3', 'call 3 starts 2']
    first, unb, closed, unc, gap = P.TS_FIRST, P.UNBOUNDED_NONVIDEO, P.CLOSED, P.CLOSED_UNCHECKED, P.TS_GAP
    assert [l for l in lines if l.startswith('row ')] == [
        'row 2 512 0 5 %d 224 0 362 90000 %d 0 0 0 0' % (first, NO),
        'row 2 513 1 5 %d 192 2 0 90000 %d 0 0 0 0' % (first | unb, NO),
        'row 2 512 0 5 %d 224 3 0 93600 %d 368 2 3 3600' % (closed, NO),
        'row 3 513 1 5 %d 192 1 0 160000 %d 184 1 3 70000' % (closed | unc | unb | gap, NO),
        'row 3 512 0 5 %d 224 2 0 97200 95400 368 2 3 1800' % (closed | unc)]
    assert [l for l in lines if l.startswith('left ')] == []
    stats = 'stats 7 1288 0 0 0 0 5 0 0 0 0 0 5 5 1 1 0 0 2 0 1 0 0 3'
    assert lines[-2:] == [stats, 'stream 16 0 since 2 3 -1']
    r = subprocess.run([pes_host, str(tmp_path / 'ts.bin'), '4', '1'], capture_output=True, text=True, timeout=120)      # a table of one row: the counters do not change
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len([l for l in lines if l.startswith('row ')]) == 2 and lines[-2:] == [stats, 'stream 16 3 since 2 3 -1']
