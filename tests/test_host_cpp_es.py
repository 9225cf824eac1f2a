"""The C++ host class of the ES bank (include/dvbs2gpu_host.hpp: EsBank) over a host bank, driven by tests/cpp/es_host.cpp beside a
PsiBank on one multiplex written by the builders of tests/psi_ref.py and tests/es_cases.py: it compiles warning-free, its watches and
codecs come from the decoded PMT, and its rows and counters are the values written out below."""
import os
import subprocess

import numpy as np
import pytest

import es_cases as K
import pes_ref as P
import psi_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'es_host')
NO = (1 << 64) - 1


@pytest.fixture(scope='module')
def es_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'es_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_es_bank_beside_the_psi_bank(es_host, tmp_path):
    rng = np.random.default_rng(4)
    fill = S.filler(0x202, 16, rng)
    V, A, M = 0x200, 0x201, 0x210
    v, m, SC = K.Line(V, cc=0), K.Line(M, cc=0), K.SC
    v.pes(b'\x77' * 10).pes(b'\x77' * 10)                                                         # calls 0 and 1: nothing is watched yet
    v.pes(SC + b'\x09\xF0' + SC + b'\x65\x88' + b'\x77' * 20).put(b'\x77' * 5 + SC + b'\x41\x98')   # call 2: AUD, an IDR picture; a P slice whose head waits
    v.put(b'\x77' * 30)                                                                           # call 3: there it is
    m.pes(SC + b'\xB3' + b'\x11' * 8 + SC + b'\xB8' + b'\x22' * 4 + SC + b'\x00\x01\x4F\x33\x33' + SC + b'\x01' + b'\x44' * 10)
    m.pes(SC + b'\x00\x01\x97\x33\x33' + SC + b'\xB7' + b'\x55' * 4)
    vp, mp = v.take(), m.take()
    ts = np.concatenate([
        S.Packetiser(0).lay([S.pat(0x77, [(0, 0x10), (1, 0x100)])]), vp[0:1], fill[0:2],                                   # call 0: the PAT
        S.Packetiser(0x100).lay([S.pmt(1, V, [(0x1b, V), (0x0f, A), (0x02, M), (0x05, 0x203)])]), fill[2:3], vp[1:2], fill[3:4],   # call 1: the PMT names 0x200 and 0x210
        vp[2:3], mp[0:1], vp[3:4], fill[4:5],                                                                             # call 2
        vp[4:5], mp[1:2], fill[5:7]])                                                                                     # call 3
    assert len(ts) == 16
    ts.tofile(tmp_path / 'ts.bin')
    r = subprocess.run([es_host, str(tmp_path / 'ts.bin'), '4', '16'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == ['call 0 rows 0', 'call 1 rows 0', 'call 2 rows 7', 'call 3 rows 4']
    assert [l for l in lines if l.startswith('row ')] == [
        'row 2 512 0 0 224 %d 0 0 0 0 100800 %d' % (P.HEADER, NO),
        'row 2 512 0 5 9 0 0 0 %d 0 %d %d' % (0xF0000001, NO, NO),
        'row 2 512 0 1 101 1 1 0 %d 5 %d %d' % (0x88777777, NO, NO),
        'row 2 528 1 0 224 %d 0 1 0 0 93600 %d' % (P.HEADER, NO),
        'row 2 528 1 2 179 0 0 1 %d 0 %d %d' % (0x11111111, NO, NO),
        'row 2 528 1 3 184 0 0 1 %d 12 %d %d' % (0x22222222, NO, NO),
        'row 2 528 1 1 0 1 1 1 %d 20 %d %d' % (0x014F3333, NO, NO),
        'row 3 512 0 1 65 2 0 0 %d 35 %d %d' % (0x98777777, NO, NO),
        'row 3 528 1 0 224 %d 0 1 0 42 97200 %d' % (P.HEADER, NO),
        'row 3 528 1 1 0 2 0 1 %d 42 %d %d' % (0x01973333, NO, NO),
        'row 3 528 1 6 183 0 0 1 %d 50 %d %d' % (0x55555555, NO, NO)]
    assert [l for l in lines if l.startswith('left ')] == []
    stats = 'stats 5 170 128 0 0 0 0 0 0 3 0 0 9 4 2 2 0 2 1 1 0 1 1 1 0 0'
    assert lines[-2:] == [stats, 'stream 16 0']
    r = subprocess.run([es_host, str(tmp_path / 'ts.bin'), '4', '2'], capture_output=True, text=True, timeout=120)      # a table of two rows: the counters do not change
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len([l for l in lines if l.startswith('row ')]) == 4 and lines[-2:] == [stats, 'stream 16 7']
