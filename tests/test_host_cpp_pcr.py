"""The C++ host class of the PCR bank (include/dvbs2gpu_host.hpp: PcrBank) over a host bank, driven by tests/cpp/pcr_host.cpp beside a
PsiBank on one multiplex written by the builders of tests/psi_ref.py and tests/pcr_ref.py: it compiles warning-free, its watches
come from the decoded PMT, and its rows and counters are the values written out below."""
import os
import subprocess

import numpy as np
import pytest

import pcr_ref as P
import psi_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'pcr_host')


@pytest.fixture(scope='module')
def pcr_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'pcr_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_pcr_bank_beside_the_psi_bank(pcr_host, tmp_path):
    rng = np.random.default_rng(4)
    fill = S.filler(0x202, 16, rng)
    pcr = lambda pid, v: P.pcr_packet(pid, v).reshape(1, -1)
    ts = np.concatenate([
        S.Packetiser(0).lay([S.pat(0x77, [(0, 0x10), (1, 0x100)])]), pcr(0x200, 0), fill[0:2],                     # call 0: the PAT; nothing watched
        S.Packetiser(0x100).lay([S.pmt(1, 0x200, [(0x1b, 0x200), (0x0f, 0x201)])]), fill[2:3], pcr(0x200, 6000), fill[3:4],   # call 1: the PMT names PID 0x200
        pcr(0x200, 8000), fill[4:5], pcr(0x200, 10014), pcr(0x201, 55),                                            # call 2: FIRST, 14 ticks fast over 2 packets
        pcr(0x200, 10014), fill[5:6], pcr(0x200, 14014), fill[6:7]])                                               # call 3: REPEATED, then measured from packet 10
    assert len(ts) == 16
    ts.tofile(tmp_path / 'ts.bin')
    r = subprocess.run([pcr_host, str(tmp_path / 'ts.bin'), '4', '8'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == ['call 0 records 0', 'call 1 records 0', 'call 2 records 2', 'call 3 records 2']
    assert [l for l in lines if l.startswith('row ')] == [
        'row 2 512 0 %d 0 0 8000 0 0 0' % P.FIRST,
        'row 2 512 0 %d %d 2 10014 2014 2 896' % (P.OK, P.ACCURACY_ERROR),
        'row 3 512 0 %d 0 0 10014 0 0 0' % P.REPEATED,
        'row 3 512 0 %d 0 2 14014 4000 4 0' % P.OK]
    assert [l for l in lines if l.startswith('left ')] == []
    assert lines[-3:] == ['stats 4 1 0 1 0 0 2 0 2 1 6014 6 4000 896', 'stream 16 3 0 -1 since 2 -1', 'rate %.3f' % (1504 * 27e6 * 6 / 6014)]
    r = subprocess.run([pcr_host, str(tmp_path / 'ts.bin'), '4', '1'], capture_output=True, text=True, timeout=120)      # a table of one row: the counters do not change
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len([l for l in lines if l.startswith('row ')]) == 2 and lines[-3] == 'stats 4 1 0 1 0 0 2 0 2 1 6014 6 4000 896' and lines[-2] == 'stream 16 3 2 -1 since 2 -1'
