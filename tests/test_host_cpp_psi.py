"""The C++ host class of the PSI section bank (include/dvbs2gpu_host.hpp: PsiBank) over a host bank, driven by tests/cpp/psi_host.cpp on
one multiplex written by the builders of tests/psi_ref.py: it compiles warning-free, and its rows, counters and decoded views are the
values written out below."""
import os
import subprocess

import numpy as np
import pytest

import psi_ref as P

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'psi_host')


@pytest.fixture(scope='module')
def psi_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'psi_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_psi_bank_on_one_multiplex(psi_host, tmp_path):
    rng = np.random.default_rng(4)
    zp, z1, z2 = P.Packetiser(0), P.Packetiser(0x100), P.Packetiser(0x101)
    pat = P.pat(0x77, [(0, 0x10), (1, 0x100), (2, 0x101)], version=3)
    pmt1 = P.pmt(1, 0x200, [(0x1b, 0x200), (0x0f, 0x201)], version=1)
    pmt2 = P.pmt(2, 0x210, [(0x02, 0x210)], version=9, program_info=bytes(300))          # 333 bytes: two packets
    ts = np.concatenate([zp.lay([pat]), P.filler(0x200, 3, rng), z1.lay([pmt1]), zp.lay([pat]), P.filler(0x200, 1, rng, 3), z2.lay([pmt2]), z1.lay([pmt1]), P.filler(0x200, 2, rng, 4)])
    assert len(ts) == 12
    ts.tofile(tmp_path / 'ts.bin')
    r = subprocess.run([psi_host, str(tmp_path / 'ts.bin'), '4', '10'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    # call 0: packets 0-3, the PAT alone (the PMT PIDs are not watched yet); 10 bytes do not hold it: one retry
    # call 1: packets 4-7: PMT 1 (slot 1), the PAT again (unchanged), the first packet of PMT 2
    # call 2: packets 8-11: PMT 2 ends (first_packet -1), PMT 1 again (unchanged)
    C = P.CHANGED
    assert [l for l in lines if l.startswith('row ')] == [
        'row 0 0 %d 0 1 3 1 0 0 119 %d 0 0' % (C, len(pat)),
        'row 1 256 %d 2 1 1 1 0 0 1 %d 0 0' % (C, len(pmt1)),
        'row 1 0 0 0 1 3 1 0 0 119 %d %d 1' % (len(pat), len(pmt1)),
        'row 2 257 %d 2 1 9 1 0 0 2 %d 0 -1' % (C, len(pmt2)),
        'row 2 256 0 2 1 1 1 0 0 1 %d %d 1' % (len(pmt1), len(pmt2))]
    total = 2 * len(pat) + 2 * len(pmt1) + len(pmt2)
    assert [l for l in lines if l.startswith('left ')] == []
    assert lines[-8] == 'stats 6 5 5 3 0 0 0 0 0 0 %d bytes=%d retries=3' % (total, total)       # every call needs more than the one before it got
    assert lines[-7:-3] == ['program 0 16', 'program 1 256', 'program 2 257', 'pat 119 3 0']
    assert lines[-3:] == ['pmt 1 1 1 512 0 27:512 15:513', 'pmt 2 2 9 528 0 2:528', 'pmt 3 -1 -1 -1 0']
