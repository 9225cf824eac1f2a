"""The C++ host class on GSE frames (include/dvbs2gpu_host.hpp: BBFrameTSParser::work, pdu_table, gse_stats, set_gse_path), driven by
tests/cpp/gse_host.cpp.  CPU: it compiles warning-free.  GPU: the rows cut the output into exactly the transmitted PDUs."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'gse_host')


@pytest.fixture(scope='module')
def gse_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'gse_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_gse_host_builds(gse_host):
    assert os.path.exists(gse_host)


@pytest.mark.gpu
@pytest.mark.parametrize('path', [0, 1])
def test_cpp_parser_hands_out_one_row_per_pdu(gse_host, tmp_path, path):
    import test_gpu_gse as T
    kbch = 14232
    pk, want = T.transmitter(np.random.default_rng(300), 12 * (kbch // 8 - 10))
    frames = T.pack_frames(pk, kbch)
    frames.tofile(tmp_path / 'frames.bin')
    r = subprocess.run([gse_host, str(tmp_path / 'frames.bin'), str(kbch), '5', str(tmp_path / 'out.bin'), str(path)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = np.fromfile(tmp_path / 'out.bin', np.uint8)
    lines = [dict(t.split('=') for t in l.split()[1:]) for l in r.stdout.splitlines()]
    rows, stats = lines[:-1], lines[-1]
    assert len(rows) == len(want)
    for row, (proto, pdu, reasm, lab) in zip(rows, want):
        a, n = int(row['offset']), int(row['bytes'])
        assert bytes(out[a:a + n]) == T.gre(proto, pdu) and int(row['protocol']) == proto and int(row['flags']) == (1 if reasm else 0) | (2 if lab else 0)
    assert sum(int(r_['bytes']) for r_ in rows) == out.size == int(stats['bytes'])
    assert (int(stats['frames']), int(stats['complete']) + int(stats['reassembled']), int(stats['fallbacks'])) == (len(frames), len(want), 0)
    assert int(stats['packets']) >= len(pk) - 20
