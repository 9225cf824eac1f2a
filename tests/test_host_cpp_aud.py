"""The C++ host class of the audio bank (include/dvbs2gpu_host.hpp: AudBank) over a host bank, driven by tests/cpp/aud_host.cpp beside
a PsiBank on one multiplex written by the builders of tests/psi_ref.py and tests/aud_cases.py: it compiles warning-free, its watches
and codecs come from the decoded PMT, and its rows and counters are the values written out below, which are the model's."""
import os
import subprocess

import numpy as np
import pytest

import aud_cases as K
import aud_ref as A
import pes_ref as P
import psi_ref as S

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'aud_host')
NO = (1 << 64) - 1


@pytest.fixture(scope='module')
def aud_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'aud_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def test_cpp_audio_bank_beside_the_psi_bank(aud_host, tmp_path):
    rng = np.random.default_rng(4)
    fill = S.filler(0x2FF, 16, rng)
    V, M, D, X = 0x200, 0x201, 0x202, 0x203
    f24, f48 = K.mpa_frame(rng, b'\x55', ver=2, layer=1, bri=1, sri=1), K.mpa_frame(rng, b'\x55', ver=2, layer=1, bri=2, sri=1)    # MPEG-2 layer III at 24 kHz: 8 and 16 kbit/s
    a30, a40 = K.adts_frame(rng, 30, b'\x55'), K.adts_frame(rng, 40, b'\x55', chan=1)
    assert (len(f24), len(f48)) == (24, 48)
    m, d = K.Line(M, cc=0), K.Line(D, cc=0)
    m.pes(b'\x77' * 10).pes(b'\x77' * 10)                                     # calls 0 and 1: nothing is watched yet
    m.pes(f24 + f24 + f48[:10]).put(f48[10:] + f24[:5])                       # call 2: two frames, a third at another bitrate; a header whose last 3 bytes wait
    m.put(f24[5:] + b'\x00' * 9)                                              # call 3: there they are; 8 bytes that are no header, and one more
    d.pes(a30 + a40[:8]).put(a40[8:] + a30[:8])
    mp, dp = m.take(), d.take()
    ts = np.concatenate([
        S.Packetiser(0).lay([S.pat(0x77, [(0, 0x10), (1, 0x100)])]), mp[0:1], fill[0:2],                                  # call 0: the PAT
        S.Packetiser(0x100).lay([S.pmt(1, V, [(0x1b, V), (0x03, M), (0x0f, D), (0x06, X)])]), fill[2:3], mp[1:2], fill[3:4],  # call 1: the PMT names 0x201 and 0x202
        mp[2:3], dp[0:1], mp[3:4], fill[4:5],                                                                             # call 2
        mp[4:5], dp[1:2], fill[5:7]])                                                                                     # call 3
    assert len(ts) == 16
    ts.tofile(tmp_path / 'ts.bin')
    r = subprocess.run([aud_host, str(tmp_path / 'ts.bin'), '4', '16'], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert [l for l in lines if l.startswith('call ')] == ['call 0 rows 0', 'call 1 rows 0', 'call 2 rows 7', 'call 3 rows 3']
    hm24, hm48, ha30, ha40 = (int.from_bytes(f[:4], 'big') for f in (f24, f48, a30, a40))
    FR, AQ, CH = A.FRAME, A.ACQUIRED, A.CHANGE
    # call, pid, slot, unit, code, detail, flags, packet, kbps, head, es_offset, pts, dts, sample_rate, frame_bytes, samples
    want = [(2, M, 0, A.PES, 0xC0, P.HEADER, 0, 0, 0, 0, 0, 100800, NO, 0, 0, 0),
            (2, M, 0, FR, 9, 0, AQ, 0, 8, hm24, 0, NO, NO, 24000, 24, 576),
            (2, M, 0, FR, 9, 0, 0, 0, 8, hm24, 24, NO, NO, 24000, 24, 576),
            (2, M, 0, FR, 9, 0, CH, 0, 16, hm48, 48, NO, NO, 24000, 48, 576),
            (2, D, 1, A.PES, 0xC0, P.HEADER, 0, 1, 0, 0, 0, 93600, NO, 0, 0, 0),
            (2, D, 1, FR, 1, 2, AQ, 1, 11, ha30, 0, NO, NO, 48000, 30, 1024),
            (2, D, 1, FR, 1, 1, CH, 1, 15, ha40, 30, NO, NO, 48000, 40, 1024),
            (3, M, 0, FR, 9, 0, CH, 0, 8, hm24, 96, NO, NO, 24000, 24, 576),
            (3, M, 0, A.LOSS, 0, 0, 0, 0, 0, 0, 120, NO, NO, 0, 0, 0),
            (3, D, 1, FR, 1, 2, CH, 1, 11, ha30, 70, NO, NO, 48000, 30, 1024)]
    assert [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith('row ')] == want
    model = A.Aud(16)                                                       # the same from the model: watched from call 2 on
    model.set_watch(0, M, A.MPA), model.set_watch(1, D, A.ADTS)
    rows = []
    for c in (2, 3):
        model.process(ts[4 * c:4 * c + 4])
        rows += [(c,) + tuple(r[k] for k in A.ROW_KEYS) for r in model.table]
    assert rows == want
    assert [l for l in lines if l.startswith('left ')] == []
    stats = 'stats ' + ' '.join(str(model.stats()[k]) for k in A.STAT_KEYS)
    assert stats == 'stats 5 235 207 0 0 0 0 0 0 2 0 0 7 220 5376 2 1 4 0 1' and lines[-2:] == [stats, 'stream 16 0']
    r = subprocess.run([aud_host, str(tmp_path / 'ts.bin'), '4', '2'], capture_output=True, text=True, timeout=120)      # a table of two rows: the counters do not change
    assert r.returncode == 0, r.stderr
    lines = r.stdout.splitlines()
    assert len([l for l in lines if l.startswith('row ')]) == 4 and lines[-2:] == [stats, 'stream 16 6']
