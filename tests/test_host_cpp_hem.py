"""The C++ host class on DVB-T2 high-efficiency-mode BBFRAMEs (include/dvbs2gpu_host.hpp: BBFrameTSParser::setModeAdaptationT2HEM), driven
by tests/cpp/hem_host.cpp on files written by the transmitter of tests/hem_ref.py.  CPU: it compiles warning-free and, where there is
no GPU, fails loudly.  GPU: with the switch on it returns the selected PLPs' TS, with it off nothing."""
import os
import subprocess

import numpy as np
import pytest

import hem_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'hem_host')


@pytest.fixture(scope='module')
def hem_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'hem_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _run(exe, tmp_path, frames, per_call, switch, sel):
    np.concatenate(frames).tofile(tmp_path / 'frames.bin')
    (tmp_path / 'sizes.txt').write_text('\n'.join(str(f.size) for f in frames) + '\n')
    r = subprocess.run([exe, str(tmp_path / 'frames.bin'), str(tmp_path / 'sizes.txt'), str(tmp_path / 'out'), str(per_call), str(int(switch))] +
                       [str(i) for i in sel], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_hem_host_builds_and_has_no_cpu_fallback(hem_host, tmp_path):
    import torch
    if not torch.cuda.is_available():                              # (with a GPU the program's results are the next test's)
        frames, ts, sel = H.random_carrier(1, True, True, mis=True)
        rc, out, err = _run(hem_host, tmp_path, frames, 4, True, sel)
        assert rc == 3 and 'no CPU fallback' in err, (rc, err)


@pytest.mark.gpu
@pytest.mark.parametrize('switch', [True, False])
def test_cpp_parser_returns_the_selected_plps(hem_host, tmp_path, switch):
    frames, ts, sel = H.random_carrier(7, True, True, mis=True)
    rc, out, err = _run(hem_host, tmp_path, frames, 5, switch, sel)
    assert rc == 0, err
    rx, want = H.run_model(frames, sel, H.CFG, step=5, hem=switch)
    lines = [dict(t.split('=') for t in l.split()[1:]) for l in out.splitlines()]
    for j, isi in enumerate(sel):
        got = np.fromfile(tmp_path / ('out%d.ts' % j), np.uint8)
        st = rx.stats(j)
        assert np.array_equal(got, want[j])
        assert [int(lines[j][k]) for k in ('isi', 'packets', 'nulls', 'frames', 'hem_frames', 'broken_joins', 'rejected', 'skipped')] == \
               [isi, st['packets'], st['nulls'], st['frames'], st['hem_frames'], st['broken_joins'], rx.rejected, rx.skipped]
        if switch:
            assert got.size > 0 and np.array_equal(got, ts[isi].reshape(-1)[:got.size]) and st['hem_frames'] > 0
        else:
            assert got.size == 0 and rx.rejected == len(frames)
