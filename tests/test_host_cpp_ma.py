"""The C++ host class in its mode-adaptation mode (include/dvbs2gpu_host.hpp: BBFrameTSParser::setModeAdaptation, selectISI, the
work() overload with a frame-size list, flush), driven by tests/cpp/ma_host.cpp on files written by the transmitter of tests/ma_ref.py.
CPU: it compiles warning-free and fails loudly without a GPU.  GPU: what it writes is what was transmitted, TEI and counters included."""
import os
import subprocess

import numpy as np
import pytest

import ma_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'ma_host')


@pytest.fixture(scope='module')
def ma_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'ma_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _files(tmp_path, frames):
    np.concatenate(frames).tofile(tmp_path / 'frames.bin')
    (tmp_path / 'sizes.txt').write_text('\n'.join(str(f.size) for f in frames) + '\n')


def _run(exe, tmp_path, per_call, cap, issy, span, sel):
    r = subprocess.run([exe, str(tmp_path / 'frames.bin'), str(tmp_path / 'sizes.txt'), str(tmp_path / 'out'), str(per_call), str(cap), str(issy), str(span)] +
                       [str(i) for i in sel], capture_output=True, text=True, timeout=600)
    return r.returncode, r.stdout, r.stderr


def test_ma_host_builds_and_has_no_cpu_fallback(ma_host, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present: the no-device path cannot be shown')
    frames, ts, sel, cfg = M.scenario(1, True, '2', True, True, npk=20)
    _files(tmp_path, frames)
    rc, out, err = _run(ma_host, tmp_path, 4, 100000, 2, 0, sel)
    assert rc == 3 and 'no CPU fallback' in err, (rc, err)


@pytest.mark.gpu
@pytest.mark.parametrize('issy_mode,span,cap', [('auto', 0, 1 << 20), ('3', 1, 400)])
def test_cpp_parser_returns_every_selected_stream(ma_host, tmp_path, issy_mode, span, cap):
    damage = (4, 19)
    frames, ts, sel, cfg = M.scenario(6, True, issy_mode, True, True, span=span, damage=damage)
    _files(tmp_path, frames)
    rc, out, err = _run(ma_host, tmp_path, 5, cap, cfg['issy_bytes'], span, sel)
    assert rc == 0, err
    rx = M.Receiver(sel, **cfg)
    want = rx.process(frames)
    tail = rx.flush()
    lines = [dict(t.split('=') for t in l.split()[1:]) for l in out.splitlines()]
    for j, isi in enumerate(sel):
        got = np.fromfile(tmp_path / ('out%d.ts' % j), np.uint8)
        assert np.array_equal(got, np.concatenate([want[j], tail[j]]))
        a, b = got.reshape(-1, 188), ts[isi]
        assert a.shape == b.shape and int((a != b).any(axis=1).sum()) == len(damage)
        st = rx.stats(j)
        assert (int(lines[j]['isi']), int(lines[j]['packets']), int(lines[j]['nulls']), int(lines[j]['ts_errs']), int(lines[j]['broken_joins'])) == \
               (isi, st['packets'], st['nulls'], len(damage), 0)
        assert (int(lines[j]['retries']) > 0) == (cap < 1000)
