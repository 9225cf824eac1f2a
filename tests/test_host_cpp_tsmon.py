"""The C++ host class of the TS monitor (include/dvbs2gpu_host.hpp: TSMonitor), driven by tests/cpp/tsmon_host.cpp on a file written
by the generator of tests/tsmon_ref.py.  CPU: it compiles warning-free and fails loudly without a GPU.  GPU: what it writes and
prints is the model's, and a call that does not fit is reported through the sticky status, not thrown."""
import os
import subprocess

import numpy as np
import pytest

import tsmon_ref as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG_DIR = os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd')
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'tsmon_host')


@pytest.fixture(scope='module')
def tsmon_host(pkg):
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'include'), os.path.join(ROOT, 'tests', 'cpp', 'tsmon_host.cpp'),
           '-o', EXE, '-L' + PKG_DIR, '-ldvbs2gpu', '-Wl,-rpath,' + PKG_DIR, '-pthread']
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    return EXE


def _mux(tmp_path):
    rng = np.random.default_rng(11)
    ts, info = T.make_mux(rng, 200, [0, 0x20, 0x21, 0x1FFE])
    for inject in T.INJECTORS:
        ts, info, _ = inject(rng, ts, info)
    ts.tofile(tmp_path / 'ts.bin')
    return ts


def _run(exe, tmp_path, per_call, cap, mode, pids):
    r = subprocess.run([exe, str(tmp_path / 'ts.bin'), str(tmp_path / 'out.bin'), str(per_call), str(cap), str(mode)] + [str(p) for p in pids],
                       capture_output=True, text=True, timeout=120)
    return r.returncode, r.stdout, r.stderr


def test_tsmon_host_builds_and_has_no_cpu_fallback(tsmon_host, tmp_path):
    import torch
    if torch.cuda.is_available():
        pytest.skip('GPU present: the no-device path cannot be shown')
    _mux(tmp_path)
    rc, out, err = _run(tsmon_host, tmp_path, 64, 64 * 188, 0, [])
    assert rc == 3 and 'no CPU fallback' in err, (rc, err)


@pytest.mark.gpu
@pytest.mark.parametrize('mode,pids,cap', [(0, [], 64 * 188), (1, [0x20, 0x1FFE], 188), (2, [0x21], 5 * 188)])
def test_cpp_monitor_equals_model(tsmon_host, tmp_path, mode, pids, cap):
    ts = _mux(tmp_path)
    rc, out, err = _run(tsmon_host, tmp_path, 64, cap, mode, pids)
    assert rc == 0, err
    m = T.Monitor()
    m.set_filter(mode=mode, pids=pids)
    want = np.concatenate([m.process(ts[a:a + 64]) for a in range(0, len(ts), 64)])
    assert np.array_equal(np.fromfile(tmp_path / 'out.bin', np.uint8), want)
    lines = out.splitlines()
    assert [int(v) for v in lines[0].split()[1:11]] == [m.stats()[k] for k in T.STAT_KEYS]
    assert [tuple(int(v) for v in l.split()[1:]) for l in lines if l.startswith('row ')] == m.table
    assert (int(lines[0].split('retries=')[1]) > 0) == (cap < 64 * 188)
