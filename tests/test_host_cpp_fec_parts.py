"""csrc/fec_parts.h -- how the pooled frames of an ACM/VCM or mixed-MODCOD call are divided into FEC parts and laid out in the job's buffers -- checked on its
own by tests/cpp/fec_parts_host.cpp: no frames, frames without a part, odd counts, one code with several iteration settings, the real (N, kbch / 8) pairs of
the short codes and of normal ones; index list, disjoint ranges, padding, result indices, first-appearance order, determinism.  No GPU, no HIP header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'fec_parts_host')


def test_fec_parts():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'cpp', 'fec_parts_host.cpp'), '-o', EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
