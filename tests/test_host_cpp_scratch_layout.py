"""csrc/scratch_layout.h, the helper every host flow declares its scratch-buffer layouts with, checked on its own by
tests/cpp/scratch_layout_host.cpp: alignment of every sub-array, no overlap, the size, zero counts, a second base.  No GPU, no HIP header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'scratch_layout_host')


def test_scratch_layout_rules():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'cpp', 'scratch_layout_host.cpp'), '-o', EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
