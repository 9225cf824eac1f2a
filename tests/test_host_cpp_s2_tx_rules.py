"""csrc/s2_tx_rules.h -- the modulator's rules: PLS codes and sizes, bit interleaver, constellation tables, PL framing with pilots and PL scrambling, the pulse's
taps and block ends, the channel's generator -- checked on its own by tests/cpp/s2_tx_rules_host.cpp, built with the address and undefined-behaviour sanitizers:
every valid PLS code against a bit-by-bit restatement, code words in exactly sized blocks.  No GPU, no HIP header, no Python in the sanitized run."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 's2_tx_rules_host')


def test_s2_tx_rules():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra', '-Werror',
           '-I' + os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'cpp', 's2_tx_rules_host.cpp'), '-o', EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
