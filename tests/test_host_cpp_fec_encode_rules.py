"""csrc/fec_encode_rules.h -- the FEC encoder's tables: BCH generator polynomials, byte table, chunk-shift rows, LDPC encode plan -- checked on its own by
tests/cpp/fec_encode_rules_host.cpp, built with the address and undefined-behaviour sanitizers: all 21 codes, the tables against shift-and-reduce, a model of the
kernel's chunked BCH arithmetic against the bit-serial LFSR, the LDPC links against QC_CODES, the funnel-shift reading of a rotated block.  No GPU, no HIP header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'fec_encode_rules_host')


def test_fec_encode_rules():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    cmd = ['g++', '-std=c++17', '-O1', '-g', '-fsanitize=address,undefined', '-fno-sanitize-recover=undefined', '-Wall', '-Wextra', '-Werror',
           '-I' + os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc'), os.path.join(ROOT, 'tests', 'cpp', 'fec_encode_rules_host.cpp'), '-o', EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
