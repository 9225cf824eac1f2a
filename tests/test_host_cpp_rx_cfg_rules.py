"""csrc/rx_cfg_rules.h -- what a receiver configuration may be (DVB-S2 handle, DVB-S bank, RRC filter) and the key of the RRC tap cache -- checked on its
own by tests/cpp/rx_cfg_rules_host.cpp: every bound from both sides, the plugin's configuration, a model of the kernels' period / tile loops at the edge of the
rule (no list, budget or stage bound is reached, the outputs fit), and the key against the taps themselves.  No GPU, no HIP header."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, 'tests', 'cpp', 'build', 'rx_cfg_rules_host')


def test_rx_cfg_rules():
    os.makedirs(os.path.dirname(EXE), exist_ok=True)
    # (-ffp-contract=off: the tap generator rounds every operation separately, as in the library's build)
    cmd = ['g++', '-std=c++17', '-O1', '-ffp-contract=off', '-Wall', '-Wextra', '-Werror', '-I' + os.path.join(ROOT, 'sdrpp-dvbs-demodulator_amd', 'csrc'),
           os.path.join(ROOT, 'tests', 'cpp', 'rx_cfg_rules_host.cpp'), '-o', EXE]
    r = subprocess.run(cmd, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    r = subprocess.run([EXE], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
