"""The integer tables of the DVB-S2 physical layer, pinned to the reference (CPU only).

tests/golden/s2_tables_golden.json records what the reference's own code gives (tests/golden/make_golden_s2tables.py): the MODCOD
table of modcod_to_cfg.cpp, the PLS codewords and SOF word of s2_defs.h, the Gold sequence and the four rotations of
s2_scrambling.cpp.  Where oracle/_ref is built the fixture is compared with the reference live; everywhere, the header
csrc/s2_params.h (through the oracle's accessor) and the oracle's PL tables are compared with the fixture.  The float symbol
tables are tied to the pinned integers by SIGN only: their values, the constellation points and the demapper's LUT need the
reference's complex arithmetic and stay unpinned."""
import hashlib
import importlib.util
import json
import os

import numpy as np
import pytest

import orc

HERE = os.path.dirname(os.path.abspath(__file__))
G = json.load(open(os.path.join(HERE, 'golden', 's2_tables_golden.json')))
SHORT_9_10 = (11, 17, 23, 28)


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def f32_hex(x):
    return '%08x' % int(np.float32(x).view(np.uint32))


def test_fixture_equals_the_reference_live():
    R = orc.ref()
    if R is None or not hasattr(R, 'ref_modcod_cfg'):
        pytest.skip('oracle/_ref not built with the S2 table accessors')
    spec = importlib.util.spec_from_file_location('make_golden_s2tables', os.path.join(HERE, 'golden', 'make_golden_s2tables.py'))
    gen = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(gen)
    live = json.loads(json.dumps(gen.collect(R)))
    assert sorted(live) == sorted(G)
    for k in G:
        assert live[k] == G[k], k


def test_fixture_is_complete_and_the_reference_is_self_consistent():
    assert [(c['modcod'], c['short'], c['pilots']) for c in G['modcod_cfg']] == [(m, s, p) for m in range(1, 29) for s in (0, 1) for p in (0, 1)]
    assert all(c['modcod_back'] == c['modcod'] for c in G['modcod_cfg'])         # get_dvbs2_modcod undoes get_dvbs2_cfg
    assert G['modcod_rejected'] == [-1, 0, 29, 100]
    assert len(G['pls_codewords']) == 128 and len(set(G['pls_codewords'])) == 128
    assert len(G['deinterleave']) == 52 and len({(c['constel'], c['rate'], c['short']) for c in G['deinterleave']}) == 52
    # ring ratios are recorded exactly where the reference assigns them
    for c in G['modcod_cfg']:
        assert (c['g1'] is not None) == (c['constel'] >= 2) and (c['g2'] is not None) == (c['constel'] == 3), c


@pytest.mark.parametrize('short', (0, 1))
@pytest.mark.parametrize('pilots', (0, 1))
def test_modcod_table_equals_fixture(short, pilots):
    """csrc/s2_params.h: constellation, rate (by name), slot count, ring ratios as bit patterns, and the PLFRAME length computed here"""
    for c in G['modcod_cfg']:
        if (c['short'], c['pilots']) != (short, pilots):
            continue
        o = orc.modcod_params(c['modcod'], short, pilots)
        if short and c['modcod'] in SHORT_9_10:
            assert c['rate'] == '9/10' and o is None          # the reference has no rule for them and returns a configuration; ours rejects them
            continue
        assert o is not None, c
        assert (o['constel'], orc.RATE_NAMES[o['rate']], o['slots']) == (c['constel'], c['rate'], c['slots']), c
        assert o['bits'] == c['constel'] + 2
        assert f32_hex(o['g1']) == (c['g1'] or f32_hex(0.0)) and f32_hex(o['g2']) == (c['g2'] or f32_hex(0.0)), c    # 0 where the reference assigns none
        slots = c['slots']
        assert o['pilot_blocks'] == ((slots - 1) // 16 if pilots else 0)
        assert o['plframe'] == 90 * (slots + 1) + (36 * ((slots - 1) // 16) if pilots else 0), c
        assert o['N'] == (16200 if short else 64800) and slots * 90 * o['bits'] == o['N']
    for bad in (-1, 0, 29, 100):
        assert orc.modcod_params(bad, short, pilots) is None


def test_pls_codewords_and_sof_equal_fixture():
    sof, sym, codes, rn = orc.pl_tables()
    assert ['%016x' % int(c) for c in codes] == G['pls_codewords']
    # the symbol tables follow from the pinned integers by sign: pi/2-BPSK, s2_defs.h:22-29,70-75
    value, length = int(G['sof']['value'], 16), G['sof']['length']
    assert length == 26 and int(G['sof']['mask'], 16) == (1 << length) - 1 and value <= int(G['sof']['mask'], 16)
    quad = {0: (1, 1), 1: (-1, 1), 2: (-1, -1), 3: (1, -1)}          # angle pi/4 + k pi/2 -> signs of (re, im)
    for s in range(length):
        bit = (value >> (length - 1 - s)) & 1
        want = quad[bit * 2 + (s & 1)]
        assert (np.sign(sof[s].real), np.sign(sof[s].imag)) == want, s
        assert abs(abs(sof[s].real) - 2 ** -0.5) < 1e-6 and abs(abs(sof[s].imag) - 2 ** -0.5) < 1e-6
    for idx in range(128):
        code = int(G['pls_codewords'][idx], 16)
        yi = np.array([(code >> (63 - i)) & 1 for i in range(64)])
        nyi = yi ^ (np.arange(64) & 1)
        assert np.array_equal(np.sign(sym[idx].real), 1 - 2 * nyi) and np.array_equal(np.sign(sym[idx].imag), 1 - 2 * yi), idx
        assert np.abs(np.abs(sym[idx].real) - 2 ** -0.5).max() < 1e-6 and np.abs(np.abs(sym[idx].imag) - 2 ** -0.5).max() < 1e-6


def test_gold_sequence_equals_fixture():
    rn = orc.pl_tables()[3]
    assert rn.size == 131072 and sha(rn) == G['gold0']['sha256']
    assert [int(x) for x in rn[:64]] == G['gold0']['first64'] and [int(x) for x in rn[33128:33192]] == G['gold0']['at33128']
    assert set(G['gold0']['first64']) | set(G['gold0']['at33128']) == {0, 1, 2, 3}         # (the windows are not one value repeated)


def test_rotations_equal_fixture():
    got = orc.pl_rotation_cases()
    assert [[float(x) for x in row] for row in got] == G['rotations']
    assert len({tuple(r[:2]) for r in G['rotations']}) == 4 and len({tuple(r[2:]) for r in G['rotations']}) == 4
    # descrambling undoes scrambling: rotation r one way, then the other
    for r in range(4):
        sre, sim = G['rotations'][r][:2]
        back = {0: (sre, sim), 1: (sim, -sre), 2: (-sre, -sim), 3: (-sim, sre)}[r]     # s2_scrambling.cpp:37-58 applied to the scrambled pair
        assert back == (1.0, 2.0), r


@pytest.mark.parametrize('case', G['deinterleave'], ids=lambda c: 'm%d-s%d' % (c['modcod'], c['short']))
def test_oracle_deinterleaver_every_modcod(case):
    n = 16200 if case['short'] else 64800
    src = (np.arange(n) * 7 % 251).astype(np.int8)
    dst = np.zeros(n, np.int8)
    orc._bind_chain().orc_s2_deinterleave(case['constel'], orc.RATE_NAMES.index(case['rate']), case['short'], src, dst)
    assert sha(dst) == case['out_sha']
