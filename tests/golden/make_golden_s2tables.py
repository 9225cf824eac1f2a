#!/usr/bin/env python3
"""Generates tests/golden/s2_tables_golden.json from the REFERENCE's own DVB-S2 physical-layer tables compiled into
oracle/_ref/libdvbs2ref.so (recipe: oracle/Makefile target `ref`; only works where the reference tree exists):

  modcod_cfg    get_dvbs2_cfg for MODCOD 1..28 x frame size x pilots (modcod_to_cfg.cpp:5-140) and the MODCOD get_dvbs2_modcod
                makes of it (:142-221).  The rate is recorded by NAME: the reference's enum has 7/8 between 5/6 and 8/9, the
                engine's has not.  dvb_cgf_holder is not initialised, so g1 is recorded only for 16APSK and 32APSK and g2 only
                for 32APSK (float bit patterns), null elsewhere.  The reference has no short-frame 9/10 rule: it returns a
                configuration for those four MODCODs, which is recorded as it is.
  pls_codewords s2_plscodes::codewords (s2_defs.h:32-80), and sof = s2_sof::VALUE / MASK / LENGTH (:15-19)
  gold0         S2Scrambling(0)'s Rn (s2_scrambling.cpp:9-28): SHA-256 of the 131072 entries, the first 64, and the 64 from
                index 33128: the last ones the longest PLFRAME uses (QPSK normal frames with pilots: 32400 + 22 * 36 = 33192
                scrambled symbols; without pilots nothing beyond Rn[32399] is ever read)
  rotations     what scramble / descramble make of (1, 2) for Rn = 0..3 (:37-81): [scrambled re, im, descrambled re, im] per r
  deinterleave  S2Deinterleaver (s2_deinterleaver.cpp:72-136) on the index ramp of make_golden.py for every (MODCOD, frame size)

Data only.  Run:  python3 tests/golden/make_golden_s2tables.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402

OUT = os.path.join(HERE, 's2_tables_golden.json')


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def f32_hex(x):
    return '%08x' % int(np.float32(x).view(np.uint32))


def ramp(n):
    return (np.arange(n) * 7 % 251).astype(np.int8)


def collect(R):
    """everything the fixture holds, from the compiled reference R"""
    G = {'modcod_cfg': [], 'deinterleave': []}
    for modcod in range(1, 29):
        for short in (0, 1):
            for pilots in (0, 1):
                o, g = np.zeros(4, np.int32), np.zeros(2, np.float32)
                assert R.ref_modcod_cfg(modcod, short, pilots, o, g) == 0
                assert 0 <= o[1] <= 3 and 0 <= o[2] <= 10 and o[3] == short, (modcod, short, pilots, o)
                G['modcod_cfg'].append(dict(modcod=modcod, short=short, pilots=pilots, slots=int(o[0]), constel=int(o[1]), rate=orc.RATE_NAMES[o[2]],
                                            g1=f32_hex(g[0]) if o[1] >= 2 else None, g2=f32_hex(g[1]) if o[1] == 3 else None,
                                            modcod_back=int(R.ref_modcod_roundtrip(modcod, short, pilots))))
            if short and orc.RATE_NAMES[o[2]] == '9/10':     # no such FECFRAME (EN 302 307-1 table 5b)
                continue
            n = 16200 if short else 64800
            dst = np.zeros(n, np.int8)
            R.ref_deinterleave(int(o[1]), int(o[2]), short, ramp(n), dst)
            G['deinterleave'].append(dict(modcod=modcod, constel=int(o[1]), rate=orc.RATE_NAMES[o[2]], short=short, out_sha=sha(dst)))
    o, g = np.zeros(4, np.int32), np.zeros(2, np.float32)
    G['modcod_rejected'] = [m for m in (-1, 0, 29, 100) if R.ref_modcod_cfg(m, 0, 0, o, g) == -1]
    codes, sof = np.zeros(128, np.uint64), np.zeros(3, np.uint32)
    R.ref_pls_codewords(codes, sof)
    G['pls_codewords'] = ['%016x' % int(c) for c in codes]
    G['sof'] = dict(value='%07x' % int(sof[0]), mask='%07x' % int(sof[1]), length=int(sof[2]))
    rn = np.zeros(131072, np.uint8)
    R.ref_gold_sequence(0, rn)
    assert rn.max() <= 3
    G['gold0'] = dict(sha256=sha(rn), first64=[int(x) for x in rn[:64]], at33128=[int(x) for x in rn[33128:33192]])
    rot = np.zeros(16, np.float32)
    assert R.ref_scramble_cases(rn, rot) == 0
    G['rotations'] = [[float(x) for x in rot[4 * r:4 * r + 4]] for r in range(4)]
    return G


def main():
    R = orc.ref()
    assert R is not None and hasattr(R, 'ref_modcod_cfg'), 'oracle/_ref/libdvbs2ref.so missing or old: run `make -C oracle ref` where the reference tree exists'
    G = collect(R)
    with open(OUT, 'w') as f:
        json.dump(G, f, indent=0)
        f.write('\n')
    print('wrote', len(G['modcod_cfg']), 'configurations,', len(G['pls_codewords']), 'codewords,', len(G['deinterleave']), 'de-interleaver cases')


if __name__ == '__main__':
    main()
