#!/usr/bin/env python3
"""Generates tests/golden/bbts_golden.json: known-answer cases for the BBFRAME -> TS / GSE parser whose expected outputs come from
the REFERENCE's own dvbs2/bbframe_ts_parser.cpp, compiled in place over the stand-in headers of oracle/shim into
oracle/_ref/libdvbs2ref.so (recipe: oracle/Makefile target `ref`).  The inputs come from this repo's transmitter side
(tests/orc_bbts.py, per EN 302 307-1 5.1.4-5.1.6 and TS 102 606) and are regenerated from seeds; digests and small integer lists only.

  ts_round_trip   clean TS round trips (the output is also the transmitted packet sequence)
  fuzz            the three fuzzed configurations in the layout earlier readers use.  `synched` in state_per_call is private in
                  the reference and taken from the restatement; the first `reference_calls` calls are reference outputs, the calls
                  from the first one with undefined behaviour in the reference on are the restatement's (regression anchors)
  ts_fuzz, gse    per call {sha256_in, undefined, n, sha256_out, fields}: return value, digest of the bytes written and the public
                  fields (orc_bbts.FIELD_KEYS) as the reference left them.  A call in which the reference's behaviour is undefined
                  (orc_bbts.walk_case) has `undefined` set and no outputs; readers start a fresh parser after it.

Run:  python3 tests/golden/make_golden_bbts.py
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc_bbts as B  # noqa: E402


def sha(a):
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()


def per_call(case):
    name, kbch, calls = case
    out = []
    for fr, rec in zip(calls, B.walk_case(name, kbch, calls)):
        c = {'sha256_in': sha(fr), 'frames': int(len(fr)), 'undefined': bool(rec['ub'])}
        if not rec['ub']:
            n, buf, fields = rec['ref']
            assert not rec['left_output']
            c.update({'n': int(n), 'sha256_out': sha(buf[:n]), 'fields': [fields[k] for k in B.FIELD_KEYS]})
        out.append(c)
    return {'name': name, 'kbch': kbch, 'calls': out}


def main():
    assert B.R() is not None, 'oracle/_ref/libdvbs2ref.so missing or stale: make -C oracle ref'
    G = {'ts_round_trip': [], 'fuzz': []}
    for kbch, dfl in B.TS_ROUND_TRIPS:
        fr, want = B.ts_round_trip_frames(kbch, dfl)
        p = B.RefBbTs(kbch)
        outs = []
        for part in (fr[:4], fr[4:]):
            n, buf = p.work_raw(part, B.call_cap(part))
            outs.append(buf[:n])
        out = np.concatenate(outs)
        assert np.array_equal(out.reshape(-1, 188), want)
        G['ts_round_trip'].append({'kbch': kbch, 'dfl_bytes': dfl, 'seed': kbch + (dfl or 0), 'nframes': len(fr), 'packets_out': len(want),
                                   'sha256_out': sha(out), 'sha256_in': sha(fr)})
    for seed, kbch, choices in B.TS_FUZZ:
        rng = np.random.default_rng(seed)
        p, r = B.OracleBbTs(kbch), B.RefBbTs(kbch)
        outs, stats, ref_calls, defined = [], [], 0, True
        for call in range(6):
            fr = B.fuzz_frames(rng, kbch, int(rng.integers(0, 6)), ts_gs_choices=choices, p_bad=0.2)
            o = p.work(fr, cap=B.call_cap(fr))
            st = p.stats()
            n, buf = r.work_raw(fr, B.call_cap(fr))
            defined = defined and not p.undefined()
            if defined:
                f = r.fields()
                assert n == o.size and np.array_equal(buf[:n], o) and all(f[k] == st[k] for k in B.FIELD_KEYS)
                ref_calls += 1
            outs.append(sha(o))
            stats.append([st['synched'], st['last_bb_proc'], st['last_gse_crc_err'], st['ts_gs'], int(o.size)])
        G['fuzz'].append({'seed': seed, 'kbch': kbch, 'ts_gs_choices': list(choices), 'calls': 6, 'reference_calls': ref_calls,
                          'sha256_out_per_call': outs, 'state_per_call': stats})
    G['ts_fuzz'] = [per_call(c) for c in B.ts_fuzz_cases()]
    G['gse'] = [per_call(c) for c in B.gse_structured_cases() + B.gse_fuzz_cases()]
    with open(os.path.join(HERE, 'bbts_golden.json'), 'w') as f:
        json.dump(G, f, indent=1)
    print('wrote bbts_golden.json')


if __name__ == '__main__':
    main()
