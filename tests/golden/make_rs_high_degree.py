#!/usr/bin/env python3
"""Searches for RS(204,188) packets that the reference's decoder DECODES with an error locator of degree 9 .. 16, and writes up to eight of
them to tests/golden/rs_high_degree.json.

Berlekamp-Massey as libcorrect writes it (reed-solomon/decode.c:31-121) ends with a locator of degree <= 8 for almost every input: degree 9
needs a zero discrepancy at step 14 and a non-zero one at step 15 (about one packet in 256), and the decoder then succeeds only if that locator has
as many distinct roots as its degree (about one polynomial of degree 9 in 9!).  The oracle (oracle/capi.cpp, orc_rs255_locator) tells the
locator order and the root count.  Two searches, MAX_TRIALS each at the most:

  random    packets with 9 .. 12 random byte errors (on the all-zero codeword: the decoder's path depends on the error pattern alone)
  directed  7 random byte errors, plus delta times the word w on the 16 parity bytes whose syndromes are (0, .., 0, 1) (w solves the 16 x 16
            Vandermonde system): S_0 .. S_14 are those of 7 errors, S_15 is off by delta, so EVERY trial ends with a locator of degree 9, and
            only the 9 distinct roots are left to chance

Hits are re-run on a random codeword through the reference's wrapper (oracle/_ref, recipe: oracle/Makefile target `ref`) for the recorded outcome.

RESULT of the run for this commit (seed 90 000):
  random    5 000 000 trials: 98 packets decoded, none of them with a locator of degree >= 9 (19 471 locators of degree 9, none above, none with 9 roots)
  directed  4 117 450 trials until the eighth packet that decoded; every locator of degree 9.  The eight are the fixture: 22 or 23 byte errors each,
            the wrapper returns 6 .. 9 (nine changed message bytes: more than the code corrects), six of them with roots in the zero padding

Run:  python3 tests/golden/make_rs_high_degree.py [max_trials]
"""
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import orc  # noqa: E402
import orc_dvbs_tail as ot  # noqa: E402
import rs_patterns as rp  # noqa: E402
from orc_dvbs import P, VP  # noqa: E402

MAX_TRIALS = 5000000
BATCH = 20000
KEEP = 8
SEED = 90000


def random_batch(rng, n):
    pos = np.argpartition(rng.random((n, 204)), 12, axis=1)[:, :12]             # 12 distinct positions per packet
    ne = rng.integers(9, 13, n)
    val = rng.integers(1, 256, (n, 12), dtype=np.uint8) * (np.arange(12)[None, :] < ne[:, None])
    pk = np.zeros((n, 204), np.uint8)
    np.put_along_axis(pk, pos, val.astype(np.uint8), axis=1)
    return pk


def directed_batch(rng, n, w_log):
    pos = np.argpartition(rng.random((n, 204)), 7, axis=1)[:, :7]
    pk = np.zeros((n, 204), np.uint8)
    np.put_along_axis(pk, pos, rng.integers(1, 256, (n, 7), dtype=np.uint8), axis=1)
    delta_log = rng.integers(0, 255, n)
    # coefficient index i = packet[203 - i]: delta * w[i] on the parity bytes
    pk[:, 203 - np.arange(16)] ^= ot._EXP[(delta_log[:, None] + w_log[None, :]) % 255].astype(np.uint8)
    return pk


def search(o, name, batch, max_trials):
    msg, loc2 = np.zeros(239, np.uint8), np.zeros(2, np.int32)
    pmsg, ploc = P(msg), P(loc2)
    hits, orders, decoded, trials, t0 = [], {}, 0, 0, time.time()
    while trials < max_trials and len(hits) < KEEP:
        n = min(BATCH, max_trials - trials)
        enc = rp.padded(batch(n))
        base = enc.ctypes.data
        for k in range(n):
            ret = o.orc_rs255_locator(VP(base + 255 * k), pmsg, ploc)
            trials += 1
            if loc2[0] >= 9:
                orders[int(loc2[0])] = orders.get(int(loc2[0]), 0) + 1
            if ret == 239:
                decoded += 1
                if loc2[0] >= 9:
                    hits.append((enc[k, 51:].copy(), int(loc2[0])))
                    if len(hits) == KEEP:
                        break
    print('%s: %d trials, %d decoded (any locator degree), %d decoded with degree >= 9; locator orders >= 9 met, decoded or not: %s; %.0f s' %
          (name, trials, decoded, len(hits), sorted(orders.items()), time.time() - t0), flush=True)
    return hits, trials


def main():
    max_trials = int(sys.argv[1]) if len(sys.argv) > 1 else MAX_TRIALS
    o = ot.L()
    rng = np.random.default_rng(SEED)
    hits, trials = search(o, 'random', lambda n: random_batch(rng, n), max_trials)
    how = 'random'
    if not hits:
        w = rp.null_vector([row + [int(r == 15)] for r, row in enumerate(rp.vandermonde(range(16), 16))])[:16]
        assert all(w) and rp.syndromes(rp.apply_errors(np.zeros(204, np.uint8), dict(enumerate(w)))) == [0] * 15 + [1]
        w_log = np.array([ot._LOG[x] for x in w])
        hits, trials = search(o, 'directed', lambda n: directed_batch(rng, n, w_log), max_trials)
        how = 'directed'
    if not hits:
        return
    R = orc.ref()
    assert R is not None and hasattr(R, 'ref_dvbsrs_create'), 'oracle/_ref/libdvbs2ref.so missing or stale: make -C oracle ref'
    R.ref_dvbsrs_create.restype = VP
    R.ref_dvbsrs_decode.argtypes = [VP, VP]
    cases = []
    for err, order in hits:
        cw = ot.rs_encode_204(rng.integers(0, 256, 188, dtype=np.uint8))
        pkt = cw ^ err
        data = pkt.copy()
        ret = R.ref_dvbsrs_decode(VP(R.ref_dvbsrs_create()), P(data))                # a fresh wrapper each
        cases.append({'order': order, 'packet': pkt.tobytes().hex(), 'sent': cw.tobytes().hex(), 'ret': int(ret), 'message': data[:188].tobytes().hex()})
    with open(os.path.join(HERE, 'rs_high_degree.json'), 'w') as f:
        json.dump({'seed': SEED, 'search': how, 'trials': trials, 'cases': cases}, f, indent=1)
    print('wrote rs_high_degree.json with %d packets' % len(cases))


if __name__ == '__main__':
    main()
