"""What the tests of the four watched-PID banks side by side (csrc/watch_bank.h: PCR, PES, ES, audio) share: one multiplex that gives
each bank two active slots, the banks with their models, and the comparison; and what the ES and the audio bank, which share their
kernels' front and their host streams' packet walk (csrc/es_stream.h, es_rules.h), must agree on when they watch the same PIDs."""
import numpy as np

import aud_cases as KA
import aud_ref as A
import es_cases as KE
import es_ref as E
import pcr_cases as KC
import pcr_ref as C
import pes_cases as KP
import pes_ref as P

PCR_PIDS = (0x122, 0x123)
VIDEO = ((0x150, E.MPEG2), (0x151, E.H264))
AUDIO = ((0x160, A.MPA), (0x161, A.ADTS))
TPP = 1000
# the words of the statistics that get_stats(slot -1) takes as maxima over the slots; every other word is a sum
MAXIMA = {'pcr': ('max_delta_ticks', 'max_abs_accuracy'), 'pes': ('max_delta_packets',), 'es': (), 'aud': ()}
SAME = {'pcr': KC.same, 'pes': KP.same, 'es': KE.same, 'aud': KA.same}


def interleaved(rng, n):
    """n packets: PCR packets of the two PCR_PIDS every 5 to 12 packets, stamped position * TPP with a jitter, and between them the
    faulty PES multiplex of es_cases on the two VIDEO PIDs; where that one has filler (PID 0x300, null packets) the faulty multiplex of
    aud_cases on the two AUDIO PIDs -> [n, 188]"""
    out = C.stamped_mux(rng, n, PCR_PIDS, tpp=TPP, gap=(5, 12), jitter=5)
    for mux, filler in ((KE.random_mux(rng, n, list(VIDEO)), (0x300,)), (KA.random_mux(rng, n, list(AUDIO)), (0x300, 0x1FFF))):
        j = 0
        for k in range(n):
            if ((int(out[k, 1]) & 0x1F) << 8 | int(out[k, 2])) in filler:
                out[k] = mux[j]
                j += 1
    return out


def watch(name, bank, stream=None):
    """the bank's (or, stream None, a model's) watches on the multiplex above: two slots each, not the first two"""
    at = () if stream is None else (stream,)
    if name == 'pcr':
        bank.set_watch(*at, 3, PCR_PIDS[0]), bank.set_watch(*at, 5, PCR_PIDS[1])
        bank.set_rate(*at, TPP << 24)
    elif name == 'pes':
        bank.set_watch(*at, 1, VIDEO[0][0]), bank.set_watch(*at, 2, VIDEO[1][0])
        bank.set_rate(*at, TPP << 24)
    elif name == 'es':
        bank.set_watch(*at, 0, *VIDEO[0]), bank.set_watch(*at, 7, *VIDEO[1])
    else:
        bank.set_watch(*at, 4, *AUDIO[0]), bank.set_watch(*at, 9, *AUDIO[1])


SLOTS = {'pcr': (3, 5), 'pes': (1, 2), 'es': (0, 7), 'aud': (4, 9)}


def model(name, max_rows):
    m = {'pcr': C.Clock, 'pes': P.Pes, 'es': E.Es, 'aud': A.Aud}[name](max_rows)
    watch(name, m)
    return m


def snapshot(bank, stream=0):
    """everything the bank's statistics calls say of a stream"""
    return [bank.stats(stream, slot) for slot in range(-1, 16)], bank.stream_stats(stream)


# ---------------------------------------------------------------------------------------- the ES and the audio bank on the same PIDs
# the twelve counters both banks' statistics begin with
COMMON_COUNTERS = ('packets', 'payload_bytes', 'es_bytes', 'bytes_unsynced', 'duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'resets',
                   'pes_starts', 'pes_invalid', 'split_headers')
PES_ROW_KEYS = ('pid', 'slot', 'code', 'detail', 'packet', 'head', 'es_offset', 'pts', 'dts')
RESYNC = 2                                      # a code row and a frame row clear the lost bit at different places


def stream_feeds():
    """name -> (packets, the PIDs to watch): the audio multiplex, and 2600 packets of the ES multiplex"""
    return {'aud': (KA.mux(), [pid for _, pid, _ in KA.WATCHES]), 'es': (KE.gpu_mux()[:2600], list(KE.PIDS.values()))}


def watch_same_pids(es, aud, pids, stream=None):
    """slot i of both banks (or, stream None, models) watches pids[i], as H264 and as ADTS"""
    at = () if stream is None else (stream,)
    for slot, pid in enumerate(pids):
        es.set_watch(*at, slot, pid, E.H264), aud.set_watch(*at, slot, pid, A.ADTS)


def same_stream_front(es, aud, stream=0):
    """the two banks agree on what their shared front decides: the common counters since reset, slot by slot, and the PES rows of the
    last call but for RESYNC -> the PES rows"""
    for slot in range(-1, 16):
        a, b = es.stats(stream, slot), aud.stats(stream, slot)
        assert {k: a[k] for k in COMMON_COUNTERS} == {k: b[k] for k in COMMON_COUNTERS}, (stream, slot)
    ra, rb = ([r for r in bank.rows(stream) if r['unit'] == 0] for bank in (es, aud))
    assert len(ra) == len(rb), (stream, len(ra), len(rb))
    for x, y in zip(ra, rb):
        assert {k: x[k] for k in PES_ROW_KEYS} == {k: y[k] for k in PES_ROW_KEYS} and x['flags'] & ~RESYNC == y['flags'] & ~RESYNC, (stream, x, y)
    return len(ra)
