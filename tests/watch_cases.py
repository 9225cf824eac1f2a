"""What the tests of the three watched-PID banks side by side (csrc/watch_bank.h: PCR, PES, ES) share: one multiplex that gives each
bank two active slots, the banks with their models, and the comparison."""
import numpy as np

import es_cases as KE
import es_ref as E
import pcr_cases as KC
import pcr_ref as C
import pes_cases as KP
import pes_ref as P

PCR_PIDS = (0x122, 0x123)
VIDEO = ((0x150, E.MPEG2), (0x151, E.H264))
TPP = 1000
# the words of the statistics that get_stats(slot -1) takes as maxima over the slots; every other word is a sum
MAXIMA = {'pcr': ('max_delta_ticks', 'max_abs_accuracy'), 'pes': ('max_delta_packets',), 'es': ()}
SAME = {'pcr': KC.same, 'pes': KP.same, 'es': KE.same}


def interleaved(rng, n):
    """n packets: PCR packets of the two PCR_PIDS every 5 to 12 packets, stamped position * TPP with a jitter, and between them the
    faulty PES multiplex of es_cases on the two VIDEO PIDs -> [n, 188]"""
    out = C.stamped_mux(rng, n, PCR_PIDS, tpp=TPP, gap=(5, 12), jitter=5)
    video = KE.random_mux(rng, n, list(VIDEO))
    j = 0
    for k in range(n):
        if ((int(out[k, 1]) & 0x1F) << 8 | int(out[k, 2])) == 0x300:
            out[k] = video[j]
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
    else:
        bank.set_watch(*at, 0, *VIDEO[0]), bank.set_watch(*at, 7, *VIDEO[1])


SLOTS = {'pcr': (3, 5), 'pes': (1, 2), 'es': (0, 7)}


def model(name, max_rows):
    m = {'pcr': C.Clock, 'pes': P.Pes, 'es': E.Es}[name](max_rows)
    watch(name, m)
    return m


def snapshot(bank, stream=0):
    """everything the bank's statistics calls say of a stream"""
    return [bank.stats(stream, slot) for slot in range(-1, 16)], bank.stream_stats(stream)
