"""Constructed cases of the PCR bank (include/dvbs2gpu.h, PCR bank), shared by the CPU tests, the GPU tests and the sanitizer run:
each is a short stream on PID `PID` in which one rule decides, with what the rule must give written out as numbers."""
import numpy as np

import pcr_ref as P

PID, OTHER = 0x120, 0x121
TPP = 1000                      # ticks per packet of the anchors: 40.608 Mbit/s
TPP_Q24 = TPP << 24
GAP = 30                        # packets between the anchors' PCR packets
M = P.MOD


def spaced(values, gap=GAP, pid=PID, rng=None, **kw):
    """PCR packets of `pid` with these values `gap` packets apart (the first at packet 0), null packets between -> [n, 188]"""
    parts = []
    for j, v in enumerate(values):
        parts += [P.pcr_packet(pid, v, cc=j, **kw).reshape(1, -1), P.null_packets(gap - 1)]
    return np.concatenate(parts)


def pairs(values, gap=GAP):
    """the (kind, flags, delta_ticks, delta_packets, accuracy) that a fresh slot at TPP must give for spaced(values)"""
    m = P.Clock()
    m.set_watch(0, PID)
    m.set_rate(TPP_Q24)
    m.process(spaced(values, gap))
    return [(r['kind'], r['flags'], r['delta_ticks'], r['delta_packets'], r['accuracy']) for r in m.table]


A, S = P.ACCURACY_ERROR, P.SATURATED
# name, PCR values 30 packets apart, the rows behind the first (kind, flags, delta_ticks, delta_packets, accuracy): literal anchors
ANCHORS = [
    ('on the rate', [5000, 35000], [(P.OK, 0, 30000, 30, 0)]),
    ('13 ticks fast', [5000, 35013], [(P.OK, 0, 30013, 30, 832)]),
    ('14 ticks fast', [5000, 35014], [(P.OK, A, 30014, 30, 896)]),
    ('14 ticks slow', [5000, 34986], [(P.OK, A, 29986, 30, -896)]),
    ('wrap of the 33-bit base', [M - 10000, 20000], [(P.OK, 0, 30000, 30, 0)]),
    ('40 ms', [0, 1080000], [(P.OK, A, 1080000, 30, (1050000 << 24) >> 18)]),
    ('40 ms and a tick', [0, 1080001], [(P.LATE, A, 1080001, 30, (1050001 << 24) >> 18)]),
    ('100 ms', [0, 2700000], [(P.LATE, A, 2700000, 30, (2670000 << 24) >> 18)]),
    ('100 ms and a tick', [0, 2700001], [(P.JUMP, 0, 2700001, 30, 0)]),
    ('one tick back', [777777, 777776], [(P.JUMP, 0, 0xFFFFFFFF, 30, 0)]),
    ('three equal values, then a pair', [1000, 1000, 1000, 91000], [(P.REPEATED, 0, 0, 0, 0), (P.REPEATED, 0, 0, 0, 0), (P.OK, 0, 90000, 90, 0)]),
]


def edge_cases():
    """-> [(name, packets [n, 188])]: every case runs on a bank that watches PID in slot 0 at rate TPP_Q24, one after the other"""
    rng = np.random.default_rng(7)
    cases = [(name, spaced(values)) for name, values, _ in ANCHORS]
    eq = spaced([50000, 50000])
    eq[GAP, 5] |= 0x80                                                   # DI with an equal value: ANNOUNCED, not REPEATED
    cases.append(('DI with an equal value', eq))
    good = lambda v, **kw: P.pcr_packet(PID, v, **kw).reshape(1, -1)
    fill = P.null_packets(GAP - 1)
    scrambled = good(1030000).copy()
    scrambled[0, 3] |= 0x80
    cases += [
        ('length 6', np.concatenate([good(100000), fill, good(130000, af_len=6), fill, good(160000)])),
        ('length 184', np.concatenate([good(200000), fill, good(230000, af_len=184, afc=2), fill, good(260000)])),
        ('length 183 with payload', np.concatenate([good(300000), fill, good(330000, af_len=183, afc=3), fill, good(360000)])),
        ('extension 300', np.concatenate([good(400000), fill, good(430000, ext=300), fill, good(460000)])),
        ('TEI and bad sync look like a PCR', np.concatenate([good(500000), fill, good(530000, tei=1), good(530000, sync=0x48), fill[:-1], good(560000)])),
        ('AFC 1 with b5 0x10 is payload', np.concatenate([good(600000), fill, good(630000, afc=1), fill, good(660000)])),
        ('AFC 2 with length 183', np.concatenate([good(700000), fill, good(730000, af_len=183, afc=2), fill, good(760000)])),
        ('length 0', np.concatenate([good(800000), fill, good(830000, af_len=0), fill, good(860000)])),
        ('flag clear', np.concatenate([good(900000), fill, good(930000, flag=0), fill, good(960000)])),
        ('scrambled and an unwatched PCR PID', np.concatenate([good(1000000), fill, P.pcr_packet(OTHER, 5).reshape(1, -1), fill, scrambled, P.payload_packets(0x300, 5, rng)])),
    ]
    return cases


# what the three packets of the middle cases give: rows of packets 0, 30 and 60 unless the middle one is no record
MIDDLE = {'length 6': ('malformed', 2), 'length 184': ('malformed', 2), 'length 183 with payload': ('malformed', 2), 'extension 300': ('malformed', 2),
          'TEI and bad sync look like a PCR': (None, 2), 'AFC 1 with b5 0x10 is payload': (None, 2), 'AFC 2 with length 183': (None, 3), 'length 0': (None, 2),
          'flag clear': (None, 2), 'scrambled and an unwatched PCR PID': (None, 2)}


def whole_stream():
    return np.concatenate([ts for _, ts in edge_cases()])


def saturation_calls(max_packets=4096, tpp=80):
    """calls of null packets with three PCR packets at positions 0, 32767 and 32767 + 32768, stamped position * tpp: the first pair has
    dN = 32767, the second 32768 -> ([calls], the literal rows of the second and third PCR)"""
    calls = [P.null_packets(max_packets) for _ in range(16)]
    for c, k, n in ((0, 0, 0), (7, max_packets - 1, 32767), (15, max_packets - 1, 65535)):
        calls[c][k] = P.pcr_packet(PID, n * tpp)
    assert P.LATE_TICKS < 32767 * tpp and 32768 * tpp <= P.JUMP_TICKS            # LATE pairs: measured (the rate is tpp << 24)
    want = [dict(pid=PID, slot=0, kind=P.LATE, flags=0, packet=max_packets - 1, pcr=32767 * tpp, delta_ticks=32767 * tpp, delta_packets=32767, accuracy=0),
            dict(pid=PID, slot=0, kind=P.LATE, flags=A | S, packet=max_packets - 1, pcr=65535 * tpp, delta_ticks=32768 * tpp, delta_packets=32768, accuracy=tpp << 6)]
    return calls, want


def same(bank, model, stream=0):
    """a bank (device or host) and the model agree on everything the last call of `stream` left"""
    assert bank.row_table(stream) == model.table, stream
    for slot in range(-1, 16):
        assert bank.stats(stream, slot) == model.stats(slot), (stream, slot)
        assert bank.rate(stream, slot) == model.rate(slot), (stream, slot)
    assert bank.stream_stats(stream) == model.stream_stats(), stream
