"""Constructed cases of the IP output bank's tests.  A case is (name, flows, segments): flows {slot: keyword arguments of set_flow}, and
segments [(rate or None: as it was, packets, flush)], each one call -- or cut into calls of a few packets, the flush flag on the last
of them.  run() feeds a case to anything with the bank's surface."""
import numpy as np

import ipout_ref as R

TS = 188
V4_SRC, V4_DST = bytes([10, 1, 2, 3]), bytes([239, 7, 7, 7])
V6_SRC, V6_DST = bytes.fromhex('20010db80000000000000000000000aa'), bytes.fromhex('ff3e00000000000000000000000043 21'.replace(' ', ''))
RATE = 1000 << 24                      # 27 MHz ticks per packet at 40.608 Mbit/s: 10 / 3 ticks of 90 kHz


def flow(family=4, mode=R.RTP_MODE, P=7, port=5004, **kw):
    f = dict(family=family, src=V4_SRC if family == 4 else V6_SRC, dst=V4_DST if family == 4 else V6_DST, src_port=40000 + port % 1000, dst_port=port,
             ttl=17, dscp=46, mode=mode, ssrc=0xC0FFEE00 | port & 255, seq_base=100, timestamp_base=5000, packets_per_datagram=P)
    f.update(kw)
    return f


def packets(pids, seed=0, bad=()):
    """one packet per entry of pids with seeded payload and a running counter; bad: the indices whose sync byte is wrong -> uint8"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (len(pids), TS), dtype=np.uint8)
    for k, pid in enumerate(pids):
        p[k, :4] = [0x47 if k not in bad else 0x48, rng.integers(0, 8) << 5 | pid >> 8, pid & 255, 0x10 | k & 15]
    return p.reshape(-1)


def zero_checksum_case():
    """slot 0, RTP over IPv4, P = 1: bytes 4 and 5 of the only packet tuned so that the UDP checksum comes out 0x0000"""
    f = flow(P=1, port=5020)
    ts = packets([0x31], seed=77)
    ts[4:6] = 0
    _, c = R.build(dict(R.FLOW_DEFAULTS, **f), [bytes(ts)], f['seq_base'], f['timestamp_base'])
    word = 0xFFFF ^ c                  # the ones'-complement sum of everything else; the word that completes it to 0xFFFF:
    w = 0xFFFF - word
    ts[4], ts[5] = w >> 8, w & 255
    return ('zero_checksum', {0: f}, [(RATE, ts, False)])


def cases():
    out = []
    # P = 1..7, both families, both modes; 0, 1, P - 1, P, P + 1 passing packets, then a flush with P - 1 held and one with nothing held
    for P in range(1, 8):
        family, mode = (4, 6)[P & 1], (R.RAW, R.RTP_MODE)[P >> 1 & 1]
        f = {P % 4: flow(family, mode, P, port=5000 + P, pid_mode=1, pids=(0x100,))}
        segs = []
        for i, n in enumerate((0, 1, P - 1, P, P + 1)):
            pids = [0x100] * n + [0x200] * 2
            segs.append((RATE if i == 0 else None, packets(pids[::-1] if i & 1 else pids, seed=10 * P + i), False))
        held = (1 + P - 1 + P + P + 1) % P
        segs.append((None, packets([0x100] * ((P - 1 - held) % P), seed=9), False))      # now P - 1 are held (none at P = 1)
        segs.append((None, packets([0x200], seed=8), True))
        segs.append((None, packets([], seed=7), True))                                    # nothing held
        out.append(('P%d_family%d_mode%d' % (P, family, mode), f, segs))
    for family in (4, 6):
        for mode in (R.RAW, R.RTP_MODE):
            out.append(('family%d_mode%d' % (family, mode), {1: flow(family, mode, 3, port=5100)},
                        [(RATE, packets([0x40, 0x41, 0x42, 0x1FFF, 0x40, 0x41, 0x42, 0x40], seed=family + mode), True)]))
    # one packet (PID 0x50) enters all four slots; drop_null; pass listed / drop listed; a bad sync byte between good packets
    four = {0: flow(4, R.RTP_MODE, 2, port=5200), 1: flow(6, R.RAW, 3, port=5201, pid_mode=1, pids=(0x50, 0x51)),
            2: flow(4, R.RAW, 1, port=5202, pid_mode=2, pids=(0x51, 0x1FFF)), 3: flow(6, R.RTP_MODE, 7, port=5203, drop_null=True)}
    pids = [0x50, 0x51, 0x1FFF, 0x52, 0x50, 0x50, 0x1FFF, 0x51, 0x52, 0x50, 0x53, 0x50, 0x51, 0x50, 0x1FFF, 0x50, 0x52]
    out.append(('four_slots', four, [(RATE, packets(pids, seed=3, bad=(3, 9)), False), (None, packets(pids[::-1], seed=4, bad=(0,)), True)]))
    # seq passes 65535 -> 0; the timestamp passes 2^32; a rate change between calls
    wrap = {2: flow(4, R.RTP_MODE, 2, port=5300, seq_base=65533, timestamp_base=2 ** 32 - 20)}
    out.append(('wraps_and_rate_change', wrap, [(RATE, packets([0x60] * 9, seed=5), False), (3 * RATE + 12345, packets([0x60] * 9, seed=6), False),
                                                (0, packets([0x60] * 4, seed=7), True)]))
    out.append(zero_checksum_case())
    return out


def set_flows(bank, case, stream=None):
    """the case's flows into a model (stream None) or into stream `stream` of a bank"""
    for slot, f in case[1].items():
        bank.set_flow(*(() if stream is None else (stream,)), slot, **f)


def calls(case, cut=None):
    """the case's calls -> [(rate to set before it or None, packets, flush)]; cut: at most that many packets per call"""
    out = []
    for rate, ts, flush in case[2]:
        step = cut * TS if cut else max(ts.size, 1)
        pieces = [ts[i:i + step] for i in range(0, ts.size, step)] or [ts]
        out += [(rate if i == 0 else None, p, flush and i == len(pieces) - 1) for i, p in enumerate(pieces)]
    return out


def selected(case, slot):
    """the packets of the whole case that the slot's flow takes, by a rule of its own -> bytes"""
    f = dict(R.FLOW_DEFAULTS, **case[1][slot])
    keep = b''
    for _, ts, _ in case[2]:
        for p in ts.reshape(-1, TS):
            pid = (int(p[1]) & 31) * 256 + int(p[2])
            listed = pid in f['pids']
            if p[0] == 0x47 and not (f['drop_null'] and pid == 8191) and (f['pid_mode'] == 0 or listed == (f['pid_mode'] == 1)):
                keep += p.tobytes()
    return keep
