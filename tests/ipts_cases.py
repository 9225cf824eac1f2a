"""Constructed datagrams for the IP-TS bank with the row each must give written out -- (flags, slot, TS packets, lost) -- at least one
per flag and every edge the header comment names, and the seeded random tables of the CPU and GPU tests.  The counters that a table
must leave are derived here from the written rows alone, not from the model."""
import itertools

import numpy as np

import ipts_ref as R

# the flows of every test stream: slots 0 and 2 match the same datagrams (the lowest wins), slot 1 is IPv6, slot 3 another port
PORT, PORT3 = 1234, 5678
FLOWS = [(4, R.V4_DST, PORT), (6, R.V6_DST, PORT), (4, R.V4_DST, PORT), (4, R.V4_DST, PORT3)]
F = {n: getattr(R, n if n != 'TS' else 'TS_ROW') for n in R.FLAG_NAMES}


def flags(names):
    return sum(F[n] for n in names.split())


def set_flows(bank_or_model, stream=None):
    for k, (fam, addr, port) in enumerate(FLOWS):
        if stream is None:
            bank_or_model.set_flow(k, fam, addr, port)
        else:
            bank_or_model.set_flow(stream, k, fam, addr, port)


def flip(d, at=-1):
    """d with one bit turned over"""
    d = bytearray(d)
    d[at] ^= 1
    return bytes(d)


def computed_zero(seq):
    """an RTP datagram whose UDP checksum comes out 0 and is therefore sent as 0xFFFF: the low half of the timestamp makes up for the rest"""
    probe = R.udp(R.rtp(R.ts_packets(2, seed=5), seq=seq, timestamp=0x12340000), checksum=0)
    pseudo = R.V4_SRC + R.V4_DST + bytes([0, 17]) + len(probe).to_bytes(2, 'big')
    fix = 0xFFFF ^ R.ones_sum(pseudo + probe)
    d = R.datagram(R.rtp(R.ts_packets(2, seed=5), seq=seq, timestamp=0x12340000 | fix))
    assert d[20 + 6:20 + 8] == b'\xff\xff'
    return d


def two_folds():
    """a datagram whose unfolded 32-bit sum, folded once, still exceeds 16 bits.  (A right checksum never does that while the sum's
    high half is small: low + high is then a multiple of 65535 below 2 x 65535.  So the checksum is a wrong one, chosen for the carry.)"""
    for v in range(0xFFFF, 0, -1):
        u = R.udp(R.rtp(R.ts_packets(7, seed=8), seq=1), checksum=v)
        s = R.word_sum(R.V4_SRC + R.V4_DST + bytes([0, 17]) + len(u).to_bytes(2, 'big') + u)
        if (s & 0xFFFF) + (s >> 16) > 0xFFFF:
            return R.ipv4(u)
    raise AssertionError('no value found')


def cases():
    """[(name, datagram or None, flag names, slot, packets, lost)] of kind RAW_IP, in the order of one table"""
    seq = itertools.count(100)                                     # the RTP rows of slot 0 in sequence, one SSRC
    seq6 = itertools.count(40000)
    t = lambda n, seed=1: R.ts_packets(n, seed=seed)
    ok = lambda n=7, **kw: R.rtp(t(n), seq=next(seq), **kw)
    broken = bytearray(t(3))
    broken[2 * 188] = 0x46                                         # the third sync byte
    out = [
        ('not delivered', None, 'NOT_DELIVERED', -1, 0, 0),
        ('version nibble 5', b'\x55' + bytes(40), 'NOT_IP', -1, 0, 0),
        ('no byte at all', b'', 'NOT_IP', -1, 0, 0),
        ('IPv4 header checksum wrong', R.ipv4(R.udp(R.rtp(t(7))), checksum=0x1234), 'BAD_IP', -1, 0, 0),
        ('IPv4 total_length beyond the row', R.ipv4(R.udp(b'x' * 20), total_length=60), 'BAD_IP', -1, 0, 0),
        ('IPv4 shorter than a header', R.ipv4(b'')[:19], 'BAD_IP', -1, 0, 0),
        ('IPv6 payload_length beyond the row', R.ipv6(R.udp(b'x' * 20, 6), payload_length=29), 'BAD_IP', -1, 0, 0),
        ('IPv4 MF set', R.ipv4(R.udp(R.rtp(t(1))), frag=0x2000), 'FRAGMENT', -1, 0, 0),
        ('IPv4 fragment offset 16', R.ipv4(R.udp(R.rtp(t(1))), frag=0x0010), 'FRAGMENT', -1, 0, 0),
        ('IPv4 DF set is no fragment', R.ipv4(R.udp(ok(1)), frag=0x4000), 'RTP TS', 0, 1, 0),
        ('IPv4 TCP', R.ipv4(bytes(20), proto=6), 'OTHER_PROTOCOL', -1, 0, 0),
        ('IPv6 TCP', R.ipv6(bytes(20), next_header=6), 'OTHER_PROTOCOL', -1, 0, 0),
        ('IPv6 hop-by-hop header is not followed', R.ipv6(bytes([17, 0, 0, 0, 0, 0, 0, 0]) + R.udp(R.rtp(t(1)), 6), next_header=0), 'OTHER_PROTOCOL', -1, 0, 0),
        ('UDP length 7', R.ipv4(R.udp(b'', length=7)), 'BAD_UDP', -1, 0, 0),
        ('UDP length beyond the IP payload', R.ipv4(R.udp(b'x' * 10, length=19)), 'BAD_UDP', -1, 0, 0),
        ('four bytes of IP payload', R.ipv4(b'\x13\x88\x04\xd2'), 'BAD_UDP', -1, 0, 0),
        ('another port', R.datagram(R.rtp(t(1)), dport=PORT + 1), 'UNWATCHED', -1, 0, 0),
        ('another address', R.datagram(R.rtp(t(1)), dst=bytes([239, 1, 1, 6])), 'UNWATCHED', -1, 0, 0),
        ('IPv6, another port', R.datagram(R.rtp(t(1)), 6, dport=PORT + 1), 'UNWATCHED', -1, 0, 0),
        ('an unwatched flow with a wrong checksum is not summed', R.datagram(R.rtp(t(1)), dport=9, checksum=0x0101), 'UNWATCHED', -1, 0, 0),
        ('IPv4 checksum wrong', R.datagram(R.rtp(t(7)), checksum=0xBEEF), 'BAD_CHECKSUM', 0, 0, 0),
        ('IPv6 checksum wrong by one', flip(R.datagram(R.rtp(t(7)), 6)), 'BAD_CHECKSUM', 1, 0, 0),
        ('IPv4 checksum 0: not computed', R.datagram(ok(), checksum=0), 'NO_CHECKSUM RTP TS', 0, 7, 0),
        ('IPv6 checksum 0', R.datagram(R.rtp(t(7)), 6, checksum=0), 'BAD_CHECKSUM', 1, 0, 0),
        ('a computed 0 sent as 0xFFFF', computed_zero(next(seq)), 'RTP TS', 0, 2, 0),
        ('a sum that needs two folds', two_folds(), 'BAD_CHECKSUM', 0, 0, 0),
        ('IPv4 with IHL 6', R.ipv4(R.udp(ok()), options=b'\x94\x04\x00\x00'), 'RTP TS', 0, 7, 0),
        ('IPv4 with IHL 15', R.ipv4(R.udp(ok()), options=bytes([1] * 40)), 'RTP TS', 0, 7, 0),
        ('IPv6 RTP', R.datagram(R.rtp(t(7), seq=next(seq6)), 6), 'RTP TS', 1, 7, 0),
        ('IPv6 raw', R.datagram(t(2), 6), 'RAW TS', 1, 2, 0),
        ('bytes behind the IP length are ignored', R.datagram(ok(2)) + b'stuffing', 'RTP TS', 0, 2, 0),
        ('RTP padding 3: an odd UDP length', R.datagram(ok(1, pad=3)), 'RTP TS', 0, 1, 0),
        ('RTP padding 1: an odd UDP length', R.datagram(ok(1, pad=1)), 'RTP TS', 0, 1, 0),
        ('RTP with 15 CSRCs', R.datagram(ok(2, cc=15)), 'RTP TS', 0, 2, 0),
        ('RTP extension of length 0', R.datagram(ok(2, ext=0)), 'RTP TS', 0, 2, 0),
        ('RTP extension of length 3', R.datagram(ok(2, ext=3, cc=2)), 'RTP TS', 0, 2, 0),
        ('RTP padding equal to the whole payload', R.datagram(R.rtp(b'', pad=20)), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP padding beyond the payload', R.datagram(R.rtp(b'', pad=3)[:-1] + b'\xc8'), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP padding count 0', R.datagram(R.rtp(t(1), pad=2)[:-1] + b'\x00'), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP CSRCs beyond the payload', R.datagram(R.rtp(b'', cc=15)[:40]), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP extension header beyond the payload', R.datagram(R.rtp(b'', ext=0)[:14]), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP extension words beyond the payload', R.datagram(R.rtp(b'', ext=0)[:14] + b'\x00\x64' + t(1)[:100]), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP version 1', R.datagram(R.rtp(t(1), version=1)), 'BAD_PAYLOAD', 0, 0, 0),
        ('five payload bytes', R.datagram(b'\x80\x21\x00\x00\x00'), 'BAD_PAYLOAD', 0, 0, 0),
        ('UDP length 8: no payload', R.datagram(b''), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP payload type 96', R.datagram(R.rtp(t(7), pt=96)), 'OTHER_PAYLOAD', 0, 0, 0),
        ('RTP payload type 33 with the marker bit', R.datagram(ok(1, marker=1)), 'RTP TS', 0, 1, 0),
        ('RTP payload of 187 bytes', R.datagram(R.rtp(t(1)[:187])), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP header alone', R.datagram(R.rtp(b'')), 'BAD_PAYLOAD', 0, 0, 0),
        ('RTP with the third sync byte wrong', R.datagram(R.rtp(bytes(broken))), 'BAD_PAYLOAD', 0, 0, 0),
        ('raw with the third sync byte wrong: read as RTP, version 1', R.datagram(bytes(broken)), 'BAD_PAYLOAD', 0, 0, 0),
        ('raw, 1 packet', R.datagram(t(1, 2)), 'RAW TS', 0, 1, 0),
        ('raw, 7 packets', R.datagram(t(7, 3)), 'RAW TS', 0, 7, 0),
        ('raw, 66 packets, no checksum', R.datagram(t(66, 4), checksum=0), 'NO_CHECKSUM RAW TS', 0, 66, 0),
        ('RTP, 1 packet', R.datagram(ok(1)), 'RTP TS', 0, 1, 0),
        ('RTP, 66 packets', R.datagram(R.rtp(t(66, 6), seq=next(seq))), 'RTP TS', 0, 66, 0),
    ]
    # the sequence rule on slot 3, its own port: 65534, 65535, 0, then 2 (one lost), 1 and 2 again (late), then another source
    s3 = lambda q, ssrc=0xCAFE0001, n=2: R.datagram(R.rtp(t(n, q & 255), seq=q, ssrc=ssrc, timestamp=90000 + q), dport=PORT3)
    out += [
        ('sequence 65534: nothing stored', s3(65534), 'RTP TS', 3, 2, 0),
        ('sequence 65535', s3(65535), 'RTP TS', 3, 2, 0),
        ('sequence 0: the wrap', s3(0), 'RTP TS', 3, 2, 0),
        ('sequence 2: one lost', s3(2), 'RTP LOSS TS', 3, 2, 1),
        ('sequence 1: late', s3(1), 'RTP LATE', 3, 0, 0),
        ('sequence 2 again: late', s3(2), 'RTP LATE', 3, 0, 0),
        ('a raw datagram between them does not touch the state', R.datagram(t(1, 9), dport=PORT3), 'RAW TS', 3, 1, 0),
        ('sequence 3', s3(3), 'RTP TS', 3, 2, 0),
        ('another SSRC', s3(500, ssrc=0xCAFE0002), 'RTP NEW_SOURCE TS', 3, 2, 0),
        ('its sequence goes on, 400 lost', s3(901, ssrc=0xCAFE0002), 'RTP LOSS TS', 3, 2, 400),
        ('half the number space back: late', s3((901 - 0x8000 + 1) & 0xFFFF, ssrc=0xCAFE0002), 'RTP LATE', 3, 0, 0),
        ('half the number space ahead: 32767 lost', s3((901 + 0x8000) & 0xFFFF, ssrc=0xCAFE0002), 'RTP LOSS TS', 3, 2, 32767),
    ]
    return out


def gre_cases():
    """the same, of kind GRE: every datagram behind the GRE header of the GSE paths"""
    t = lambda n, seed=1: R.ts_packets(n, seed=seed)
    return [
        ('GRE, IPv4 RTP', b'\x00\x00\x08\x00' + R.datagram(R.rtp(t(7), seq=1)), 'RTP TS', 0, 7, 0),
        ('GRE, IPv6 raw', b'\x00\x00\x86\xdd' + R.datagram(t(3), 6), 'RAW TS', 1, 3, 0),
        ('GRE with the MPLS protocol type', b'\x00\x00\x88\x47' + R.datagram(R.rtp(t(7), seq=2)), 'NOT_IP', -1, 0, 0),
        ('the two-byte header of a non-IP PDU', b'\x88\x47', 'NOT_IP', -1, 0, 0),
        ('GRE with a flag set', b'\x20\x00\x08\x00' + R.datagram(R.rtp(t(7), seq=2)), 'NOT_IP', -1, 0, 0),
        ('GRE says IPv6 over an IPv4 datagram', b'\x00\x00\x86\xdd' + R.datagram(R.rtp(t(1), seq=2))[:30], 'BAD_IP', -1, 0, 0),
        ('GRE, not delivered', None, 'NOT_DELIVERED', -1, 0, 0),
        ('GRE, IPv4 RTP, the next', b'\x00\x00\x08\x00' + R.datagram(R.rtp(t(2), seq=2)), 'RTP TS', 0, 2, 0),
    ]


def expected_rows(cs):
    return [(flags(f), s, p, l) for _, _, f, s, p, l in cs]


def expected_stats(cs, delivered=True):
    """the stream's counters (IpTsBank.stats(stream, -1)) behind the cases on a fresh bank, from the written rows alone"""
    st = dict.fromkeys(R.STAT_KEYS, 0)
    st['rows'] = len(cs)
    for fl, s, p, l in expected_rows(cs):
        for k, name in enumerate(R.STREAM_KEYS[1:]):
            st[name] += fl >> k & 1
        for k, name in enumerate(R.SLOT_KEYS[1:11]):
            st[name] += fl >> (7 + k) & 1
        st['matched'] += s >= 0
        st['ts_packets'] += p
        st['lost'] += l
        st['bytes_delivered'] += 188 * p if delivered else 0
    return st


def table_of(cs, shift=0, gap=0):
    return R.lay([d for _, d, *_ in cs], shift=shift, gap=gap, seed=len(cs))


# ------------------------------------------------------------------------------------------------- random tables
def random_table(seed, n, kind=R.RAW_IP, shift=None):
    """n seeded datagrams that meet every rule: mostly good RTP and raw datagrams of the four flows with running sequence numbers, and
    every fault now and then -> (data, table)"""
    rng = np.random.default_rng(seed)
    seqs = {0: int(rng.integers(0, 65536)), 1: 65500, 3: 10}
    ssrc = {0: 1, 1: 2, 3: 3}
    flow = {0: dict(family=4, dport=PORT), 1: dict(family=6, dport=PORT), 3: dict(family=4, dport=PORT3)}
    out = []
    for i in range(n):
        k = (0, 1, 3)[int(rng.integers(0, 3))]
        npk = int(rng.choice([1, 2, 7, 7, 7, 11]))
        ts = R.ts_packets(npk, seed=int(rng.integers(0, 1 << 30)))
        what = int(rng.integers(0, 40))

        def good(step=1, **kw):
            seqs[k] = (seqs[k] + step) & 0xFFFF
            return R.rtp(ts, seq=seqs[k], ssrc=ssrc[k], timestamp=int(rng.integers(0, 1 << 32)), **kw)
        fam = flow[k]['family']
        if what == 0:
            d = None
        elif what == 1:
            d = bytes(rng.integers(0, 256, int(rng.integers(0, 60)), dtype=np.uint8))
            d = (b'\x75' + d[1:]) if d else d
        elif what == 2:
            d = R.ipv4(R.udp(good()), checksum=int(rng.integers(1, 65536))) if rng.random() < 0.5 else R.ipv6(R.udp(good(), 6), payload_length=60000)
        elif what == 3:
            d = R.ipv4(R.udp(good()), frag=int(rng.choice([0x2000, 0x0001, 0x2100])))
        elif what == 4:
            d = R.ipv4(bytes(24), proto=6) if rng.random() < 0.5 else R.ipv6(bytes(24), next_header=58)
        elif what == 5:
            d = R.ipv4(R.udp(b'abcd', length=int(rng.choice([0, 7, 13, 400]))))
        elif what in (6, 7):
            d = R.datagram(good(), fam, dport=int(rng.integers(2000, 3000)))
        elif what == 8:
            d = bytearray(R.datagram(good(), **flow[k]))
            d[-1 - int(rng.integers(0, 180))] ^= 1 << int(rng.integers(0, 8))
            d = bytes(d)
        elif what == 9:
            d = R.datagram(good(), **flow[k], checksum=0)
        elif what == 10:
            d = R.datagram(R.rtp(ts[:-1 - int(rng.integers(0, 100))], seq=5, version=int(rng.choice([2, 2, 1]))), **flow[k])
        elif what == 11:
            d = R.datagram(R.rtp(ts, seq=5, pt=int(rng.choice([0, 96, 34]))), **flow[k])
        elif what in (12, 13, 14):
            d = R.datagram(ts, **flow[k])
        elif what == 15:
            ssrc[k] += 16
            d = R.datagram(good(int(rng.integers(1, 1000))), **flow[k])
        elif what in (16, 17):
            d = R.datagram(good(int(rng.integers(2, 40))), **flow[k])
        elif what == 18:
            d = R.datagram(R.rtp(ts, seq=(seqs[k] - int(rng.integers(0, 50))) & 0xFFFF, ssrc=ssrc[k]), **flow[k])
        elif what == 19:
            d = R.datagram(good(cc=int(rng.integers(0, 16)), ext=int(rng.choice([0, 1, 5])), pad=int(rng.integers(0, 9))), **flow[k])
        elif what == 20:
            d = R.ipv4(R.udp(good(), dport=PORT), options=bytes(4 * int(rng.integers(1, 11))))
        else:
            d = R.datagram(good(), **flow[k])
        if d is not None and kind == R.GRE:
            d = (b'\x00\x00\x08\x00' if d[:1] and d[0] >> 4 == 4 else b'\x00\x00\x86\xdd' if rng.random() < 0.97 else b'\x00\x00\x88\x47') + d
        out.append(d)
    return R.lay(out, shift=int(rng.integers(0, 16)) if shift is None else shift, gap=5, seed=seed)


def calls_of(table, per_call):
    """the table cut into calls of per_call rows (0: one call)"""
    step = per_call or max(len(table), 1)
    return [table[a:a + step] for a in range(0, max(len(table), 1), step)]
