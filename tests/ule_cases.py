"""Constructed cases of the ULE bank, each by name: the TS packets of edge_cases() and, in ROWS, what the slot's table must say of
them, written out as numbers.  The slot watches PID with the NPA filter (NPA, MASK) -- the 23 high bits of an IPv4 multicast MAC -- and
accepts SNDUs without an address; ROWS_NO_ACCEPT says what a slot with the same filter that does not accept them makes of the cases
with D = 1.  The continuity counter runs through the cases in order, so they can be fed one by one to one bank or back to back
(whole_stream)."""
import numpy as np

import psi_ref as S
import ule_ref as R

PID = 0x0452
NPA, MASK = bytes.fromhex('01005e000000'), bytes.fromhex('ffffff800000')
GROUP = bytes.fromhex('01005e000105')                              # matches under the mask
OTHER = bytes.fromhex('01005e800105')                              # does not
ROW_FIELDS = R.ROW_KEYS


def _bytes(n, seed):
    return bytes((seed + 7 * i) & 255 for i in range(n))


def dgram(n, seed=0, sport=5004, dport=1234, **kw):
    """an IPv4/UDP datagram of n bytes"""
    return R.ipv4(R.udp(sport, dport, _bytes(n - 28 - len(kw.get('options', b'')), seed)), **kw)


def ip4(n, seed=0, npa=GROUP, **kw):
    """the SNDU around dgram(n, seed): n + 14 bytes to an address, n + 8 without"""
    return R.sndu(0x0800, dgram(n, seed, **kw), npa=npa)


FIVE = [(5, 0x40 + i, _bytes(8, 90 + i)) for i in range(4)]        # four optional headers of H-LEN 5: 40 bytes


def full_head(seed=70):
    """the SNDU whose row needs all 128 leading bytes: NPA, 40 bytes of optional headers, a bridged frame, an IPv4 header of 60 bytes, UDP"""
    return R.sndu(*R.extended(FIVE, *R.bridged(0x0800, dgram(300, seed, options=_bytes(40, seed + 1)))), npa=GROUP)


def edge_cases():
    """-> [(name, [k, 188])]"""
    z = R.Packetiser(PID)
    out = []

    def lay(name, sndus, **kw):
        out.append((name, z.lay(sndus, **kw)))

    lay('one IPv4/UDP datagram in one TS packet, End Indicator behind', [ip4(60, 1)], pad=True)
    lay('a 1400-byte datagram over 8 packets', [ip4(1400, 2)])
    lay('Length 4092: the largest SNDU, datagram 4082', [ip4(4082, 3)])
    lay('two SNDUs packed in one TS packet, 0xFF behind', [ip4(32, 4), ip4(33, 5)], pad=True)
    lay('base header split after 1 byte', [ip4(168, 6), ip4(40, 7)])
    lay('base header split after 2 bytes', [ip4(167, 8), ip4(41, 9)])
    lay('base header split after 3 bytes', [ip4(166, 10), ip4(42, 11)])
    lay('an SNDU that ends on the last payload byte', [ip4(169, 12)], pad=True)
    lay('a one-byte 0xFF remainder', [ip4(168, 13)], pad=True)
    lay('D = 1: no address', [ip4(50, 14, npa=None)])
    lay('an address that matches under the mask and one that does not', [ip4(60, 15, npa=bytes.fromhex('01005e7fffff')), ip4(60, 16, npa=OTHER)])
    lay('a Test SNDU', [R.sndu(0x0000, _bytes(20, 17), npa=GROUP)])
    lay('a bridged IPv4 frame without an NPA: mac is the bridged destination', [R.sndu(*R.bridged(0x0800, dgram(44, 18), dst=bytes.fromhex('01005e000777')))])
    lay('a bridged IPv4 frame to an NPA', [R.sndu(*R.bridged(0x0800, dgram(44, 19), dst=bytes.fromhex('01005e000777')), npa=GROUP)])
    lay('an optional header of H-LEN 1', [R.sndu(*R.extended([(1, 0x00, b'')], 0x0800, dgram(40, 20)), npa=GROUP)])
    lay('an optional header of H-LEN 5', [R.sndu(*R.extended([(5, 0x33, _bytes(8, 21))], 0x86DD, R.ipv6(R.udp(546, 547, _bytes(10, 22)))), npa=GROUP)])
    lay('four optional headers of H-LEN 5: 40 bytes are followed', [R.sndu(*R.extended(FIVE, 0x0800, dgram(40, 23)), npa=GROUP)])
    lay('42 bytes of optional headers', [R.sndu(*R.extended(FIVE + [(1, 0x07, b'')], 0x0800, dgram(40, 24)), npa=GROUP)])
    lay('an optional header that runs beyond the SNDU', [R.sndu(0x0534, _bytes(6, 25), npa=GROUP)])
    lay('a bridged IPv4 frame behind an optional header', [R.sndu(*R.extended([(2, 0x11, b'\xab\xcd')], *R.bridged(0x0800, dgram(60, 26))), npa=GROUP)])
    lay('TS-Concat, PRIV-Concat and an unknown mandatory header', [R.sndu(t, _bytes(30, 27), npa=GROUP) for t in (0x0002, 0x0003, 0x00C8)])
    lay('a bridged frame of 13 bytes', [R.sndu(0x0001, _bytes(13, 28), npa=GROUP)])
    lay('ARP, and a bridged LLC frame', [R.sndu(0x0806, bytes(28), npa=GROUP), R.sndu(*R.bridged(0x0026, _bytes(38, 29)), npa=GROUP)])
    lay('IPv6/UDP', [R.sndu(0x86DD, R.ipv6(R.udp(4000, 4001, _bytes(100, 30))), npa=GROUP)])
    lay('IHL 15 with options, and TCP', [ip4(120, 31, options=_bytes(40, 32)), R.sndu(0x0800, R.ipv4(R.tcp(443, 50000, _bytes(9, 33)), proto=6), npa=GROUP)])
    lay('a bad header checksum, and an IPv6 payload_length beyond avail',
        [ip4(60, 34, checksum=0x1234), R.sndu(0x86DD, R.ipv6(R.udp(1, 2, _bytes(10, 35)), payload_length=19), npa=GROUP)])
    lay('total_length below avail: stuffing trimmed', [R.sndu(0x0800, dgram(60, 36) + bytes(7), npa=GROUP)])
    lay('Length 3 with D = 1 and Length 9 with D = 0', [R.sndu(0x0800, b'', length=3)[:7], R.sndu(0x0800, b'', npa=GROUP, length=9)[:13]])
    ts = z.lay([ip4(500, 37)])
    ts[1, 77] ^= 0x10
    out.append(('one flipped bit', ts))
    lay('Length 4093: the chain ends', [bytes([0x0F, 0xFD, 0x08, 0x00]) + _bytes(20, 38), ip4(40, 39)], pad=True)
    ts = z.lay([ip4(500, 40)])
    out.append(('a continuity error inside an SNDU', np.concatenate([np.delete(ts, 1, axis=0), z.lay([ip4(30, 41)])])))
    ts = z.lay([ip4(500, 42)])
    ts[1, 3] |= 0x80
    out.append(('a TS packet with TSC set', np.concatenate([ts, z.lay([ip4(31, 43)])])))
    for name, ptr in (('a pointer short of the open SNDU\'s end', 112), ('a pointer beyond the open SNDU\'s end: slack', 120)):
        a, b = ip4(286, 44), ip4(35, 45)                           # 300 bytes: 183 in the first TS packet, 117 left
        rest = (a[183:] + b'\x5a\x5a\x5a')[:ptr]
        out.append((name, np.array([S.packet(PID, z._next(), b'\x00' + a[:183], pusi=1), S.packet(PID, z._next(), bytes([ptr]) + rest + b, pusi=1)], np.uint8)))
    sec = full_head()
    thin, z.cc = R.thin_packets(PID, z.cc, sec[:130])
    tail = sec[130:]
    rest = [S.packet(PID, z._next(), tail[:184]), S.packet(PID, z._next(), tail[184:], af_len=184 - len(tail[184:]) - 1)]
    out.append(('the first 128 bytes one per TS packet', np.concatenate([thin, np.array(rest, np.uint8).reshape(-1, 188)])))
    return out


def whole_stream(cases=None):
    return np.concatenate([ts for _, ts in (cases or edge_cases())])


def many_pieces(npieces, cc=0, seed=50, size=900):
    """one SNDU of `size` bytes over exactly `npieces` TS packets: the first ones carry one to three bytes behind adaptation fields"""
    sec = R.sndu(0x0800, dgram(size - 14, seed, options=_bytes(8, seed + 1)), npa=GROUP)
    assert len(sec) == size
    for full in range(npieces - 1):                                # thin packets first, then one that takes `mid` bytes, then `full` whole payloads
        n_thin = npieces - 1 - full
        thin_bytes = sum(1 + (i % 3) for i in range(n_thin))
        mid = size - thin_bytes - 184 * full
        if 1 <= mid <= 183:
            break
    else:
        raise ValueError('no such cutting')
    thin, cc = R.thin_packets(PID, cc, sec[:thin_bytes], per_packet=(1, 2, 3))
    assert len(thin) == n_thin
    pos, out = thin_bytes, [thin]
    cc = (cc + 1) & 15
    out.append(S.packet(PID, cc, sec[pos:pos + mid], af_len=184 - mid - 1).reshape(1, 188))
    pos += mid
    while pos < size:
        cc = (cc + 1) & 15
        out.append(S.packet(PID, cc, sec[pos:pos + 184]).reshape(1, 188))
        pos += 184
    ts = np.concatenate(out)
    assert len(ts) == npieces
    return ts, cc, sec


def random_feed(rng, pids, n_packets, npas=(GROUP, bytes.fromhex('01005e000106'), bytes.fromhex('0200c0ffee01'), None)):
    """ULE feeds on `pids` with datagrams to several addresses and to none, extension headers, bridged frames, other Types and
    faults, interleaved with a filler PID"""
    streams = []
    for pid in pids:
        z, parts = R.Packetiser(pid, cc=int(rng.integers(16))), []
        while sum(len(p) for p in parts) < n_packets:
            sndus = []
            for _ in range(int(rng.integers(1, 6))):
                kind, npa = rng.random(), npas[int(rng.integers(len(npas)))]
                data = bytes(rng.integers(0, 256, int(rng.choice([0, 10, 100, 183, 700, 2000])), dtype=np.uint8))
                d4 = R.ipv4(R.udp(int(rng.integers(65536)), 1234, data), options=bytes(4 * int(rng.integers(0, 3))))
                hdrs = [(int(h), int(rng.integers(256)), bytes(2 * int(h) - 2)) for h in rng.integers(1, 6, int(rng.integers(0, 6)))]
                if kind < 0.4:
                    sndus.append(R.sndu(0x0800, d4 + bytes(int(rng.integers(0, 3))), npa=npa))
                elif kind < 0.55:
                    sndus.append(R.sndu(*R.extended(hdrs, 0x0800, d4), npa=npa))
                elif kind < 0.65:
                    sndus.append(R.sndu(*R.extended(hdrs[:2], *R.bridged(int(rng.choice([0x0800, 0x86DD, 0x0806, 0x0040])), d4)), npa=npa))
                elif kind < 0.72:
                    sndus.append(R.sndu(0x86DD, R.ipv6(R.udp(7, 9, data)), npa=npa))
                elif kind < 0.8:
                    sndus.append(R.sndu(0x0800, R.ipv4(data, proto=int(rng.choice([1, 6, 17])), checksum=int(rng.integers(65536)) if rng.random() < 0.5 else None,
                                                       frag=int(rng.integers(3))), npa=npa))
                elif kind < 0.9:
                    sndus.append(R.sndu(int(rng.choice([0, 2, 3, 0x00FE, 0x0806, 0x0501])), data[:int(rng.integers(0, 40))], npa=npa))
                else:
                    n = int(rng.integers(0, 12))
                    sndus.append(R.sndu(0x0800, b'', length=n)[:4 + n])
            ts = z.lay(sndus, flush=rng.random() < 0.5, af_len=None if rng.random() < 0.8 else int(rng.integers(0, 100)), pad=rng.random() < 0.3)
            if len(ts) > 2 and rng.random() < 0.5:
                ts = S.INJECTORS[int(rng.integers(len(S.INJECTORS)))](ts, int(rng.integers(1, len(ts) - 1)))[0]
            parts.append(ts)
        streams.append(np.concatenate(parts)[:n_packets])
    streams.append(S.filler(0x99, n_packets // 4, rng))
    return S.interleave(rng, streams)


def wild_packets(seed, n_packets, pid=0x40):
    """seeded random packets on `pid` and a second PID: a random feed in which about one packet in six is damaged -- random bytes
    all over, a random adaptation field control and length, a random pointer, a random continuity counter, TSC, TEI or a wrong sync
    byte -- so that SNDUs complete, split, drop and fail their checks"""
    rng = np.random.default_rng(seed)
    ts = random_feed(rng, [pid, pid + 1], n_packets).copy()
    for k in range(len(ts)):
        p, kind = ts[k], rng.random()
        if kind > 0.17:
            continue
        if kind < 0.03:
            p[4:] = rng.integers(0, 256, 184, dtype=np.uint8)
        elif kind < 0.06:
            p[3] = (p[3] & 0xCF) | int(rng.integers(4)) << 4
            p[4] = int(rng.integers(256))
        elif kind < 0.09:
            p[1] |= 0x40
            ps = 5 + int(p[4]) if p[3] & 0x20 else 4
            if ps < 188:
                p[ps] = int(rng.integers(256)) if rng.random() < 0.3 else int(rng.integers(188 - ps))
        elif kind < 0.11:
            p[3] = (p[3] & 0xF0) | int(rng.integers(16))
        elif kind < 0.13:
            p[int(rng.integers(4, 188))] ^= 1 << int(rng.integers(8))
        elif kind < 0.14:
            p[3] |= 0x80
        elif kind < 0.15:
            p[1] |= 0x80
        elif kind < 0.16:
            p[0] = 0x46
        else:
            p[5:7] = [0x7F, 0xFF]                                  # where an SNDU starts behind a pointer of 0: the bad length
    return ts


G, M_7F, M_80, BR, Z = GROUP, bytes.fromhex('01005e7fffff'), OTHER, bytes.fromhex('01005e000777'), bytes(6)
A, B = 3232235521, 3758096645                                      # 192.168.0.1, 224.0.1.5
# (flags, family, protocol, mac, ip_at, extension_bytes, src_port, dst_port, src4, dst4, length, offset, bytes, first_packet, last_packet, ethertype,
#  stuffing) of every row of every case, fed one by one with delivery
ROWS = {
    'one IPv4/UDP datagram in one TS packet, End Indicator behind': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 74, 0, 60, 0, 0, 0x0800, 0)],
    'a 1400-byte datagram over 8 packets': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 1414, 0, 1400, 0, 7, 0x0800, 0)],
    'Length 4092: the largest SNDU, datagram 4082': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 4096, 0, 4082, 0, 22, 0x0800, 0)],
    'two SNDUs packed in one TS packet, 0xFF behind': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 46, 0, 32, 0, 0, 0x0800, 0),
        (512, 4, 17, G, 10, 0, 5004, 1234, A, B, 47, 32, 33, 0, 0, 0x0800, 0)],
    'base header split after 1 byte': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 182, 0, 168, 0, 0, 0x0800, 0),
        (512, 4, 17, G, 10, 0, 5004, 1234, A, B, 54, 168, 40, 0, 1, 0x0800, 0)],
    'base header split after 2 bytes': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 181, 0, 167, 0, 0, 0x0800, 0),
        (512, 4, 17, G, 10, 0, 5004, 1234, A, B, 55, 167, 41, 0, 1, 0x0800, 0)],
    'base header split after 3 bytes': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 180, 0, 166, 0, 0, 0x0800, 0),
        (512, 4, 17, G, 10, 0, 5004, 1234, A, B, 56, 166, 42, 0, 1, 0x0800, 0)],
    'an SNDU that ends on the last payload byte': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 183, 0, 169, 0, 0, 0x0800, 0)],
    'a one-byte 0xFF remainder': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 182, 0, 168, 0, 0, 0x0800, 0)],
    'D = 1: no address': [(520, 4, 17, Z, 4, 0, 5004, 1234, A, B, 58, 0, 50, 0, 0, 0x0800, 0)],
    'an address that matches under the mask and one that does not': [(512, 4, 17, M_7F, 10, 0, 5004, 1234, A, B, 74, 0, 60, 0, 0, 0x0800, 0),
        (4, 0, 0, M_80, 0, 0, 0, 0, 0, 0, 74, -1, 0, 0, 0, 0, 0)],
    'a Test SNDU': [(16, 0, 0, G, 0, 0, 0, 0, 0, 0, 34, -1, 0, 0, 0, 0, 0)],
    'a bridged IPv4 frame without an NPA: mac is the bridged destination': [(552, 4, 17, BR, 18, 0, 5004, 1234, A, B, 66, 0, 44, 0, 0, 0x0800, 0)],
    'a bridged IPv4 frame to an NPA': [(544, 4, 17, G, 24, 0, 5004, 1234, A, B, 72, 0, 44, 0, 0, 0x0800, 0)],
    'an optional header of H-LEN 1': [(512, 4, 17, G, 12, 2, 5004, 1234, A, B, 56, 0, 40, 0, 0, 0x0800, 0)],
    'an optional header of H-LEN 5': [(512, 6, 17, G, 20, 10, 546, 547, 0, 0, 82, 0, 58, 0, 0, 0x86DD, 0)],
    'four optional headers of H-LEN 5: 40 bytes are followed': [(512, 4, 17, G, 50, 40, 5004, 1234, A, B, 94, 0, 40, 0, 0, 0x0800, 0)],
    '42 bytes of optional headers': [(64, 0, 0, G, 0, 0, 0, 0, 0, 0, 96, -1, 0, 0, 0, 0x0107, 0)],
    'an optional header that runs beyond the SNDU': [(64, 0, 0, G, 0, 0, 0, 0, 0, 0, 20, -1, 0, 0, 0, 0x0534, 0)],
    'a bridged IPv4 frame behind an optional header': [(544, 4, 17, G, 28, 4, 5004, 1234, A, B, 92, 0, 60, 0, 0, 0x0800, 0)],
    'TS-Concat, PRIV-Concat and an unknown mandatory header': [(64, 0, 0, G, 0, 0, 0, 0, 0, 0, 44, -1, 0, 0, 0, 0x0002, 0),
        (64, 0, 0, G, 0, 0, 0, 0, 0, 0, 44, -1, 0, 0, 0, 0x0003, 0),
        (64, 0, 0, G, 0, 0, 0, 0, 0, 0, 44, -1, 0, 0, 0, 0x00C8, 0)],
    'a bridged frame of 13 bytes': [(64, 0, 0, G, 0, 0, 0, 0, 0, 0, 27, -1, 0, 0, 0, 0x0001, 0)],
    'ARP, and a bridged LLC frame': [(128, 0, 0, G, 0, 0, 0, 0, 0, 0, 42, -1, 0, 0, 0, 0x0806, 0),
        (160, 0, 0, G, 0, 0, 0, 0, 0, 0, 66, -1, 0, 0, 0, 0x0026, 0)],
    'IPv6/UDP': [(512, 6, 17, G, 10, 0, 4000, 4001, 0, 0, 162, 0, 148, 0, 0, 0x86DD, 0)],
    'IHL 15 with options, and TCP': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 134, 0, 120, 0, 0, 0x0800, 0),
        (512, 4, 6, G, 10, 0, 443, 50000, A, B, 63, 120, 49, 0, 1, 0x0800, 0)],
    'a bad header checksum, and an IPv6 payload_length beyond avail': [(256, 0, 0, G, 0, 0, 0, 0, 0, 0, 74, -1, 0, 0, 0, 0x0800, 0),
        (256, 0, 0, G, 0, 0, 0, 0, 0, 0, 72, -1, 0, 0, 0, 0x86DD, 0)],
    'total_length below avail: stuffing trimmed': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 81, 0, 60, 0, 0, 0x0800, 7)],
    'Length 3 with D = 1 and Length 9 with D = 0': [(1, 0, 0, Z, 0, 0, 0, 0, 0, 0, 7, -1, 0, 0, 0, 0, 0),
        (1, 0, 0, Z, 0, 0, 0, 0, 0, 0, 13, -1, 0, 0, 0, 0, 0)],
    'one flipped bit': [(2, 0, 0, Z, 0, 0, 0, 0, 0, 0, 514, -1, 0, 0, 2, 0, 0)],
    'Length 4093: the chain ends': [],
    'a continuity error inside an SNDU': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 44, 0, 30, 2, 2, 0x0800, 0)],
    'a TS packet with TSC set': [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 45, 0, 31, 3, 3, 0x0800, 0)],
    "a pointer short of the open SNDU's end": [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 49, 0, 35, 1, 1, 0x0800, 0)],
    "a pointer beyond the open SNDU's end: slack": [(512, 4, 17, G, 10, 0, 5004, 1234, A, B, 300, 0, 286, 0, 1, 0x0800, 0),
        (512, 4, 17, G, 10, 0, 5004, 1234, A, B, 49, 286, 35, 1, 1, 0x0800, 0)],
    'the first 128 bytes one per TS packet': [(544, 4, 17, G, 64, 40, 5004, 1234, A, B, 368, 0, 300, 0, 131, 0x0800, 0)],
}
# the cases with D = 1 in a slot that does not accept them: NO_ADDRESS | FILTERED
ROWS_NO_ACCEPT = {
    'D = 1: no address': [(12, 0, 0, Z, 0, 0, 0, 0, 0, 0, 58, -1, 0, 0, 0, 0, 0)],
    'a bridged IPv4 frame without an NPA: mac is the bridged destination': [(12, 0, 0, Z, 0, 0, 0, 0, 0, 0, 66, -1, 0, 0, 0, 0, 0)],
}
# what the whole run of cases leaves in the slot's counters, and in those of the slot that does not accept unaddressed SNDUs
STATS = dict(packets=208, sndus=46, crc_errors=1, filtered=1, no_address=2, test=1, bridged=5, extension=6, other_protocol=2, bad_ip=2, datagrams=31, datagrams_delivered=31, bytes_delivered=8058, dropped_sndus=3, malformed_sndus=3, slack=1, malformed_packets=0, scrambled_packets=1)
STATS_NO_ACCEPT = dict(STATS, filtered=3, bridged=4, datagrams=29, datagrams_delivered=29, bytes_delivered=7964)
