"""Constructed cases of the MPE bank, each by name: the TS packets of edge_cases() and, in ROWS, what the slot's table must say of
them, written out as numbers.  The slot watches PID with the MAC filter (MAC, MASK): the 23 high bits of an IPv4 multicast address.
The continuity counter runs through the cases in order, so they can be fed one by one to one bank or back to back (whole_stream)."""
import numpy as np

import mpe_ref as R
import psi_ref as S

PID = 0x0451
MAC, MASK = bytes.fromhex('01005e000000'), bytes.fromhex('ffffff800000')
GROUP = bytes.fromhex('01005e000105')                              # matches under the mask
ROW_FIELDS = ('flags', 'family', 'protocol', 'mac', 'section_number', 'last_section_number', 'src_port', 'dst_port', 'src4', 'dst4', 'length', 'offset', 'bytes',
              'first_packet', 'last_packet', 'ethertype', 'stuffing')


def _bytes(n, seed):
    return bytes((seed + 7 * i) & 255 for i in range(n))


def dgram(n, seed=0, sport=5004, dport=1234, **kw):
    """an IPv4/UDP datagram of n bytes"""
    return R.ipv4(R.udp(sport, dport, _bytes(n - 28 - len(kw.get('options', b'')), seed)), **kw)


def edge_cases():
    """-> [(name, [k, 188])]"""
    z, q = R.Packetiser(PID), S.Packetiser(PID)
    out = []

    def lay(name, sections, **kw):
        out.append((name, z.lay(sections, **kw)))

    def lay_padded(name, sections, **kw):                          # the section bank's packetiser: 0xFF behind the last section
        q.cc = z.cc
        out.append((name, q.lay(sections, **kw)))
        z.cc = q.cc

    lay('one IPv4/UDP datagram in one TS packet', [R.section(dgram(60, 1))])
    lay('a 1400-byte datagram over 8 packets', [R.section(dgram(1400, 2))])
    lay('the largest section: 4096 bytes, datagram 4080', [R.section(dgram(4080, 3))])
    lay_padded('two sections chained in one TS packet, 0xFF behind', [R.section(dgram(32, 4)), R.section(dgram(33, 5))])
    lay('header split after 1 byte', [R.section(dgram(166, 6)), R.section(dgram(40, 7))])
    lay('header split after 2 bytes', [R.section(dgram(165, 8)), R.section(dgram(41, 9))])
    ts = z.lay([R.section(dgram(500, 10))])
    ts[1, 77] ^= 0x10
    out.append(('one flipped bit', ts))
    lay('ssi clear: unchecked, delivered', [R.section(dgram(50, 11), ssi=0)])
    lay('LLC/SNAP 0x0800', [R.section(R.llc_snap(0x0800) + dgram(44, 12), llc=1)])
    lay('LLC/SNAP 0x86DD', [R.section(R.llc_snap(0x86DD) + R.ipv6(R.udp(546, 547, _bytes(10, 13))), llc=1)])
    lay('LLC/SNAP 0x0806', [R.section(R.llc_snap(0x0806) + bytes(28), llc=1)])
    lay('a wrong LLC', [R.section(R.llc_snap(0x0800, llc=b'\xaa\xaa\x03\x00\x00\x01') + dgram(44, 14), llc=1)])
    lay('IPv6/UDP', [R.section(R.ipv6(R.udp(4000, 4001, _bytes(100, 15))))])
    lay('IHL 15 with options', [R.section(dgram(120, 16, options=_bytes(40, 17)))])
    lay('a bad header checksum', [R.section(dgram(60, 18, checksum=0x1234))])
    lay('IHL 4', [R.section(dgram(60, 19, ihl=4))])
    lay('total_length above avail', [R.section(dgram(60, 20, total_length=61))])
    lay('total_length below avail: stuffing trimmed', [R.section(dgram(60, 21), stuffing=7)])
    lay('IPv6 payload_length beyond avail', [R.section(R.ipv6(R.udp(1, 2, _bytes(10, 22)), payload_length=19))])
    lay('an IPv4 fragment with a non-zero offset', [R.section(dgram(60, 23, frag=0x2010))])
    lay('ICMP', [R.section(R.ipv4(bytes([8, 0, 0xF7, 0xFF, 0, 0, 0, 0]), proto=1))])
    lay('TCP', [R.section(R.ipv4(R.tcp(443, 50000, _bytes(9, 24)), proto=6))])
    lay('payload scrambling', [R.section(dgram(60, 25), pscr=2)])
    lay('address scrambling', [R.section(dgram(60, 26), ascr=1)])
    lay('non-zero section numbers', [R.section(dgram(60, 27), number=0, last=1), R.section(dgram(60, 28), number=1, last=1)])
    lay('table_id 0x3B and 0x78', [R.raw_section(0x3B, _bytes(30, 29)), R.raw_section(0x78, _bytes(50, 30), ssi=1)])
    lay('a 0x3E section of 15 bytes', [R.raw_section(0x3E, _bytes(12, 31), ssi=1)])
    lay_padded('section_length 4094: the chain ends', [bytes([0x3E, 0xBF, 0xFE]) + _bytes(20, 32), R.section(dgram(40, 33))])
    ts = z.lay([R.section(dgram(500, 34))])
    out.append(('a continuity error inside a section', np.concatenate([np.delete(ts, 1, axis=0), z.lay([R.section(dgram(30, 35))])])))
    ts = z.lay([R.section(dgram(500, 36))])
    ts[1, 3] |= 0x80
    out.append(('a TS packet with TSC set', np.concatenate([ts, z.lay([R.section(dgram(31, 37))])])))
    lay('a MAC that matches under the mask and one that does not',
        [R.section(dgram(60, 38), mac=bytes.fromhex('01005e7fffff')), R.section(dgram(60, 39), mac=bytes.fromhex('01005e800105'))])
    sec = R.section(R.llc_snap(0x0800) + dgram(300, 40, options=_bytes(40, 41)), llc=1)
    thin, z.cc = R.thin_packets(PID, z.cc, sec[:90])
    rest = [S.packet(PID, z._next(), sec[90 + 184 * i:90 + 184 * (i + 1)]) for i in range(1)]
    tail = sec[90 + 184:]
    last = S.packet(PID, z._next(), tail, af_len=184 - len(tail) - 1)
    out.append(('the first 84 bytes one to three per TS packet', np.concatenate([thin, np.array(rest + [last], np.uint8).reshape(-1, 188)])))
    return out


def whole_stream(cases=None):
    return np.concatenate([ts for _, ts in (cases or edge_cases())])


def many_pieces(npieces, cc=0, seed=50, size=900):
    """one section of `size` bytes over exactly `npieces` TS packets: the first npieces - k carry one to three bytes behind adaptation fields"""
    sec = R.section(dgram(size - 16, seed, options=_bytes(8, seed + 1)))
    assert len(sec) == size
    # thin packets first, then one packet that takes `mid` bytes, then `full` whole payloads
    for full in range(npieces - 1):
        n_thin = npieces - 1 - full
        thin_bytes = sum(1 + (i % 3) for i in range(n_thin))
        mid = size - thin_bytes - 184 * full
        if 1 <= mid <= 183:
            break
    else:
        raise ValueError('no such cutting')
    thin, cc = R.thin_packets(PID, cc, sec[:thin_bytes])
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


def random_feed(rng, pids, n_packets, macs=(GROUP, bytes.fromhex('01005e000106'), bytes.fromhex('0200c0ffee01'))):
    """MPE feeds on `pids` with datagrams to several MAC addresses, other sections and faults, interleaved with a filler PID"""
    streams = []
    for pid in pids:
        z, parts = R.Packetiser(pid, cc=int(rng.integers(16))), []
        while sum(len(p) for p in parts) < n_packets:
            secs = []
            for _ in range(int(rng.integers(1, 6))):
                kind, mac = rng.random(), macs[int(rng.integers(len(macs)))]
                data = bytes(rng.integers(0, 256, int(rng.choice([0, 10, 100, 183, 700, 2000])), dtype=np.uint8))
                if kind < 0.5:
                    secs.append(R.section(R.ipv4(R.udp(int(rng.integers(65536)), 1234, data), options=bytes(4 * int(rng.integers(0, 3)))), mac=mac,
                                          stuffing=int(rng.integers(0, 3)), ssi=int(rng.random() < 0.9)))
                elif kind < 0.65:
                    secs.append(R.section(R.llc_snap(int(rng.choice([0x0800, 0x86DD, 0x0806]))) + R.ipv6(R.udp(7, 9, data)), mac=mac, llc=1))
                elif kind < 0.75:
                    secs.append(R.section(R.ipv4(data, proto=int(rng.choice([1, 6, 17])), checksum=int(rng.integers(65536)) if rng.random() < 0.5 else None,
                                                 frag=int(rng.integers(3))), mac=mac))
                elif kind < 0.85:
                    secs.append(R.section(R.ipv4(data), mac=mac, number=int(rng.integers(2)), last=int(rng.integers(2)), pscr=int(rng.random() < 0.3)))
                else:
                    secs.append(R.raw_section(int(rng.choice([0x3B, 0x3E, 0x78])), data[:int(rng.integers(0, 40))], ssi=int(rng.integers(2))))
            ts = z.lay(secs, flush=rng.random() < 0.5, af_len=None if rng.random() < 0.8 else int(rng.integers(0, 100)))
            if len(ts) > 2 and rng.random() < 0.5:
                ts = S.INJECTORS[int(rng.integers(len(S.INJECTORS)))](ts, int(rng.integers(1, len(ts) - 1)))[0]
            parts.append(ts)
        streams.append(np.concatenate(parts)[:n_packets])
    streams.append(S.filler(0x99, n_packets // 4, rng))
    return S.interleave(rng, streams)


def wild_packets(seed, n_packets, pid=0x40):
    """seeded random packets on `pid` and a second PID: a random feed in which about one packet in six is damaged -- random bytes
    all over, a random adaptation field control and length, a random pointer, a random continuity counter, TSC, TEI or a wrong sync
    byte -- so that sections complete, split, drop and fail their checks"""
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
            p[5:8] = [0x3E, 0xFF, 0xFF]                            # where a section starts behind a pointer of 0: the bad length
    return ts


G, M_7F, M_80, Z = GROUP,bytes.fromhex('01005e7fffff'), bytes.fromhex('01005e800105'), bytes(6)
A, B = 3232235521, 3758096645                                      # 192.168.0.1, 224.0.1.5
# (flags, family, protocol, mac, section_number, last_section_number, src_port, dst_port, src4, dst4, length, offset, bytes, first_packet, last_packet,
#  ethertype, stuffing) of every row of every case, fed one by one with delivery
ROWS = {
    'one IPv4/UDP datagram in one TS packet': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 76, 0, 60, 0, 0, 0, 0)],
    'a 1400-byte datagram over 8 packets': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 1416, 0, 1400, 0, 7, 0, 0)],
    'the largest section: 4096 bytes, datagram 4080': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 4096, 0, 4080, 0, 22, 0, 0)],
    'two sections chained in one TS packet, 0xFF behind': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 48, 0, 32, 0, 0, 0, 0),
                                                           (512, 4, 17, G, 0, 0, 5004, 1234, A, B, 49, 32, 33, 0, 0, 0, 0)],
    'header split after 1 byte': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 182, 0, 166, 0, 0, 0, 0), (512, 4, 17, G, 0, 0, 5004, 1234, A, B, 56, 166, 40, 0, 1, 0, 0)],
    'header split after 2 bytes': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 181, 0, 165, 0, 0, 0, 0), (512, 4, 17, G, 0, 0, 5004, 1234, A, B, 57, 165, 41, 0, 1, 0, 0)],
    'one flipped bit': [(4, 0, 0, Z, 0, 0, 0, 0, 0, 0, 516, -1, 0, 0, 2, 0, 0)],
    'ssi clear: unchecked, delivered': [(520, 4, 17, G, 0, 0, 5004, 1234, A, B, 66, 0, 50, 0, 0, 0, 0)],
    'LLC/SNAP 0x0800': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 68, 0, 44, 0, 0, 0x0800, 0)],
    'LLC/SNAP 0x86DD': [(512, 6, 17, G, 0, 0, 546, 547, 0, 0, 82, 0, 58, 0, 0, 0x86DD, 0)],
    'LLC/SNAP 0x0806': [(128, 0, 0, G, 0, 0, 0, 0, 0, 0, 52, -1, 0, 0, 0, 0x0806, 0)],
    'a wrong LLC': [(128, 0, 0, G, 0, 0, 0, 0, 0, 0, 68, -1, 0, 0, 0, 0, 0)],
    'IPv6/UDP': [(512, 6, 17, G, 0, 0, 4000, 4001, 0, 0, 164, 0, 148, 0, 0, 0, 0)],
    'IHL 15 with options': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 136, 0, 120, 0, 0, 0, 0)],
    'a bad header checksum': [(256, 0, 0, G, 0, 0, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'IHL 4': [(256, 0, 0, G, 0, 0, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'total_length above avail': [(256, 0, 0, G, 0, 0, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'total_length below avail: stuffing trimmed': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 83, 0, 60, 0, 0, 0, 7)],
    'IPv6 payload_length beyond avail': [(256, 0, 0, G, 0, 0, 0, 0, 0, 0, 74, -1, 0, 0, 0, 0, 0)],
    'an IPv4 fragment with a non-zero offset': [(512, 4, 17, G, 0, 0, 0, 0, A, B, 76, 0, 60, 0, 0, 0, 0)],
    'ICMP': [(512, 4, 1, G, 0, 0, 0, 0, A, B, 44, 0, 28, 0, 0, 0, 0)],
    'TCP': [(512, 4, 6, G, 0, 0, 443, 50000, A, B, 65, 0, 49, 0, 0, 0, 0)],
    'payload scrambling': [(16, 0, 0, G, 0, 0, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'address scrambling': [(16, 0, 0, G, 0, 0, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'non-zero section numbers': [(64, 0, 0, G, 0, 1, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0), (64, 0, 0, G, 1, 1, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'table_id 0x3B and 0x78': [(1, 0, 0, Z, 0, 0, 0, 0, 0, 0, 33, -1, 0, 0, 0, 0, 0), (1, 0, 0, Z, 0, 0, 0, 0, 0, 0, 53, -1, 0, 0, 0, 0, 0)],
    'a 0x3E section of 15 bytes': [(2, 0, 0, Z, 0, 0, 0, 0, 0, 0, 15, -1, 0, 0, 0, 0, 0)],
    'section_length 4094: the chain ends': [],
    'a continuity error inside a section': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 46, 0, 30, 2, 2, 0, 0)],
    'a TS packet with TSC set': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 47, 0, 31, 3, 3, 0, 0)],
    'a MAC that matches under the mask and one that does not': [(512, 4, 17, M_7F, 0, 0, 5004, 1234, A, B, 76, 0, 60, 0, 0, 0, 0),
                                                                (32, 0, 0, M_80, 0, 0, 0, 0, 0, 0, 76, -1, 0, 0, 0, 0, 0)],
    'the first 84 bytes one to three per TS packet': [(512, 4, 17, G, 0, 0, 5004, 1234, A, B, 324, 0, 300, 0, 46, 0x0800, 0)],
}
# what the whole run of cases leaves in the slot's counters
STATS = dict(packets=116, sections=37, other_table=2, crc_errors=1, unchecked=1, scrambled_sections=2, filtered=1, fragments=2, other_protocol=2, bad_ip=4,
             datagrams=22, datagrams_delivered=22, bytes_delivered=7055, dropped_sections=2, malformed_sections=2, malformed_packets=0, scrambled_packets=1)
