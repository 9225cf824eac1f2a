"""Python model of the IP-TS bank's rules, written from the header comment (include/dvbs2gpu.h, IP-TS bank): the sequential
definition, row by row, with a checksum of its own (the ones'-complement sum as a remainder modulo 65535, not a folded loop).  With it
the builders of IPv4 / IPv6 / UDP / RTP datagrams, right and faulty.  The yardstick of the bank's tests."""
import numpy as np

TS = 188
SLOTS = 4
RAW_IP, GRE = 0, 1
(NOT_DELIVERED, NOT_IP, BAD_IP, FRAGMENT, OTHER_PROTOCOL, BAD_UDP, UNWATCHED, BAD_CHECKSUM, NO_CHECKSUM, BAD_PAYLOAD, OTHER_PAYLOAD, RAW, RTP, NEW_SOURCE, LOSS, LATE,
 TS_ROW) = (1 << k for k in range(17))
FLAG_NAMES = ('NOT_DELIVERED', 'NOT_IP', 'BAD_IP', 'FRAGMENT', 'OTHER_PROTOCOL', 'BAD_UDP', 'UNWATCHED', 'BAD_CHECKSUM', 'NO_CHECKSUM', 'BAD_PAYLOAD', 'OTHER_PAYLOAD',
              'RAW', 'RTP', 'NEW_SOURCE', 'LOSS', 'LATE', 'TS')
STREAM_KEYS = ('rows', 'not_delivered', 'not_ip', 'bad_ip', 'fragments', 'other_protocol', 'bad_udp', 'unwatched')
SLOT_KEYS = ('matched', 'bad_checksum', 'no_checksum', 'bad_payload', 'other_payload', 'raw', 'rtp', 'new_source', 'loss_events', 'late', 'ts', 'ts_packets',
             'bytes_delivered', 'lost')
STAT_KEYS = STREAM_KEYS + SLOT_KEYS
ROW_KEYS = ('flags', 'slot', 'family', 'payload_type', 'src_port', 'dst_port', 'rtp_seq', 'ts_at', 'rtp_timestamp', 'rtp_ssrc', 'packets', 'lost', 'offset', 'bytes')
LAYOUT = dict(gre_header_bytes=4, ipv4_src_at=12, ipv6_src_at=8, ipv6_dst_at=24, ipv4_more_fragments=0x2000, udp_protocol=17, udp_header_bytes=8, udp_length_at=4,
              udp_checksum_at=6, ts_packet_bytes=188, ts_sync=0x47, rtp_min_header=12, rtp_version=2, rtp_payload_type_mp2t=33, rtp_seq_at=2, rtp_timestamp_at=4,
              rtp_ssrc_at=8, late_from=0x8000, head_bytes=128, slots=4, row_bytes=40, view_bytes=40)


def ones_sum(data):
    """the ones'-complement sum, carries folded in, of `data` as big-endian 16-bit words (an odd last byte padded with a zero byte): a
    number's remainder modulo 2^16 - 1 is the end-around-carry sum of its 16-bit digits, with 0xFFFF standing for a non-zero multiple"""
    data = bytes(data)
    n = int.from_bytes(data + b'\x00' * (len(data) & 1), 'big')
    return 0 if n == 0 else (n % 0xFFFF or 0xFFFF)


def word_sum(data):
    """the plain sum of the same words, unfolded (what tells how many folds a checksum needs)"""
    data = bytes(data) + b'\x00' * (len(data) & 1)
    return int(np.frombuffer(data, '>u2').astype(np.int64).sum())


def _be(b, i, n=2):
    return int.from_bytes(b[i:i + n], 'big')


def _syncs(b, at, n):
    return all(b[at + TS * k] == 0x47 for k in range(n))


def row_of(d, kind, flows):
    """rules 2 to 8 of one delivered datagram d (bytes) -> the row as a dict, but for the sequence rule and the offset"""
    r = dict.fromkeys(ROW_KEYS, 0)
    r['slot'] = r['offset'] = -1

    def end(flag):
        r['flags'] |= flag
        return r
    at = 0
    if kind == GRE:
        if len(d) < 4 or d[:4] not in (b'\x00\x00\x08\x00', b'\x00\x00\x86\xdd'):
            return end(NOT_IP)
        family, at = (4 if d[2] == 8 else 6), 4
    else:
        family = d[0] >> 4 if d else 0
        if family not in (4, 6):
            return end(NOT_IP)
    avail = len(d) - at
    if family == 4:
        if avail < 20:
            return end(BAD_IP)
        hl, tl = 4 * (d[at] & 15), _be(d, at + 2)
        if hl < 20 or hl > avail or tl < hl or tl > avail or ones_sum(d[at:at + hl]) != 0xFFFF:
            return end(BAD_IP)
        r['family'] = 4
        if _be(d, at + 6) & 0x3FFF:
            return end(FRAGMENT)
        proto, src, dst, pseudo = d[at + 9], d[at + 12:at + 16], d[at + 16:at + 20], lambda L: bytes([0, 17, L >> 8, L & 255])
    else:
        if avail < 40 or 40 + _be(d, at + 4) > avail:
            return end(BAD_IP)
        r['family'] = 6
        hl, tl = 40, 40 + _be(d, at + 4)
        proto, src, dst, pseudo = d[at + 6], d[at + 8:at + 24], d[at + 24:at + 40], lambda L: L.to_bytes(4, 'big') + bytes([0, 0, 0, 17])
    if proto != 17:
        return end(OTHER_PROTOCOL)
    u, room = at + hl, tl - hl
    if room < 8 or not 8 <= _be(d, u + 4) <= room:
        return end(BAD_UDP)
    L = _be(d, u + 4)
    r['src_port'], r['dst_port'] = _be(d, u), _be(d, u + 2)
    for k, f in enumerate(flows):
        if f is not None and f[0] == family and bytes(f[1]) == dst and f[2] == r['dst_port']:
            r['slot'] = k
            break
    else:
        return end(UNWATCHED)
    if _be(d, u + 6) == 0:
        if family == 6:
            return end(BAD_CHECKSUM)
        r['flags'] |= NO_CHECKSUM
    elif ones_sum(src + dst + pseudo(L) + d[u:u + L]) != 0xFFFF:      # (every part has an even length but the last)
        return end(BAD_CHECKSUM)
    pay, plen = u + 8, L - 8
    if plen > 0 and plen % TS == 0 and _syncs(d, pay, plen // TS):
        r.update(ts_at=pay, packets=plen // TS, bytes=plen)
        return end(RAW | TS_ROW)
    if plen < 12 or d[pay] >> 6 != 2:
        return end(BAD_PAYLOAD)
    hdr, pad = 12 + 4 * (d[pay] & 15), 0
    if hdr > plen:
        return end(BAD_PAYLOAD)
    if d[pay] >> 4 & 1:
        if hdr + 4 > plen:
            return end(BAD_PAYLOAD)
        hdr += 4 + 4 * _be(d, pay + hdr + 2)
        if hdr > plen:
            return end(BAD_PAYLOAD)
    if d[pay] >> 5 & 1:
        pad = d[pay + plen - 1]
        if pad < 1 or hdr + pad > plen:
            return end(BAD_PAYLOAD)
    r['payload_type'] = d[pay + 1] & 127
    if r['payload_type'] != 33:
        return end(OTHER_PAYLOAD)
    left = plen - hdr - pad
    if left <= 0 or left % TS or not _syncs(d, pay + hdr, left // TS):
        return end(BAD_PAYLOAD)
    r.update(rtp_seq=_be(d, pay + 2), rtp_timestamp=_be(d, pay + 4, 4), rtp_ssrc=_be(d, pay + 8, 4), ts_at=pay + hdr, packets=left // TS, bytes=left)
    return end(RTP)


class Stream:
    """one stream: four flow slots (family, address bytes, port) or None, their RTP states and counters"""

    def __init__(self):
        self.flows = [None] * SLOTS
        self.seq = [None] * SLOTS                                     # (last_seq, ssrc)
        self.st = dict.fromkeys(STREAM_KEYS, 0)
        self.slot_st = [dict.fromkeys(SLOT_KEYS, 0) for _ in range(SLOTS)]
        self.table = []

    def set_flow(self, slot, family, addr=None, port=0):
        self.flows[slot] = (family, bytes(addr), port) if family else None
        self.seq[slot] = None
        self.slot_st[slot] = dict.fromkeys(SLOT_KEYS, 0)

    def reset(self):
        self.seq = [None] * SLOTS
        self.st = dict.fromkeys(STREAM_KEYS, 0)
        self.slot_st = [dict.fromkeys(SLOT_KEYS, 0) for _ in range(SLOTS)]
        self.table = []

    def sizes(self, data, table, kind=RAW_IP):
        """the bytes per slot that process() would deliver, with nothing advanced"""
        keep = (list(self.seq), dict(self.st), [dict(s) for s in self.slot_st], self.table)
        out = self.process(data, table, kind)
        self.seq, self.st, self.slot_st, self.table = keep
        return [len(o) for o in out]

    def process(self, data, table, kind=RAW_IP, deliver=True):
        """data: the datagram bytes; table: (offset, bytes) per input row -> the TS packets per slot (a list of four uint8 arrays), or
        None with deliver=False; self.table: the call's rows as IpTsBank.row_table gives them"""
        data = bytes(np.asarray(data, np.uint8).tobytes())
        out, rows = [bytearray() for _ in range(SLOTS)], []
        for off, nb in np.asarray(table, np.int64).reshape(-1, 2):
            self.st['rows'] += 1
            if off < 0:
                r = dict.fromkeys(ROW_KEYS, 0)
                r.update(flags=NOT_DELIVERED, slot=-1, offset=-1)
            else:
                d = data[off:off + max(int(nb), 0)]
                r = row_of(d, kind, self.flows)
                if r['flags'] & RTP:
                    st, new = self.seq[r['slot']], (r['rtp_seq'], r['rtp_ssrc'])
                    late = False
                    if st is not None and st[1] != new[1]:
                        r['flags'] |= NEW_SOURCE
                    elif st is not None:
                        gap = (new[0] - st[0] - 1) % 65536
                        late = gap >= 0x8000
                        if late:
                            r['flags'] |= LATE
                            r['packets'] = r['bytes'] = 0
                        elif gap:
                            r['flags'] |= LOSS
                            r['lost'] = gap
                    if not late:
                        self.seq[r['slot']] = new
                        r['flags'] |= TS_ROW
                if r['flags'] & TS_ROW and deliver:
                    r['offset'] = len(out[r['slot']])
                    out[r['slot']] += d[r['ts_at']:r['ts_at'] + r['bytes']]
            for k, name in enumerate(STREAM_KEYS[1:]):
                self.st[name] += r['flags'] >> k & 1
            if r['slot'] >= 0:
                s = self.slot_st[r['slot']]
                s['matched'] += 1
                for k, name in enumerate(SLOT_KEYS[1:11]):
                    s[name] += r['flags'] >> (7 + k) & 1
                s['lost'] += r['lost']
                s['ts_packets'] += r['packets']
                s['bytes_delivered'] += r['bytes'] if r['offset'] >= 0 else 0
            rows.append(r)
        self.table = rows
        return [np.frombuffer(bytes(o), np.uint8) for o in out] if deliver else None

    def stats(self, slot=-1):
        """as IpTsBank.stats: a slot's counters (the stream's own 0), or with -1 the stream's own and the sum over the slots"""
        res = dict.fromkeys(STAT_KEYS, 0)
        if slot < 0:
            res.update(self.st)
        for s in (self.slot_st if slot < 0 else [self.slot_st[slot]]):
            for k in SLOT_KEYS:
                res[k] += s[k]
        return res


# ------------------------------------------------------------------------------------------------- builders
V4_SRC, V4_DST = bytes([192, 168, 0, 1]), bytes([239, 1, 1, 5])
V6_SRC, V6_DST = bytes.fromhex('20010db8000000000000000000000001'), bytes.fromhex('ff3e0000000000000000000000001234')


def ts_packets(n, pid=0x100, cc=0, seed=0):
    """n TS packets of one PID with running continuity counters and seeded payload -> bytes"""
    rng = np.random.default_rng(seed)
    p = rng.integers(0, 256, (n, TS), dtype=np.uint8)
    for k in range(n):
        p[k, :4] = [0x47, pid >> 8, pid & 255, 0x10 | (cc + k) & 15]
    return p.tobytes()


def rtp(payload, seq=0, timestamp=0, ssrc=0x11223344, pt=33, cc=0, ext=None, pad=0, version=2, marker=0):
    """an RTP packet: cc CSRC words, ext: None or the number of extension words behind the 4 extension bytes, pad: padding bytes (the
    last holds the count)"""
    h = bytes([version << 6 | (pad > 0) << 5 | (ext is not None) << 4 | cc, marker << 7 | pt]) + seq.to_bytes(2, 'big') + timestamp.to_bytes(4, 'big')
    h += ssrc.to_bytes(4, 'big') + bytes(range(4 * cc))
    if ext is not None:
        h += b'\xbe\xde' + ext.to_bytes(2, 'big') + bytes(4 * ext)
    return h + bytes(payload) + (bytes(pad - 1) + bytes([pad]) if pad else b'')


def udp(payload, family=4, src=None, dst=None, sport=5000, dport=1234, checksum=None, length=None):
    """a UDP datagram with the right checksum (a computed 0 is sent as 0xFFFF) over the pseudo-header of `family`; checksum and length
    override what is right"""
    src, dst = src or (V4_SRC if family == 4 else V6_SRC), dst or (V4_DST if family == 4 else V6_DST)
    n = 8 + len(payload)
    L = n if length is None else length
    h = bytearray(sport.to_bytes(2, 'big') + dport.to_bytes(2, 'big') + L.to_bytes(2, 'big') + b'\x00\x00') + bytes(payload)
    if checksum is None:
        pseudo = src + dst + (bytes([0, 17]) + L.to_bytes(2, 'big') if family == 4 else L.to_bytes(4, 'big') + bytes([0, 0, 0, 17]))
        checksum = (0xFFFF ^ ones_sum(pseudo + bytes(h[:n]))) or 0xFFFF
    h[6:8] = checksum.to_bytes(2, 'big')
    return bytes(h)


def ipv4(payload, src=V4_SRC, dst=V4_DST, proto=17, options=b'', frag=0, total_length=None, checksum=None, ttl=64):
    hl = 20 + len(options)
    tl = hl + len(payload) if total_length is None else total_length
    h = bytearray([0x40 | hl // 4, 0, tl >> 8, tl & 255, 0, 0, frag >> 8, frag & 255, ttl, proto, 0, 0]) + src + dst + bytes(options)
    h[10:12] = ((0xFFFF ^ ones_sum(h)) if checksum is None else checksum).to_bytes(2, 'big')
    return bytes(h) + bytes(payload)


def ipv6(payload, src=V6_SRC, dst=V6_DST, next_header=17, payload_length=None):
    pl = len(payload) if payload_length is None else payload_length
    return bytes([0x60, 0, 0, 0, pl >> 8, pl & 255, next_header, 64]) + src + dst + bytes(payload)


def datagram(payload, family=4, dport=1234, dst=None, **kw):
    """payload in UDP in IPv4 / IPv6 to the builders' default addresses; kw goes to udp()"""
    if family == 4:
        return ipv4(udp(payload, 4, dst=dst, dport=dport, **kw), dst=dst or V4_DST)
    return ipv6(udp(payload, 6, dst=dst, dport=dport, **kw), dst=dst or V6_DST)


def lay(datagrams, shift=0, gap=0, seed=0):
    """datagrams (bytes, or None: not delivered) back to back behind `shift` bytes, `gap`: up to that many random bytes between them ->
    (data uint8, table int32 [n, 2])"""
    rng = np.random.default_rng(seed)
    buf, tab = bytearray(rng.integers(0, 256, shift, dtype=np.uint8).tobytes()), []
    for d in datagrams:
        if d is None:
            tab.append((-1, 0))
            continue
        tab.append((len(buf), len(d)))
        buf += d
        if gap:
            buf += rng.integers(0, 256, int(rng.integers(0, gap + 1)), dtype=np.uint8).tobytes()
    return np.frombuffer(bytes(buf), np.uint8), np.array(tab, np.int32).reshape(-1, 2)
