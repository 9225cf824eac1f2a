"""Python model of the MPE bank's rules (include/dvbs2gpu.h, MPE bank): the sequential definition, packet by packet, written from the
header comment, with its own CRC-32/MPEG and internet checksum, both pinned to published values below.  With it builders of
datagram_sections, LLC/SNAP headers, IPv4 / IPv6 / UDP / TCP datagrams and a pointer-field packetiser (tests/t2mi_ref.py's, which sets
PUSI wherever a unit starts).  The yardstick of the bank's tests."""
import numpy as np

from psi_ref import TS, packet
from t2mi_ref import Packetiser  # noqa: F401  (the tests lay sections with it)

SLOTS = 4
OTHER_TABLE, MALFORMED, CRC_ERROR, UNCHECKED, SCRAMBLED, FILTERED, FRAGMENT, OTHER_PROTOCOL, BAD_IP, DATAGRAM = (1 << k for k in range(10))
STAT_KEYS = ('packets', 'sections', 'other_table', 'crc_errors', 'unchecked', 'scrambled_sections', 'filtered', 'fragments', 'other_protocol', 'bad_ip',
             'datagrams', 'datagrams_delivered', 'bytes_delivered', 'dropped_sections', 'malformed_sections', 'malformed_packets', 'scrambled_packets')
ROW_KEYS = ('flags', 'family', 'protocol', 'mac', 'section_number', 'last_section_number', 'src_port', 'dst_port', 'src4', 'dst4', 'length', 'offset',
            'bytes', 'first_packet', 'last_packet', 'ethertype', 'stuffing')
# the syntax the model relies on, from memory of EN 301 192, RFC 791, RFC 8200 and RFC 1042 (dvbs2gpu_mpe_layout)
LAYOUT = dict(header_bytes=3, length_mask=0x0FFF, max_section_length=4093, max_section_bytes=4096, table_id=0x3E, mpe_header_bytes=12, crc_bytes=4,
              min_section_bytes=16, mac_at=[11, 10, 9, 8, 4, 3], flags_at=5, section_number_at=6, last_section_number_at=7, llc_snap_bytes=8, ethertype_at=6,
              ethertype_ipv4=0x0800, ethertype_ipv6=0x86DD, ipv4_min_header=20, ipv4_total_length_at=2, ipv4_fragment_at=6, ipv4_protocol_at=9,
              ipv4_src_at=12, ipv4_dst_at=16, ipv6_header=40, ipv6_payload_length_at=4, ipv6_next_header_at=6, head_bytes=84)
ZERO = bytes(6)


def _crc_table():
    t = []
    for i in range(256):
        c = i << 24
        for _ in range(8):
            c = ((c << 1) ^ 0x04C11DB7 if c & 0x80000000 else c << 1) & 0xFFFFFFFF
        t.append(c)
    return t


_CRC_TABLE = _crc_table()


def crc32_mpeg(data, crc=0xFFFFFFFF):
    for b in bytes(data):
        crc = ((crc << 8) & 0xFFFFFFFF) ^ _CRC_TABLE[(crc >> 24) ^ b]
    return crc


def ones_sum(data):
    """the ones'-complement sum of big-endian 16-bit words, carries folded in (an odd last byte is the high half of a word)"""
    data = bytes(data) + bytes(len(data) & 1)
    s = sum(data[i] << 8 | data[i + 1] for i in range(0, len(data), 2))
    while s >> 16:
        s = (s & 0xFFFF) + (s >> 16)
    return s


def inet_checksum(data):
    return ones_sum(data) ^ 0xFFFF


# the two published anchors: the check value of CRC-32/MPEG-2, and the header checksum of the IPv4 example that the textbooks carry
assert crc32_mpeg(b'123456789') == 0x0376E6E7
assert inet_checksum(bytes.fromhex('450000730000400040110000c0a80001c0a800c7')) == 0xB861
assert ones_sum(bytes.fromhex('45000073000040004011b861c0a80001c0a800c7')) == 0xFFFF


def row_of(b, mac_value=ZERO, mac_mask=ZERO):
    """the row of an emitted section `b` but for offset, first_packet and last_packet -> (row, where the datagram starts or None)"""
    total = len(b)
    row = dict(flags=0, family=0, protocol=0, mac=ZERO, section_number=0, last_section_number=0, src_port=0, dst_port=0, src4=0, dst4=0, length=total,
               offset=-1, bytes=0, first_packet=-1, last_packet=-1, ethertype=0, stuffing=0)

    def end(flag):
        row['flags'] |= flag
        return row, None

    if b[0] != 0x3E:
        return end(OTHER_TABLE)
    if total < 16:
        return end(MALFORMED)
    if b[1] >> 7:
        if crc32_mpeg(b) != 0:
            return end(CRC_ERROR)
    else:
        row['flags'] |= UNCHECKED
    mac = bytes([b[11], b[10], b[9], b[8], b[4], b[3]])
    row.update(mac=mac, section_number=b[6], last_section_number=b[7])
    if b[5] >> 4 & 3 or b[5] >> 2 & 3:
        return end(SCRAMBLED)
    if any((m ^ v) & k for m, v, k in zip(mac, mac_value, mac_mask)):
        return end(FILTERED)
    if b[6] or b[7]:
        return end(FRAGMENT)
    body = b[12:total - 4]
    at = 12
    if b[5] >> 1 & 1:
        if len(body) < 8 or body[:6] != b'\xaa\xaa\x03\x00\x00\x00':
            return end(OTHER_PROTOCOL)
        row['ethertype'] = body[6] << 8 | body[7]
        family = {0x0800: 4, 0x86DD: 6}.get(row['ethertype'], 0)
        body, at = body[8:], 20
    else:
        family = body[0] >> 4 if body else 0
    if family not in (4, 6):
        return end(OTHER_PROTOCOL)
    avail = len(body)
    if family == 4:
        if avail < 20:
            return end(BAD_IP)
        hl, tl = 4 * (body[0] & 15), body[2] << 8 | body[3]
        if hl < 20 or hl > avail or not hl <= tl <= avail or ones_sum(body[:hl]) != 0xFFFF:
            return end(BAD_IP)
        row.update(family=4, bytes=tl, stuffing=avail - tl, protocol=body[9], src4=int.from_bytes(body[12:16], 'big'), dst4=int.from_bytes(body[16:20], 'big'))
        ports = hl if (body[6] << 8 | body[7]) & 0x1FFF == 0 and tl >= hl + 4 else None
    else:
        if avail < 40 or 40 + (body[4] << 8 | body[5]) > avail:
            return end(BAD_IP)
        pl = body[4] << 8 | body[5]
        row.update(family=6, bytes=40 + pl, stuffing=avail - 40 - pl, protocol=body[6])
        ports = 40 if pl >= 4 else None
    if ports is not None and row['protocol'] in (6, 17):
        row.update(src_port=body[ports] << 8 | body[ports + 1], dst_port=body[ports + 2] << 8 | body[ports + 3])
    row['flags'] |= DATAGRAM
    return row, at


_COUNTER_OF = {OTHER_TABLE: 'other_table', MALFORMED: 'malformed_sections', CRC_ERROR: 'crc_errors', UNCHECKED: 'unchecked', SCRAMBLED: 'scrambled_sections',
               FILTERED: 'filtered', FRAGMENT: 'fragments', OTHER_PROTOCOL: 'other_protocol', BAD_IP: 'bad_ip', DATAGRAM: 'datagrams'}


class Slot:
    """one slot of one stream: a complete reassembler"""

    def __init__(self, pid=-1, mac=None, mask=None):
        self.pid = pid
        self.mac, self.mask = (bytes(mac or ZERO), bytes(mask or ZERO)) if pid >= 0 else (ZERO, ZERO)
        self.seen, self.last, self.dup = False, 0, False
        self.buf, self.first = bytearray(), -1
        self.st = dict.fromkeys(STAT_KEYS, 0)
        self.table = []

    def _step(self, afc, cc, di):
        """the TS monitor's automaton -> 'first', 'disc', 'ok', 'dup' or 'err'"""
        if not self.seen:
            self.seen, self.last, self.dup = True, cc, False
            return 'first'
        last, dup = self.last, self.dup
        self.last, self.dup = cc, False
        if di:
            return 'disc'
        if not afc & 1:
            return 'err' if cc != last else 'ok'
        if cc == (last + 1) & 15:
            return 'ok'
        if cc == last and not dup:
            self.dup = True
            return 'dup'
        return 'err'

    def _drop(self):
        if self.buf:
            self.st['dropped_sections'] += 1
        self.buf = bytearray()

    def _emit(self, k, out):
        b, st = bytes(self.buf), self.st
        st['sections'] += 1
        row, at = row_of(b, self.mac, self.mask)
        row.update(first_packet=self.first, last_packet=k)
        for flag, key in _COUNTER_OF.items():
            st[key] += bool(row['flags'] & flag)
        if at is not None and out is not None:
            row['offset'] = len(out)
            out += b[at:at + row['bytes']]
            st['datagrams_delivered'] += 1
            st['bytes_delivered'] += row['bytes']
        self.table.append(row)

    def _feed(self, data, k, out):
        """-> ('done' | 'open' | 'bad', bytes used)"""
        n, buf = 0, self.buf
        while n < len(data):
            if len(buf) < 3:
                buf.append(data[n])
                n += 1
                if len(buf) < 3:
                    continue
                if (buf[1] << 8 | buf[2]) & 0x0FFF > 4093:
                    self.st['malformed_sections'] += 1
                    self.buf = bytearray()
                    return 'bad', n
            else:
                take = min(3 + ((buf[1] << 8 | buf[2]) & 0x0FFF) - len(buf), len(data) - n)
                buf += data[n:n + take]
                n += take
            if len(buf) == 3 + ((buf[1] << 8 | buf[2]) & 0x0FFF):
                self._emit(k, out)
                self.buf = bytearray()
                return 'done', n
        return 'open', n

    def process(self, ts, deliver=True):
        """ts: uint8, whole packets -> the delivered datagrams back to back (numpy uint8; None with deliver=False); self.table: the rows"""
        ts = np.asarray(ts, np.uint8).reshape(-1, TS)
        out = bytearray() if deliver else None
        self.table, self.first = [], -1
        for k, pk in enumerate(ts if self.pid >= 0 else ()):
            p = bytes(pk)
            pid = (p[1] & 0x1f) << 8 | p[2]
            if p[0] != 0x47 or p[1] >> 7 or pid == 0x1FFF or pid != self.pid:
                continue
            st = self.st
            tsc, afc, cc, pusi = p[3] >> 6, (p[3] >> 4) & 3, p[3] & 15, (p[1] >> 6) & 1
            di = p[5] >> 7 if (afc & 2) and p[4] > 0 else 0
            st['packets'] += 1
            if tsc:
                st['scrambled_packets'] += 1
                self._drop()
                self._step(afc, cc, di)
                continue
            v = self._step(afc, cc, di)
            if v == 'dup':
                continue
            if v in ('err', 'disc'):
                self._drop()
            if not afc & 1:
                continue
            ps = 5 + p[4] if afc & 2 else 4
            if ps >= TS:
                st['malformed_packets'] += 1
                self._drop()
                continue
            if not pusi:
                if self.buf:
                    self._feed(p[ps:], k, out)
                continue
            ptr = p[ps]
            if ptr > TS - ps - 1:
                st['malformed_packets'] += 1
                self._drop()
                continue
            if self.buf:
                what, _ = self._feed(p[ps + 1:ps + 1 + ptr], k, out)
                if what == 'open':
                    self._drop()
            at = ps + 1 + ptr
            while at < TS and p[at] != 0xFF:
                self.first = k
                what, used = self._feed(p[at:], k, out)
                if what != 'done':
                    break
                at += used
        return None if out is None else np.frombuffer(bytes(out), np.uint8)


class Mpe:
    """one stream: four independent slots"""

    def __init__(self):
        self.slot = [Slot() for _ in range(SLOTS)]

    def set_watch(self, slot, pid, mac=None, mask=None):
        self.slot[slot] = Slot(pid, mac, mask)

    def process(self, ts, deliver=True):
        """-> per slot the delivered bytes (None with deliver=False)"""
        return [s.process(ts, deliver) for s in self.slot]

    def table(self, slot):
        return self.slot[slot].table

    def stats(self, slot=-1):
        sel = self.slot if slot < 0 else [self.slot[slot]]
        return {k: int(sum(s.st[k] for s in sel)) for k in STAT_KEYS}


# ------------------------------------------------------------------------------------------------- builders
def ipv4(payload, proto=17, src=0xC0A80001, dst=0xE0000105, options=b'', frag=0, total_length=None, checksum=None, ihl=None, ident=0, ttl=64):
    """an IPv4 datagram with a right header checksum; total_length, checksum and ihl override what is right (faults)"""
    assert len(options) % 4 == 0
    hl = 20 + len(options)
    tl = hl + len(payload) if total_length is None else total_length
    h = bytearray([0x40 | (hl // 4 if ihl is None else ihl), 0, tl >> 8, tl & 255, ident >> 8, ident & 255, frag >> 8, frag & 255, ttl, proto, 0, 0])
    h += src.to_bytes(4, 'big') + dst.to_bytes(4, 'big') + bytes(options)
    c = inet_checksum(h[:4 * (h[0] & 15)] if 4 * (h[0] & 15) <= len(h) else h) if checksum is None else checksum
    h[10], h[11] = c >> 8, c & 255
    return bytes(h) + bytes(payload)


def ipv6(payload, next_header=17, src=bytes(range(16)), dst=bytes(range(16, 32)), payload_length=None):
    pl = len(payload) if payload_length is None else payload_length
    return bytes([0x60, 0, 0, 0, pl >> 8, pl & 255, next_header, 64]) + bytes(src) + bytes(dst) + bytes(payload)


def udp(sport, dport, data):
    """a UDP header (checksum 0: none) and its data"""
    n = 8 + len(data)
    return bytes([sport >> 8, sport & 255, dport >> 8, dport & 255, n >> 8, n & 255, 0, 0]) + bytes(data)


def tcp(sport, dport, data=b''):
    return bytes([sport >> 8, sport & 255, dport >> 8, dport & 255]) + bytes(8) + bytes([0x50, 0x10, 0x20, 0x00, 0, 0, 0, 0]) + bytes(data)


def llc_snap(ethertype, llc=b'\xaa\xaa\x03\x00\x00\x00'):
    return bytes(llc) + bytes([ethertype >> 8, ethertype & 255])


def section(body, mac=b'\x01\x00\x5e\x00\x01\x05', table_id=0x3E, ssi=1, llc=0, pscr=0, ascr=0, number=0, last=0, stuffing=0, section_length=None):
    """a datagram_section around `body` (what follows the 12 header bytes: LLC/SNAP where the caller wants it, the datagram) and
    `stuffing` zero bytes, with a right CRC-32 (ssi 1) or four checksum bytes nobody verifies (ssi 0)"""
    body = bytes(body) + bytes(stuffing)
    n = 9 + len(body) + 4 if section_length is None else section_length
    assert n <= 4095
    mac = bytes(mac)
    b = bytes([table_id, ssi << 7 | 0x30 | n >> 8, n & 255, mac[5], mac[4], 0xC0 | pscr << 4 | ascr << 2 | llc << 1 | 1, number, last, mac[3], mac[2], mac[1],
               mac[0]]) + body
    return b + (crc32_mpeg(b).to_bytes(4, 'big') if ssi else b'\x13\x81\x86\x00')


def raw_section(table_id, body, ssi=0):
    """any other section of 3 + len(body) bytes"""
    return bytes([table_id, ssi << 7 | 0x30 | len(body) >> 8, len(body) & 255]) + bytes(body)


def thin_packets(pid, cc, data, per_packet=(1, 2, 3), pusi_first=True):
    """`data` in TS packets that carry one to three payload bytes each behind long adaptation fields (the first: PUSI, pointer 0)
    -> ([k, 188], the next continuity counter)"""
    out, pos, i = [], 0, 0
    while pos < len(data):
        take = per_packet[i % len(per_packet)]
        first = pusi_first and pos == 0
        body = (b'\x00' if first else b'') + data[pos:pos + take]
        cc = (cc + 1) & 15
        out.append(packet(pid, cc, body, pusi=int(first), af_len=184 - len(body) - 1))
        pos += take
        i += 1
    return np.array(out, np.uint8).reshape(-1, TS), cc
