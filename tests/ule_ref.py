"""Python model of the ULE bank's rules (include/dvbs2gpu.h, ULE bank): the sequential definition, packet by packet, written from the
header comment.  Its CRC-32/MPEG and internet checksum are tests/mpe_ref.py's, pinned there to published check values (and asserted
again below); the IPv4 / IPv6 / UDP builders are that file's too.  With it builders of SNDUs, optional extension headers and bridged
frames, and a ULE packetiser: payload pointer, packing, End Indicator and 0xFF padding, headers split over two TS packets.  The
yardstick of the bank's tests."""
import numpy as np

from mpe_ref import crc32_mpeg, inet_checksum, ipv4, ipv6, ones_sum, tcp, udp  # noqa: F401  (the tests build datagrams with them)
from psi_ref import TS, packet
from t2mi_ref import Packetiser as _Packed

assert crc32_mpeg(b'123456789') == 0x0376E6E7
assert inet_checksum(bytes.fromhex('450000730000400040110000c0a80001c0a800c7')) == 0xB861

SLOTS = 4
MALFORMED, CRC_ERROR, FILTERED, NO_ADDRESS, TEST, BRIDGED, EXTENSION, OTHER_PROTOCOL, BAD_IP, DATAGRAM = (1 << k for k in range(10))
STAT_KEYS = ('packets', 'sndus', 'crc_errors', 'filtered', 'no_address', 'test', 'bridged', 'extension', 'other_protocol', 'bad_ip', 'datagrams',
             'datagrams_delivered', 'bytes_delivered', 'dropped_sndus', 'malformed_sndus', 'slack', 'malformed_packets', 'scrambled_packets')
ROW_KEYS = ('flags', 'family', 'protocol', 'mac', 'ip_at', 'extension_bytes', 'src_port', 'dst_port', 'src4', 'dst4', 'length', 'offset', 'bytes', 'first_packet',
            'last_packet', 'ethertype', 'stuffing')
# the syntax the model relies on, from memory of RFC 4326, RFC 5163, RFC 791 and RFC 8200 (dvbs2gpu_ule_layout)
LAYOUT = dict(header_bytes=4, length_bytes=2, d_bit=0x80, length_mask=0x7FFF, max_length=4092, max_sndu_bytes=4096, type_at=2, npa_bytes=6, crc_bytes=4,
              min_length_d1=4, min_length_d0=10, type_test=0, type_bridged=1, type_ts_concat=2, type_priv_concat=3, ethertype_floor=1536, hlen_shift=8, hlen_mask=7,
              max_hlen=5, max_extension_bytes=40, mac_header_bytes=14, bridged_ethertype_at=12, ethertype_ipv4=0x0800, ethertype_ipv6=0x86DD, ipv4_min_header=20,
              ipv4_total_length_at=2, ipv4_fragment_at=6, ipv4_protocol_at=9, ipv4_src_at=12, ipv4_dst_at=16, ipv6_header=40, ipv6_payload_length_at=4,
              ipv6_next_header_at=6, head_bytes=128)
ZERO = bytes(6)


def _total(b0, b1):
    """an SNDU's bytes from its first two, None: the bad length"""
    n = (b0 << 8 | b1) & 0x7FFF
    return None if n > 4092 else 4 + n


def row_of(b, npa_value=ZERO, npa_mask=ZERO, accept_unaddressed=False):
    """the row of an emitted SNDU `b` but for offset, first_packet and last_packet -> (row, where the datagram starts or None)"""
    total = len(b)
    row = dict(flags=0, family=0, protocol=0, mac=ZERO, ip_at=0, extension_bytes=0, src_port=0, dst_port=0, src4=0, dst4=0, length=total, offset=-1, bytes=0,
               first_packet=-1, last_packet=-1, ethertype=0, stuffing=0)

    def end(flag, **kw):
        row['flags'] |= flag
        row.update(kw)
        return row, None

    d = b[0] >> 7
    if total - 4 < (4 if d else 10):                               # 1
        return end(MALFORMED)
    if crc32_mpeg(b) != 0:                                         # 2
        return end(CRC_ERROR)
    if d:                                                          # 3
        row['flags'] |= NO_ADDRESS
        at = 4
        if not accept_unaddressed:
            return end(FILTERED)
    else:
        row['mac'] = bytes(b[4:10])
        at = 10
        if any((m ^ v) & k for m, v, k in zip(row['mac'], npa_value, npa_mask)):
            return end(FILTERED)
    stop = total - 4
    typ, ext = b[2] << 8 | b[3], 0
    while typ < 1536 and typ >> 8 & 7:                             # 4
        n = 2 * (typ >> 8 & 7)
        ext += n
        if ext > 40 or at + n > stop:
            return end(EXTENSION, ethertype=typ)
        at += n
        typ = b[at - 2] << 8 | b[at - 1]
    row['extension_bytes'] = ext
    if typ < 1536:                                                 # 5
        if typ == 0:
            return end(TEST)
        if typ != 1 or stop - at < 14:
            return end(EXTENSION, ethertype=typ)
        row['flags'] |= BRIDGED
        if d:
            row['mac'] = bytes(b[at:at + 6])
        typ = b[at + 12] << 8 | b[at + 13]
        at += 14
    row['ethertype'] = typ                                         # 6
    body = b[at:stop]
    avail = len(body)
    if typ == 0x0800:                                              # 7 to 9: the IP rules, the MPE bank's too
        if avail < 20:
            return end(BAD_IP)
        hl, tl = 4 * (body[0] & 15), body[2] << 8 | body[3]
        if hl < 20 or hl > avail or not hl <= tl <= avail or ones_sum(body[:hl]) != 0xFFFF:
            return end(BAD_IP)
        row.update(family=4, bytes=tl, stuffing=avail - tl, protocol=body[9], src4=int.from_bytes(body[12:16], 'big'), dst4=int.from_bytes(body[16:20], 'big'))
        ports = hl if (body[6] << 8 | body[7]) & 0x1FFF == 0 and tl >= hl + 4 else None
    elif typ == 0x86DD:
        if avail < 40 or 40 + (body[4] << 8 | body[5]) > avail:
            return end(BAD_IP)
        pl = body[4] << 8 | body[5]
        row.update(family=6, bytes=40 + pl, stuffing=avail - 40 - pl, protocol=body[6])
        ports = 40 if pl >= 4 else None
    else:
        return end(OTHER_PROTOCOL)
    if ports is not None and row['protocol'] in (6, 17):
        row.update(src_port=body[ports] << 8 | body[ports + 1], dst_port=body[ports + 2] << 8 | body[ports + 3])
    row['flags'] |= DATAGRAM
    row['ip_at'] = at
    return row, at


_COUNTER_OF = {MALFORMED: 'malformed_sndus', CRC_ERROR: 'crc_errors', FILTERED: 'filtered', NO_ADDRESS: 'no_address', TEST: 'test', BRIDGED: 'bridged',
               EXTENSION: 'extension', OTHER_PROTOCOL: 'other_protocol', BAD_IP: 'bad_ip', DATAGRAM: 'datagrams'}


class Slot:
    """one slot of one stream: a complete reassembler"""

    def __init__(self, pid=-1, npa=None, mask=None, accept_unaddressed=False):
        self.pid = pid
        self.npa, self.mask = (bytes(npa or ZERO), bytes(mask or ZERO)) if pid >= 0 else (ZERO, ZERO)
        self.accept = bool(accept_unaddressed) and pid >= 0
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
            self.st['dropped_sndus'] += 1
        self.buf = bytearray()

    def _emit(self, k, out):
        b, st = bytes(self.buf), self.st
        st['sndus'] += 1
        row, at = row_of(b, self.npa, self.mask, self.accept)
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
            if len(buf) < 2:
                buf.append(data[n])
                n += 1
                if len(buf) < 2:
                    continue
                if _total(buf[0], buf[1]) is None:
                    self.st['malformed_sndus'] += 1
                    self.buf = bytearray()
                    return 'bad', n
            else:
                take = min(_total(buf[0], buf[1]) - len(buf), len(data) - n)
                buf += data[n:n + take]
                n += take
            if len(buf) == _total(buf[0], buf[1]):
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
                what, used = self._feed(p[ps + 1:ps + 1 + ptr], k, out)
                if what == 'open':
                    self._drop()
                elif what == 'done' and used < ptr:
                    st['slack'] += 1
            at = ps + 1 + ptr
            while at < TS and p[at] != 0xFF:
                self.first = k
                what, used = self._feed(p[at:], k, out)
                if what != 'done':
                    break
                at += used
        return None if out is None else np.frombuffer(bytes(out), np.uint8)


class Ule:
    """one stream: four independent slots"""

    def __init__(self):
        self.slot = [Slot() for _ in range(SLOTS)]

    def set_watch(self, slot, pid, npa=None, mask=None, accept_unaddressed=False):
        self.slot[slot] = Slot(pid, npa, mask, accept_unaddressed)

    def process(self, ts, deliver=True):
        """-> per slot the delivered bytes (None with deliver=False)"""
        return [s.process(ts, deliver) for s in self.slot]

    def table(self, slot):
        return self.slot[slot].table

    def stats(self, slot=-1):
        sel = self.slot if slot < 0 else [self.slot[slot]]
        return {k: int(sum(s.st[k] for s in sel)) for k in STAT_KEYS}


# ------------------------------------------------------------------------------------------------- builders
def sndu(typ, body, npa=None, length=None, crc=None):
    """an SNDU of Type `typ` around `body` (what follows the Type field and the NPA: extension headers, a MAC header, the PDU), to the
    address `npa` (None: D = 1, none), with a right CRC-32; length and crc override what is right (faults)"""
    body = (b'' if npa is None else bytes(npa)) + bytes(body)
    n = len(body) + 4 if length is None else length
    assert n <= 0x7FFF
    b = bytes([(npa is None) << 7 | n >> 8, n & 255, typ >> 8, typ & 255]) + body
    return b + (crc32_mpeg(b) if crc is None else crc).to_bytes(4, 'big')


def extended(headers, typ, body):
    """optional extension headers in front of (typ, body): headers = [(H-LEN 1..5, H-Type 0..255, the 2 H-LEN - 2 bytes of the header)]
    -> (the Type for the base header, the body)"""
    out, first = b'', None
    for i, (hlen, htype, data) in enumerate(headers):
        assert 1 <= hlen <= 5 and len(data) == 2 * hlen - 2
        t = hlen << 8 | htype
        if first is None:
            first = t
        else:
            out += bytes([t >> 8, t & 255])
        out += bytes(data)
    if first is None:
        return typ, bytes(body)
    return first, out + bytes([typ >> 8, typ & 255]) + bytes(body)


def bridged(ethertype, payload, dst=b'\x01\x00\x5e\x00\x01\x05', src=b'\x02\x00\x00\x00\x00\x09'):
    """a bridged frame -> (Type 0x0001, MAC header and payload)"""
    return 1, bytes(dst) + bytes(src) + bytes([ethertype >> 8, ethertype & 255]) + bytes(payload)


class Packetiser(_Packed):
    """lays SNDUs of one PID into TS packets as RFC 4326 packs them: back to back, PUSI and a payload pointer in every TS packet in
    which an SNDU starts (tests/t2mi_ref.py's packing, which keeps the continuity counter and the bytes that the last TS packet could not
    take -- a base header split after 1, 2 or 3 bytes comes about by the sizes alone)"""

    def lay(self, sndus, flush=True, af_len=None, pad=False):
        """pad False: as tests/t2mi_ref.py's lay() (flush: the last TS packet is shortened by an adaptation field to end with the last
        byte; else whole TS packets only and the rest waits).  pad True: the last TS packet is filled with 0xFF behind the last SNDU --
        the End Indicator 0xFFFF and padding, or a single 0xFF where one byte is left -> [k, 188]"""
        if not pad:
            return super().lay(sndus, flush=flush, af_len=af_len)
        out = [super().lay(sndus, flush=False, af_len=af_len)]
        if self.data:
            base = 184 if af_len is None else 183 - af_len
            first = self.starts[0] if self.starts else None
            body = (b'' if first is None else bytes([first])) + self.data
            assert len(body) <= base
            body += b'\xff' * (base - len(body))
            out.append(np.array(packet(self.pid, self._next(), body, pusi=int(first is not None), af_len=af_len), np.uint8).reshape(1, TS))
            self.data, self.starts = b'', []
        return np.concatenate(out)


def thin_packets(pid, cc, data, per_packet=(1,), pusi_first=True):
    """`data` in TS packets that carry per_packet[i] payload bytes each behind long adaptation fields (the first: PUSI, pointer 0)
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
