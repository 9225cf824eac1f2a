"""Python model of the T2-MI bank's rules (include/dvbs2gpu.h, T2-MI bank): the sequential definition, packet by packet, with a
table form of the bitwise CRC-32/MPEG of tests/psi_ref.py.  With it builders of T2-MI packets and BBFRAME payloads and a pointer-field packetiser that
sets PUSI in every TS packet where a T2-MI packet starts and pads with adaptation fields (there is no stuffing rule).  The yardstick
of the bank's tests."""
import numpy as np

import psi_ref
from psi_ref import TS, packet

SLOTS = 4
CRC_ERROR, COUNT_ERROR, BBFRAME, INTL_FRAME_START, BAD_PAYLOAD = 1, 2, 4, 8, 16
STAT_KEYS = ('packets', 't2mi_packets', 'crc_errors', 'count_errors', 'bbframes', 'bad_payload', 'bbframes_delivered', 'bytes_delivered',
             'dropped_packets', 'malformed_packets', 'scrambled_packets', 'pointer_slack')
ROW_KEYS = ('packet_type', 'packet_count', 'superframe_idx', 'stream_id', 'flags', 'plp_id', 'frame_idx', 'payload_bits', 'length', 'offset',
            'bbframe_bytes', 'first_packet', 'last_packet')
# the syntax the model relies on, from memory of ETSI TS 102 773 (dvbs2gpu_t2mi_layout)
LAYOUT = dict(header_bytes=6, crc_bytes=4, min_packet_bytes=10, max_packet_bytes=8202, bbframe_type=0, bbframe_prefix_bytes=3, min_bbframe_bytes=10,
              max_bbframe_bytes=7274, stream_id_mask=7)


_CRC_TABLE = [psi_ref.crc32_mpeg(bytes([i]), 0) for i in range(256)]


def crc32_mpeg(data, crc=0xFFFFFFFF):
    """psi_ref.crc32_mpeg, a byte at a time by table (the tests feed megabytes)"""
    for b in bytes(data):
        crc = ((crc << 8) & 0xFFFFFFFF) ^ _CRC_TABLE[(crc >> 24) ^ b]
    return crc


assert all(crc32_mpeg(d) == psi_ref.crc32_mpeg(d) for d in (b'', b'123456789', bytes(range(256)) * 3))


def total_of(b4, b5):
    return 6 + (((b4 << 8 | b5) + 7) >> 3) + 4


class Slot:
    """one slot of one stream: a complete reassembler"""

    def __init__(self, pid=-1, plp=-1):
        self.pid, self.plp = pid, plp if pid >= 0 else -1
        self.seen, self.last, self.dup = False, 0, False
        self.buf, self.has_count, self.last_count, self.first = bytearray(), False, 0, -1
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
            self.st['dropped_packets'] += 1
        self.buf = bytearray()

    def _emit(self, k, out):
        b, st = bytes(self.buf), self.st
        st['t2mi_packets'] += 1
        bits = b[4] << 8 | b[5]
        row = dict(packet_type=b[0], packet_count=b[1], superframe_idx=b[2] >> 4, stream_id=b[3] & 7, flags=0, plp_id=0, frame_idx=0, payload_bits=bits,
                   length=len(b), offset=-1, bbframe_bytes=0, first_packet=self.first, last_packet=k)
        if crc32_mpeg(b) != 0:
            st['crc_errors'] += 1
            row['flags'] = CRC_ERROR
            self.table.append(row)
            return
        if self.has_count and b[1] != (self.last_count + 1) & 255:
            row['flags'] |= COUNT_ERROR
            st['count_errors'] += 1
        self.has_count, self.last_count = True, b[1]
        if b[0] == 0:
            if bits >= 24:
                row.update(frame_idx=b[6], plp_id=b[7])
            if bits < 24 + 80 or (bits - 24) % 8 or (bits - 24) // 8 > 7274:
                row['flags'] |= BAD_PAYLOAD
                st['bad_payload'] += 1
            else:
                n = (bits - 24) // 8
                row['flags'] |= BBFRAME | (INTL_FRAME_START if b[8] >> 7 else 0)
                row['bbframe_bytes'] = n
                st['bbframes'] += 1
                if out is not None and self.plp in (-1, b[7]):
                    row['offset'] = len(out)
                    out += b[9:9 + n]
                    st['bbframes_delivered'] += 1
                    st['bytes_delivered'] += n
        self.table.append(row)

    def _feed(self, data, k, out):
        """-> (emitted, bytes used)"""
        n, buf = 0, self.buf
        while n < len(data):
            want = 6 if len(buf) < 6 else total_of(buf[4], buf[5])
            take = min(want - len(buf), len(data) - n)
            buf += data[n:n + take]
            n += take
            if len(buf) >= 6 and len(buf) == total_of(buf[4], buf[5]):
                self._emit(k, out)
                self.buf = bytearray()
                return True, n
        return False, n

    def process(self, ts, deliver=True):
        """ts: uint8, whole packets -> the delivered BBFRAMEs back to back (numpy uint8; None with deliver=False); self.table: the rows"""
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
                done, used = self._feed(p[ps + 1:ps + 1 + ptr], k, out)
                if not done:
                    self._drop()
                elif used < ptr:
                    st['pointer_slack'] += 1
            at = ps + 1 + ptr
            while at < TS:
                self.first = k
                done, used = self._feed(p[at:], k, out)
                if not done:
                    break
                at += used
        return None if out is None else np.frombuffer(bytes(out), np.uint8)

    def frame_bytes(self):
        return [r['bbframe_bytes'] for r in self.table if r['offset'] >= 0]


class T2mi:
    """one stream: four independent slots"""

    def __init__(self):
        self.slot = [Slot() for _ in range(SLOTS)]

    def set_watch(self, slot, pid, plp=-1):
        self.slot[slot] = Slot(pid, plp)

    def process(self, ts, deliver=True):
        """-> per slot the delivered bytes (None with deliver=False)"""
        return [s.process(ts, deliver) for s in self.slot]

    def table(self, slot):
        return self.slot[slot].table

    def frame_bytes(self, slot):
        return self.slot[slot].frame_bytes()

    def stats(self, slot=-1):
        sel = self.slot if slot < 0 else [self.slot[slot]]
        return {k: int(sum(s.st[k] for s in sel)) for k in STAT_KEYS}


# ------------------------------------------------------------------------------------------------- builders
def t2mi_packet(ptype, count, payload, payload_bits=None, superframe=0, stream_id=0):
    """a T2-MI packet with a right CRC; payload_bits None: 8 per payload byte, else the payload is cut or zero-padded to its bytes"""
    bits = 8 * len(payload) if payload_bits is None else payload_bits
    n = (bits + 7) >> 3
    body = (bytes(payload) + bytes(n))[:n]
    b = bytes([ptype, count & 255, superframe << 4, stream_id & 7, bits >> 8, bits & 255]) + body
    return b + crc32_mpeg(b).to_bytes(4, 'big')


def bbframe_payload(frame_idx, plp, start, bbframe):
    return bytes([frame_idx & 255, plp, start << 7]) + bytes(bbframe)


def bb_packet(count, plp, bbframe, frame_idx=0, start=0, **kw):
    return t2mi_packet(0, count, bbframe_payload(frame_idx, plp, start, bbframe), **kw)


class Packetiser:
    """lays T2-MI packets of one PID into TS packets behind pointer fields; keeps the PID's continuity counter and the bytes that the
    last TS packet could not take"""

    def __init__(self, pid, cc=0):
        self.pid, self.cc = pid, cc
        self.data, self.starts = b'', []

    def _next(self):
        self.cc = (self.cc + 1) & 15
        return self.cc

    def lay(self, packets, flush=True, af_len=None):
        """the packets back to back; PUSI and a pointer in every TS packet in which one starts.  flush: the last TS packet is shortened
        by an adaptation field to end with the last byte, else whole TS packets only and the rest waits.  af_len: an adaptation field
        of that length in every TS packet that is not shortened anyway -> [k, 188]"""
        for p in packets:
            self.starts.append(len(self.data))
            self.data += bytes(p)
        base = 184 if af_len is None else 183 - af_len
        out, pos = [], 0
        while pos < len(self.data):
            first = next((s for s in self.starts if pos <= s < pos + base), None)
            pusi = first is not None and first < pos + base - 1
            room = base - 1 if pusi else (base - 1 if first is not None else base)   # a start in the last byte of a PUSI-less packet: end it before
            take = min(room, len(self.data) - pos)
            if take < room and not flush:
                break
            body = (bytes([first - pos]) if pusi else b'') + self.data[pos:pos + take]
            af = af_len if len(body) == base else 184 - len(body) - 1
            out.append(packet(self.pid, self._next(), body, pusi=int(pusi), af_len=None if len(body) == 184 else af))
            pos += take
        self.data, self.starts = self.data[pos:], [s - pos for s in self.starts if s >= pos]
        return np.array(out, np.uint8).reshape(-1, TS)
