"""Python model of the PSI section bank's rules (include/dvbs2gpu.h, PSI section bank): the sequential definition, packet by packet,
with its own bitwise CRC-32/MPEG.  With it builders of PAT, PMT and generic sections, a packetiser that lays sections into TS packets
with a chosen pointer field, stuffing, adaptation fields and other PIDs in between, and fault injectors that say what each fault must
cost.  The yardstick of the bank's tests."""
import numpy as np

TS = 188
SLOTS = 16
CRC_ERROR, CHANGED = 1, 2
STAT_KEYS = ('packets', 'sections', 'valid', 'changed', 'crc_errors', 'dropped_sections', 'malformed_sections', 'malformed_packets',
             'scrambled_packets', 'unexpected_table_id', 'bytes_delivered')
ROW_KEYS = ('pid', 'flags', 'table_id', 'ssi', 'version', 'current_next', 'section_number', 'last_section_number', 'table_id_ext', 'length',
            'offset', 'first_packet')
# the section syntax the model relies on, from memory of ISO/IEC 13818-1 2.4.4 (dvbs2gpu_psi_layout)
LAYOUT = dict(header_bytes=3, length_mask=0x0FFF, max_section_length=4093, max_section_bytes=4096, min_long_section=12, ext_at=3, version_at=5,
              section_number_at=6, last_section_number_at=7, long_header_bytes=8, crc_bytes=4, pat_loop_at=8, pat_stride=4, pmt_pcr_at=8,
              pmt_info_length_at=10, pmt_loop_at=12, pmt_stride=5)


def crc32_mpeg(data, crc=0xFFFFFFFF):
    for b in bytes(data):
        crc ^= b << 24
        for _ in range(8):
            crc = ((crc << 1) ^ 0x04C11DB7 if crc & 0x80000000 else crc << 1) & 0xFFFFFFFF
    return crc


assert crc32_mpeg(b'123456789') == 0x0376E6E7                     # the published check value of CRC-32/MPEG-2


class Assembler:
    """one stream"""

    def __init__(self):
        self.watch = [[-1, -1] for _ in range(SLOTS)]
        self.watch[0] = [0, 0]
        self.deliver = 0
        self.slot = [self._fresh() for _ in range(SLOTS)]
        self.st = [dict.fromkeys(STAT_KEYS, 0) for _ in range(SLOTS)]
        self.view = [None] * SLOTS
        self.table = []

    @staticmethod
    def _fresh():
        return dict(seen=False, last=0, dup=False, buf=bytearray(), has=False, last4=0, first=-1)

    def set_watch(self, slot, pid, expect=-1):
        self.watch[slot] = [pid, expect if pid >= 0 else -1]
        self.slot[slot], self.st[slot], self.view[slot] = self._fresh(), dict.fromkeys(STAT_KEYS, 0), None

    def _step(self, s, afc, cc, di):
        """the TS monitor's automaton -> 'first', 'disc', 'ok', 'dup' or 'err'"""
        if not s['seen']:
            s.update(seen=True, last=cc, dup=False)
            return 'first'
        last, dup = s['last'], s['dup']
        s.update(last=cc, dup=False)
        if di:
            return 'disc'
        if not afc & 1:
            return 'err' if cc != last else 'ok'
        if cc == (last + 1) & 15:
            return 'ok'
        if cc == last and not dup:
            s['dup'] = True
            return 'dup'
        return 'err'

    def _drop(self, i):
        if self.slot[i]['buf']:
            self.st[i]['dropped_sections'] += 1
        self.slot[i]['buf'] = bytearray()

    def _emit(self, i, out):
        s, st, b = self.slot[i], self.st[i], bytes(self.slot[i]['buf'])
        ssi = b[1] >> 7
        if ssi and len(b) < LAYOUT['min_long_section']:
            st['malformed_sections'] += 1
            return
        st['sections'] += 1
        if self.watch[i][1] >= 0 and b[0] != self.watch[i][1]:
            st['unexpected_table_id'] += 1
        valid = not ssi or crc32_mpeg(b) == 0
        flags = 0
        if not valid:
            st['crc_errors'] += 1
            flags |= CRC_ERROR
        else:
            st['valid'] += 1
            l4 = int.from_bytes(b[-4:], 'big')
            if not s['has'] or l4 != s['last4']:
                flags |= CHANGED
                st['changed'] += 1
            s['has'], s['last4'] = True, l4
        row = dict(pid=self.watch[i][0], flags=flags, table_id=b[0], ssi=ssi, version=0, current_next=0, section_number=0, last_section_number=0,
                   table_id_ext=0, length=len(b), offset=-1, first_packet=s['first'])
        if ssi:
            row.update(table_id_ext=b[3] << 8 | b[4], version=(b[5] >> 1) & 31, current_next=b[5] & 1, section_number=b[6], last_section_number=b[7])
        if flags & CHANGED and ssi and b[0] in (0, 2) and b[5] & 1:
            self.view[i] = b
        if out is not None and (self.deliver == 0 or flags & CHANGED):
            row['offset'] = len(out)
            out += b
            st['bytes_delivered'] += len(b)
        self.table.append(row)

    def _feed(self, i, data, out):
        """-> ('open' | 'done' | 'bad', bytes used)"""
        s, n = self.slot[i], 0
        for n, byte in enumerate(data, 1):
            s['buf'].append(byte)
            b = s['buf']
            if len(b) < 3:
                continue
            sl = ((b[1] & 0x0F) << 8) | b[2]
            if sl > LAYOUT['max_section_length']:
                self.st[i]['malformed_sections'] += 1
                s['buf'] = bytearray()
                return 'bad', n
            if len(b) == 3 + sl:
                self._emit(i, out)
                s['buf'] = bytearray()
                return 'done', n
        return 'open', n

    def process(self, ts, deliver=True):
        """ts: uint8, whole packets -> the delivered bytes (numpy uint8; None with deliver=False); self.table: the call's rows"""
        ts = np.asarray(ts, np.uint8).reshape(-1, TS)
        out = bytearray() if deliver else None
        self.table = []
        for s in self.slot:
            s['first'] = -1
        pids = {w[0]: i for i, w in enumerate(self.watch) if w[0] >= 0}
        for k, pk in enumerate(ts):
            p = bytes(pk)
            pid = (p[1] & 0x1f) << 8 | p[2]
            if p[0] != 0x47 or p[1] >> 7 or pid == 0x1FFF or pid not in pids:
                continue
            i = pids[pid]
            s, st = self.slot[i], self.st[i]
            tsc, afc, cc, pusi = p[3] >> 6, (p[3] >> 4) & 3, p[3] & 15, (p[1] >> 6) & 1
            di = p[5] >> 7 if (afc & 2) and p[4] > 0 else 0
            st['packets'] += 1
            if tsc:
                st['scrambled_packets'] += 1
                self._drop(i)
                self._step(s, afc, cc, di)
                continue
            v = self._step(s, afc, cc, di)
            if v == 'dup':
                continue
            if v in ('err', 'disc'):
                self._drop(i)
            if not afc & 1:
                continue
            ps = 5 + p[4] if afc & 2 else 4
            if ps >= TS:
                st['malformed_packets'] += 1
                self._drop(i)
                continue
            if not pusi:
                if s['buf']:
                    self._feed(i, p[ps:], out)
                continue
            ptr = p[ps]
            if ptr > TS - ps - 1:
                st['malformed_packets'] += 1
                self._drop(i)
                continue
            if s['buf'] and self._feed(i, p[ps + 1:ps + 1 + ptr], out)[0] == 'open':
                self._drop(i)
            at = ps + 1 + ptr
            while at < TS and p[at] != 0xFF:
                s['first'] = k
                res, used = self._feed(i, p[at:], out)
                if res != 'done':
                    break
                at += used
        return None if out is None else np.frombuffer(bytes(out), np.uint8)

    def stats(self, slot=-1):
        sel = self.st if slot < 0 else [self.st[slot]]
        return {k: int(sum(s[k] for s in sel)) for k in STAT_KEYS}

    def programs(self):
        for b in self.view:
            if b is not None and b[0] == 0:
                return parse_pat(b)
        return dict(transport_stream_id=-1, version=-1, malformed=0), []

    def program_map(self, slot):
        b = self.view[slot]
        if b is None or b[0] != 2:
            return dict(program_number=-1, version=-1, pcr_pid=-1, malformed=0), []
        return parse_pmt(b)


def parse_pat(b):
    hdr = dict(transport_stream_id=b[3] << 8 | b[4], version=(b[5] >> 1) & 31, malformed=0)
    end = len(b) - 4
    if (end - 8) % 4:
        return dict(hdr, malformed=1), []
    return hdr, [(b[i] << 8 | b[i + 1], (b[i + 2] & 0x1f) << 8 | b[i + 3]) for i in range(8, end, 4)]


def parse_pmt(b):
    if len(b) < 16:
        return dict(program_number=-1, version=-1, pcr_pid=-1, malformed=1), []
    hdr = dict(program_number=b[3] << 8 | b[4], version=(b[5] >> 1) & 31, pcr_pid=(b[8] & 0x1f) << 8 | b[9], malformed=0)
    end, rows = len(b) - 4, []
    i = 12 + ((b[10] & 0x0f) << 8 | b[11])
    while i < end:
        if i + 5 > end:
            break
        e = (b[i], (b[i + 1] & 0x1f) << 8 | b[i + 2])
        i += 5 + ((b[i + 3] & 0x0f) << 8 | b[i + 4])
        if i > end:
            break
        rows.append(e)
    if i != end:
        return dict(hdr, malformed=1), []
    return hdr, rows


# ------------------------------------------------------------------------------------------------- builders
def long_section(table_id, ext, body, version=0, current_next=1, number=0, last=0, private=0):
    """a section with section_syntax_indicator and a right CRC; body: the bytes between the long header and the CRC"""
    n = 5 + len(body) + 4
    assert n <= 4093
    b = bytes([table_id, 0x80 | private << 6 | 0x30 | n >> 8, n & 255, ext >> 8, ext & 255, 0xC0 | version << 1 | current_next, number, last]) + bytes(body)
    return b + crc32_mpeg(b).to_bytes(4, 'big')


def short_section(table_id, body):
    assert len(body) <= 4093
    return bytes([table_id, 0x30 | len(body) >> 8, len(body) & 255]) + bytes(body)


def pat(tsid, programs, version=0, current_next=1):
    """programs: [(program_number, pid)]"""
    body = b''.join(bytes([n >> 8, n & 255, 0xE0 | p >> 8, p & 255]) for n, p in programs)
    return long_section(0, tsid, body, version, current_next)


def pmt(program, pcr_pid, streams, version=0, program_info=b'', es_info=b'', es_info_length=None):
    """streams: [(stream_type, pid)]; es_info_length overrides the length field of the LAST stream (a fault)"""
    body = bytes([0xE0 | pcr_pid >> 8, pcr_pid & 255, 0xF0 | len(program_info) >> 8, len(program_info) & 255]) + bytes(program_info)
    for i, (t, p) in enumerate(streams):
        n = es_info_length if es_info_length is not None and i == len(streams) - 1 else len(es_info)
        body += bytes([t, 0xE0 | p >> 8, p & 255, 0xF0 | n >> 8, n & 255]) + bytes(es_info)
    return long_section(2, program, body, version)


def packet(pid, cc, payload=b'', pusi=0, af_len=None, tsc=0, di=0, fill=0xFF):
    """one TS packet: af_len None no adaptation field, else adaptation_field_length; the payload is padded with `fill`.  An adaptation
    field that leaves no room makes AFC 3 without payload (the fault of rule 3) unless payload is None (AFC 2)."""
    afc = (0 if payload is None else 1) | (0 if af_len is None else 2)
    p = bytearray([0x47, pusi << 6 | pid >> 8, pid & 255, tsc << 6 | afc << 4 | cc & 15])
    if af_len is not None:
        p.append(af_len)
        if af_len > 0:
            p += bytes([di << 7]) + b'\xff' * (af_len - 1)
    p = p[:TS]
    room = TS - len(p)
    body = bytes(payload or b'')[:room]
    return np.frombuffer(bytes(p + body + bytes([fill]) * (room - len(body))), np.uint8)


class Packetiser:
    """lays sections of one PID into packets; keeps the PID's continuity counter"""

    def __init__(self, pid, cc=0):
        self.pid, self.cc = pid, cc

    def _next(self):
        self.cc = (self.cc + 1) & 15
        return self.cc

    def lay(self, sections, pointer=0, before=b'', af_len=None, stuffing=True, cont_af=None):
        """the sections back to back behind a pointer field of `pointer` (preceded by `pointer` bytes `before`, padded with 0xFF) in a
        PUSI packet, continued in packets without PUSI (adaptation_field_length cont_af each); the last packet is padded with 0xFF.
        stuffing False: nothing is padded, the caller's bytes fill the last packet exactly -> [k, 188]"""
        data = b''.join(bytes(s) for s in sections)
        head = bytes([pointer]) + (bytes(before) + b'\xff' * pointer)[:pointer]
        room = TS - 4 - (0 if af_len is None else 1 + af_len)
        out = [packet(self.pid, self._next(), head + data[:room - len(head)], pusi=1, af_len=af_len)]
        data = data[max(room - len(head), 0):]
        room = TS - 4 - (0 if cont_af is None else 1 + cont_af)
        while data:
            out.append(packet(self.pid, self._next(), data[:room], af_len=cont_af))
            data = data[room:]
        assert stuffing or len(head) + sum(len(bytes(s)) for s in sections) >= 1
        return np.array(out, np.uint8).reshape(-1, TS)

    def other(self, n=1, payload=b''):
        """packets without PUSI that only continue (or bring nothing)"""
        return np.array([packet(self.pid, self._next(), payload) for _ in range(n)], np.uint8).reshape(-1, TS)


def filler(pid, n, rng, cc0=0):
    """n packets of another PID with random payload"""
    out = rng.integers(0, 256, (n, TS), dtype=np.uint8)
    out[:, 0], out[:, 1], out[:, 2] = 0x47, pid >> 8, pid & 255
    out[:, 3] = 0x10 | ((cc0 + np.arange(n)) & 15)
    return out


def interleave(rng, streams):
    """the packets of several PIDs, each in its own order, in one random order -> [n, 188]"""
    idx = np.concatenate([np.full(len(s), i) for i, s in enumerate(streams)])
    rng.shuffle(idx)
    at = [0] * len(streams)
    out = []
    for i in idx:
        out.append(streams[i][at[i]])
        at[i] += 1
    return np.array(out, np.uint8).reshape(-1, TS)


# ------------------------------------------------------------------------------------------------- fault injectors
# each takes the packets of ONE section laid by Packetiser.lay over at least three packets (the middle packet k is hit) and returns
# the damaged packets and what the fault costs against the clean run, when the next section starts in a PUSI packet with pointer 0
def drop_middle(ts, k):
    return np.delete(ts, k, axis=0), dict(packets=-1, sections=-1, valid=-1, changed=-1, dropped_sections=1)


def announce_discontinuity(ts, k):
    ts = ts.copy()
    room = ts[k, 4:].copy()
    ts[k, 3] |= 0x20
    ts[k, 4], ts[k, 5] = 1, 0x80
    ts[k, 6:] = room[:TS - 6]
    return ts, dict(sections=-1, valid=-1, changed=-1, dropped_sections=1)


def scramble(ts, k):
    ts = ts.copy()
    ts[k, 3] |= 0x80
    return ts, dict(sections=-1, valid=-1, changed=-1, dropped_sections=1, scrambled_packets=1)


def flip_bit(ts, k):
    ts = ts.copy()
    ts[k, 100] ^= 0x04
    return ts, dict(valid=-1, changed=-1, crc_errors=1)


def duplicate(ts, k):
    return np.insert(ts, k + 1, ts[k], axis=0), dict(packets=1)


INJECTORS = (drop_middle, announce_discontinuity, scramble, flip_bit, duplicate)
