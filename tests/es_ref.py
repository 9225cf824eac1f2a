"""Python model of the ES bank's rules (include/dvbs2gpu.h, ES bank): the sequential definition, packet by packet and byte by byte, on
Python's bytes and unbounded integers, written from the rules' text (the scanner keeps a bytes object, not a shifted word; the
classification is a table walk).  The PES start is pes_ref.parse_start: the rule is the PES bank's.  The yardstick of the bank's
tests."""
import numpy as np

import pes_ref as P

TS = 188
SLOTS = 16
MPEG2, H264, H265 = 1, 2, 3
PES, PICTURE, SEQUENCE, GOP, PARAM, AUD, END = range(7)
SLICE, OTHER, BAD = 'slices', 'other_codes', 'bad_codes'
PIC_I, PIC_P, PIC_B = 1, 2, 3
KEY, RESYNC, UNSYNCED, SPLIT_HEADER = 1, 2, 4, 8
NO_TS = (1 << 64) - 1
UNIT_KEY = {PICTURE: 'pictures', SEQUENCE: 'sequences', GOP: 'gops', PARAM: 'params', AUD: 'auds', END: 'ends'}
STAT_KEYS = ('packets', 'payload_bytes', 'es_bytes', 'bytes_unsynced', 'duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'resets',
             'pes_starts', 'pes_invalid', 'split_headers', 'codes', 'pictures', 'pictures_i', 'pictures_p', 'pictures_b', 'key_pictures', 'sequences', 'gops',
             'params', 'auds', 'ends', 'slices', 'other_codes', 'bad_codes')
ROW_KEYS = ('pid', 'slot', 'unit', 'code', 'detail', 'flags', 'packet', 'head', 'es_offset', 'pts', 'dts')


def classify(codec, code, head):
    """-> (unit or the name of the counter of a code without a row, detail, key)"""
    if codec == MPEG2:
        if code == 0x00:
            t = head >> 19 & 7
            return PICTURE, t if t in (1, 2, 3) else 0, t == 1
        if code in (0xB3, 0xB8, 0xB7):
            return {0xB3: SEQUENCE, 0xB8: GOP, 0xB7: END}[code], 0, False
        return (SLICE if 0x01 <= code <= 0xAF else OTHER), 0, False
    if codec == H264:
        if code & 0x80:
            return BAD, 0, False
        t = code & 31
        if t in (1, 5):
            if not head >> 31:
                return SLICE, 0, False
            bits = format(head >> 24 & 127, '07b')
            zeros = len(bits) - len(bits.lstrip('0'))
            detail = 0
            if zeros <= 3:
                v = int(bits[zeros:2 * zeros + 1], 2) - 1
                if v <= 9:
                    detail = {0: PIC_P, 1: PIC_B, 2: PIC_I}.get(v % 5, 0)
            return PICTURE, detail, t == 5
        return {7: SEQUENCE, 8: PARAM, 9: AUD, 10: END, 11: END}.get(t, OTHER), 0, False
    if codec == H265:
        if code & 0x80 or head >> 24 & 7 == 0:
            return BAD, 0, False
        t = code >> 1 & 63
        if t <= 9 or 16 <= t <= 21:
            if not head >> 23 & 1:
                return SLICE, 0, False
            return PICTURE, PIC_I if t >= 16 else 0, t >= 16
        return {33: SEQUENCE, 32: PARAM, 34: PARAM, 35: AUD, 36: END, 37: END}.get(t, OTHER), 0, False
    raise ValueError(codec)


class Slot:
    def __init__(self, codec=0):
        self.codec = codec
        self.cc = None
        self.synced = self.lost = False
        self.kept = b''                              # the accepted bytes since the last reset, the last 7 of them
        self.es_count = 0
        self.st = dict.fromkeys(STAT_KEYS, 0)


class Es:
    """one stream"""

    def __init__(self, max_rows=1 << 30):
        self.max_rows = max_rows
        self.watch = [-1] * SLOTS
        self.codec = [0] * SLOTS
        self.reset()

    def reset(self):
        self.slot = [Slot(c) for c in self.codec]
        self.packets = self.rows_dropped = 0
        self.table, self.nrows = [], 0

    def set_watch(self, slot, pid, codec=0):
        self.watch[slot], self.codec[slot] = pid, codec if pid >= 0 else 0
        self.slot[slot] = Slot(self.codec[slot])

    def _row(self, s, **kw):
        kw['flags'] |= RESYNC if s.lost else 0
        s.lost = False
        self.nrows += 1
        if len(self.table) < self.max_rows:
            self.table.append(kw)
        else:
            self.rows_dropped += 1

    @staticmethod
    def _reset(s):
        s.kept, s.lost = b'', True

    def process(self, ts):
        """ts: uint8, whole packets -> the rows of the call; self.table: the call's first max_rows rows"""
        ts = np.asarray(ts, np.uint8).reshape(-1, TS)
        self.table, self.nrows = [], 0
        slots = {p: i for i, p in enumerate(self.watch) if p >= 0}
        for k, pk in enumerate(ts):
            p = bytes(pk)
            pid, tsc, afc, cc = (p[1] & 0x1f) << 8 | p[2], p[3] >> 6, (p[3] >> 4) & 3, p[3] & 15
            if p[0] != 0x47 or p[1] >> 7 or pid == 0x1FFF or pid not in slots:
                continue
            i = slots[pid]
            s, st = self.slot[i], self.slot[i].st
            st['packets'] += 1
            di = bool(afc & 2 and p[4] > 0 and p[5] >> 7)
            verdict, s.cc = P.cc_step(s.cc, afc & 1, cc, di)
            if verdict == 'duplicate':
                st['duplicates'] += 1
                continue
            st['cc_errors'] += verdict == 'cc_error'
            resets = verdict in ('cc_error', 'disc')
            if resets:
                self._reset(s)
            if not afc & 1:
                st['resets'] += resets
                continue
            if afc == 3 and p[4] > 182:
                st['malformed_packets'] += 1
                st['resets'] += 1
                self._reset(s)
                continue
            at = 4 if afc == 1 else 5 + p[4]
            pay = p[at:]
            st['payload_bytes'] += len(pay)
            if tsc:
                st['scrambled_packets'] += 1
                resets = True
                self._reset(s)
            segment = b''
            if p[1] >> 6 & 1:
                kind, sid, declared, pts, dts = P.parse_start(pay, tsc)
                valid = kind == P.HEADER and 9 + pay[8] <= len(pay)
                flags = 0 if valid else UNSYNCED | (SPLIT_HEADER if kind == P.HEADER else 0)
                self._row(s, pid=pid, slot=i, unit=PES, code=sid, detail=kind, flags=flags, packet=k, head=declared, es_offset=s.es_count, pts=pts, dts=dts)
                st['pes_starts'] += 1
                st['pes_invalid'] += not valid
                st['split_headers'] += bool(flags & SPLIT_HEADER)
                s.synced = valid
                if valid:
                    segment = pay[9 + pay[8]:]
                else:
                    resets = True
                    self._reset(s)
            elif not tsc:
                if s.synced:
                    segment = pay
                else:
                    st['bytes_unsynced'] += len(pay)
            st['resets'] += resets
            st['es_bytes'] += len(segment)
            for b in segment:
                w = s.kept + bytes([b])
                if len(w) == 8 and w[:3] == b'\x00\x00\x01':
                    code, head = w[3], int.from_bytes(w[4:], 'big')
                    unit, detail, key = classify(s.codec, code, head)
                    st['codes'] += 1
                    if isinstance(unit, str):
                        st[unit] += 1
                    else:
                        st[UNIT_KEY[unit]] += 1
                        if unit == PICTURE:
                            st['key_pictures'] += key
                            if detail:
                                st[{PIC_I: 'pictures_i', PIC_P: 'pictures_p', PIC_B: 'pictures_b'}[detail]] += 1
                        self._row(s, pid=pid, slot=i, unit=unit, code=code, detail=detail, flags=KEY if key else 0, packet=k, head=head,
                                  es_offset=s.es_count - 7, pts=NO_TS, dts=NO_TS)
                s.kept = w[-7:]
                s.es_count += 1
        self.packets += len(ts)
        return self.nrows

    def stats(self, slot=-1):
        sel = [s.st for s in self.slot] if slot < 0 else [self.slot[slot].st]
        return {k: int(sum(s[k] for s in sel)) for k in STAT_KEYS}

    def stream_stats(self):
        return dict(packets=self.packets, rows_dropped=self.rows_dropped)
