"""Python model of the audio bank's rules (include/dvbs2gpu.h, audio bank): the sequential definition, packet by packet and byte by
byte, on Python's bytes and unbounded integers, written from the rules' text (the window is a bytes object, the bitrates are the
written-out tables, the parameters a tuple of the named fields).  The packet steps are those of es_ref.Es, the PES start is
pes_ref.parse_start.  The yardstick of the bank's tests."""
import numpy as np

import pes_ref as P

TS = 188
SLOTS = 16
MPA, ADTS, AC3 = 1, 2, 3
PES, FRAME, LOSS = range(3)
ACQUIRED, RESYNC, UNSYNCED, SPLIT_HEADER, CHANGE = 1, 2, 4, 8, 16
NO_TS = (1 << 64) - 1
STAT_KEYS = ('packets', 'payload_bytes', 'es_bytes', 'bytes_unsynced', 'duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'resets',
             'pes_starts', 'pes_invalid', 'split_headers', 'frames', 'frame_bytes_total', 'samples_total', 'acquisitions', 'sync_losses', 'param_changes',
             'unaligned_starts', 'bytes_unlocked')
ROW_KEYS = ('pid', 'slot', 'unit', 'code', 'detail', 'flags', 'packet', 'kbps', 'head', 'es_offset', 'pts', 'dts', 'sample_rate', 'frame_bytes', 'samples')

MPA_KBPS = {
    'V1L1': [32 * i for i in range(1, 15)],
    'V1L2': [32, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384],
    'V1L3': [32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320],
    'V2L1': [32, 48, 56, 64, 80, 96, 112, 128, 144, 160, 176, 192, 224, 256],
    'V2L23': [8, 16, 24, 32, 40, 48, 56, 64, 80, 96, 112, 128, 144, 160]}
MPA_RATES = [44100, 48000, 32000]
ADTS_RATES = [96000, 88200, 64000, 48000, 44100, 32000, 24000, 22050, 16000, 12000, 11025, 8000, 7350]
AC3_KBPS = [32, 40, 48, 56, 64, 80, 96, 112, 128, 160, 192, 224, 256, 320, 384, 448, 512, 576, 640]


def parse(codec, w):
    """w: 8 bytes -> None, or dict(frame_bytes, sample_rate, samples, kbps, code, detail, params); params: a tuple of everything but
    padding and length"""
    bits = int.from_bytes(w, 'big')
    f = lambda at, n: bits >> (64 - at - n) & ((1 << n) - 1)          # n bits from bit `at` of the window
    if codec == MPA:
        sync, ver, layer, prot, bri, sri, pad, mode = f(0, 11), f(11, 2), f(13, 2), f(15, 1), f(16, 4), f(20, 2), f(22, 1), f(24, 2)
        if sync != 0x7FF or ver == 1 or layer == 0 or bri in (0, 15) or sri == 3:
            return None
        lay = 4 - layer
        kbps = MPA_KBPS[('V1L%d' % lay) if ver == 3 else 'V2L1' if lay == 1 else 'V2L23'][bri - 1]
        fs = MPA_RATES[sri] // {3: 1, 2: 2, 0: 4}[ver]
        if lay == 1:
            nbytes, samples = (12 * kbps * 1000 // fs + pad) * 4, 384
        elif lay == 2 or ver == 3:
            nbytes, samples = 144 * kbps * 1000 // fs + pad, 1152
        else:
            nbytes, samples = 72 * kbps * 1000 // fs + pad, 576
        return dict(frame_bytes=nbytes, sample_rate=fs, samples=samples, kbps=kbps, code=ver << 2 | layer, detail=mode, params=(MPA, ver, layer, prot, bri, sri, mode))
    if codec == ADTS:
        sync, ident, layer, absent, profile, sfi, chan, length, blocks = f(0, 12), f(12, 1), f(13, 2), f(15, 1), f(16, 2), f(18, 4), f(23, 3), f(30, 13), f(54, 2)
        if sync != 0xFFF or layer != 0 or sfi > 12 or length < (7 if absent else 9):
            return None
        fs, samples = ADTS_RATES[sfi], 1024 * (blocks + 1)
        return dict(frame_bytes=length, sample_rate=fs, samples=samples, kbps=length * 8 * fs // (samples * 1000), code=ident << 2 | profile, detail=chan,
                    params=(ADTS, ident, absent, profile, sfi, chan, blocks))
    if codec == AC3:
        if w[:2] != b'\x0B\x77':
            return None
        bsid = f(40, 5)
        if bsid <= 10:
            fscod, frmsizecod, bsmod, acmod = f(32, 2), f(34, 6), f(45, 3), f(48, 3)
            if fscod == 3 or frmsizecod > 37:
                return None
            br = AC3_KBPS[frmsizecod >> 1]
            words = {0: 2 * br, 2: 3 * br, 1: 320 * br // 147 + (frmsizecod & 1)}[fscod]
            return dict(frame_bytes=2 * words, sample_rate=[48000, 44100, 32000][fscod], samples=1536, kbps=br, code=bsid, detail=acmod,
                        params=(AC3, 0, fscod, frmsizecod >> 1, bsid, bsmod, acmod))
        if bsid <= 16:
            strmtyp, substreamid, frmsiz, fscod, c2, acmod, lfeon = f(16, 2), f(18, 3), f(21, 11), f(32, 2), f(34, 2), f(36, 3), f(39, 1)
            if (fscod == 3 and c2 == 3) or 2 * (frmsiz + 1) < 7:
                return None
            fs, blocks = ([24000, 22050, 16000][c2], 6) if fscod == 3 else ([48000, 44100, 32000][fscod], [1, 2, 3, 6][c2])
            nbytes, samples = 2 * (frmsiz + 1), 256 * blocks
            return dict(frame_bytes=nbytes, sample_rate=fs, samples=samples, kbps=nbytes * 8 * fs // (samples * 1000), code=bsid, detail=acmod | lfeon << 3,
                        params=(AC3, 1, strmtyp, substreamid, fscod, c2, acmod, lfeon, bsid))
        return None
    raise ValueError(codec)


class Slot:
    def __init__(self, codec=0):
        self.codec = codec
        self.cc = None
        self.synced = self.lost = self.locked = False
        self.kept = b''                              # the accepted bytes since the last reset, the last 7 of them
        self.es_count = self.next = 0
        self.params = None                           # of the frame before `next`; None: none since the acquisition
        self.st = dict.fromkeys(STAT_KEYS, 0)


class Aud:
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
        row = dict(kbps=0, pts=NO_TS, dts=NO_TS, sample_rate=0, frame_bytes=0, samples=0)
        row.update(kw)
        row['flags'] |= RESYNC if s.lost else 0
        s.lost = False
        self.nrows += 1
        if len(self.table) < self.max_rows:
            self.table.append(row)
        else:
            self.rows_dropped += 1

    @staticmethod
    def _reset(s):
        s.kept, s.lost, s.locked = b'', True, False

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
                    if not s.locked:
                        s.locked, s.next, s.params = True, s.es_count, None
                        st['acquisitions'] += 1
                    elif s.next != s.es_count:
                        st['unaligned_starts'] += 1
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
                st['bytes_unlocked'] += not s.locked
                w = s.kept + bytes([b])
                if len(w) == 8 and s.locked and s.es_count - 7 == s.next:
                    got = parse(s.codec, w)
                    acq = ACQUIRED if s.params is None else 0
                    head = int.from_bytes(w[:4], 'big')
                    if got is None:
                        st['sync_losses'] += 1
                        s.locked = False
                        self._row(s, pid=pid, slot=i, unit=LOSS, code=0, detail=0, flags=acq, packet=k, head=head, es_offset=s.next)
                    else:
                        change = not acq and got['params'] != s.params
                        st['frames'] += 1
                        st['frame_bytes_total'] += got['frame_bytes']
                        st['samples_total'] += got['samples']
                        st['param_changes'] += change
                        self._row(s, pid=pid, slot=i, unit=FRAME, code=got['code'], detail=got['detail'], flags=acq | (CHANGE if change else 0), packet=k, head=head,
                                  es_offset=s.next, kbps=got['kbps'], sample_rate=got['sample_rate'], frame_bytes=got['frame_bytes'], samples=got['samples'])
                        s.next += got['frame_bytes']
                        s.params = got['params']
                s.kept = w[-7:]
                s.es_count += 1
        self.packets += len(ts)
        return self.nrows

    def stats(self, slot=-1):
        sel = [s.st for s in self.slot] if slot < 0 else [self.slot[slot].st]
        return {k: int(sum(s[k] for s in sel)) for k in STAT_KEYS}

    def stream_stats(self):
        return dict(packets=self.packets, rows_dropped=self.rows_dropped)
