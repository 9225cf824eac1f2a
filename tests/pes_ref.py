"""Python model of the PES bank's rules (include/dvbs2gpu.h, PES bank): the sequential definition, packet by packet, in Python's
unbounded integers, written from the rules' text.  With it builders for TS packets that carry PES packet starts and bodies.  The
yardstick of the bank's tests."""
import numpy as np

TS = 188
SLOTS = 16
SCRAMBLED, SHORT, BAD_START, PLAIN, MALFORMED, HEADER = range(6)
CLOSED, CLOSED_GAP, CLOSED_MISMATCH, CLOSED_UNCHECKED, UNBOUNDED_NONVIDEO, TS_FIRST, TS_BACKWARD, TS_GAP, PTS_LATE, DTS_AFTER_PTS = (1 << i for i in range(10))
NO_TS = (1 << 64) - 1
MOD, HALF = 1 << 33, 1 << 32
GAP_TICKS = 63000
LATE_TICKS = 18900000
PLAIN_IDS = (0xBC, 0xBE, 0xBF, 0xF0, 0xF1, 0xF2, 0xF8, 0xFF)
U32 = (1 << 32) - 1
KIND_KEY = {SCRAMBLED: 'starts_scrambled', SHORT: 'starts_short', BAD_START: 'starts_bad_start', PLAIN: 'starts_plain', MALFORMED: 'starts_malformed',
            HEADER: 'starts_header'}
STAT_KEYS = ('packets', 'payload_bytes', 'duplicates', 'cc_errors', 'scrambled_packets', 'malformed_packets', 'starts', 'starts_scrambled', 'starts_short',
             'starts_bad_start', 'starts_plain', 'starts_malformed', 'starts_header', 'with_pts', 'with_dts', 'closed_ok', 'closed_mismatch', 'closed_gap',
             'closed_unchecked', 'ts_backward', 'ts_gap', 'pts_late', 'dts_after_pts', 'max_delta_packets')
MAX_KEYS = ('max_delta_packets',)
ROW_KEYS = ('pid', 'slot', 'kind', 'flags', 'stream_id', 'packet', 'declared', 'pts', 'dts', 'closed_bytes', 'closed_packets', 'delta_packets', 'delta_ts')
FLAG_KEY = {CLOSED_MISMATCH: 'closed_mismatch', CLOSED_GAP: 'closed_gap', CLOSED_UNCHECKED: 'closed_unchecked', TS_BACKWARD: 'ts_backward', TS_GAP: 'ts_gap',
            PTS_LATE: 'pts_late', DTS_AFTER_PTS: 'dts_after_pts'}


def late_packets(tpp_q24):
    return (LATE_TICKS << 24) // tpp_q24


def _timestamp(b, prefix):
    """five bytes -> the 33-bit value, or None where a marker bit is 0 or the prefix is wrong"""
    if b[0] >> 4 != prefix or not (b[0] & 1 and b[2] & 1 and b[4] & 1):
        return None
    return (b[0] >> 1 & 7) << 30 | b[1] << 22 | (b[2] >> 1) << 15 | b[3] << 7 | b[4] >> 1


def parse_start(pay, tsc):
    """the payload bytes of a packet with PUSI -> (kind, stream_id, declared, pts, dts)"""
    L = len(pay)
    if tsc:
        return SCRAMBLED, 0, 0, NO_TS, NO_TS
    if L < 6:
        return SHORT, 0, 0, NO_TS, NO_TS
    sid = pay[3]
    if pay[:3] != b'\x00\x00\x01':
        return BAD_START, sid, 0, NO_TS, NO_TS
    declared = pay[4] << 8 | pay[5]
    if sid in PLAIN_IDS:
        return PLAIN, sid, declared, NO_TS, NO_TS
    if L < 9:
        return SHORT, sid, declared, NO_TS, NO_TS
    fl, hdl = pay[7] >> 6, pay[8]
    if pay[6] & 0xC0 != 0x80 or fl == 1 or (fl == 2 and hdl < 5) or (fl == 3 and hdl < 10):
        return MALFORMED, sid, declared, NO_TS, NO_TS
    if (fl == 2 and L < 14) or (fl == 3 and L < 19):
        return SHORT, sid, declared, NO_TS, NO_TS
    pts = dts = NO_TS
    if fl >= 2:
        pts = _timestamp(pay[9:14], fl)
    if fl == 3:
        dts = _timestamp(pay[14:19], 1)
    if pts is None or dts is None:
        return MALFORMED, sid, declared, NO_TS, NO_TS
    return HEADER, sid, declared, pts, dts


def cc_step(state, payload, cc, di):
    """the TS monitor's continuity automaton; state None (never seen) or [last cc, dup_used] -> (verdict, state)"""
    if state is None:
        return 'first', [cc, False]
    if di:
        return 'disc', [cc, False]
    last, dup = state
    if not payload:
        return ('cc_error' if cc != last else 'ok'), [cc, False]
    if cc == (last + 1) & 15:
        return 'ok', [cc, False]
    if cc == last and not dup:
        return 'duplicate', [cc, True]
    return 'cc_error', [cc, False]


class Slot:
    def __init__(self):
        self.cc = None
        self.open = None                            # None, or dict(declared, bytes, packets, gap)
        self.ts = None                              # None, or (last_T, ref_n)
        self.st = dict.fromkeys(STAT_KEYS, 0)
        self.last_n = -1


class Pes:
    """one stream"""

    def __init__(self, max_rows=1 << 30):
        self.max_rows = max_rows
        self.watch = [-1] * SLOTS
        self.tpp = 0
        self.reset()

    def reset(self):
        self.slot = [Slot() for _ in range(SLOTS)]
        self.packets = self.rows_dropped = 0
        self.table, self.starts = [], 0

    def set_watch(self, slot, pid):
        self.watch[slot] = pid
        self.slot[slot] = Slot()

    def set_rate(self, tpp):
        self.tpp = tpp

    def _start(self, i, pid, k, pay, tsc):
        s, st, n = self.slot[i], self.slot[i].st, self.packets + k
        kind, sid, declared, pts, dts = parse_start(pay, tsc)
        flags, cb, cp, dn, dt = 0, 0, 0, 0, 0
        if kind == HEADER and declared == 0 and not 0xE0 <= sid <= 0xEF:
            flags |= UNBOUNDED_NONVIDEO
        if s.open is not None:
            o = s.open
            cb, cp = min(o['bytes'], U32), min(o['packets'], U32)
            flags |= CLOSED
            if o['gap']:
                flags |= CLOSED_GAP
            elif o['declared'] == 0:
                flags |= CLOSED_UNCHECKED
            elif cb != o['declared'] + 6:
                flags |= CLOSED_MISMATCH
            if not flags & (CLOSED_GAP | CLOSED_UNCHECKED | CLOSED_MISMATCH):
                st['closed_ok'] += 1
        s.open = dict(declared=declared, bytes=len(pay), packets=1, gap=False)
        if kind == HEADER and pts != NO_TS:
            T = dts if dts != NO_TS else pts
            st['with_pts'] += 1
            st['with_dts'] += dts != NO_TS
            if dts != NO_TS and (pts - dts) % MOD >= HALF:
                flags |= DTS_AFTER_PTS
            if s.ts is None:
                flags |= TS_FIRST
            else:
                dT, dN = (T - s.ts[0]) % MOD, n - s.ts[1]
                if dT >= HALF:
                    flags |= TS_BACKWARD
                elif dT > GAP_TICKS:
                    flags |= TS_GAP
                if self.tpp and dN > late_packets(self.tpp):
                    flags |= PTS_LATE
                dt = max(-(1 << 31), min((1 << 31) - 1, dT - MOD if dT >= HALF else dT))
                dn = min(dN, U32)
            s.ts = (T, n)
        st['starts'] += 1
        st[KIND_KEY[kind]] += 1
        for f, key in FLAG_KEY.items():
            st[key] += bool(flags & f)
        st['max_delta_packets'] = max(st['max_delta_packets'], dn)
        s.last_n = n
        self.starts += 1
        if len(self.table) < self.max_rows:
            self.table.append(dict(pid=pid, slot=i, kind=kind, flags=flags, stream_id=sid, packet=k, declared=declared, pts=pts, dts=dts, closed_bytes=cb,
                                   closed_packets=cp, delta_packets=dn, delta_ts=dt))
        else:
            self.rows_dropped += 1

    def process(self, ts):
        """ts: uint8, whole packets -> the starts of the call; self.table: the call's first max_rows rows"""
        ts = np.asarray(ts, np.uint8).reshape(-1, TS)
        self.table, self.starts = [], 0
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
            verdict, s.cc = cc_step(s.cc, afc & 1, cc, di)
            if verdict == 'duplicate':
                st['duplicates'] += 1
                continue
            st['cc_errors'] += verdict == 'cc_error'
            if verdict in ('cc_error', 'disc') and s.open is not None:
                s.open['gap'] = True
            if not afc & 1:
                continue
            if afc == 3 and p[4] > 182:
                st['malformed_packets'] += 1
                if s.open is not None:
                    s.open['gap'] = True
                continue
            at = 4 if afc == 1 else 5 + p[4]
            L = TS - at
            st['payload_bytes'] += L
            st['scrambled_packets'] += tsc != 0
            if p[1] >> 6 & 1:
                self._start(i, pid, k, p[at:], tsc)
            elif s.open is not None:
                s.open['bytes'] += L
                s.open['packets'] += 1
        self.packets += len(ts)
        return self.starts

    def stats(self, slot=-1):
        sel = [s.st for s in self.slot] if slot < 0 else [self.slot[slot].st]
        return {k: int(max(s[k] for s in sel) if k in MAX_KEYS else sum(s[k] for s in sel)) for k in STAT_KEYS}

    def stream_stats(self):
        return dict(packets=self.packets, rows_dropped=self.rows_dropped, packets_since_start=[self.packets - s.last_n if s.last_n >= 0 else -1 for s in self.slot])


# ------------------------------------------------------------------------------------------------- builders
def ts_bytes(prefix, t, markers=(1, 1, 1)):
    """the five bytes of a 33-bit timestamp behind a 4-bit prefix; markers: the three marker bits"""
    t = int(t) % MOD
    return bytes([prefix << 4 | (t >> 30 & 7) << 1 | markers[0], t >> 22 & 255, (t >> 15 & 127) << 1 | markers[1], t >> 7 & 255, (t & 127) << 1 | markers[2]])


def ts_packet(pid, cc, payload, af_len=None, pusi=0, tsc=0, di=0, afc=None, tei=0, sync=0x47, fill=0x5A):
    """one TS packet: af_len None is AFC 1 (184 payload bytes), else AFC 3 with adaptation_field_length af_len (183 - af_len payload
    bytes); afc overrides the field (2: no payload).  `payload` is cut or padded with `fill` to the room there is."""
    afc = (1 if af_len is None else 3) if afc is None else afc
    head = bytes([sync, tei << 7 | pusi << 6 | pid >> 8, pid & 255, tsc << 6 | afc << 4 | cc & 15])
    if afc & 2:
        a = 183 if af_len is None else af_len
        head += bytes([a]) + (bytes([di << 7]) + b'\xff' * (a - 1) if a > 0 else b'')
    head = head[:TS]
    room = TS - len(head)
    body = bytes(payload)[:room] if afc & 1 else b''
    return np.frombuffer(head + body + bytes([fill]) * (room - len(body)), np.uint8)


def pes_head(stream_id=0xE0, pts=None, dts=None, declared=0, flags=None, hdl=None, b6=0x80, start=b'\x00\x00\x01', pts_prefix=None, dts_prefix=1,
             pts_markers=(1, 1, 1), dts_markers=(1, 1, 1)):
    """the first bytes of a PES packet: start code, stream_id, PES_packet_length and, but for the header-less stream ids, the optional
    header with the timestamps there are.  flags / hdl / prefixes / markers override what follows from pts and dts: the faults"""
    out = start + bytes([stream_id, declared >> 8, declared & 255])
    if stream_id in PLAIN_IDS:
        return out
    fl = (0 if pts is None else 2 if dts is None else 3) if flags is None else flags
    stamps = b''
    if pts is not None:
        stamps += ts_bytes(fl if pts_prefix is None else pts_prefix, pts, pts_markers)
    if dts is not None:
        stamps += ts_bytes(dts_prefix, dts, dts_markers)
    return out + bytes([b6, fl << 6, len(stamps) if hdl is None else hdl]) + stamps


def pes_packet(pid, cc, stream_id=0xE0, pts=None, dts=None, declared=0, af_len=None, tsc=0, di=0, fill=0x5A, **kw):
    """a TS packet with PUSI that starts a PES packet (pes_head's arguments in kw)"""
    return ts_packet(pid, cc, pes_head(stream_id, pts, dts, declared, **kw), af_len=af_len, pusi=1, tsc=tsc, di=di, fill=fill)


def body_packet(pid, cc, af_len=None, **kw):
    """a TS packet without PUSI: 184 or 183 - af_len bytes of a PES packet's body"""
    return ts_packet(pid, cc, b'', af_len=af_len, **kw)


def null_packets(n):
    out = np.full((n, TS), 0xFF, np.uint8)
    out[:, 0], out[:, 1], out[:, 2], out[:, 3] = 0x47, 0x1F, 0xFF, 0x10
    return out


def pes_stream(pid, cc0, sizes, pts0=None, step=3600, stream_id=0xE0, declare=True, dts_lag=None):
    """whole PES packets of `pid`, back to back: sizes[i] payload bytes each (header included), the last TS packet of each padded by an
    adaptation field as a multiplexer does; PTS pts0 + i * step (None: no timestamps) -> ([n, 188], the next counter)"""
    out, cc = [], cc0
    for i, size in enumerate(sizes):
        pts = None if pts0 is None else pts0 + i * step
        dts = None if pts is None or dts_lag is None else pts - dts_lag
        left, first = size, True
        while left > 0:
            take = min(left, 184)
            af = None if take == 184 else 183 - take
            out.append(pes_packet(pid, cc, stream_id, pts, dts, size - 6 if declare else 0, af_len=af) if first else body_packet(pid, cc, af_len=af))
            cc, left, first = cc + 1, left - take, False
    return np.array(out), cc & 15


def random_mux(rng, n, pids, other=0x300, tpp=1000, faults=True):
    """n packets: on every PID of `pids` PES packets of random sizes with PTS (some with DTS) that follow the packet position at `tpp`
    27 MHz ticks per packet, interleaved at random with packets of PID `other` and null packets; with faults, a share of the packets is
    dropped, repeated, scrambled, given a DI or an odd adaptation field -> [n, 188]"""
    state = {p: dict(cc=int(rng.integers(0, 16)), left=0, size=0) for p in pids}
    out = []
    while len(out) < n:
        r = rng.random()
        if r < 0.1:
            out.append(null_packets(1)[0])
            continue
        if r < 0.2:
            out.append(ts_packet(other, len(out), b'', fill=int(rng.integers(0, 256))))
            continue
        pid = pids[int(rng.integers(0, len(pids)))]
        s = state[pid]
        k = len(out)
        if s['left'] <= 0:
            s['size'] = s['left'] = int(rng.integers(20, 900))
            pts = k * tpp // 300 + int(rng.integers(0, 50))
            kw = dict(pts=pts if rng.random() < 0.8 else None, declared=s['size'] - 6 if rng.random() < 0.8 else 0,
                      stream_id=int(rng.choice([0xE0, 0xC0, 0xBD, 0xBE, 0xE1])))
            if kw['pts'] is not None and rng.random() < 0.4:
                kw['dts'] = pts - int(rng.integers(-400, 4000))
            take = min(s['left'], 184)
            if faults and rng.random() < 0.1:
                kw.update([dict(pts_markers=(1, 0, 1)), dict(flags=1), dict(start=b'\x00\x01\x01'), dict(tsc=2), dict(b6=0x40), dict(hdl=3)][int(rng.integers(0, 6))])
            if faults and rng.random() < 0.15:
                take = int(rng.choice([1, 5, 6, 8, 9, 13, 14, 18, 19, 40]))
            pk = pes_packet(pid, s['cc'], af_len=None if take == 184 else 183 - take, **kw)
        else:
            take = min(s['left'], 184)
            pk = body_packet(pid, s['cc'], af_len=None if take == 184 else 183 - take)
        s['left'] -= take
        s['cc'] = (s['cc'] + 1) & 15
        if faults:
            f = rng.random()
            if f < 0.03:
                continue                                                # lost
            if f < 0.06:
                out.append(pk)                                          # repeated (and perhaps once more below)
                if rng.random() < 0.3:
                    out.append(pk)
            elif f < 0.08:
                pk = pk.copy()
                pk[3] |= 0x80                                           # scrambled
            elif f < 0.10:
                pk = ts_packet(pid, s['cc'] - 1, b'', af_len=183, afc=3)  # an adaptation field that leaves no payload
            elif f < 0.12:
                pk = ts_packet(pid, s['cc'] - 1, b'', afc=2, di=int(rng.random() < 0.5))
                s['cc'] = (s['cc'] - 1) & 15                            # no payload: the counter does not advance
        out.append(pk)
    return np.array(out[:n])
