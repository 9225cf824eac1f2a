"""Mode adaptation of DVB-S2 TS carriers (EN 302 307-1 5.1.2-5.1.6, Annex D) in pure numpy / Python, both directions, written
independently of the library: a transmitter (TS per ISI -> null-packet deletion with DNP, ISSY, CRC-8 chaining -> data fields ->
BBFRAMEs of several ISIs interleaved) and a receiver model of the rules the library's mode-adaptation mode follows
(DESIGN section 9).  Test infrastructure only; the receiver model is the yardstick of tests/test_ma_cpu.py and tests/test_gpu_ma.py."""
import numpy as np

from orc_bbts import bbheader

# the slot layout, in one place: [CRC-8 of the previous UP][UP][ISSY 0/2/3][DNP 0/1]; dvbs2gpu_bbts_ma_get_layout reports the library's
LAYOUT = {'crc_off': 0, 'up_off': 1, 'up_len': 187, 'issy_off': 188}
NULL_PACKET = np.array([0x47, 0x1f, 0xff, 0x10] + [0xff] * 184, np.uint8)
NO_START = 65535

_TAB = np.zeros(256, np.uint8)
for _i in range(256):
    _c = _i
    for _ in range(8):
        _c = ((_c << 1) ^ 0xD5) & 0xff if _c & 0x80 else (_c << 1) & 0xff
    _TAB[_i] = _c


def crc8(data):
    """x^8+x^7+x^6+x^4+x^2+1, MSB first, zero initial state: the BBHEADER's CRC-8, here over user-packet bytes"""
    c = 0
    for b in bytes(data):
        c = int(_TAB[c ^ b])
    return c


def slot_len(issy, npd):
    return LAYOUT['issy_off'] + issy + (1 if npd else 0)


def crc_span(slot, span):
    a = LAYOUT['up_off']
    return slot[a:a + LAYOUT['up_len']] if span == 0 else slot[a:]


# ------------------------------------------------------------------------------------------------------------- transmitter
def make_ts(n, rng, null_runs=True):
    """n data packets with random content (never PID 0x1fff), runs of canonical null packets in between; ends with a data packet"""
    out, last = [], 0
    for _ in range(n):
        p = rng.integers(0, 256, 188, dtype=np.uint8)
        p[0] = 0x47
        p[1] &= 0x7f                                   # transport_error_indicator clear
        if (p[1] & 0x1f) == 0x1f and p[2] == 0xff:
            p[2] = 0xfe
        out.append(p)
        if null_runs and rng.random() < 0.3:
            run = int(rng.choice([1, 2, 5, 40, 300])) if rng.random() < 0.5 else 1
            out += [NULL_PACKET.copy() for _ in range(run)]
        else:
            last = len(out)
    return np.array(out[:max(last, 1)] if is_null(out[-1]) else out, np.uint8)


def is_null(p):
    return (p[1] & 0x1f) == 0x1f and p[2] == 0xff


def issy_field(kind, nbytes, value):
    """kind 'short': 0 + 15-bit ISCR; 'long': 10 + 22-bit ISCR (3 bytes only); 'bufs': 11xx...; -> nbytes bytes"""
    if kind == 'short':
        v = [(value >> 8) & 0x7f, value & 0xff, 0]
    elif kind == 'long':
        assert nbytes == 3
        v = [0x80 | ((value >> 16) & 0x3f), (value >> 8) & 0xff, value & 0xff]
    else:
        v = [0xC0 | ((value >> 8) & 0x3f), value & 0xff, 0]
    return v[:nbytes]


def slot_stream(ts, issy=0, npd=False, span=0, issy_kinds=None, damage=()):
    """-> (uint8 stream of slots, list of TS packet indices [first, last] each slot stands for).  issy_kinds(k) names slot k's
    ISSY field ('short', 'long', 'bufs'); damage: slot numbers whose UP gets a bit error after the CRC was computed."""
    L = slot_len(issy, npd)
    slots, spans = [], []
    dnp, prev_crc, first = 0, 0, 0
    for i, p in enumerate(ts):
        if npd and is_null(p) and dnp < 255:
            dnp += 1
            continue
        k = len(slots)
        s = np.zeros(L, np.uint8)
        s[0] = prev_crc
        s[1:188] = p[1:]
        if issy:
            kind = issy_kinds(k) if issy_kinds else ('short' if issy == 2 else 'long')
            s[188:188 + issy] = issy_field(kind, issy, (977 * k + 13) & 0x3fffff)
        if npd:
            s[L - 1] = dnp
        prev_crc = crc8(crc_span(s, span))
        slots.append(s)
        spans.append((first, i))
        dnp, first = 0, i + 1
    for k in damage:
        slots[k][1 + (7 * k) % 187] ^= 0x10
    return np.concatenate(slots), spans


def frames_of_stream(stream, L, kbch_list, isi=0, sis=False, issyi=False, npd=False, dfl_list=None):
    """cut one ISI's slot stream into the data fields of BBFRAMEs of the given sizes (bits); the last frame takes what is left.
    -> list of (frame, (first byte, end byte) of the stream it holds)"""
    out, off, f = [], 0, 0
    while off < stream.size:
        kbch = kbch_list[f % len(kbch_list)]
        fb = kbch // 8
        D = min(fb - 10, dfl_list[f % len(dfl_list)] if dfl_list else fb - 10, stream.size - off)
        nxt = -(-off // L) * L
        syncd = (nxt - off) * 8 if nxt < off + D else NO_START
        fr = np.zeros(fb, np.uint8)
        fr[:10] = bbheader(3, D * 8, syncd, upl_bits=1504, sync=0x47, sis=1 if sis else 0, ccm=0, issyi=int(issyi), npd=int(npd), isi=0 if sis else isi)
        fr[10:10 + D] = stream[off:off + D]
        out.append((fr, (off, off + D)))
        off += D
        f += 1
    return out


def interleave(per_isi, order):
    """per_isi: {isi: [frames]}; order: ISI numbers, repeated cyclically, naming whose next frame is sent -> one list"""
    pos = {k: 0 for k in per_isi}
    out, i = [], 0
    while any(pos[k] < len(v) for k, v in per_isi.items()):
        k = order[i % len(order)]
        i += 1
        if pos[k] < len(per_isi[k]):
            out.append(per_isi[k][pos[k]])
            pos[k] += 1
    return out


# ---------------------------------------------------------------------------------------------------------- receiver model
def header_ok(fr):
    """-> dict of BBHEADER fields, or None: CRC-8 over the 10 bytes, DFL a whole number of bytes that fits the frame, SYNCD inside the
    data field or 65535"""
    if fr.size < 10 or crc8(fr[:10]) != 0:
        return None
    b = [int(x) for x in fr[:10]]
    h = {'ts_gs': b[0] >> 6, 'sis': (b[0] >> 5) & 1, 'issyi': (b[0] >> 3) & 1, 'npd': (b[0] >> 2) & 1, 'dfl': b[4] << 8 | b[5], 'syncd': b[7] << 8 | b[8]}
    h['isi'] = 0 if h['sis'] else b[1]
    if h['dfl'] % 8 or h['dfl'] > (fr.size - 10) * 8 or not (h['syncd'] == NO_START or h['syncd'] < h['dfl']):
        return None
    return h


LANE_KEYS = ('packets', 'nulls', 'ts_errs', 'broken_joins', 'undecided', 'frames', 'issy_bytes', 'iscr_valid', 'last_iscr', 'carried')


class Lane:
    def __init__(self, isi, issy):
        self.isi, self.issy = isi, issy
        self.carry, self.Lc = np.zeros(0, np.uint8), 0
        self.out = []
        self.st = dict.fromkeys(LANE_KEYS, 0)

    def stats(self):
        d = dict(self.st)
        d.update(issy_bytes=self.issy, carried=int(self.carry.size), isi=self.isi)
        return d


class Receiver:
    """one stream: up to 8 selected ISIs"""

    def __init__(self, sel=(0,), issy_bytes=0, crc_span=0, reinsert_nulls=True, check_crc=True):
        assert len(sel) <= 8
        self.cfg = (issy_bytes, crc_span, reinsert_nulls, check_crc)
        self.lanes = [Lane(i, issy_bytes) for i in sel]
        self.seen = set()
        self.rejected = self.skipped = 0

    def _emit(self, ln, slot, chk, npd, issy):
        _, span, reinsert, check = self.cfg
        dnp = int(slot[-1]) if npd and reinsert else 0
        for _ in range(dnp):
            ln.out.append(NULL_PACKET)
        ln.st['nulls'] += dnp
        p = np.empty(188, np.uint8)
        p[0] = 0x47
        p[1:] = slot[1:188]
        if check and chk is not None and crc8(crc_span(slot, span)) != chk:
            p[1] |= 0x80
            ln.st['ts_errs'] += 1
        ln.st['packets'] += 1
        ln.out.append(p)
        if issy:
            f = [int(x) for x in slot[188:188 + issy]]
            if f[0] < 0x80:
                ln.st['last_iscr'], ln.st['iscr_valid'] = f[0] << 8 | f[1], 1
            elif f[0] < 0xC0 and issy == 3:
                ln.st['last_iscr'], ln.st['iscr_valid'] = (f[0] & 0x3f) << 16 | f[1] << 8 | f[2], 1

    def _frame(self, fr):
        h = header_ok(fr)
        if h is None:
            self.rejected += 1
            return
        self.seen.add(h['isi'])
        ln = next((l for l in self.lanes if l.isi == h['isi']), None)
        if h['ts_gs'] != 3 or ln is None:
            self.skipped += 1
            return
        ln.st['frames'] += 1
        df = h['dfl'] // 8
        data = fr[10:10 + df]
        nostart = h['syncd'] == NO_START
        s0 = df if nostart else h['syncd'] // 8
        issy = 0
        if h['issyi']:
            if ln.issy == 0 and not nostart and s0 + 188 < df:
                top = int(data[s0 + 188])
                ln.issy = 2 if top < 0x80 else 3 if top < 0xC0 else 0
            if ln.issy == 0:
                ln.st['undecided'] += 1
                ln.carry = ln.carry[:0]
                return
            issy = ln.issy
        L = slot_len(issy, h['npd'])
        c = ln.carry.size
        if nostart:
            if c > 0:
                if ln.Lc == L and c + df <= L:
                    ln.carry = np.concatenate([ln.carry, data])
                else:
                    ln.st['broken_joins'] += 1
                    ln.carry = ln.carry[:0]
            return
        n = (df - s0 - 1) // L
        if c > 0:
            if ln.Lc == L and c + s0 == L:
                self._emit(ln, np.concatenate([ln.carry, data[:s0]]), int(data[s0]), h['npd'], issy)
            else:
                ln.st['broken_joins'] += 1
        for k in range(n):
            p = s0 + k * L
            self._emit(ln, data[p:p + L], int(data[p + L]), h['npd'], issy)
        ln.carry, ln.Lc = data[s0 + n * L:].copy(), L
        ln.npd_c, ln.issy_c = h['npd'], issy

    def process(self, frames):
        """-> list (one per selected ISI) of uint8 arrays: the TS bytes these frames complete"""
        for ln in self.lanes:
            ln.out = []
        for fr in frames:
            self._frame(np.asarray(fr, np.uint8))
        return [np.concatenate(ln.out) if ln.out else np.zeros(0, np.uint8) for ln in self.lanes]

    def flush(self):
        """a whole slot held back for its CRC-8 leaves unchecked"""
        for ln in self.lanes:
            ln.out = []
            if ln.carry.size and ln.carry.size == ln.Lc:
                self._emit(ln, ln.carry, None, ln.npd_c, ln.issy_c)
                ln.carry = ln.carry[:0]
        return [np.concatenate(ln.out) if ln.out else np.zeros(0, np.uint8) for ln in self.lanes]

    def stats(self, slot):
        d = self.lanes[slot].stats()
        d.update(rejected_frames=self.rejected, skipped_frames=self.skipped)
        return d

    def seen_mask(self):
        m = [0] * 8
        for i in self.seen:
            m[i >> 5] |= 1 << (i & 31)
        return m


# ------------------------------------------------------------------------------------------------------------- test carriers
STAT_KEYS = LANE_KEYS + ('isi', 'rejected_frames', 'skipped_frames')


def scenario(seed, mis, issy_mode, npd, mixed, npk=90, span=0, damage=()):
    """one carrier: -> (frames in transmission order, {isi: TS as sent}, selection, receiver configuration).
    mis: three ISIs (two of them selected) instead of one SIS stream; issy_mode 'none' / '2' / '3' / 'auto'; mixed: short and
    normal BBFRAMEs of three codes in turn instead of one size; damage: slot numbers hit by a bit error on every ISI."""
    rng = np.random.default_rng(seed)
    isis = (5, 200, 17) if mis else (0,)
    issy = {'none': 0, '2': 2, '3': 3, 'auto': 2 + seed % 2}[issy_mode]
    kinds = (lambda k: 'bufs' if k % 7 == 4 else 'short' if issy == 2 or k % 3 == 1 else 'long') if issy else None
    sizes = [14232, 58192, 3072, 48408] if mixed else [14232]
    ts, per = {}, {}
    for n, i in enumerate(isis):
        ts[i] = make_ts(npk + 10 * n, rng, null_runs=npd)
        st, _ = slot_stream(ts[i], issy, npd, span, kinds, damage)
        per[i] = [f for f, _ in frames_of_stream(st, slot_len(issy, npd), sizes[n:] + sizes[:n], isi=i, sis=not mis, issyi=issy > 0, npd=npd)]
    frames = interleave(per, [5, 200, 200, 17, 5] if mis else [0])
    sel = (200, 5) if mis else (0,)
    cfg = {'issy_bytes': 0 if issy_mode in ('none', 'auto') else issy, 'crc_span': span, 'reinsert_nulls': 1, 'check_crc': 1}
    return frames, ts, sel, cfg


GRID = [(seed, mis, im, npd, mixed) for seed in (1, 2) for mis in (False, True) for im in ('none', '2', '3', 'auto') for npd in (False, True)
        for mixed in (False, True)]
