"""DVB-T2 high-efficiency-mode (HEM) BBFRAMEs in pure numpy / Python, both directions, written independently of the library from the
rules in include/dvbs2gpu.h (EN 302 755 5.1.7 / 5.1.8 from memory): a transmitter (TS -> 187-byte UPs, null-packet deletion with DNP,
the ISSY field in the BBHEADER, data fields of given sizes with SYNCD, header CRC-8 ^ MODE, padding behind DFL) and a receiver model
that parses HEM frames by those rules and normal-mode frames by the model of tests/ma_ref.py, in one lane state.  Test infrastructure
only; the receiver model is the yardstick of tests/test_hem_cpu.py and tests/test_gpu_hem.py."""
import numpy as np

import ma_ref as M
from ma_ref import NO_START, NULL_PACKET, Receiver, crc8, interleave, is_null, make_ts
from orc_bbts import bbheader

# the slot layout, in one place: [UP][DNP 0/1]; dvbs2gpu_bbts_ma_get_hem_layout reports the library's
LAYOUT = {'up_off': 0, 'up_len': 187, 'dnp_off': 187, 'mode': 1}
STAT_KEYS = M.STAT_KEYS + ('hem_frames',)
_HEM = 1000                                                # a lane's Lc is this + the slot length while its carry is HEM bytes


def slot_len(npd):
    return LAYOUT['dnp_off'] + (1 if npd else 0)


# ------------------------------------------------------------------------------------------------------------- transmitter
def slot_stream(ts, npd=False):
    """-> uint8 stream of HEM slots: the packets without their sync bytes, null packets deleted into the DNP byte behind the next one"""
    slots, dnp = [], 0
    for p in ts:
        if npd and is_null(p) and dnp < 255:
            dnp += 1
            continue
        slots.append(np.concatenate([p[1:], np.array([dnp] if npd else [], np.uint8)]))
        dnp = 0
    return np.concatenate(slots).astype(np.uint8)


def iscr_of(k):
    """the ISSY field announced for slot k: ('short' | 'long', value)"""
    return ('short', (977 * k + 13) & 0x7fff) if k % 3 else ('long', (70001 * k + 5) & 0x3fffff)


def frames_of_stream(stream, L, dfls, isi=0, sis=False, issyi=False, npd=False, ts_gs=3, frame_bytes=None, pad=None):
    """cut one PLP's slot stream into HEM BBFRAMEs: frame f holds dfls[f] data-field bytes (cyclic; the last takes what is left) and
    is frame_bytes long, or 10 + DFL/8 + pad[f] (pad cyclic, default none).  The bytes behind DFL are filled with 0xA5.  -> frames"""
    out, off, f = [], 0, 0
    while off < stream.size:
        D = min(dfls[f % len(dfls)], stream.size - off)
        nxt = -(-off // L) * L
        start = nxt < off + D
        fb = frame_bytes if frame_bytes else 10 + D + (pad[f % len(pad)] if pad else 0)
        assert fb >= 10 + D
        kind, v = iscr_of(nxt // L) if start else ('short', 0x7abc)       # a frame in which no UP starts: a field nobody may take
        fld = M.issy_field(kind, 3, v) if issyi else [0, 0, 0]
        fr = np.full(fb, 0xA5, np.uint8)
        fr[:10] = bbheader(ts_gs, D * 8, (nxt - off) * 8 if start else NO_START, upl_bits=fld[0] << 8 | fld[1], sync=fld[2], sis=1 if sis else 0, ccm=0,
                           issyi=int(issyi), npd=int(npd), isi=0 if sis else isi)
        fr[9] ^= LAYOUT['mode']
        fr[10:10 + D] = stream[off:off + D]
        out.append(fr)
        off += D
        f += 1
    return out


# ---------------------------------------------------------------------------------------------------------- receiver model
class HemReceiver(Receiver):
    """tests/ma_ref.py's receiver with the HEM switch: normal-mode frames go to the base class, HEM frames are parsed here; both
    use the same lanes, so a carry of the other mode is a broken join"""

    def __init__(self, sel=(0,), hem=True, **cfg):
        super().__init__(sel, **cfg)
        self.hem = hem
        for ln in self.lanes:
            ln.st['hem_frames'] = 0

    def _emit_hem(self, ln, slot, npd):
        dnp = int(slot[-1]) if npd and self.cfg[2] else 0
        ln.out += [NULL_PACKET] * dnp
        ln.st['nulls'] += dnp
        ln.out.append(np.concatenate([np.array([0x47], np.uint8), slot[:LAYOUT['up_len']]]))
        ln.st['packets'] += 1

    def _frame(self, fr):
        c = crc8(fr[:9]) if fr.size >= 10 else -1
        if not (self.hem and c >= 0 and int(fr[9]) == c ^ LAYOUT['mode']):
            return super()._frame(fr)                              # normal mode, or rejected there
        g = fr.copy()
        g[9] = c
        h = M.header_ok(g)                                         # DFL and SYNCD: the same conditions
        if h is None:
            self.rejected += 1
            return
        self.seen.add(h['isi'])
        ln = next((l for l in self.lanes if l.isi == h['isi']), None)
        if h['ts_gs'] != 3 or ln is None:
            self.skipped += 1
            return
        ln.st['frames'] += 1
        ln.st['hem_frames'] += 1
        df = h['dfl'] // 8
        data = fr[10:10 + df]
        L = slot_len(h['npd'])
        c, same = ln.carry.size, ln.Lc == _HEM + L
        if h['syncd'] == NO_START:
            if c > 0:
                if same and c + df <= L:
                    ln.carry = np.concatenate([ln.carry, data])
                else:
                    ln.st['broken_joins'] += 1
                    ln.carry = ln.carry[:0]
            return
        s0 = h['syncd'] // 8
        if c > 0:
            if same and c + s0 == L:
                self._emit_hem(ln, np.concatenate([ln.carry, data[:s0]]), h['npd'])
            else:
                ln.st['broken_joins'] += 1
        n = (df - s0) // L
        for k in range(n):
            self._emit_hem(ln, data[s0 + k * L:s0 + (k + 1) * L], h['npd'])
        if h['issyi']:
            f = [int(fr[2]), int(fr[3]), int(fr[6])]
            if f[0] < 0x80:
                ln.st['last_iscr'], ln.st['iscr_valid'] = f[0] << 8 | f[1], 1
            elif f[0] < 0xC0:
                ln.st['last_iscr'], ln.st['iscr_valid'] = (f[0] & 0x3f) << 16 | f[1] << 8 | f[2], 1
        ln.carry, ln.Lc = data[s0 + n * L:].copy(), _HEM + L
        ln.npd_c, ln.issy_c = h['npd'], 0

    def flush(self):
        """a HEM carry is a partial slot: nothing leaves and it is cleared (a whole one, completed by a SYNCD = 65535 frame, leaves)"""
        hem = [ln.Lc >= _HEM and ln.carry.size > 0 for ln in self.lanes]
        held = [ln.carry for ln in self.lanes]
        for ln, is_hem in zip(self.lanes, hem):
            if is_hem:
                ln.carry = ln.carry[:0]
        out = super().flush()
        for j, ln in enumerate(self.lanes):
            if hem[j] and held[j].size == ln.Lc - _HEM:
                ln.out = []
                self._emit_hem(ln, held[j], ln.npd_c)
                out[j] = np.concatenate(ln.out)
        return out


# ------------------------------------------------------------------------------------------------------------- test carriers
def run_model(frames, sel, cfg, step=4, hem=True):
    rx = HemReceiver(sel, hem=hem, **cfg)
    outs = [[] for _ in sel]
    for a in range(0, len(frames), step):
        for j, o in enumerate(rx.process(frames[a:a + step])):
            outs[j].append(o)
    for j, o in enumerate(rx.flush()):
        outs[j].append(o)
    return rx, [np.concatenate(o) for o in outs]


CFG = {'issy_bytes': 0, 'crc_span': 0, 'reinsert_nulls': 1, 'check_crc': 1}


def ts_for(rng, nbytes, npd):
    """enough packets for about nbytes of slots"""
    return make_ts(max(2, nbytes // 187), rng, null_runs=npd)


def random_carrier(seed, npd, issyi, mis=False, nframes=12):
    """frames of 60 to 800 bytes with random cuts, some with padding behind DFL -> (frames, {isi: TS}, selection)"""
    rng = np.random.default_rng(seed)
    isis = (5, 200, 17) if mis else (0,)
    per, ts = {}, {}
    share = nframes // len(isis)
    for i in isis:
        dfls = [int(x) for x in rng.integers(50, 700, share)]
        ts[i] = ts_for(rng, sum(dfls), npd)
        st = slot_stream(ts[i], npd)[:sum(dfls)]                   # cut where the frames end: the last packet may stay open
        per[i] = frames_of_stream(st, slot_len(npd), dfls, isi=i, sis=not mis, issyi=issyi, npd=npd, pad=[0, 0, 37, 0, 90])
    frames = interleave(per, [5, 200, 200, 17, 5] if mis else [0])
    return frames, ts, ((200, 5) if mis else (0,))


# data-field sizes for 188-byte slots (NPD on) that meet, in this order: a slot that ends with its data field (tail 0) and SYNCD = 0
# behind it; two data fields shorter than what the open slot lacks (SYNCD 65535) and a third that completes it with its first byte,
# the DNP; DFL = 0; and a SYNCD 65535 data field that completes the slot exactly, so that the DNP is the last carried byte
EDGE_DFLS = [376, 300, 40, 35, 200, 0, 101, 76, 250, 120]


def edge_carrier(seed=3):
    rng = np.random.default_rng(seed)
    ts = ts_for(rng, sum(EDGE_DFLS) + 400, True)
    st = slot_stream(ts, True)
    frames = frames_of_stream(st, 188, EDGE_DFLS + [400], sis=True, issyi=True, npd=True, pad=[0, 11, 0, 0, 150])
    return frames, ts


def mixed_modes(seed=4):
    """HEM -> NM -> HEM in one lane, each section cut before its last frame so that a carry of the other mode meets the next one.
    -> (frames, [TS of each section])"""
    rng = np.random.default_rng(seed)
    parts, out = [make_ts(8, rng, null_runs=False) for _ in range(3)], []
    for k, ts in enumerate(parts):
        if k == 1:
            st, _ = M.slot_stream(ts)
            fr = [f for f, _ in M.frames_of_stream(st, 188, [4800], sis=True)][:-1]
        else:
            fr = frames_of_stream(slot_stream(ts), 187, [431, 290, 517], sis=True)[:-1]
        out += fr
    return out, parts


def carriers():
    """name -> (frames, selection): what the host bank and the kernels are compared with the model on"""
    out = {}
    for seed, npd, issyi, mis in [(1, False, False, False), (2, True, True, False), (3, True, False, True), (4, False, True, True)]:
        frames, _, sel = random_carrier(seed, npd, issyi, mis)
        frames = list(frames)
        frames[5] = frames[5].copy()
        frames[5][9] ^= 0x40                                       # neither c nor c ^ 1: rejected, and the lane's next join breaks
        out['random seed %d npd %d issyi %d mis %d' % (seed, npd, issyi, mis)] = (frames, sel)
    out['edge cuts'] = (edge_carrier()[0], (0,))
    out['edge cuts, frame 2 removed'] = ([f for k, f in enumerate(edge_carrier()[0]) if k != 2], (0,))
    out['HEM NM HEM'] = (mixed_modes()[0], (0,))
    gs = random_carrier(6, False, False, False)[0]
    extra = frames_of_stream(np.arange(300, dtype=np.uint8), 187, [150], sis=True, ts_gs=1)      # HEM frames that are not TS: skipped
    out['HEM GSE frames between'] = (gs[:4] + extra[:1] + gs[4:8] + extra[1:] + gs[8:], (0,))
    return out
