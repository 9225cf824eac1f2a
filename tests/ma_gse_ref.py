"""GSE over multistream / ACM carriers (TS 102 606-1) in pure Python, both directions, written independently of the library and built
on tests/ma_ref.py and orc_bbts.bbheader: a transmitter (PDUs -> GSE packets, fragmented to fit data fields of any size, per ISI, at
most three frag ids open per ISI, all four label types, padding) and a receiver model of the rules of the library's mode-adaptation
GSE (include/dvbs2gpu.h).  Test infrastructure only: the yardstick of tests/test_ma_gse_cpu.py and tests/test_gpu_ma_gse.py."""
import numpy as np

import ma_ref as M
from orc_bbts import bbheader, crc32_mpeg

LABEL_BYTES = {0: 6, 1: 3, 2: 0, 3: 0}
PDU_REASSEMBLED, PDU_LABEL = 1, 2
SLOT_BYTES = 65536
GSE_KEYS = ('frames', 'packets', 'complete_pdus', 'reassembled_pdus', 'crc_failures', 'dropped_no_slot', 'dropped_overflow', 'dropped_no_fit',
            'bytes_delivered', 'malformed_frames', 'open_slots', 'last_crc_err')


def gre(proto, pdu):
    return bytes([0, 0]) + (bytes([proto >> 8, proto & 0xff]) if proto in (0x0800, 0x86DD) else b'') + bytes(pdu)


# ------------------------------------------------------------------------------------------------------------- transmitter
def header(S, E, lt, length):
    assert 0 <= length < 4096
    return bytes([(S << 7) | (E << 6) | (lt << 4) | (length >> 8), length & 0xff])


def complete_packet(proto, pdu, lt=2, label=b''):
    body = bytes([proto >> 8, proto & 0xff]) + bytes(label) + bytes(pdu)
    return header(1, 1, lt, len(body)) + body


def start_packet(frag_id, proto, pdu, piece, lt=2, label=b''):
    """-> (packet, what is left to send: the rest of the PDU + its CRC-32)"""
    total = 2 + len(label) + len(pdu)
    tl, pr = bytes([total >> 8, total & 0xff]), bytes([proto >> 8, proto & 0xff])
    crc = crc32_mpeg(tl + pr + bytes(label) + bytes(pdu))
    body = bytes([frag_id]) + tl + pr + bytes(label) + bytes(pdu[:piece])
    return header(1, 0, lt, len(body)) + body, bytes(pdu[piece:]) + crc.to_bytes(4, 'big')


def next_packet(frag_id, rest, piece, lt=3):
    """a middle packet of `piece` bytes, or the END when that is all of `rest`"""
    body = bytes([frag_id]) + rest[:piece]
    return header(0, 1 if piece == len(rest) else 0, lt, len(body)) + body, rest[piece:]


class Tx:
    """one ISI: queues PDUs and fills data fields with GSE packets.  Up to `max_open` PDUs are in flight at once, each under its own
    frag id; a data field may end in padding."""

    def __init__(self, rng, max_open=3, p_pad=0.15):
        self.rng, self.max_open, self.p_pad = rng, max_open, p_pad
        self.queue, self.open, self.next_id, self.sent = [], [], 0, []

    def push(self, proto, pdu, lt):
        label = bytes(self.rng.integers(0, 256, LABEL_BYTES[lt], dtype=np.uint8))
        self.queue.append((proto, bytes(pdu), lt, label))

    def busy(self):
        return bool(self.queue or self.open)

    def _frag_id(self):
        while any(o['id'] == self.next_id for o in self.open):
            self.next_id = (self.next_id + 1) % 256
        i, self.next_id = self.next_id, (self.next_id + 1) % 256
        return i

    def fill(self, D):
        """-> at most D bytes of GSE packets (what follows them in the data field is padding)"""
        out, rng = b'', self.rng
        while self.busy():
            room = D - len(out)
            if out and rng.random() < self.p_pad:
                break
            go_on = self.open and (not self.queue or len(self.open) == self.max_open or rng.random() < 0.5)
            if go_on:
                o = self.open[int(rng.integers(0, len(self.open)))]
                if room < 3 + 4:
                    break
                piece = min(len(o['rest']), room - 3, 4094)
                if piece < len(o['rest']):                            # a middle packet leaves the whole CRC-32 for the END
                    piece = min(piece, len(o['rest']) - 4)
                    if piece <= 0:
                        break
                pkt, o['rest'] = next_packet(o['id'], o['rest'], piece)
                if not o['rest']:
                    self.open.remove(o)
                    self.sent.append(o['pdu'])
                out += pkt
                continue
            proto, pdu, lt, label = self.queue[0]
            whole = 4 + len(label) + len(pdu)
            if whole <= room and whole - 2 < 4096 and rng.random() < 0.75:
                out += complete_packet(proto, pdu, lt, label)
                self.sent.append((proto, pdu, lt))
                self.queue.pop(0)
            elif len(self.open) < self.max_open and room >= 7 + len(label) + 1 and len(pdu) > 0:
                piece = min(len(pdu), room - 7 - len(label), 4095 - 5 - len(label))
                if whole <= room:
                    piece = min(piece, max(1, len(pdu) // 2))
                i = self._frag_id()
                pkt, rest = start_packet(i, proto, pdu, piece, lt, label)
                self.open.append({'id': i, 'rest': rest, 'pdu': (proto, pdu, lt)})
                self.queue.pop(0)
                out += pkt
            else:
                break
        assert len(out) <= D
        return out


def gse_frame(data, frame_bytes, isi=0, sis=False, dfl_bytes=None, issyi=0, npd=0, upl_bits=0):
    """one BBFRAME of frame_bytes bytes with `data` at the start of its data field; DFL covers the whole field (zero padding after the
    packets) unless dfl_bytes says otherwise"""
    D = frame_bytes - 10 if dfl_bytes is None else dfl_bytes
    assert len(data) <= D <= frame_bytes - 10
    fr = np.zeros(frame_bytes, np.uint8)
    fr[:10] = bbheader(1, D * 8, 0, upl_bits=upl_bits, sync=0, sis=1 if sis else 0, ccm=0, issyi=issyi, npd=npd, isi=0 if sis else isi)
    fr[10:10 + len(data)] = np.frombuffer(bytes(data), np.uint8)
    return fr


def make_pdus(rng, n, big=False, lts=(0, 1, 2, 3)):
    out = []
    for k in range(n):
        r = rng.random()
        size = int(rng.integers(0, 40)) if r < 0.25 else int(rng.integers(40, 1500)) if r < 0.85 else int(rng.integers(1500, 9000 if big else 3000))
        proto = [0x0800, 0x86DD, 0x0806, 0x88B5][int(rng.integers(0, 4))]
        out.append((proto, bytes(rng.integers(0, 256, size, dtype=np.uint8)), int(lts[int(rng.integers(0, len(lts)))])))
    return out


def gse_frames(rng, isi, sizes, npdus, sis=False, big=False, lts=(0, 1, 2, 3)):
    """-> (frames of one ISI, the PDUs as sent, in the order their last packet leaves)"""
    tx = Tx(rng)
    for proto, pdu, lt in make_pdus(rng, npdus, big, lts):
        tx.push(proto, pdu, lt)
    frames, f = [], 0
    while tx.busy():
        fb = sizes[f % len(sizes)]
        data = tx.fill(fb - 10)
        exact = len(data) > 0 and rng.random() < 0.3               # DFL ends with the last packet: no padding at all
        frames.append(gse_frame(data, fb, isi, sis, dfl_bytes=len(data) if exact else None))
        f += 1
    return frames, tx.sent


# ---------------------------------------------------------------------------------------------------------- receiver model
class Receiver(M.Receiver):
    """ma_ref.Receiver + GSE: the GSE frames of a selected ISI are walked when `gse` is on; each lane has three reassembly slots and
    the rows (offset in the lane's output of the call, bytes, protocol type, flags) of the last process()"""

    def __init__(self, sel=(0,), gse=True, **cfg):
        super().__init__(sel, **cfg)
        self.gse = gse
        for ln in self.lanes:
            ln.slots = [None, None, None]
            ln.g = dict.fromkeys(GSE_KEYS, 0)
            ln.rows = []

    def _deliver(self, ln, proto, pdu, flags):
        b = gre(proto, pdu)
        ln.rows.append((sum(len(x) for x in ln.out), len(b), proto, flags))
        ln.out.append(np.frombuffer(b, np.uint8))
        ln.g['reassembled_pdus' if flags & PDU_REASSEMBLED else 'complete_pdus'] += 1
        ln.g['bytes_delivered'] += len(b)

    def _walk(self, ln, data):
        g, df, at = ln.g, len(data), 0
        g['frames'] += 1
        while at < df:
            h1 = data[at]
            S, E, lt = h1 >> 7, (h1 >> 6) & 1, (h1 >> 4) & 3
            if not S and not E and lt == 0:
                return                                                 # padding
            if at + 2 > df:
                g['malformed_frames'] += 1
                return
            length = (h1 & 15) << 8 | data[at + 1]
            fixed = 2 if S and E else 5 if S else 1
            label = LABEL_BYTES[lt] if S else 0
            if length < fixed + label + (4 if E and not S else 0) or at + 2 + length > df:
                g['malformed_frames'] += 1
                return
            pkt = data[at + 2:at + 2 + length]
            payload = pkt[fixed + label:]
            at += 2 + length
            g['packets'] += 1
            if S and E:
                self._deliver(ln, pkt[0] << 8 | pkt[1], payload, PDU_LABEL if label else 0)
                continue
            fid = pkt[0]
            if S:
                k = next((i for i, s in enumerate(ln.slots) if s is None or s['id'] == fid), None)
                if k is None:
                    g['dropped_no_slot'] += 1
                    continue
                ln.slots[k] = {'id': fid, 'proto': pkt[3] << 8 | pkt[4], 'label': bool(label), 'buf': bytearray(payload), 'crc': crc32_mpeg(pkt[1:])}
                continue
            k = next((i for i, s in enumerate(ln.slots) if s is not None and s['id'] == fid), None)
            if k is None:
                continue
            s = ln.slots[k]
            if len(s['buf']) + len(payload) > SLOT_BYTES:
                ln.slots[k] = None
                g['dropped_overflow'] += 1
            elif not E:
                s['buf'] += payload
                s['crc'] = crc32_mpeg(payload, s['crc'])
            else:
                ln.slots[k] = None
                s['buf'] += payload[:-4]
                g['last_crc_err'] = int(crc32_mpeg(payload[:-4], s['crc']) != int.from_bytes(payload[-4:], 'big'))
                if g['last_crc_err']:
                    g['crc_failures'] += 1
                else:
                    self._deliver(ln, s['proto'], s['buf'], PDU_REASSEMBLED | (PDU_LABEL if s['label'] else 0))

    def _frame(self, fr):
        h = M.header_ok(fr)
        if self.gse and h is not None and h['ts_gs'] == 1:
            ln = next((l for l in self.lanes if l.isi == h['isi']), None)
            upl = int(fr[2]) << 8 | int(fr[3])
            if ln is not None and upl == 0 and not h['issyi'] and not h['npd']:
                self.seen.add(h['isi'])
                ln.st['frames'] += 1
                self._walk(ln, bytes(fr[10:10 + h['dfl'] // 8]))
                return
        super()._frame(fr)

    def process(self, frames):
        for ln in self.lanes:
            ln.rows = []
        return super().process(frames)

    def gse_stats(self, slot):
        ln = self.lanes[slot]
        d = dict(ln.g)
        d['open_slots'] = sum(s is not None for s in ln.slots)
        return d

    def rows(self, slot):
        return list(self.lanes[slot].rows)


# ------------------------------------------------------------------------------------------------------------- test carriers
def scenario(seed, mis, mixed, nisi=2, with_ts=False, npdus=None, big=False):
    """one well-formed carrier -> (frames in transmission order, {isi: what it carries}, selection).
    mis False: one SIS stream (ISI 0).  True: nisi ISIs carry GSE and one more (9) is sent but not selected.  mixed: frame sizes of
    several codes in turn, 384 and 7274 bytes among them, instead of one size.  with_ts: the first selected ISI also carries TS frames
    (and one more ISI is TS only), so its lane gets both.  `carries`: {'gse': [(proto, pdu, lt)], 'ts': packets or None}"""
    rng = np.random.default_rng(seed)
    sizes = [7274, 384, 1779, 6051, 2001] if mixed else [1779]
    npdus = npdus if npdus is not None else 12 if mis else 30      # at most 48 frames per carrier
    gse_isis = ([5, 200, 17][:nisi] + [9]) if mis else [0]
    per, carries = {}, {}
    for n, i in enumerate(gse_isis):
        fr, sent = gse_frames(rng, i, sizes[n % len(sizes):] + sizes[:n % len(sizes)], 5 if i == 9 else npdus + 2 * n, sis=not mis, big=big)
        per[i] = [('g', f) for f in fr]
        carries[i] = {'gse': sent, 'ts': None}
    order = [5, 200, 200, 17, 9, 5] if mis else [0]
    if with_ts:
        ts_isis = [gse_isis[0]] + ([33] if mis else [])
        for i in ts_isis:
            ts = M.make_ts(25, rng, null_runs=False)
            st, _ = M.slot_stream(ts)
            fr = [f for f, _ in M.frames_of_stream(st, M.slot_len(0, False), [14232, 3072], isi=i, sis=not mis)]
            carries.setdefault(i, {'gse': [], 'ts': None})['ts'] = ts
            mixed_list, a, b = [], per.get(i, []), [('t', f) for f in fr]
            while a or b:                                              # TS and GSE frames of the ISI in turn, runs of random length
                src = a if a and (not b or rng.random() < 0.5) else b
                mixed_list.append(src.pop(0))
            per[i] = mixed_list
        order = order + [33] if mis else order
    frames = [f for _, f in M.interleave(per, [k for k in order if k in per])]
    sel = tuple([200, 5, 17][:nisi] + ([33] if with_ts else [])) if mis else (0,)
    sel = tuple(i for i in sel if i in per)
    return frames, carries, sel


GRID = [(1, False, False, 1, False), (2, False, True, 1, False), (3, True, False, 2, False), (4, True, True, 2, False), (5, True, True, 3, False),
        (6, True, True, 2, True), (7, False, True, 1, True), (8, True, False, 3, True)]


def split_output(out, rows):
    """a lane's output of one call -> (the GRE packets the rows name, the bytes no row covers, in order)"""
    pdus, rest, at = [], [], 0
    for off, n, proto, flags in rows:
        rest.append(out[at:off])
        pdus.append((proto, bytes(out[off:off + n]), flags))
        at = off + n
    rest.append(out[at:])
    return pdus, np.concatenate(rest) if rest else np.zeros(0, np.uint8)
